// The pure decisions of the binned ray tracer's host side (capi/pass_plan.hpp) on the CPU:
//   1. the kept-pass plan over every combination of valid / key equal / count known / count above the cap / same kind of pass /
//      MIRT_BIN_REUSE off, against the statements the three sites used to carry each for itself;
//   2. the three capacity rules of a pair list at 0, 1, 4095, 2^20 and 2^31 pairs: the values, no wrap of the size_t arithmetic,
//      and room in the 32 bits a list's capacity is kept in;
//   3. the depth shells stay within BIN_MAX_KEYS: light cubes for every grid in {64, 128, 256} x 1 .. MIRT_MAX_LIGHTS positions
//      whose keys fit at all, camera frames for every tile count up to the limit of frame_fits_binning, under every environment value;
//   4. the faces of fill_light_frames: consecutive bases, tab == 1 + k, the six axis frames, the shell parameters, and
//      shell_iw == 0 for a degenerate range;
//   5. the view makers' empty-cube rule: without rows the row pointer is the origin table's, with rows the row table's (fake
//      addresses, nothing is dereferenced);
//   6. the FNV helper: the published FNV-1a value of "a", and mixing in pieces equals mixing at once;
//   7. whether a ray query bins (query_bins), over every mode and every combination of its three conditions: what each mode
//      promises, stated per mode.
#include "../../cpp-raytracer-rasterizer_amd/capi/pass_plan.hpp"

#include <cstdio>
#include <cstdlib>

using namespace mirt;

#define CHECK(c) do { if (!(c)) { printf("FAILED %s (line %d)\n", #c, __LINE__); return 1; } } while (0)

static int kept_pass_cases()
{
    for (int m = 0; m < 64; m++) {
        const bool valid = m & 1, key_equal = m & 2, known = m & 4, above = m & 8, same_kind = m & 16, reuse_off = m & 32;
        // the statements of binned_pass and transient_light_pass before they were one function ...
        bool fresh = !valid || !key_equal;
        const bool may_guess = same_kind;
        if (!fresh && known && above) fresh = true;
        const bool reuse = !fresh && !reuse_off;
        const PassPlan p = kept_pass_plan(valid, key_equal, known, above, same_kind, reuse_off);
        CHECK(p.fresh == fresh && p.may_guess == may_guess && p.reuse == reuse);
        // ... and what follows from them: a pass is never both run and kept, a pass whose key changed always runs, and a kept pass whose
        // list overflowed runs again whatever else holds
        CHECK(!(p.fresh && p.reuse));
        if (!valid || !key_equal) CHECK(p.fresh);
        if (known && above) CHECK(p.fresh);
        if (reuse_off) CHECK(!p.reuse);
        if (valid && key_equal && !(known && above) && !reuse_off) CHECK(p.reuse);
    }
    return 0;
}

static int capacity_cases()
{
    const uint32_t counts[] = { 0u, 1u, 4095u, 1u << 20, 1u << 31 };
    const unsigned long long wanted[] = { 4096ull, 4097ull, 10238ull, 1576960ull, 3221229568ull };
    const unsigned long long grown[] = { 5120ull, 5121ull, 12797ull, 1971200ull, 4026536960ull };
    const unsigned long long readback[] = { 4096ull, 4097ull, 8702ull, 1183744ull, 2415923200ull };
    for (int i = 0; i < 5; i++) {
        const uint32_t k = counts[i];
        const size_t w = pairs_wanted(k), gr = pairs_grown(w), rb = pairs_after_readback(k);
        CHECK((unsigned long long)w == wanted[i] && (unsigned long long)gr == grown[i] && (unsigned long long)rb == readback[i]);
        CHECK(w > k && gr >= w && rb > k);                   // nothing wrapped
        CHECK(gr <= 0xFFFFFFFFull && rb <= 0xFFFFFFFFull);   // a list's capacity is a 32-bit count
    }
    return 0;
}

static int shell_cases()
{
    const int envs[] = { 0, 1, 2, 7, 16, 64, 65, -3 };
    for (int env : envs) {
        for (int grid : { 64, 128, 256 })
            for (int nl = 1; nl <= MIRT_MAX_LIGHTS; nl++) {
                const int ns = light_shells_rule(nl, grid, 0u, env);
                const long long bins = 6ll * grid * grid * nl;
                CHECK(ns >= 1 && ns <= 64);
                if (cube_keys_fit(nl, grid)) CHECK(bins * ns + 64 <= (long long)BIN_MAX_KEYS);
                else CHECK(ns == 1);
                const int start = (env >= 1 && env <= 64) ? env : 16;
                CHECK(ns <= start);
                if (ns < start && ns > 1) CHECK(bins * (ns * 2) + 64 > (long long)BIN_MAX_KEYS || (start >> 1) < ns * 2);
            }
        CHECK(light_shells_rule(0, 64, 0u, env) == light_shells_rule(1, 64, 0u, env));   // no light: one cube's worth
        const long long limit = (long long)BIN_MAX_KEYS - 64;                            // the most tiles frame_fits_binning lets through
        for (long long tiles = 1; tiles <= limit; tiles += (tiles < 70000 || tiles > limit - 70000) ? 1 : 997) {
            const int ns = camera_shells_rule(tiles, env);
            CHECK(ns >= 1 && ns <= 64 && tiles * ns + 64 <= (long long)BIN_MAX_KEYS);
        }
    }
    CHECK(camera_shells_rule(1, 0) == 8 && camera_shells_rule(0, 0) == 8 && camera_shells_rule(240 * 135, 0) == 8);
    CHECK(camera_shells_rule((4ll << 20) / 3, 0) == 3 && camera_shells_rule(4ll << 20, 0) == 1);
    CHECK(light_shells_rule(1, 64, 0u, 0) == 16 && light_shells_rule(32, 64, 0u, 0) == 8 && light_shells_rule(1, 256, 0u, 0) == 16);
    // frame_fits_binning counts 8 x 8-pixel tiles
    CHECK(frame_fits_binning(1, 1) && frame_fits_binning(1920, 1080) && frame_fits_binning(7680, 4320) && frame_fits_binning(23000, 23000));
    CHECK(!frame_fits_binning(32768, 32768) && !frame_fits_binning(23200, 23200));
    CHECK(frame_fits_binning(8 * 2896, 8 * 2896) && !frame_fits_binning(8 * 2897, 8 * 2897));   // 2896^2 + 64 <= 8388607 < 2897^2 + 64
    return 0;
}

static int frame_cases()
{
    const float lo[3] = { -1.0f, -1.0f, -1.0f }, hi[3] = { 1.0f, 1.0f, 1.0f };
    double dn = -1.0, df = -1.0;
    const float inside[3] = { 0.0f, 0.5f, -0.5f }, outside[3] = { 4.0f, 0.0f, 0.0f };
    CHECK(shell_range(inside, lo, hi, &dn, &df) && dn == 0.0 && std::fabs(df - std::sqrt(5.5)) < 1e-12);
    CHECK(shell_range(outside, lo, hi, &dn, &df) && dn == 3.0 && std::fabs(df - std::sqrt(27.0)) < 1e-12);
    const float nan3[3] = { NAN, 0.0f, 0.0f };
    CHECK(!shell_range(nan3, lo, hi, &dn, &df));
    CHECK(!shell_range(inside, inside, inside, &dn, &df) && dn == 0.0 && df == 0.0);   // a box that is the point itself

    // origins: row 0 is the camera's place, rows 1 .. the light positions; the last light sits in a degenerate box of its own below
    const float origins[12] = { 9, 9, 9, 0.0f, -0.5f, -0.75f, 4.0f, 0.0f, 0.0f, 0.25f, 0.25f, 0.25f };
    const int nl = 3, B = 128, shells = 4;
    const uint32_t base = 5;
    BinFrameDesc fr[6 * 3];
    fill_light_frames(fr, origins, nl, B, shells, base, lo, hi);
    for (int k = 0; k < nl; k++) {
        const float *lpos = origins + 3 * (k + 1);
        CHECK(shell_range(lpos, lo, hi, &dn, &df));
        for (int face = 0; face < 6; face++) {
            const BinFrameDesc &d = fr[k * 6 + face];
            const int ax = face >> 1;
            CHECK(d.base == base + (uint32_t)(k * 6 + face) * (uint32_t)(B * B) && d.tab == 1 + k);
            for (int c = 0; c < 3; c++) {
                CHECK(d.P0[c] == (c == ax ? ((face & 1) ? -1.0f : 1.0f) : 0.0f));
                CHECK(d.Pu[c] == (c == (ax + 1) % 3 ? 1.0f : 0.0f) && d.Pv[c] == (c == (ax + 2) % 3 ? 1.0f : 0.0f));
                CHECK(d.rw[c] == d.P0[c] && d.ru[c] == d.Pu[c] && d.rv[c] == d.Pv[c]);
                CHECK(d.S[c] == lpos[c]);
            }
            CHECK(d.nbu == B && d.nbv == B && d.j0 == 0 && d.j1 == B && d.ulo == -1.0f && d.vlo == -1.0f && d.du == 2.0f / B && d.dv == 2.0f / B && d.dmax == 2.0f);
            CHECK(d.nshell == shells && d.shell_d0 == (float)dn && d.shell_iw == (float)(shells / (df - dn)) && d.shell_iw > 0.0f);
        }
    }
    // a degenerate range -- the box is the light's position, or the position is not a number: everything goes into shell 0
    fill_light_frames(fr, origins, 1, 64, 16, 0u, origins + 3, origins + 3);
    for (int face = 0; face < 6; face++) CHECK(fr[face].shell_iw == 0.0f && fr[face].nshell == 16 && fr[face].base == (uint32_t)face * 4096u);
    const float bad[6] = { 0, 0, 0, NAN, 0.0f, 0.0f };
    fill_light_frames(fr, bad, 1, 64, 16, 0u, lo, hi);
    for (int face = 0; face < 6; face++) CHECK(fr[face].shell_iw == 0.0f);
    return 0;
}

static int view_cases()
{
    // plain fake addresses: nothing is dereferenced
    const uint32_t *off = reinterpret_cast<const uint32_t *>(0x1000), *tri = reinterpret_cast<const uint32_t *>(0x4000);
    const LightRow *rows = reinterpret_cast<const LightRow *>(0x2000);
    const OriginRow *tab = reinterpret_cast<const OriginRow *>(0x3000);
    const BinFrameDesc *frames = reinterpret_cast<const BinFrameDesc *>(0x5000);
    const CubeView with = make_cube_view(off, rows, true, tab, tri, frames, 128, 8);
    CHECK(with.light_rows == rows && with.light_off == off && with.light_tri == tri && with.light_frames == frames && with.cube_bins == 128 && with.shells == 8);
    const CubeView without = make_cube_view(off, rows, false, tab, tri, frames, 64, 1);
    CHECK(without.light_rows == tab && without.light_off == off && without.cube_bins == 64 && without.shells == 1);
    const CubeView never_built = make_cube_view(off, nullptr, false, tab, nullptr, frames, 64, 1);   // a cube that never had a pair
    CHECK(never_built.light_rows == tab && never_built.light_rows != nullptr);
    return 0;
}

static int fnv_cases()
{
    CHECK(Fnv(0).mix("a", 1).h == 0xaf63dc4c8601ec8cull && Fnv(0).h == 0xcbf29ce484222325ull);
    const int v[3] = { 7, -1, 1 << 30 };
    CHECK(Fnv(42).mix(&v[0], 4).mix(&v[1], 4).mix(&v[2], 4).h == Fnv(42).mix(v, 12).h);
    CHECK(Fnv(42).mix(v, 12).h != Fnv(43).mix(v, 12).h && Fnv(42).mix(v, 12).h != Fnv(42).mix(v, 8).h);
    return 0;
}

static int query_bins_cases()
{
    for (int mode : { (int)MIRT_QUERY_AUTO, (int)MIRT_QUERY_BRUTE, (int)MIRT_QUERY_BINNED })
        for (int m = 0; m < 8; m++) {
            const bool may_bin = m & 1, held = m & 2, auto_says = m & 4;
            const bool got = query_bins(may_bin, mode, held, auto_says);
            // nothing bins what the frame path would not, BRUTE never bins, BINNED bins whatever it may, and AUTO bins what it may
            // when the cube is held or its rule says so, and nothing else: between them the three decide all 24 cases
            if (!may_bin || mode == MIRT_QUERY_BRUTE) CHECK(!got);
            if (may_bin && mode == MIRT_QUERY_BINNED) CHECK(got);
            if (mode == MIRT_QUERY_AUTO) CHECK(got == (may_bin && (held || auto_says)));
        }
    return 0;
}

int main()
{
    if (kept_pass_cases() || capacity_cases() || shell_cases() || frame_cases() || view_cases() || fnv_cases() || query_bins_cases()) return 1;
    printf("ok\n");
    return 0;
}
