// pass_plan.hpp -- the decisions of the binned ray tracer's host side that are pure arithmetic, free of library state: whether a
// kept pass still serves, how a pair list is sized, how many depth shells fit the sort's keys, the frame descriptors of the light
// cubes, whether a ray query bins, and the view a walk kernel gets of a cube's tables.  binned.cpp and query.cpp apply them to the
// streams' state and the uploaded scene; tests/cpp/pass_plan_test.cpp checks them on the CPU.
#pragma once

#include "../query/rt_query.hpp"
#include "cube_plan.hpp"

#include <cmath>
#include <cstring>

namespace mirt {

// FNV-1a over the bytes of what a pass or a cube depends on, starting from a seed (the scene's version): the keys never leave the
// process, only their equalities matter.
struct Fnv {
    uint64_t h;
    explicit Fnv(uint64_t seed) : h(0xcbf29ce484222325ull ^ seed) {}
    Fnv &mix(const void *p, size_t nb) { for (size_t i = 0; i < nb; i++) { h ^= ((const unsigned char *)p)[i]; h *= 0x100000001b3ull; } return *this; }
};

// ---- a kept pass ----
// What a stream does with the pass it holds when one for a new key is asked for.  fresh: the pass is run -- its key is new, or the
// list it kept turned out too small (its published count says so: the frame fell back to brute force and so would every later
// frame of this view, so the list must grow); may_guess: a count of an earlier pass of the same kind may size the list without a
// read-back (a camera-only count says nothing about light cubes); reuse: the pass is not run at all.
struct PassPlan { bool fresh, may_guess, reuse; };
inline PassPlan kept_pass_plan(bool valid, bool key_equal, bool count_known, bool count_above_cap, bool same_kind, bool reuse_off)
{
    const bool fresh = !valid || !key_equal || (count_known && count_above_cap);
    return PassPlan{ fresh, same_kind, !fresh && !reuse_off };
}

// ---- sizing a pair list ----
// A guessed list: room for half as many pairs again as the last count seen; when that needs a larger list, a quarter more than
// wanted; after a read-back that found the list too small, an eighth more than counted.
inline size_t pairs_wanted(uint32_t known) { return (size_t)known + known / 2 + 4096; }
inline size_t pairs_grown(size_t want) { return want + want / 4; }
inline size_t pairs_after_readback(uint32_t total) { return (size_t)total + total / 8 + 4096; }

// ---- depth shells within the sort's key space (env: the environment's value, 0 = not set) ----
// Per light-cube bin: as many as the keys allow, at most 16 (a bin's list grows with the square of the distance from the light;
// 16 shells leave a ray at a quarter of the scene's depth ~2 % of it).
inline int light_shells_rule(int nlights, int cube_bins, uint32_t keys_in_front, int env)
{
    const long long bins = 6ll * cube_bins * cube_bins * std::max(nlights, 1);
    int ns = (env >= 1 && env <= 64) ? env : 16;
    while (ns > 1 && bins * ns + keys_in_front + 64 > (long long)BIN_MAX_KEYS) ns >>= 1;
    return ns;
}
// Of the camera bins for a frame of `tiles` bins (the tiles' lists come out of the sort roughly front to back).
inline int camera_shells_rule(long long tiles, int env)
{
    int ns = (int)std::min<long long>(8, std::max<long long>(1, (4ll << 20) / std::max<long long>(tiles, 1)));
    if (env >= 1 && env <= 64) ns = env;
    while (ns > 1 && tiles * ns + 64 > (long long)BIN_MAX_KEYS) ns >>= 1;
    return ns;
}
// Can a frame of this size be binned at all?  (one sort key per 8 x 8-pixel tile at least)
inline bool frame_fits_binning(int W, int H)
{
    const long long tiles = (long long)((W + BIN_TILE - 1) / BIN_TILE) * ((H + BIN_TILE - 1) / BIN_TILE);
    return tiles + 64 <= (long long)BIN_MAX_KEYS;
}

// Nearest and farthest distance from `pos` to the box [lo, hi]: the range the depth shells of a ray family divide.
inline bool shell_range(const float *pos, const float *lo3, const float *hi3, double *dn, double *df)
{
    double n2 = 0.0, f2 = 0.0;
    for (int c = 0; c < 3; c++) {
        const double p = pos[c], lo = lo3[c], hi = hi3[c];
        const double near = p < lo ? lo - p : (p > hi ? p - hi : 0.0), far = std::max(std::fabs(p - lo), std::fabs(p - hi));
        n2 += near * near; f2 += far * far;
    }
    *dn = std::sqrt(n2); *df = std::sqrt(f2);
    return std::isfinite(*dn) && std::isfinite(*df) && *df > *dn;
}

// Frame descriptors of the light cubes: six faces of B x B bins around every light position, every bin's list ordered in
// `shells` depth shells of the candidates' `near` bound (sort key = (base + bin) * shells + shell; `base_bins` = where light 0's
// face 0 starts, in bins of `shells` keys).  A shadow ray walks only the shells up to the one its 0.99 r falls into (k_rt_trace2).
// Light position k is origins[3 * (k + 1) ..]: row 0 is the camera's.  [lo3, hi3]: the scene's bounding box.
inline void fill_light_frames(BinFrameDesc *frames, const float *origins, int nlights, int cube_bins, int shells, uint32_t base_bins,
                              const float *lo3, const float *hi3)
{
    memset(frames, 0, sizeof(BinFrameDesc) * 6 * nlights);
    for (int k = 0; k < nlights; k++) {
        const float *lpos = origins + 3 * (k + 1);
        double dn = 0.0, df = 0.0;
        const bool okr = shell_range(lpos, lo3, hi3, &dn, &df);
        for (int face = 0; face < 6; face++) {
            BinFrameDesc &d = frames[k * 6 + face];
            const int ax = face >> 1;
            d.P0[ax] = (face & 1) ? -1.0f : 1.0f;         // negD ~ s*e_k + u*e_(k+1) + v*e_(k+2)
            d.Pu[(ax + 1) % 3] = 1.0f;
            d.Pv[(ax + 2) % 3] = 1.0f;
            d.rw[ax] = d.P0[ax]; d.ru[(ax + 1) % 3] = 1.0f; d.rv[(ax + 2) % 3] = 1.0f;   // g = m*(s e_k + u e_k1 + v e_k2)
            memcpy(d.S, lpos, 12);                            // light position k (jittered sample with soft shadows)
            d.dmax = 2.0f;
            d.ulo = -1.0f; d.vlo = -1.0f; d.du = 2.0f / (float)cube_bins; d.dv = 2.0f / (float)cube_bins;
            d.pad_lo = -3.814697265625e-06f; d.pad_hi = 3.814697265625e-06f;
            d.nbu = cube_bins; d.nbv = cube_bins; d.j0 = 0; d.j1 = cube_bins;
            d.base = base_bins; d.tab = 1 + k;
            // every face of every light carries `shells` keys per bin (the key layout needs one count for all); a light whose
            // range is degenerate puts everything into shell 0
            d.nshell = shells;
            d.shell_d0 = (float)dn;
            d.shell_iw = okr ? (float)(shells / (df - dn)) : 0.0f;
            base_bins += (uint32_t)(cube_bins * cube_bins);
        }
    }
}

// ---- a query: through a cube's bins, or by brute force ----
// The one rule of DirectLight, the single fan and the many-origin call.  may_bin: the call is inside what the frame path would bin
// (the filter's proven range, keys the sort can hold) -- outside it nothing bins, whatever the mode; held: the cube of every pass
// of the call is there already, so that binning costs no build; auto_bins: the call's own AUTO rule (query.cpp).
inline bool query_bins(bool may_bin, int mode, bool held, bool auto_bins)
{
    return may_bin && mode != MIRT_QUERY_BRUTE && (mode == MIRT_QUERY_BINNED || held || auto_bins);
}

// ---- the view of a cube's tables ----
// What a walk kernel -- a query's, or the trace kernel of a binned frame -- reads of a light cube.  A lane with no row left still
// loads row 0 each step and ignores it, and a cube without a single pair has no row table: the loads are pointed at the cube's
// origin table then, which always has a row.
inline CubeView make_cube_view(const uint32_t *off, const LightRow *rows, bool has_rows, const OriginRow *origin_tab, const uint32_t *row_tri,
                               const BinFrameDesc *frames, int cube_bins, int shells)
{
    return CubeView{ off, has_rows ? rows : origin_tab, row_tri, frames, cube_bins, shells };
}

}  // namespace mirt
