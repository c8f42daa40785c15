// The arithmetic of the ray queries along several directions in one call (capi/along_plan.hpp) on the CPU: the slots of a group,
// the pass ranges of a call, the sort key's composition and decomposition -- and, with a file of triangles (argv[1]: n x 15
// floats), that a group's lists ARE the single grids' lists: the (slot, cell, shell, triangle) set a group of three directions
// files under its keys equals the union of the three sets along_tri_setup / along_cell_may_hit give for each direction alone.
#include "../../cpp-raytracer-rasterizer_amd/capi/along_plan.hpp"

#include <cstdio>
#include <cstdlib>
#include <set>
#include <tuple>
#include <vector>

using namespace mirt;

static int failures = 0;
#define CHECK(cond, ...) do { if (!(cond)) { failures++; printf("FAIL %s:%d: ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); } } while (0)

static void plan_checks()
{
    // slots per group: 32 up to B = 128, 15 at B = 256
    for (int B = ALONG_BINS_MIN; B <= ALONG_BINS_MAX; B *= 2) {
        const int slots = alongs_slots(B, ALONG_SHELLS);
        CHECK(slots == (B <= 128 ? 32 : 15), "B %d: %d slots", B, slots);
        CHECK(slots <= MIRT_MAX_LIGHTS, "B %d: more slots than the walk kernels stage", B);
        // the largest key of a full group stays within what one sort pass holds
        const uint32_t K = along_keys(B, ALONG_SHELLS), top = alongs_key((uint32_t)slots - 1u, K - 1u, K);
        CHECK(top == alongs_group_keys(slots, B, ALONG_SHELLS) - 1u, "B %d: top key %u", B, top);
        CHECK(top <= BIN_MAX_KEYS - 64u, "B %d: key %u beyond the sort's %u", B, top, BIN_MAX_KEYS - 64u);
        CHECK((unsigned long long)(slots + 1) * K > BIN_MAX_KEYS - 64u || slots == MIRT_MAX_LIGHTS, "B %d: a slot more would fit", B);
        // composition and decomposition round-trip over every slot, at the largest key, the every-ray list's and the first
        const uint32_t every = (uint32_t)(B * B) * ALONG_SHELLS;
        for (uint32_t s = 0; s < (uint32_t)slots; s++)
            for (uint32_t local : { 0u, 1u, every, every + ALONG_SHELLS - 1u, K - 1u }) {
                const uint32_t key = alongs_key(s, local, K);
                CHECK(alongs_key_slot(key, K) == s && alongs_key_local(key, K) == local, "B %d slot %u local %u: key %u", B, s, local, key);
                CHECK(key >= s * K && key < (s + 1u) * K, "B %d slot %u: key %u outside the slot's range", B, s, key);
            }
    }
    CHECK(along_bins_for(32768) == 128 && along_bins_for(32769) == 256, "B = 256 applies from 32 769 triangles on");
    // the pass ranges
    const int counts[7] = { 1, 15, 16, 32, 33, 70, 256 };
    for (int slots : { 32, 15 })
        for (int nd : counts) {
            std::vector<AlongsPass> plan;
            CHECK(alongs_pass_plan(nd, slots, &plan), "%d directions, %d slots: no plan", nd, slots);
            CHECK((int)plan.size() == (nd + slots - 1) / slots, "%d directions, %d slots: %d passes", nd, slots, (int)plan.size());
            int next = 0;
            for (size_t p = 0; p < plan.size(); p++) {
                CHECK(plan[p].first == next && plan[p].count >= 1 && plan[p].count <= slots, "%d directions: pass %d is [%d, +%d)", nd, (int)p, plan[p].first, plan[p].count);
                CHECK(p + 1 == plan.size() || plan[p].count == slots, "%d directions: pass %d is not full", nd, (int)p);
                CHECK(alongs_group_of_pass(p) == (int)(p % 8), "pass %d keeps group %d", (int)p, alongs_group_of_pass(p));
                next += plan[p].count;
            }
            CHECK(next == nd, "%d directions: the passes cover %d", nd, next);
        }
    std::vector<AlongsPass> none;
    CHECK(!alongs_pass_plan(0, 32, &none) && !alongs_pass_plan(4, 0, &none) && none.empty(), "a plan for nothing");
    {
        std::vector<AlongsPass> p70, p33;
        alongs_pass_plan(70, 32, &p70);
        alongs_pass_plan(33, 15, &p33);
        CHECK(p70.size() == 3 && p70[2].first == 64 && p70[2].count == 6, "70 directions in groups of 32");
        CHECK(p33.size() == 3 && p33[2].first == 30 && p33[2].count == 3, "33 directions in groups of 15");
    }
    CHECK(alongs_fold_source(0, true) == 1 && alongs_fold_source(0, false) == 2 && alongs_fold_source(2, false) == 2 && alongs_fold_source(2, true) == 1 &&
          alongs_fold_source(1, false) == 1, "cube_source over the passes");
}

typedef std::tuple<uint32_t, uint32_t, uint32_t, uint32_t> Filed;   // slot, cell, shell, triangle

// What the single-direction grid files for direction `a` (along.hpp), as (slot, cell, shell, triangle).
static void single_set(const AlongDesc &a, uint32_t slot, const std::vector<float> &tris, std::set<Filed> *out, long *every)
{
    const int n = (int)(tris.size() / 15);
    for (int i = 0; i < n; i++) {
        const float *t15 = &tris[(size_t)15 * i];
        const v3 v0 = ld3(t15), e1 = sub3(ld3(t15 + 3), v0), e2 = sub3(ld3(t15 + 6), v0);
        const AlongTri t = along_tri_setup(a, v0, e1, e2, cross3(e1, e2));
        if (t.kind == ALONG_EVERY) { out->insert(Filed(slot, (uint32_t)(a.B * a.B), 0u, (uint32_t)i)); (*every)++; continue; }
        const uint32_t shell = bin_shell_of(t.near, a.shell_d0, a.shell_iw, a.shells);
        for (int cj = t.j0; cj <= t.j1; cj++)
            for (int ci = t.i0; ci <= t.i1; ci++)
                if (along_cell_may_hit(a, t, ci, cj)) out->insert(Filed(slot, (uint32_t)(cj * a.B + ci), shell, (uint32_t)i));
    }
}

static int group_check(const char *path)
{
    FILE *fp = fopen(path, "rb");
    if (!fp) return 2;
    std::vector<float> tris;
    float row[15];
    while (fread(row, sizeof row, 1, fp) == 1) tris.insert(tris.end(), row, row + 15);
    fclose(fp);
    const int n = (int)(tris.size() / 15);
    float lo[3] = { INFINITY, INFINITY, INFINITY }, hi[3] = { -INFINITY, -INFINITY, -INFINITY };
    for (size_t i = 0; i < tris.size(); i++)
        if (i % 15 < 9) { lo[i % 3] = fminf(lo[i % 3], tris[i]); hi[i % 3] = fmaxf(hi[i % 3], tris[i]); }
    // the oblique direction, an axis, a face diagonal
    const float dirs[3][3] = { { 0.37f, -0.52f, 0.81f }, { 0.0f, 0.0f, 1.0f }, { 1.0f, 1.0f, 0.0f } };
    const int B = along_bins_for(n), slots = 3;
    const uint32_t K = along_keys(B, ALONG_SHELLS);
    AlongDesc descs[3];
    std::set<Filed> want;
    long every = 0;
    for (int s = 0; s < slots; s++) {
        if (!along_make_desc(dirs[s], lo, hi, B, ALONG_SHELLS, &descs[s])) { printf("FAIL: no descriptor for direction %d\n", s); return 1; }
        single_set(descs[s], (uint32_t)s, tris, &want, &every);
    }
    // the group: one pair list of (key, slot * n + triangle) as k_alongs_pairs files it, one lane per (triangle, slot) ...
    std::vector<std::pair<uint32_t, uint32_t>> pairs;
    for (int s = 0; s < slots; s++)
        for (int i = 0; i < n; i++) {
            const float *t15 = &tris[(size_t)15 * i];
            const v3 v0 = ld3(t15), e1 = sub3(ld3(t15 + 3), v0), e2 = sub3(ld3(t15 + 6), v0);
            const AlongDesc &d = descs[s];
            const AlongTri t = along_tri_setup(d, v0, e1, e2, cross3(e1, e2));
            const uint32_t val = (uint32_t)s * (uint32_t)n + (uint32_t)i;
            if (t.kind == ALONG_EVERY) { pairs.push_back({ alongs_key((uint32_t)s, (uint32_t)(d.B * d.B) * (uint32_t)d.shells, K), val }); continue; }
            const uint32_t shell = bin_shell_of(t.near, d.shell_d0, d.shell_iw, d.shells);
            for (int cj = t.j0; cj <= t.j1; cj++)
                for (int ci = t.i0; ci <= t.i1; ci++)
                    if (along_cell_may_hit(d, t, ci, cj)) pairs.push_back({ alongs_key((uint32_t)s, (uint32_t)(cj * d.B + ci) * (uint32_t)d.shells + shell, K), val });
        }
    // ... and read back through the key's decomposition
    std::set<Filed> got;
    for (const auto &p : pairs) {
        const uint32_t slot = alongs_key_slot(p.first, K), local = alongs_key_local(p.first, K);
        CHECK(p.first < alongs_group_keys(slots, B, ALONG_SHELLS), "key %u beyond the group's", p.first);
        CHECK(p.second / (uint32_t)n == slot, "pair value %u names slot %u, its key slot %u", p.second, p.second / (uint32_t)n, slot);
        got.insert(Filed(slot, local / ALONG_SHELLS, local % ALONG_SHELLS, p.second % (uint32_t)n));
    }
    CHECK(got.size() == pairs.size(), "%zu pairs, %zu distinct", pairs.size(), got.size());
    CHECK(got == want, "the group files %zu entries, the three single grids %zu", got.size(), want.size());
    size_t per_slot[3] = { 0, 0, 0 };
    for (const Filed &f : got) per_slot[std::get<0>(f)]++;
    printf("n %d B %d pairs %zu (%zu %zu %zu) every %ld\n", n, B, got.size(), per_slot[0], per_slot[1], per_slot[2], every);
    CHECK(per_slot[0] >= (size_t)n && per_slot[1] >= (size_t)n && per_slot[2] >= (size_t)n, "a slot files fewer pairs than triangles");
    return 0;
}

int main(int argc, char **argv)
{
    plan_checks();
    if (argc >= 2) {
        const int rc = group_check(argv[1]);
        if (rc) return rc;
    }
    if (failures) { printf("%d failures\n", failures); return 1; }
    printf("ok\n");
    return 0;
}
