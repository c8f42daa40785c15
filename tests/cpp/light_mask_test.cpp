// The shadow mask's word and bit arithmetic (query/light_mask.hpp) on the CPU, with the pass plans a call really runs
// (capi/cube_plan.hpp: fan_pass_plan):
//   1. for every first, count with 1 <= count <= 32 and first + count <= 256 the pieces of the pass [first, first + count) cover
//      exactly its bits, in order, in at most two words, and never reach across a word's end;
//   2. for every plan fan_pass_plan returns for npos in 1 .. 256, scenes of 30, 2000, 100 000 and 1 000 000 triangles and the grid
//      overrides none, 64, 128 and 256, applying the passes in order with the kernels' own store (light_mask_store) over random
//      decision bits -- into words pre-filled with garbage, for a record in the middle of a list -- reproduces the flat bit array
//      with zeros at and beyond npos, and touches no word of another record or beyond the last plane -- and so does, for each of
//      them, a random tiling of [0, npos) into ranges of 1 .. 32 positions: these plans are all full ranges, whose passes fill whole
//      words, and a plan may be any such tiling;
//   3. plane indices are computed in size_t: 8 planes of 2^29 records lie past 2^31 words.
#include "../../cpp-raytracer-rasterizer_amd/capi/cube_plan.hpp"
#include "../../cpp-raytracer-rasterizer_amd/query/light_mask.hpp"

#include <cstdio>
#include <cstdlib>
#include <type_traits>

using namespace mirt;

#define CHECK(c) do { if (!(c)) { printf("FAILED %s (line %d): first %d, count %d, npos %d, n %d, override %d\n", #c, __LINE__, first, count, npos, n, ov); return 1; } } while (0)

static_assert(MIRT_MAX_LIGHT_POSITIONS == 256 && MIRT_MAX_LIGHTS == LIGHT_MASK_BITS, "a full pass fills one word");
static_assert(std::is_same<decltype(light_mask_index(0, (size_t)0, (size_t)0)), size_t>::value, "plane indices are size_t");

static uint32_t rng_state = 12345u;
static uint32_t rng() { rng_state = rng_state * 1664525u + 1013904223u; return rng_state >> 8; }

int main()
{
    int first = 0, count = 0, npos = 0, n = 0, ov = 0;
    long passes = 0, plans = 0, straddles = 0;

    // 1. the pieces of every pass
    for (first = 0; first < MIRT_MAX_LIGHT_POSITIONS; first++)
        for (count = 1; count <= LIGHT_MASK_BITS && first + count <= MIRT_MAX_LIGHT_POSITIONS; count++) {
            const LightMaskPieces ps = light_mask_pieces(first, count);
            CHECK(ps.n == 1 || ps.n == 2);
            const LightMaskPiece pc[2] = { ps.head, ps.tail };
            int next_local = 0;
            for (int k = 0; k < ps.n; k++) {
                CHECK(pc[k].count >= 1 && pc[k].shift >= 0 && pc[k].shift + pc[k].count <= LIGHT_MASK_BITS);
                CHECK(pc[k].from == next_local);
                // local bit from + b is global position first + from + b: word and bit as the layout says
                for (int b = 0; b < pc[k].count; b++) {
                    const int j = first + pc[k].from + b;
                    CHECK(pc[k].word == j / 32 && pc[k].shift + b == j % 32);
                }
                next_local += pc[k].count;
            }
            CHECK(next_local == count);
            CHECK(ps.n == 1 || (ps.tail.word == ps.head.word + 1 && ps.tail.shift == 0));
            passes++;
        }
    first = count = 0;

    // 2. whole plans over random decisions
    const int scenes[] = { 30, 2000, 100000, 1000000 };
    const int overrides[] = { 0, 64, 128, 256 };
    const size_t nhits = 5, rec = 3;
    for (int oi = 0; oi < 4; oi++)
        for (int si = 0; si < 4; si++)
            for (npos = 1; npos <= MIRT_MAX_LIGHT_POSITIONS; npos++) {
                ov = overrides[oi]; n = scenes[si];
                std::vector<FanPass> planned, tiling;
                CHECK(fan_pass_plan(npos, n, ov, &planned));
                for (int at = 0; at < npos;) {
                    const int c = std::min(npos - at, 1 + (int)(rng() % 32u));
                    tiling.push_back({ at, c, 0 });
                    at += c;
                }
                for (int which = 0; which < 2; which++) {
                const std::vector<FanPass> &plan = which ? tiling : planned;
                bool decision[MIRT_MAX_LIGHT_POSITIONS];
                for (int j = 0; j < npos; j++) decision[j] = (rng() & 1u) != 0;
                const int words = light_mask_words(npos);
                CHECK(words == (npos + 31) / 32 && words >= 1 && words <= 8);
                std::vector<uint32_t> mask((size_t)(words + 1) * nhits);
                for (uint32_t &w : mask) w = 0x5A5A5A5Au ^ rng();
                const std::vector<uint32_t> before = mask;
                for (const FanPass &p : plan) {
                    first = p.first; count = p.count;
                    CHECK(count >= 1 && count <= LIGHT_MASK_BITS);
                    straddles += light_mask_pieces(first, count).n == 2;
                    uint32_t bits = 0u;
                    for (int k = 0; k < p.count; k++) bits |= (uint32_t)decision[p.first + k] << k;
                    // (garbage above the pass's own bits must not leak into the words)
                    if (p.count < 32) bits |= rng() << p.count;
                    light_mask_store(mask.data(), nhits, rec, p.first, p.count, bits);
                }
                first = count = 0;
                for (int w = 0; w <= words; w++)
                    for (size_t i = 0; i < nhits; i++) {
                        const size_t at = light_mask_index(w, nhits, i);
                        if (w == words || i != rec) { CHECK(mask[at] == before[at]); continue; }
                        uint32_t want = 0u;
                        for (int b = 0; b < 32; b++)
                            if (32 * w + b < npos && decision[32 * w + b]) want |= 1u << b;
                        CHECK(mask[at] == want);
                    }
                plans++;
                }
            }
    npos = n = ov = 0;
    CHECK(straddles > 1000);

    // 3. past 2^31 words
    CHECK(light_mask_index(7, (size_t)1 << 29, ((size_t)1 << 29) - 1) == ((size_t)1 << 32) - 1);
    CHECK(light_mask_index(7, (size_t)0x7fffffff, 5) == (size_t)7 * 0x7fffffff + 5);
    CHECK(light_mask_words(0) == 0 && light_mask_words(1) == 1 && light_mask_words(32) == 1 && light_mask_words(33) == 2 && light_mask_words(256) == 8);

    printf("ok: %ld passes, %ld plans checked (%ld of their passes straddle two words)\n", passes, plans, straddles);
    return 0;
}
