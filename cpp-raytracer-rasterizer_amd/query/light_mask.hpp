// light_mask.hpp -- the shadow mask of DirectLight (raytracer.cpp:306-315): one bit per (record, light position), set where the
// reference executes `D = vec3(0)` (:314).  What the kernels that write and read a mask (rt_query.hip), the host that sizes it
// (../capi/query.cpp) and tests/cpp/light_mask_test.cpp share: the word count, the place of a word and how the bits of one pass
// (light_passes.hpp) get into their words.
//
// Layout.  Position j = light * samples + sample is bit j & 31 of word j >> 5 of its record; the words are plane-major like the
// carry of light_passes.hpp -- word w of record i at mask[w * nhits + i] -- so that the lanes of a wave read and write neighbouring
// words.  Bits at or beyond the call's position count are 0.
//
// Passes.  A call of more than MIRT_MAX_LIGHTS positions runs in passes over consecutive ranges [first, first + count), count <=
// 32, in order on one stream; a range may start anywhere (fan_pass_plan returns shorter ranges where the sort's key space asks for
// them), so a pass's bits cover a part of one word or the end of one and the start of the next: at most two pieces.  The ranges
// tile [0, npos) in order, so the piece that starts a word (shift 0) is always the first to touch it: it STORES the word, zeros
// above its own bits, and every later piece of the word (shift > 0, of the same lane in a later pass) ORs its bits in.  No word is
// ever read before it was stored, nothing is zeroed beforehand, and the bits beyond npos stay the zeros of the last store.
#pragma once

#include "../csrc/mirt_math.hpp"

#include <stddef.h>

namespace mirt {

constexpr int LIGHT_MASK_BITS = 32;               // positions per word: MIRT_MAX_LIGHTS, a full pass

// Words (planes) of a mask of npos positions: MIRT_MASK_WORDS of include/mirt.h.
MIRT_HD int light_mask_words(int npos) { return (npos + LIGHT_MASK_BITS - 1) / LIGHT_MASK_BITS; }

// Where word w of record i lies in a mask of nhits records; in size_t: 8 planes of 2^29 records are past 2^31 words.
MIRT_HD size_t light_mask_index(int w, size_t nhits, size_t i) { return (size_t)w * nhits + i; }

// A part of a pass inside one word: the pass's local bits [from, from + count) are the word's bits [shift, shift + count).
struct LightMaskPiece { int word, shift, from, count; };
struct LightMaskPieces { int n; LightMaskPiece head, tail; };      // tail: the start of the next word, when n == 2

// The one or two pieces of the pass [first, first + count), 1 <= count <= 32.
MIRT_HD LightMaskPieces light_mask_pieces(int first, int count)
{
    LightMaskPieces r;
    const int shift = first & (LIGHT_MASK_BITS - 1);
    const int head = count < LIGHT_MASK_BITS - shift ? count : LIGHT_MASK_BITS - shift;
    r.head = LightMaskPiece{ first / LIGHT_MASK_BITS, shift, 0, head };
    r.tail = LightMaskPiece{ first / LIGHT_MASK_BITS + 1, 0, head, count - head };
    r.n = count > head ? 2 : 1;
    return r;
}

// The lowest `count` bits set, 0 <= count <= 32.
MIRT_HD uint32_t light_mask_low(int count) { return count >= LIGHT_MASK_BITS ? 0xffffffffu : (1u << count) - 1u; }

// One piece of record i's decisions `bits` (bit k: local position k of the pass) into its word: stored where the piece starts
// the word, ORed in where it continues it.
MIRT_HD void light_mask_store_piece(uint32_t *mask, size_t nhits, size_t i, const LightMaskPiece &p, uint32_t bits)
{
    uint32_t *w = mask + light_mask_index(p.word, nhits, i);
    const uint32_t v = ((bits >> p.from) & light_mask_low(p.count)) << p.shift;
    *w = p.shift ? (*w | v) : v;
}

// Record i's decisions of the pass [first, first + count) into its words (the rule above).
MIRT_HD void light_mask_store(uint32_t *mask, size_t nhits, size_t i, int first, int count, uint32_t bits)
{
    const LightMaskPieces ps = light_mask_pieces(first, count);
    light_mask_store_piece(mask, nhits, i, ps.head, bits);
    if (ps.n == 2) light_mask_store_piece(mask, nhits, i, ps.tail, bits);
}

}  // namespace mirt
