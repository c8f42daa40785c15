// light_passes.hpp -- DirectLight (raytracer.cpp:265-327) cut into passes of at most MIRT_MAX_LIGHTS light positions: what the
// kernels of a pass (rt_query.hip), the host that plans the passes (../capi/query.cpp) and tests/cpp/light_passes_test.cpp share.
//
// DirectLight is one flat loop over the positions j = light * samples + sample with two accumulators: result += D_j for every
// position (never reset between lights: the reference's double count, :319), and result2 += result whenever j closes a light,
// (j + 1) % samples == 0 (:322).  Cut at any j, the pass that starts there continues from the (result, result2) the pass before
// it left: the same additions on the same operands in the same order, so no bit changes wherever the cuts fall -- inside a light
// too.  A pass knows the global index `first` of its position 0; its local position k is global position first + k.
#pragma once

#include "../csrc/mirt_math.hpp"

namespace mirt {

// Whether local position k of a pass that starts at global position `first` is the last sample of its light: result2 += result.
MIRT_HD bool light_pass_closes(int first, int k, int samples) { return (first + k + 1) % samples == 0; }

// QueryLightFrame::pass_flags of a carrying pass.  The first pass starts from zeros instead of loading the carry; the last one
// ends as a call of one pass does (result2 * colour into rgb) instead of storing the carry.
enum { LIGHT_PASS_FIRST = 1, LIGHT_PASS_LAST = 2 };

// The carry of record i between two passes: six planes of nhits floats, result.xyz then result2.xyz, so that the lanes of a wave
// read and write neighbouring words.
constexpr int LIGHT_CARRY_WORDS = 6;

}  // namespace mirt
