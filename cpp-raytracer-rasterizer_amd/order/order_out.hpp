// order_out.hpp -- what an ordered call adds to the walk it runs on, once: the block every frame of the ordered kernels embeds
// (ordered_hits.hpp, ordered_along.hpp, ordered_fans.hpp), the host passes from entry point to launch (../capi/order*.cpp) and the
// device reads and writes through (order_device.hpp).
#pragma once

#include <stdint.h>

namespace mirt {

struct OrderOut {
    const uint32_t *after;       // nrays records of HIT_WORDS words, or NULL: only distance and index are read
    int max_hits;                // 1 .. K of the instantiation
    int32_t *counts;             // nrays
    uint32_t *hits;              // the OUTPUT: nrays * max_hits records of HIT_WORDS words, ray-major (the frame's own `hits` is not read)
};

}  // namespace mirt
