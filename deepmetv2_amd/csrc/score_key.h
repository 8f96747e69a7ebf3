// score_key.h -- the canonical score order as one unsigned 64-bit comparison, shared by the ranked selection
// (csrc/select.hip) and the edge matching (csrc/edge_match.hip).
#pragma once
#include "common.h"

namespace dmet {

// "largest canonical score, lowest index" as one unsigned comparison.  High word: the order-preserving map of the fp32
// bits (sign set: all bits flipped, else the sign bit set), after -0.0 became +0.0 and every NaN 0xFFFFFFFF (above +inf,
// whose image is 0xFF800000).  Low word: ~index.  Keys with distinct indices are distinct, and every key is > 0x007FFFFF
// << 32 (the image of -inf), so small words (0: a padding slot or "no offer") are free for other meanings.
__device__ __forceinline__ uint64_t select_key(float v, uint32_t i)
{
    uint32_t u = __float_as_uint(v);
    uint32_t hi;
    if ((u & 0x7FFFFFFFu) > 0x7F800000u) {
        hi = 0xFFFFFFFFu;
    } else {
        if (u == 0x80000000u) u = 0u;
        hi = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
    }
    return ((uint64_t)hi << 32) | (uint64_t)(uint32_t)~i;
}

}  // namespace dmet
