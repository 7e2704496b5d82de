// The order of the meters as ONE integer per class, one definition for every kernel that ranks the classes of a logits row
// (metrics.hip: egk_class_report, egk_topk_softmax; action.hip: egk_action_topk).
#pragma once
#include "common.h"

namespace egk {

// The order of label_rank_kernel as ONE integer per class: the f32 value as a monotone 32-bit key (NaN -> 0, below the key of -inf;
// -0 and +0 share a key) above the complemented class index, so that the larger integer is the better class, no two classes of a
// row share one, and 0 means "no class".  top1 / top2 are the largest and the second largest of the row.
__device__ __forceinline__ unsigned long long rank_key(float v, int c) {
    unsigned k;
    if (v != v) {
        k = 0u;
    } else {
        const unsigned b = __float_as_uint(v == 0.f ? 0.f : v);
        k = (b & 0x80000000u) ? ~b : (b | 0x80000000u);
    }
    return ((unsigned long long)k << 32) | (unsigned long long)(0xffffffffu - (unsigned)c);
}

__device__ __forceinline__ unsigned long long wave_max_u64(unsigned long long v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned long long b = __shfl_xor(v, o, 64);
        v = v > b ? v : b;
    }
    return v;
}

}  // namespace egk
