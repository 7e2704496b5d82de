// The row arithmetic of a logits row at a temperature, one definition for every kernel that scores a row at beta = 1 / T
// (calibrate.hip: the launches of include/egopack_calibrate.h; action.hip: egk_action_topk with a beta).
#pragma once
#include <math.h>

#include "common.h"

namespace egk {

constexpr int TEMP_SLOTS = 8;
constexpr int TEMP_RES = WAVE * TEMP_SLOTS;  // a row of at most 512 classes stays in registers: class lane + 64 * i in slot i

// fl(beta * z): ONE separately rounded f32 product.  The multiply is written here, under the pragma, so it carries no contract flag
// and nothing it is inlined into can fuse it with the subtraction that follows (scaled_seed of common.h, the same reasoning).
__device__ __forceinline__ float temp_scaled(float beta, float z) {
#pragma clang fp contract(off)
    return beta * z;
}

// The log-sum-exp of the scaled row: the sibling of ce_row_plain's forward (csrc/ce_row.h) with x_c = fl(beta z_c) in the place of
// the logit -- the same lane striding (c = lane, lane + 64, ...), the same wave reductions, the same operations in the same order,
// so at beta == 1 (x_c == z_c exactly) it returns ce_row_plain's bits.  RES: the row is in ``z`` (slot i = class lane + 64 * i),
// which walks the classes of a lane in the order of the strided loop; otherwise it is read from ``lr``.
template <typename X, bool RES>
__device__ __forceinline__ float temp_row_lse(const X* __restrict__ lr, int C, float beta, const float (&z)[TEMP_SLOTS], int lane) {
    float mx = -INFINITY, se = 0.f;
    if (RES) {
#pragma unroll
        for (int i = 0; i < TEMP_SLOTS; ++i)
            if (lane + WAVE * i < C) mx = fmaxf(mx, temp_scaled(beta, z[i]));
        mx = wave_max(mx);
#pragma unroll
        for (int i = 0; i < TEMP_SLOTS; ++i)
            if (lane + WAVE * i < C) se += expf(temp_scaled(beta, z[i]) - mx);
    } else {
        for (int c = lane; c < C; c += 64) mx = fmaxf(mx, temp_scaled(beta, ld1t(lr + c)));
        mx = wave_max(mx);
        for (int c = lane; c < C; c += 64) se += expf(temp_scaled(beta, ld1t(lr + c)) - mx);
    }
    se = wave_sum(se);
    return mx + logf(se);
}

}  // namespace egk
