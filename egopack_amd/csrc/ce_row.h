// The plain cross-entropy row function, one definition for every kernel that forms a cross entropy of a logits row: the loss
// kernels (loss.hip), the validation report and the top-k export (metrics.hip: egk_class_report, egk_topk_softmax).  Two kernels that call it with the same arguments
// form the same f32 value: the same lane striding, the same wave reductions, the same operations in the same order.
#pragma once
#include <math.h>

#include "common.h"

namespace egk {

// ---- cross entropy: one wave per row ------------------------------------------------------------
// One row of one head, written once for the three kernels.  FWD: the wave reduces the row and returns its loss (lse_io = the
// log-sum-exp it formed); !FWD: lse_io is the saved log-sum-exp.  GRAD: columns [0, pad) of ``dr`` are written -- the gradient
// below C, 0 in [C, pad) and in ignored rows (t < 0 or t >= C), whose loss is 0.
//
// The plain arithmetic:   loss = lse - (1-eps)*x_t - eps/C * sum_c x_c,   dx_c = g * (exp(x_c - lse) - [c==t](1-eps) - eps/C)
// X: the element type of the logits row (float everywhere but in egk_topk_softmax's bf16 launch, which widens every element as it
// is read: ld1t of a float is the plain load, so the f32 instantiations are what they were).
template <typename T, bool FWD, bool GRAD, typename X = float>
__device__ __forceinline__ float ce_row_plain(const X* __restrict__ lr, int C, int pad, long long t, float smoothing, float g,
                                              float& lse_io, T* __restrict__ dr, int lane) {
    const bool live = t >= 0 && t < C;
    float loss = 0.f, l;
    if (FWD) {
        float mx = -INFINITY;
        for (int c = lane; c < C; c += 64) mx = fmaxf(mx, ld1t(lr + c));
        mx = wave_max(mx);
        float se = 0.f, sx = 0.f;
        for (int c = lane; c < C; c += 64) {
            const float v = ld1t(lr + c);
            se += expf(v - mx);
            sx += v;
        }
        se = wave_sum(se);
        sx = wave_sum(sx);
        l = mx + logf(se);
        lse_io = l;
        if (live) loss = l - (1.f - smoothing) * ld1t(lr + t) - (smoothing > 0.f ? smoothing / C * sx : 0.f);
    } else {
        l = lse_io;
    }
    if (GRAD) {
        const float sm = smoothing > 0.f ? smoothing / C : 0.f;
        for (int c = lane; c < pad; c += 64) {
            float d = 0.f;
            if (live && c < C) d = g * (expf(ld1t(lr + c) - l) - (c == t ? 1.f - smoothing : 0.f) - sm);
            st1t(dr + c, d);
        }
    }
    return loss;
}

}  // namespace egk
