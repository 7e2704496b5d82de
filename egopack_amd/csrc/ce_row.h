// The plain cross-entropy arithmetic, one definition for every kernel that forms a cross entropy of a logits row: the loss kernels
// (loss.hip: the plain launches and the two-target one), the validation report and the top-k export (metrics.hip: egk_class_report,
// egk_topk_softmax).  Two kernels that call it with the same arguments form the same f32 value: the same lane striding, the same
// wave reductions, the same operations in the same order.
#pragma once
#include <math.h>

#include "common.h"

namespace egk {

// ---- cross entropy: one wave per row ------------------------------------------------------------
// The two pieces of the plain forward pass (default contraction: no pragma).  Every lane returns the row's log-sum-exp and holds
// sum_c x_c in ``sx``.
template <typename X>
__device__ __forceinline__ float ce_row_lse(const X* __restrict__ lr, int C, int lane, float& sx) {
    float mx = -INFINITY;
    for (int c = lane; c < C; c += 64) mx = fmaxf(mx, ld1t(lr + c));
    mx = wave_max(mx);
    float se = 0.f;
    sx = 0.f;
    for (int c = lane; c < C; c += 64) {
        const float v = ld1t(lr + c);
        se += expf(v - mx);
        sx += v;
    }
    se = wave_sum(se);
    sx = wave_sum(sx);
    return mx + logf(se);
}
// the loss of one LIVE label t given those two
template <typename X>
__device__ __forceinline__ float ce_label_loss(const X* __restrict__ lr, float l, float sx, long long t, float smoothing, int C) {
    return l - (1.f - smoothing) * ld1t(lr + t) - (smoothing > 0.f ? smoothing / C * sx : 0.f);
}

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
        float sx;
        l = ce_row_lse(lr, C, lane, sx);
        lse_io = l;
        if (live) loss = ce_label_loss(lr, l, sx, t, smoothing, C);
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

// ---- two labels per row (include/egopack_mixup.h) -------------------------------------------------
// What the two labels add to the plain row: every operation rounded separately (the header's order).  With la == 1, lb == 0 every
// extra factor is an exact 1 and every extra term an exact 0.
template <typename T>
__device__ __forceinline__ float ce_mix_tail(const float* __restrict__ lr, int C, int pad, long long a, long long b, bool alive,
                                             bool blive, float lam, float ca, float cb, float l, float smoothing, float g,
                                             T* __restrict__ dr, int lane) {
#pragma clang fp contract(off)  // (the f32 and the bf16 instantiation form the same f32 value: no fusing that depends on the code around)
    const float la = alive ? lam : 0.f, lb = blive ? 1.f - lam : 0.f, W = la + lb;
    float loss = la > 0.f ? la * ca : 0.f;
    if (lb > 0.f) loss = loss + lb * cb;
    const float sm = smoothing > 0.f ? smoothing / C : 0.f;
    const float hs = 1.f - smoothing, Wsm = W * sm;
    for (int c = lane; c < pad; c += 64) {
        float d = 0.f;
        if (W > 0.f && c < C) {
            const float p = expf(ld1t(lr + c) - l);
            const float oh = (c == a ? la : 0.f) + (c == b ? lb : 0.f);
            d = g * (W * p - hs * oh - Wsm);
        }
        st1t(dr + c, d);
    }
    return loss;
}

// One row of one head against labels a and b: the plain row's log-sum-exp and logit sum ONCE, the plain loss of each live label
// (the very functions ce_row_plain is built from: a row with lam == 1 has the plain launch's bits), then the tail.
template <typename T>
__device__ __forceinline__ float ce_row_mix(const float* __restrict__ lr, int C, int pad, long long a, long long b, float lam,
                                            float smoothing, float g, T* __restrict__ dr, int lane) {
    float sx;
    const float l = ce_row_lse(lr, C, lane, sx);
    const bool alive = a >= 0 && a < C, blive = b >= 0 && b < C;
    float ca = 0.f, cb = 0.f;
    if (alive) ca = ce_label_loss(lr, l, sx, a, smoothing, C);
    if (blive) cb = ce_label_loss(lr, l, sx, b, smoothing, C);
    return ce_mix_tail<T>(lr, C, pad, a, b, alive, blive, lam, ca, cb, l, smoothing, g, dr, lane);
}

}  // namespace egk
