// Loss kernels: cross entropy with ignore_index / label smoothing, plain, class-balanced (include/egopack_ce_balanced.h), shaped
// (the tail of egk_ce_task) and against two labels per row (egk_ce_mix_fused_multi, include/egopack_mixup.h), BCE-with-logits,
// plain and shaped (include/egopack_bce_balanced.h), and the sigmoid losses against one-hot targets.  One definition of every
// piece: a template flag picks the balanced / shaped arithmetic, a mode the fused kernel's row function; the row walk, the grids,
// the task argument and the host-side packing are shared.  All HBM-bound / latency-bound.
#include <math.h>

#include "bce_shaped.h"
#include "ce_row.h"
#include "common.h"

namespace egk {

constexpr int WPB = 4;
static inline int row_grid(int rows) {
    int g = cdiv(rows, WPB);
    return g < 1 ? 1 : (g > 2048 ? 2048 : g);
}

// ---- cross entropy: one wave per row ------------------------------------------------------------
// (the plain row function, ce_row_plain, is in ce_row.h: the validation report of metrics.hip forms its loss with it too)

// The weighted arithmetic, balanced and shaped (w: per-class weights, a: per-class logit offsets, m: per-class margins, any may be
// null; gamma: focal exponent >= 0; egk_ce_task in egopack_hip.h):
//   z_c = x_c + a_c - [c == t] m_t,  S = the balanced loss on z,  q = softmax(z)_t,  loss = (1 - q)^gamma S,
//   dS_j = (1-eps) w_t (p_j - [j==t]) + eps/C (W p_j - w_j),  dz_j = g [(1 - q)^gamma dS_j + S gamma q (1 - q)^(gamma - 1) (p_j - [j == t])].
// FWD reduces max, sum exp, W = sum w and sum w (z - max) in one pass after the maximum; !FWD reduces only W (when smoothing needs
// it), lane by lane in the forward pass's order.  The smoothing term is formed around the row maximum, W (lse - max) -
// sum w (z - max): the same value as W lse - sum w z without the cancellation of two large sums.  It rounds differently from the
// plain arithmetic by design: neither is expressed through the other.
// SHAPED = false forms neither the margin select nor the focal factors (m, gamma, grad are not read): the balanced row.  SHAPED is
// always the forward pass; with m null and gamma 0 every extra operation is absent or exact and the row has the balanced row's
// bits.  1 - q = -expm1f(-(lse - z_t)), no cancellation; at q = 1 both factors are 0 by definition (0 * inf otherwise).
// ``grad`` = false writes no gradient (the forward-only form of the shaped launch).
template <typename T, bool FWD, bool GRAD, bool SHAPED>
__device__ __forceinline__ float ce_row_weighted(const float* __restrict__ lr, const float* __restrict__ w, const float* __restrict__ a,
                                                 const float* __restrict__ m, int C, int pad, long long t, float smoothing, float gamma,
                                                 float g, bool grad, float& lse_io, T* __restrict__ dr, int lane) {
#pragma clang fp contract(off)  // (the f32 and the bf16 instantiation form the same f32 value: no fusing that depends on the code around)
    static_assert(FWD || !SHAPED, "the shaped row is always the forward pass");
    const bool live = t >= 0 && t < C;
    const int tc = live ? (int)t : -1;
    const float sm = smoothing > 0.f ? smoothing / C : 0.f;
    float mt = 0.f;
    if constexpr (SHAPED) mt = live && m ? m[tc] : 0.f;
    auto z = [&](int c) {
        const float v = lr[c] + (a ? a[c] : 0.f);
        if constexpr (SHAPED) return c == tc ? v - mt : v;
        else return v;
    };
    float W = 0.f, loss = 0.f, fS = 1.f, cf = 0.f, l;
    if (FWD) {
        float mx = -INFINITY;
        for (int c = lane; c < C; c += 64) mx = fmaxf(mx, z(c));
        mx = wave_max(mx);
        float se = 0.f, swx = 0.f;
        for (int c = lane; c < C; c += 64) {
            const float v = z(c) - mx;
            const float wc = w ? w[c] : 1.f;
            se += expf(v);
            W += wc;
            swx += wc * v;
        }
        se = wave_sum(se);
        W = wave_sum(W);
        swx = wave_sum(swx);
        const float lg = logf(se);
        l = mx + lg;
        lse_io = l;
        if (live) {
            const float wt = w ? w[tc] : 1.f;
            const float zt = z(tc);
            const float S = (1.f - smoothing) * wt * (l - zt) + (smoothing > 0.f ? sm * (W * lg - swx) : 0.f);
            loss = S;
            if constexpr (SHAPED)
                if (gamma > 0.f) {
                    const float d = fmaxf(l - zt, 0.f);  // -log q (a rounding below 0 would hand powf a negative base)
                    const float q = expf(-d), u = -expm1f(-d);
                    fS = u > 0.f ? powf(u, gamma) : 0.f;
                    cf = u > 0.f ? S * gamma * q * powf(u, gamma - 1.f) : 0.f;
                    loss = fS * S;
                }
        }
    } else {
        l = lse_io;
        if (sm > 0.f) {
            for (int c = lane; c < C; c += 64) W += w ? w[c] : 1.f;
            W = wave_sum(W);
        }
    }
    if (GRAD && (!SHAPED || grad)) {
        const float hard = live ? (1.f - smoothing) * (w ? w[tc] : 1.f) : 0.f;
        for (int c = lane; c < pad; c += 64) {
            float d = 0.f;
            if (live && c < C) {
                const float p = expf(z(c) - l);
                const float e = p - (c == tc ? 1.f : 0.f);
                d = hard * e;
                if (sm > 0.f) d += sm * (W * p - (w ? w[c] : 1.f));
                if constexpr (SHAPED)
                    if (gamma > 0.f) d = fS * d + cf * e;
                d *= g;
            }
            st1t(dr + c, d);
        }
    }
    return loss;
}

// BAL = false never reads ``w`` / ``a``
template <typename T, bool BAL, bool FWD, bool GRAD>
__device__ __forceinline__ float ce_row(const float* __restrict__ lr, const float* __restrict__ w, const float* __restrict__ a, int C,
                                        int pad, long long t, float smoothing, float g, float& lse_io, T* __restrict__ dr, int lane) {
    if constexpr (BAL) return ce_row_weighted<T, FWD, GRAD, false>(lr, w, a, nullptr, C, pad, t, smoothing, 0.f, g, true, lse_io, dr, lane);
    else return ce_row_plain<T, FWD, GRAD>(lr, C, pad, t, smoothing, g, lse_io, dr, lane);
}

// loss[n] (+)= CE(logits[n, :], y[n * ys]); lse[n] saved for the backward launch
template <bool BAL>
__global__ __launch_bounds__(256) void ce_fwd_kernel(const float* __restrict__ logits, long long ld, const long long* __restrict__ y,
                                                     long long ys, const float* __restrict__ w, const float* __restrict__ a,
                                                     float* __restrict__ loss, float* __restrict__ lse, int rows, int C,
                                                     float smoothing, int accumulate) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const RowWalk rw = row_walk(blockIdx.x, gridDim.x, 0, rows, wave, WPB);  // (XCD x owns a contiguous eighth of the rows: common.h)
    for (int row = rw.first; row < rw.end; row += rw.step) {
        float l;
        const float o = ce_row<float, BAL, true, false>(logits + (long long)row * ld, w, a, C, 0, y[(long long)row * ys], smoothing,
                                                        0.f, l, nullptr, lane);
        if (lane == 0) {
            lse[row] = l;
            loss[row] = accumulate ? loss[row] + o : o;
        }
    }
}

template <typename T, bool BAL>
__global__ __launch_bounds__(256) void ce_bwd_kernel(const float* __restrict__ logits, long long ld, const long long* __restrict__ y,
                                                     long long ys, const float* __restrict__ w, const float* __restrict__ a,
                                                     const float* __restrict__ lse, const float* __restrict__ gloss,
                                                     T* __restrict__ dlogits, long long ldd, int rows, int C, float smoothing) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const RowWalk rw = row_walk(blockIdx.x, gridDim.x, 0, rows, wave, WPB);  // (XCD x owns a contiguous eighth of the rows: common.h)
    for (int row = rw.first; row < rw.end; row += rw.step) {
        float l = lse[row];
        ce_row<T, BAL, false, true>(logits + (long long)row * ld, w, a, C, C, y[(long long)row * ys], smoothing, gloss[row], l,
                                    dlogits + (long long)row * ldd, lane);
    }
}

// ---- fused multi-head, multi-task cross entropy: loss AND its gradient in one launch -----------------------------------------
// The training heads of the engine know the gradient of the objective with respect to every loss-vector element when the
// loss is computed: objective = sum_t w_t * mean(loss_t)  =>  d objective / d loss_t[n] = w_t / N_t, a constant.  One wave
// per row then does, for every head h of the task (verb, noun): loss[n] += CE_h(n) and
//   dlogits_h[n, c] = gscale * (softmax_h(n)[c] - target_h(n)[c])      (0 for ignored rows)
// written straight into the classifier bank's operand buffer, zero-filling the bank's pad columns [C_h, pad_h) on the way
// (the buffer needs no memset).  Replaces 2 forward + 2 backward launches per two-head task; blockIdx.y = task (the AR and LTA
// heads of a multi-task step in ONE launch).
constexpr int CE_MAX_HEADS = 4;
constexpr int CE_MAX_TASKS = 4;
static_assert(CE_MAX_HEADS == EGK_CE_MIX_MAX_HEADS && CE_MAX_TASKS == EGK_CE_MIX_MAX_TASKS, "the two-target entry point packs into CETasks");
struct CEHeads {
    const float* logits[CE_MAX_HEADS];
    const float* w[CE_MAX_HEADS];  // null in the plain instantiation, never read there
    const float* a[CE_MAX_HEADS];
    long long ld[CE_MAX_HEADS];
    long long dcol[CE_MAX_HEADS];  // first column of the head's block in the gradient buffer
    int C[CE_MAX_HEADS];
    int pad[CE_MAX_HEADS];         // columns [C, pad) of the gradient block are set to zero
};
struct CETasks {
    CEHeads H[CE_MAX_TASKS];
    const long long* y[CE_MAX_TASKS];
    float* loss[CE_MAX_TASKS];
    void* dlogits[CE_MAX_TASKS];
    long long ys[CE_MAX_TASKS];
    long long ldd[CE_MAX_TASKS];
    int n_heads[CE_MAX_TASKS];
    int rows[CE_MAX_TASKS];
    float gscale[CE_MAX_TASKS];
    const float* scale[CE_MAX_TASKS];  // the task factor of gscale in device memory (egk_ce_fused_multi_s / egk_ce_w_fused_multi_s), or null
};
// One kernel, four modes: which row function a launch runs, and with it what the launch reads.
enum CEMode {
    CE_PLAIN,     // ce_row_plain: neither the vectors nor the side data
    CE_BALANCED,  // ce_row_weighted: the vectors (null or not)
    CE_SHAPED,    // ce_row_weighted<SHAPED>: the vectors and the tail of egk_ce_task
    CE_MIX        // ce_row_mix: the second labels and the coefficients of include/egopack_mixup.h
};
// The mode's side data, one argument next to CETasks: CE_SHAPED reads ``shape``, CE_MIX reads ``mix``, the other two nothing.
struct CEShape {
    const float* m[CE_MAX_TASKS][CE_MAX_HEADS];
    const float* gloss[CE_MAX_TASKS];  // null: every row's seed is the task's gscale
    float gamma[CE_MAX_TASKS];
    int loss_only[CE_MAX_TASKS];       // 1: no gradient is written (dlogits may be null)
};
struct CEMix {
    const long long* yb[CE_MAX_TASKS];  // laid out as y: the label of head h of row n at [n * ys + h]
    const float* lam[CE_MAX_TASKS];
};
union CESide {
    CEShape shape;
    CEMix mix;
};
template <typename T, CEMode M>
__global__ __launch_bounds__(256) void ce_fused_multi_kernel(const CETasks P, const CESide S, float smoothing) {
    const int k = blockIdx.y;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const CEHeads& H = P.H[k];
    const int n_heads = P.n_heads[k], rows = P.rows[k];
    const long long* __restrict__ y = P.y[k];
    const long long ys = P.ys[k], ldd = P.ldd[k];
    float* __restrict__ loss = P.loss[k];
    T* __restrict__ dlogits = (T*)P.dlogits[k];
    const float gscale = scaled_seed(P.gscale[k], P.scale[k]);  // (common.h: one rounded product, the seed itself without a scale)
    const RowWalk rw = row_walk(blockIdx.x, gridDim.x, 0, rows, wave, WPB);  // (XCD x owns a contiguous eighth of the rows: common.h)
    for (int row = rw.first; row < rw.end; row += rw.step) {
        float total = 0.f, g = gscale, lam = 1.f;
        if constexpr (M == CE_SHAPED) {
            const float* __restrict__ gl = S.shape.gloss[k];
            if (gl) g = scaled_seed(gscale, gl + row);
        }
        if constexpr (M == CE_MIX) lam = S.mix.lam[k][row];
        for (int h = 0; h < n_heads; ++h) {
            const float* __restrict__ lr = H.logits[h] + (long long)row * H.ld[h];
            T* __restrict__ dr = dlogits + (long long)row * ldd + H.dcol[h];
            const long long t = y[(long long)row * ys + h];
            float l;
            if constexpr (M == CE_PLAIN)
                total += ce_row_plain<T, true, true>(lr, H.C[h], H.pad[h], t, smoothing, g, l, dr, lane);
            else if constexpr (M == CE_BALANCED)
                total += ce_row_weighted<T, true, true, false>(lr, H.w[h], H.a[h], nullptr, H.C[h], H.pad[h], t, smoothing, 0.f, g, true, l, dr, lane);
            else if constexpr (M == CE_SHAPED)
                total += ce_row_weighted<T, true, true, true>(lr, H.w[h], H.a[h], S.shape.m[k][h], H.C[h], H.pad[h], t, smoothing,
                                                              S.shape.gamma[k], g, !S.shape.loss_only[k], l, dr, lane);
            else
                total += ce_row_mix<T>(lr, H.C[h], H.pad[h], t, S.mix.yb[k][(long long)row * ys + h], lam, smoothing, g, dr, lane);
        }
        if (lane == 0) loss[row] = total;
    }
}

// ---- BCE with logits: one thread per node ----------------------------------------------------------------
// SHAPED: a class factor and a focal exponent applied inside (bce_shaped.h; rowdot_bce_kernel<SHAPED> in norm_ops.hip is the
// one-pass form); ``sh`` is not read otherwise.
template <bool SHAPED>
__global__ __launch_bounds__(256) void bce_fwd_kernel(const float* __restrict__ x, const long long* __restrict__ y,
                                                      float* __restrict__ loss, int n, const BceShape sh) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    if constexpr (SHAPED) {
        loss[i] = bce_shaped_loss(x[i], y[i], sh);
    } else {
        const float v = x[i], t = (float)y[i];
        // torch: (1 - t) * x + max(-x, 0) + log1p(exp(-|x|))
        loss[i] = (1.f - t) * v + fmaxf(-v, 0.f) + log1pf(expf(-fabsf(v)));
    }
}
template <typename T, bool SHAPED>
__global__ __launch_bounds__(256) void bce_bwd_kernel(const float* __restrict__ x, const long long* __restrict__ y,
                                                      const float* __restrict__ gloss, T* __restrict__ dx, int n, const BceShape sh) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    if constexpr (SHAPED) {
        st1t(dx + i, bce_shaped_grad(x[i], y[i], gloss[i], sh));
    } else {
        const float v = x[i];
        st1t(dx + i, (1.f / (1.f + expf(-v)) - (float)y[i]) * gloss[i]);
    }
}

// ---- sigmoid losses against one-hot class targets (OSCCTask.compute_loss 'bce' / 'focal', reference oscc.py:91-96) ---
// element i = (row, c) of [rows, C] logits; target t = (y[row] == c).  kind 0: BCE-with-logits; kind 1: torchvision
// sigmoid_focal_loss(alpha, gamma):  p_t = sigmoid(z), z = (2t-1) x;  L = a_t (1-p_t)^gamma (-log p_t),
// a_t = alpha t + (1-alpha)(1-t) (alpha < 0: no weighting);  dL/dx = (2t-1) a_t (1-p_t)^gamma (gamma p_t log p_t - (1-p_t)).
__device__ __forceinline__ float log_sigmoid(float z) { return -(fmaxf(-z, 0.f) + log1pf(expf(-fabsf(z)))); }

__global__ __launch_bounds__(256) void onehot_sigmoid_fwd_kernel(const float* __restrict__ x, const long long* __restrict__ y,
                                                                 float* __restrict__ loss, int n, int C, int kind, float alpha,
                                                                 float gamma) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float v = x[i];
    const float t = y[i / C] == (long long)(i % C) ? 1.f : 0.f;
    const float ce = (1.f - t) * v + fmaxf(-v, 0.f) + log1pf(expf(-fabsf(v)));
    if (kind == 0) {
        loss[i] = ce;
        return;
    }
    const float p = 1.f / (1.f + expf(-v));
    const float pt = p * t + (1.f - p) * (1.f - t);
    float l = ce * (gamma == 2.f ? (1.f - pt) * (1.f - pt) : powf(1.f - pt, gamma));
    if (alpha >= 0.f) l *= alpha * t + (1.f - alpha) * (1.f - t);
    loss[i] = l;
}
template <typename T>
__global__ __launch_bounds__(256) void onehot_sigmoid_bwd_kernel(const float* __restrict__ x, const long long* __restrict__ y,
                                                                 const float* __restrict__ gloss, T* __restrict__ dx, int n,
                                                                 int C, int kind, float alpha, float gamma) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float v = x[i];
    const float t = y[i / C] == (long long)(i % C) ? 1.f : 0.f;
    float d;
    if (kind == 0) {
        d = 1.f / (1.f + expf(-v)) - t;
    } else {
        const float sg = 2.f * t - 1.f, z = sg * v;
        const float pt = 1.f / (1.f + expf(-z)), q = 1.f - pt;
        const float mod = gamma == 2.f ? q * q : powf(q, gamma);
        const float a = alpha >= 0.f ? alpha * t + (1.f - alpha) * (1.f - t) : 1.f;
        d = sg * a * mod * (gamma * pt * log_sigmoid(z) - q);
    }
    st1t(dx + i, d * gloss[i]);
}

// ---- host side: one launcher per kernel, named by the entry point it serves ------------------------------------------------
#define CE_VEC_ALIGNED "misaligned vector pointer -- weight and offset are read one float at a time and must be 4-byte aligned"
// what egk_ce_fwd / _bwd and their _w forms refuse beside null pointers; 0 or EGK_EINVAL
static int ce_check_rows(const char* who, const float* w, const float* a, int32_t rows, int32_t C, int32_t dtype) {
    EGK_REQUIRE(C >= 1, "%s: C must be >= 1", who);
    EGK_REQUIRE(rows >= 0, "%s: rows must be >= 0", who);
    EGK_REQUIRE(aligned_to(4, {w, a}), "%s: " CE_VEC_ALIGNED, who);
    EGK_REQUIRE(dtype == EGK_F32 || dtype == EGK_BF16, "%s: unknown activation dtype %d", who, (int)dtype);
    return 0;
}

template <bool BAL>
static int ce_fwd_launch(const char* who, int kid, egk_stream_t stream, const float* logits, int64_t ld, const int64_t* y,
                         int64_t y_stride, const float* w, const float* a, float* loss, float* lse, int32_t rows, int32_t C,
                         float smoothing, int32_t accumulate) {
    EGK_REQUIRE(logits && y && loss && lse, "%s: null pointer", who);
    if (int e = ce_check_rows(who, w, a, rows, C, EGK_F32)) return e;
    if (rows == 0) return 0;
    hipStream_t s = (hipStream_t)stream;
    ProfScope prof(kid, s, 0, 4.0 * rows * C);
    hipLaunchKernelGGL(ce_fwd_kernel<BAL>, dim3(row_grid(rows)), dim3(256), 0, s, logits, (long long)ld, (const long long*)y,
                       (long long)y_stride, w, a, loss, lse, rows, C, smoothing, accumulate);
    return check_launch(who);
}

template <bool BAL>
static int ce_bwd_launch(const char* who, int kid, egk_stream_t stream, const float* logits, int64_t ld, const int64_t* y,
                         int64_t y_stride, const float* w, const float* a, const float* lse, const float* gloss, void* dlogits,
                         int64_t ldd, int32_t rows, int32_t C, float smoothing, int32_t dtype) {
    EGK_REQUIRE(logits && y && lse && gloss && dlogits, "%s: null pointer", who);
    if (int e = ce_check_rows(who, w, a, rows, C, dtype)) return e;
    if (rows == 0) return 0;
    hipStream_t s = (hipStream_t)stream;
    ProfScope prof(kid, s, 0, 8.0 * rows * C);
    EGK_DISPATCH_T(dtype, hipLaunchKernelGGL((ce_bwd_kernel<T, BAL>), dim3(row_grid(rows)), dim3(256), 0, s, logits, (long long)ld,
                                             (const long long*)y, (long long)y_stride, w, a, lse, gloss, (T*)dlogits, (long long)ldd,
                                             rows, C, smoothing));
    return check_launch(who);
}

// The one packer of the fused cross entropies: validates and packs the tasks of egk_ce_fused, egk_ce_fused_multi,
// egk_ce_w_fused_multi, their two _s forms and egk_ce_mix_fused_multi, and launches them on the grid (row_grid(longest task), count).
// ``mode``: CE_PLAIN (``tasks``), CE_BALANCED (``wtasks``: the tasks with their vectors) or CE_MIX (``tasks`` with ``y_b`` / ``lam``,
// one device pointer per task, checked by the caller).  The tail of egk_ce_task (margin, gloss, focal_gamma, loss_only) turns the
// first two into CE_SHAPED (it takes the vectors, null or not) when any task sets any of it; all zero: the mode and the bits of the
// launch without the tail.  ``scales``: null, or one device float per task that multiplies the task's gscale inside the kernel;
// ``need_scales`` (the _s entry points of include/egopack_task_scale.h): the array and every entry of it must be there.  The slots
// behind ``count`` repeat the last task with no rows: no wild pointers in the argument.
static int ce_fused_launch(const char* who, int kid, egk_stream_t stream, CEMode mode, const egk_ce_task* tasks,
                           const egk_ce_w_task* wtasks, int32_t count, float smoothing, int32_t dtype,
                           const float* const* scales = nullptr, bool need_scales = false, const int64_t* const* y_b = nullptr,
                           const float* const* lam = nullptr) {
    const bool bal = mode == CE_BALANCED;
    EGK_REQUIRE(bal ? (const void*)wtasks : (const void*)tasks, "%s: null pointer", who);
    EGK_REQUIRE(!need_scales || scales, "%s: null pointer (scales)", who);
    EGK_REQUIRE(count >= 1 && count <= CE_MAX_TASKS, "%s: 1 .. %d tasks", who, CE_MAX_TASKS);
    EGK_REQUIRE(dtype == EGK_F32 || dtype == EGK_BF16, "%s: unknown activation dtype %d", who, (int)dtype);
    CETasks P;
    CESide S;
    bool shaped = false;  // some task sets a field of the struct's tail: all zero is the launch without the tail
    double bytes = 0;
    int max_rows = 0;
    for (int i = 0; i < CE_MAX_TASKS; ++i) {
        const int j = i < count ? i : count - 1;
        const egk_ce_task& t = bal ? wtasks[j].base : tasks[j];
        EGK_REQUIRE(t.n_heads >= 1 && t.n_heads <= CE_MAX_HEADS, "%s: 1 .. %d heads (task %d)", who, CE_MAX_HEADS, i);
        EGK_REQUIRE(t.loss_only == 0 || t.loss_only == 1, "%s: loss_only must be 0 or 1, got %d (task %d)", who, (int)t.loss_only, i);
        EGK_REQUIRE(t.y && t.loss && (t.dlogits || t.loss_only), "%s: null pointer in task %d", who, i);
        EGK_REQUIRE(t.rows >= 0, "%s: rows must be >= 0 (task %d)", who, i);
        EGK_REQUIRE(isfinite(t.focal_gamma) && t.focal_gamma >= 0.f, "%s: focal_gamma must be finite and >= 0, got %g (task %d)", who,
                    (double)t.focal_gamma, i);
        EGK_REQUIRE(!(t.loss_only && t.gloss), "%s: loss_only and gloss are both set (task %d) -- a forward-only pass takes no row seeds",
                    who, i);
        EGK_REQUIRE(t.reserved == 0, "%s: the reserved field of task %d is not 0", who, i);
        EGK_REQUIRE(aligned_to(4, {t.gloss}), "%s: the row seeds (gloss) of task %d are not 4-byte aligned", who, i);
        for (int h = 0; h < CE_MAX_HEADS; ++h) {
            EGK_REQUIRE(h < t.n_heads || !t.margin[h], "%s: margin[%d] is set but task %d has %d heads", who, h, i, (int)t.n_heads);
            EGK_REQUIRE(aligned_to(4, {t.margin[h]}), "%s: misaligned margin pointer -- margins are read one float at a time and must be "
                        "4-byte aligned (head %d of task %d)", who, h, i);
            shaped = shaped || t.margin[h];
        }
        shaped = shaped || t.gloss || t.loss_only || t.focal_gamma > 0.f;
        if (mode == CE_MIX) {
            S.mix.yb[i] = (const long long*)y_b[j]; S.mix.lam[i] = lam[j];
        } else {
            for (int h = 0; h < CE_MAX_HEADS; ++h) S.shape.m[i][h] = t.margin[h];
            S.shape.gloss[i] = t.gloss; S.shape.gamma[i] = t.focal_gamma; S.shape.loss_only[i] = t.loss_only;
        }
        CEHeads& H = P.H[i];
        for (int h = 0; h < CE_MAX_HEADS; ++h) {
            const int k = h < t.n_heads ? h : t.n_heads - 1;
            EGK_REQUIRE(t.logits[k], "%s: null pointer (logits of head %d of task %d)", who, k, i);
            EGK_REQUIRE(t.C[k] >= 1, "%s: C must be >= 1 (head %d of task %d)", who, k, i);
            EGK_REQUIRE(t.pad[k] >= t.C[k], "%s: pad must be >= C (head %d of task %d)", who, k, i);
            H.w[h] = bal ? wtasks[j].weight[k] : nullptr;
            H.a[h] = bal ? wtasks[j].offset[k] : nullptr;
            EGK_REQUIRE(aligned_to(4, {H.w[h], H.a[h]}), "%s: " CE_VEC_ALIGNED " (head %d of task %d)", who, k, i);
            H.logits[h] = t.logits[k]; H.ld[h] = t.ld[k]; H.dcol[h] = t.dcol[k]; H.C[h] = t.C[k]; H.pad[h] = t.pad[k];
            if (i < count && h < t.n_heads) bytes += 6.0 * t.rows * t.C[k];
        }
        P.n_heads[i] = t.n_heads; P.y[i] = (const long long*)t.y; P.ys[i] = t.y_stride; P.loss[i] = t.loss;
        P.dlogits[i] = t.dlogits; P.ldd[i] = t.ldd; P.rows[i] = i < count ? t.rows : 0; P.gscale[i] = t.gscale;
        P.scale[i] = scales ? scales[j] : nullptr;
        EGK_REQUIRE(!need_scales || P.scale[i], "%s: null pointer (scale of task %d)", who, i);
        EGK_REQUIRE(aligned_to(4, {P.scale[i]}), "%s: the scale of task %d is not 4-byte aligned", who, i);
        if (i < count && t.rows > max_rows) max_rows = t.rows;
    }
    if (max_rows == 0) return 0;
    if (shaped && mode != CE_MIX) mode = CE_SHAPED;  // (the mix entry point builds its tasks itself: their tails are zero)
    hipStream_t s = (hipStream_t)stream;
    ProfScope prof(kid, s, 0, bytes);
#define CE_LAUNCH_MODE(M)                                                                                                          \
    case M:                                                                                                                        \
        EGK_DISPATCH_T(dtype, hipLaunchKernelGGL((ce_fused_multi_kernel<T, M>), dim3(row_grid(max_rows), count), dim3(256), 0, s, P, S, \
                                                 smoothing));                                                                      \
        break
    switch (mode) {
        CE_LAUNCH_MODE(CE_PLAIN);
        CE_LAUNCH_MODE(CE_BALANCED);
        CE_LAUNCH_MODE(CE_SHAPED);
        CE_LAUNCH_MODE(CE_MIX);
    }
#undef CE_LAUNCH_MODE
    return check_launch(who);
}

template <bool SHAPED>
static int bce_fwd_launch(const char* who, int kid, egk_stream_t stream, const float* logits, const int64_t* y, float* loss, int32_t n,
                          const BceShape sh) {
    EGK_REQUIRE(logits && y && loss, "%s: null pointer", who);
    EGK_REQUIRE(n >= 0, "%s: n must be >= 0", who);
    EGK_REQUIRE(bce_shape_ok(sh.pos, sh.neg, sh.gamma), "%s: pos, neg and gamma must be finite and >= 0 (got %g, %g, %g)", who,
                (double)sh.pos, (double)sh.neg, (double)sh.gamma);
    if (n == 0) return 0;
    hipStream_t s = (hipStream_t)stream;
    ProfScope prof(kid, s, 0, 16.0 * n);
    hipLaunchKernelGGL(bce_fwd_kernel<SHAPED>, dim3(cdiv(n, 256)), dim3(256), 0, s, logits, (const long long*)y, loss, n, sh);
    return check_launch(who);
}

template <bool SHAPED>
static int bce_bwd_launch(const char* who, int kid, egk_stream_t stream, const float* logits, const int64_t* y, const float* gloss,
                          void* dlogits, int32_t n, const BceShape sh, int32_t dtype) {
    EGK_REQUIRE(logits && y && gloss && dlogits, "%s: null pointer", who);
    EGK_REQUIRE(n >= 0, "%s: n must be >= 0", who);
    EGK_REQUIRE(bce_shape_ok(sh.pos, sh.neg, sh.gamma), "%s: pos, neg and gamma must be finite and >= 0 (got %g, %g, %g)", who,
                (double)sh.pos, (double)sh.neg, (double)sh.gamma);
    EGK_REQUIRE(dtype == EGK_F32 || dtype == EGK_BF16, "%s: unknown activation dtype %d", who, (int)dtype);
    if (n == 0) return 0;
    hipStream_t s = (hipStream_t)stream;
    ProfScope prof(kid, s, 0, 20.0 * n);
    EGK_DISPATCH_T(dtype, hipLaunchKernelGGL((bce_bwd_kernel<T, SHAPED>), dim3(cdiv(n, 256)), dim3(256), 0, s, logits,
                                             (const long long*)y, gloss, (T*)dlogits, n, sh));
    return check_launch(who);
}

}  // namespace egk

using namespace egk;

extern "C" {

int egk_ce_fwd(egk_stream_t stream, const float* logits, int64_t ld, const int64_t* y, int64_t y_stride, float* loss,
               float* lse, int32_t rows, int32_t C, float smoothing, int32_t accumulate) {
    return ce_fwd_launch<false>("egk_ce_fwd", KID_CE_FWD, stream, logits, ld, y, y_stride, nullptr, nullptr, loss, lse, rows, C,
                                smoothing, accumulate);
}

int egk_ce_w_fwd(egk_stream_t stream, const float* logits, int64_t ld, const int64_t* y, int64_t y_stride, const float* weight,
                 const float* offset, float* loss, float* lse, int32_t rows, int32_t C, float smoothing, int32_t accumulate) {
    return ce_fwd_launch<true>("egk_ce_w_fwd", KID_CE_BALANCED, stream, logits, ld, y, y_stride, weight, offset, loss, lse, rows, C,
                               smoothing, accumulate);
}

int egk_ce_bwd(egk_stream_t stream, const float* logits, int64_t ld, const int64_t* y, int64_t y_stride, const float* lse,
               const float* gloss, void* dlogits, int64_t ldd, int32_t rows, int32_t C, float smoothing, int32_t dtype) {
    return ce_bwd_launch<false>("egk_ce_bwd", KID_CE_BWD, stream, logits, ld, y, y_stride, nullptr, nullptr, lse, gloss, dlogits, ldd,
                                rows, C, smoothing, dtype);
}

int egk_ce_w_bwd(egk_stream_t stream, const float* logits, int64_t ld, const int64_t* y, int64_t y_stride, const float* weight,
                 const float* offset, const float* lse, const float* gloss, void* dlogits, int64_t ldd, int32_t rows, int32_t C,
                 float smoothing, int32_t dtype) {
    return ce_bwd_launch<true>("egk_ce_w_bwd", KID_CE_BALANCED, stream, logits, ld, y, y_stride, weight, offset, lse, gloss, dlogits,
                               ldd, rows, C, smoothing, dtype);
}

// the single-task form with its heads in arrays: one task of egk_ce_fused_multi, the same kernel on a (row_grid(rows), 1) grid
int egk_ce_fused(egk_stream_t stream, const float* const* logits, const int64_t* ld, const int32_t* C, const int32_t* pad,
                 const int64_t* dcol, int32_t n_heads, const int64_t* y, int64_t y_stride, float* loss, void* dlogits, int64_t ldd,
                 int32_t rows, float smoothing, float gscale, int32_t dtype) {
    EGK_REQUIRE(logits && ld && C && pad && dcol && y && loss && dlogits, "egk_ce_fused: null pointer");
    EGK_REQUIRE(n_heads >= 1 && n_heads <= CE_MAX_HEADS, "egk_ce_fused: 1 .. %d heads", CE_MAX_HEADS);
    egk_ce_task t{};
    for (int h = 0; h < n_heads; ++h) {
        t.logits[h] = logits[h]; t.ld[h] = ld[h]; t.C[h] = C[h]; t.pad[h] = pad[h]; t.dcol[h] = dcol[h];
    }
    t.n_heads = n_heads; t.y = y; t.y_stride = y_stride; t.loss = loss; t.dlogits = dlogits; t.ldd = ldd; t.rows = rows;
    t.gscale = gscale;
    return ce_fused_launch("egk_ce_fused", KID_CE_FWD, stream, CE_PLAIN, &t, nullptr, 1, smoothing, dtype);
}

int egk_ce_fused_multi(egk_stream_t stream, const egk_ce_task* tasks, int32_t count, float smoothing, int32_t dtype) {
    return ce_fused_launch("egk_ce_fused_multi", KID_CE_FWD, stream, CE_PLAIN, tasks, nullptr, count, smoothing, dtype);
}

int egk_ce_w_fused_multi(egk_stream_t stream, const egk_ce_w_task* tasks, int32_t count, float smoothing, int32_t dtype) {
    return ce_fused_launch("egk_ce_w_fused_multi", KID_CE_BALANCED, stream, CE_BALANCED, nullptr, tasks, count, smoothing, dtype);
}

int egk_ce_fused_multi_s(egk_stream_t stream, const egk_ce_task* tasks, const float* const* scales, int32_t count, float smoothing,
                         int32_t dtype) {
    return ce_fused_launch("egk_ce_fused_multi_s", KID_TASK_SCALE, stream, CE_PLAIN, tasks, nullptr, count, smoothing, dtype, scales, true);
}

int egk_ce_w_fused_multi_s(egk_stream_t stream, const egk_ce_w_task* tasks, const float* const* scales, int32_t count, float smoothing,
                           int32_t dtype) {
    return ce_fused_launch("egk_ce_w_fused_multi_s", KID_TASK_SCALE, stream, CE_BALANCED, nullptr, tasks, count, smoothing, dtype, scales, true);
}

// the two-target form: the array form of egk_ce_fused per task, with its own pointer checks (y_b, lam and the alignments that only
// this entry point refuses); the packer does the rest
int egk_ce_mix_fused_multi(egk_stream_t stream, int32_t count, const float* const* logits, const int64_t* ld, const int32_t* C,
                           const int32_t* pad, const int64_t* dcol, const int32_t* n_heads, const int64_t* const* y,
                           const int64_t* const* y_b, const int64_t* y_stride, const float* const* lam, float* const* loss,
                           void* const* dlogits, const int64_t* ldd, const int32_t* rows, const float* gscale,
                           const float* const* scales, float smoothing, int32_t dtype) {
    EGK_REQUIRE(logits && ld && C && pad && dcol && n_heads && y && y_b && y_stride && lam && loss && dlogits && ldd && rows && gscale,
                "egk_ce_mix_fused_multi: null pointer (a host array)");
    EGK_REQUIRE(count >= 1 && count <= EGK_CE_MIX_MAX_TASKS, "egk_ce_mix_fused_multi: 1 .. %d tasks (got %d)", EGK_CE_MIX_MAX_TASKS, count);
    egk_ce_task t[EGK_CE_MIX_MAX_TASKS] = {};
    for (int j = 0; j < count; ++j) {
        EGK_REQUIRE(n_heads[j] >= 1 && n_heads[j] <= EGK_CE_MIX_MAX_HEADS, "egk_ce_mix_fused_multi: 1 .. %d heads (task %d)",
                    EGK_CE_MIX_MAX_HEADS, j);
        EGK_REQUIRE(y[j] && y_b[j], "egk_ce_mix_fused_multi: null pointer (y or y_b of task %d)", j);
        EGK_REQUIRE(lam[j], "egk_ce_mix_fused_multi: null pointer (lam of task %d)", j);
        EGK_REQUIRE(loss[j] && dlogits[j], "egk_ce_mix_fused_multi: null pointer (loss or dlogits of task %d)", j);
        EGK_REQUIRE(aligned_to(8u, {y[j], y_b[j]}), "egk_ce_mix_fused_multi: y / y_b of task %d are not 8-byte aligned", j);
        EGK_REQUIRE(aligned_to(4u, {lam[j], loss[j]}), "egk_ce_mix_fused_multi: lam / loss of task %d are not 4-byte aligned", j);
        EGK_REQUIRE(aligned_to(dtype == EGK_BF16 ? 2u : 4u, {dlogits[j]}), "egk_ce_mix_fused_multi: dlogits of task %d is not aligned to its element", j);
        for (int h = 0; h < n_heads[j]; ++h) {
            const int k = EGK_CE_MIX_MAX_HEADS * j + h;
            EGK_REQUIRE(aligned_to(4u, {logits[k]}), "egk_ce_mix_fused_multi: the logits of head %d of task %d are not 4-byte aligned", h, j);
            t[j].logits[h] = logits[k]; t[j].ld[h] = ld[k]; t[j].C[h] = C[k]; t[j].pad[h] = pad[k]; t[j].dcol[h] = dcol[k];
        }
        t[j].n_heads = n_heads[j]; t[j].y = y[j]; t[j].y_stride = y_stride[j]; t[j].loss = loss[j]; t[j].dlogits = dlogits[j];
        t[j].ldd = ldd[j]; t[j].rows = rows[j]; t[j].gscale = gscale[j];
    }
    return ce_fused_launch("egk_ce_mix_fused_multi", KID_CE_MIX, stream, CE_MIX, t, nullptr, count, smoothing, dtype, scales, false, y_b, lam);
}

int egk_bce_fwd(egk_stream_t stream, const float* logits, const int64_t* y, float* loss, int32_t n) {
    return bce_fwd_launch<false>("egk_bce_fwd", KID_BCE_FWD, stream, logits, y, loss, n, BceShape{1.f, 1.f, 0.f});
}

int egk_bce_w_fwd(egk_stream_t stream, const float* logits, const int64_t* y, float* loss, int32_t n, float pos, float neg,
                  float gamma) {
    return bce_fwd_launch<true>("egk_bce_w_fwd", KID_BCE_BALANCED, stream, logits, y, loss, n, BceShape{pos, neg, gamma});
}

int egk_bce_bwd(egk_stream_t stream, const float* logits, const int64_t* y, const float* gloss, void* dlogits, int32_t n,
                int32_t dtype) {
    return bce_bwd_launch<false>("egk_bce_bwd", KID_BCE_BWD, stream, logits, y, gloss, dlogits, n, BceShape{1.f, 1.f, 0.f}, dtype);
}

int egk_bce_w_bwd(egk_stream_t stream, const float* logits, const int64_t* y, const float* gloss, void* dlogits, int32_t n, float pos,
                  float neg, float gamma, int32_t dtype) {
    return bce_bwd_launch<true>("egk_bce_w_bwd", KID_BCE_BALANCED, stream, logits, y, gloss, dlogits, n, BceShape{pos, neg, gamma}, dtype);
}

int egk_onehot_sigmoid_loss_fwd(egk_stream_t stream, const float* logits, const int64_t* y, float* loss, int32_t rows, int32_t C,
                                int32_t kind, float alpha, float gamma) {
    EGK_REQUIRE(logits && y && loss, "egk_onehot_sigmoid_loss_fwd: null pointer");
    EGK_REQUIRE(C >= 1 && (kind == 0 || kind == 1), "egk_onehot_sigmoid_loss_fwd: bad C / kind");
    const int n = rows * C;
    if (n == 0) return 0;
    hipStream_t s = (hipStream_t)stream;
    ProfScope prof(KID_BCE_FWD, s, 0, 8.0 * n + 8.0 * rows);
    hipLaunchKernelGGL(onehot_sigmoid_fwd_kernel, dim3(cdiv(n, 256)), dim3(256), 0, s, logits, (const long long*)y, loss, n, C,
                       kind, alpha, gamma);
    return check_launch("egk_onehot_sigmoid_loss_fwd");
}

int egk_onehot_sigmoid_loss_bwd(egk_stream_t stream, const float* logits, const int64_t* y, const float* gloss, void* dlogits,
                                int32_t rows, int32_t C, int32_t kind, float alpha, float gamma, int32_t dtype) {
    EGK_REQUIRE(logits && y && gloss && dlogits, "egk_onehot_sigmoid_loss_bwd: null pointer");
    EGK_REQUIRE(C >= 1 && (kind == 0 || kind == 1), "egk_onehot_sigmoid_loss_bwd: bad C / kind");
    const int n = rows * C;
    if (n == 0) return 0;
    hipStream_t s = (hipStream_t)stream;
    ProfScope prof(KID_BCE_BWD, s, 0, 12.0 * n + 8.0 * rows);
    EGK_DISPATCH_T(dtype, hipLaunchKernelGGL(onehot_sigmoid_bwd_kernel<T>, dim3(cdiv(n, 256)), dim3(256), 0, s, logits,
                                             (const long long*)y, gloss, (T*)dlogits, n, C, kind, alpha, gamma));
    return check_launch("egk_onehot_sigmoid_loss_bwd");
}

}  // extern "C"
