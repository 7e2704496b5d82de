// Class-balanced cross entropy (include/egopack_ce_balanced.h): the row pass of loss_optim.hip's cross entropies with a
// per-class weight vector and a per-class logit offset applied inside it.  One wave per row, the row ownership (row_walk) and the
// grid of the plain kernels, which this unit leaves alone: a caller that passes no vector never comes here.
#include <math.h>

#include "common.h"

namespace egk {

namespace {

constexpr int CEW_WPB = 4;
constexpr int CEW_MAX_HEADS = 4;
constexpr int CEW_MAX_TASKS = 4;

// One row of one head, written once for the three kernels.  x'_c = x_c + a_c; FWD: the wave reduces max, sum exp, W = sum w and
// sum w (x' - max) in one pass after the maximum and returns the row's loss (lse_io = the log-sum-exp it formed); !FWD: lse_io is
// the saved log-sum-exp and only W is reduced (when smoothing needs it), lane by lane in the forward pass's order.  GRAD: columns
// [0, pad) of ``dr`` are written -- g * [(1-eps) w_t (p_j - [j==t]) + eps/C (W p_j - w_j)] below C, 0 in [C, pad) and in ignored
// rows.  The smoothing term is formed around the row maximum, W (lse - max) - sum w (x' - max): the same value as W lse - sum w x'
// without the cancellation of two large sums.
template <typename T, bool FWD, bool GRAD>
__device__ __forceinline__ float ce_w_row(const float* __restrict__ lr, const float* __restrict__ w, const float* __restrict__ a,
                                          int C, int pad, long long t, float smoothing, float g, float& lse_io, T* __restrict__ dr,
                                          int lane) {
#pragma clang fp contract(off)  // (the f32 and the bf16 instantiation form the same f32 value: no fusing that depends on the code around)
    const bool live = t >= 0 && t < C;
    const float sm = smoothing > 0.f ? smoothing / C : 0.f;
    float W = 0.f, loss = 0.f, l;
    if (FWD) {
        float mx = -INFINITY;
        for (int c = lane; c < C; c += 64) mx = fmaxf(mx, lr[c] + (a ? a[c] : 0.f));
        mx = wave_max(mx);
        float se = 0.f, swx = 0.f;
        for (int c = lane; c < C; c += 64) {
            const float v = lr[c] + (a ? a[c] : 0.f) - mx;
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
            const float wt = w ? w[t] : 1.f;
            const float xt = lr[t] + (a ? a[t] : 0.f);
            loss = (1.f - smoothing) * wt * (l - xt) + (smoothing > 0.f ? sm * (W * lg - swx) : 0.f);
        }
    } else {
        l = lse_io;
        if (sm > 0.f) {
            for (int c = lane; c < C; c += 64) W += w ? w[c] : 1.f;
            W = wave_sum(W);
        }
    }
    if (GRAD) {
        const float hard = live ? (1.f - smoothing) * (w ? w[t] : 1.f) : 0.f;
        for (int c = lane; c < pad; c += 64) {
            float d = 0.f;
            if (live && c < C) {
                const float p = expf(lr[c] + (a ? a[c] : 0.f) - l);
                d = hard * (p - (c == t ? 1.f : 0.f));
                if (sm > 0.f) d += sm * (W * p - (w ? w[c] : 1.f));
                d *= g;
            }
            st1t(dr + c, d);
        }
    }
    return loss;
}

__global__ __launch_bounds__(256) void ce_w_fwd_kernel(const float* __restrict__ logits, long long ld, const long long* __restrict__ y,
                                                       long long ys, const float* __restrict__ w, const float* __restrict__ a,
                                                       float* __restrict__ loss, float* __restrict__ lse, int rows, int C,
                                                       float smoothing, int accumulate) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const RowWalk rw = row_walk(blockIdx.x, gridDim.x, 0, rows, wave, CEW_WPB);  // (XCD x owns a contiguous eighth of the rows: common.h)
    for (int row = rw.first; row < rw.end; row += rw.step) {
        float l;
        const float o = ce_w_row<float, true, false>(logits + (long long)row * ld, w, a, C, 0, y[(long long)row * ys], smoothing, 0.f,
                                                     l, nullptr, lane);
        if (lane == 0) {
            lse[row] = l;
            loss[row] = accumulate ? loss[row] + o : o;
        }
    }
}

template <typename T>
__global__ __launch_bounds__(256) void ce_w_bwd_kernel(const float* __restrict__ logits, long long ld, const long long* __restrict__ y,
                                                       long long ys, const float* __restrict__ w, const float* __restrict__ a,
                                                       const float* __restrict__ lse, const float* __restrict__ gloss,
                                                       T* __restrict__ dlogits, long long ldd, int rows, int C, float smoothing) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const RowWalk rw = row_walk(blockIdx.x, gridDim.x, 0, rows, wave, CEW_WPB);  // (XCD x owns a contiguous eighth of the rows: common.h)
    for (int row = rw.first; row < rw.end; row += rw.step) {
        float l = lse[row];
        ce_w_row<T, false, true>(logits + (long long)row * ld, w, a, C, C, y[(long long)row * ys], smoothing, gloss[row], l,
                                 dlogits + (long long)row * ldd, lane);
    }
}

struct CEWHeads {
    const float* logits[CEW_MAX_HEADS];
    const float* w[CEW_MAX_HEADS];
    const float* a[CEW_MAX_HEADS];
    long long ld[CEW_MAX_HEADS];
    long long dcol[CEW_MAX_HEADS];  // first column of the head's block in the gradient buffer
    int C[CEW_MAX_HEADS];
    int pad[CEW_MAX_HEADS];         // columns [C, pad) of the gradient block are set to zero
};
struct CEWTasks {
    CEWHeads H[CEW_MAX_TASKS];
    const long long* y[CEW_MAX_TASKS];
    float* loss[CEW_MAX_TASKS];
    void* dlogits[CEW_MAX_TASKS];
    long long ys[CEW_MAX_TASKS];
    long long ldd[CEW_MAX_TASKS];
    int n_heads[CEW_MAX_TASKS];
    int rows[CEW_MAX_TASKS];
    float gscale[CEW_MAX_TASKS];
};

// loss AND gradient of up to four tasks in one launch (blockIdx.y = task): egk_ce_fused_multi's contract with the vectors
template <typename T>
__global__ __launch_bounds__(256) void ce_w_fused_multi_kernel(const CEWTasks P, float smoothing) {
    const int k = blockIdx.y;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const CEWHeads& H = P.H[k];
    const int n_heads = P.n_heads[k], rows = P.rows[k];
    const long long* __restrict__ y = P.y[k];
    const long long ys = P.ys[k], ldd = P.ldd[k];
    float* __restrict__ loss = P.loss[k];
    T* __restrict__ dlogits = (T*)P.dlogits[k];
    const float gscale = P.gscale[k];
    const RowWalk rw = row_walk(blockIdx.x, gridDim.x, 0, rows, wave, CEW_WPB);  // (XCD x owns a contiguous eighth of the rows: common.h)
    for (int row = rw.first; row < rw.end; row += rw.step) {
        float total = 0.f;
        for (int h = 0; h < n_heads; ++h) {
            float l;
            total += ce_w_row<T, true, true>(H.logits[h] + (long long)row * H.ld[h], H.w[h], H.a[h], H.C[h], H.pad[h],
                                             y[(long long)row * ys + h], smoothing, gscale, l,
                                             dlogits + (long long)row * ldd + H.dcol[h], lane);
        }
        if (lane == 0) loss[row] = total;
    }
}

inline int cew_row_grid(int rows) {
    int g = cdiv(rows, CEW_WPB);
    return g < 1 ? 1 : (g > 2048 ? 2048 : g);
}

}  // namespace

}  // namespace egk

using namespace egk;

extern "C" {

int egk_ce_w_fwd(egk_stream_t stream, const float* logits, int64_t ld, const int64_t* y, int64_t y_stride, const float* weight,
                 const float* offset, float* loss, float* lse, int32_t rows, int32_t C, float smoothing, int32_t accumulate) {
    EGK_REQUIRE(logits && y && loss && lse, "egk_ce_w_fwd: null pointer");
    EGK_REQUIRE(C >= 1, "egk_ce_w_fwd: C must be >= 1");
    EGK_REQUIRE(rows >= 0, "egk_ce_w_fwd: rows must be >= 0");
    EGK_REQUIRE(aligned_to(4, {weight, offset}), "egk_ce_w_fwd: misaligned vector pointer -- weight and offset are read one float at a time and must be 4-byte aligned");
    if (rows == 0) return 0;
    hipStream_t s = (hipStream_t)stream;
    ProfScope prof(KID_CE_BALANCED, s, 0, 4.0 * rows * C);
    hipLaunchKernelGGL(ce_w_fwd_kernel, dim3(cew_row_grid(rows)), dim3(256), 0, s, logits, (long long)ld, (const long long*)y,
                       (long long)y_stride, weight, offset, loss, lse, rows, C, smoothing, accumulate);
    return check_launch("egk_ce_w_fwd");
}

int egk_ce_w_bwd(egk_stream_t stream, const float* logits, int64_t ld, const int64_t* y, int64_t y_stride, const float* weight,
                 const float* offset, const float* lse, const float* gloss, void* dlogits, int64_t ldd, int32_t rows, int32_t C,
                 float smoothing, int32_t dtype) {
    EGK_REQUIRE(logits && y && lse && gloss && dlogits, "egk_ce_w_bwd: null pointer");
    EGK_REQUIRE(C >= 1, "egk_ce_w_bwd: C must be >= 1");
    EGK_REQUIRE(rows >= 0, "egk_ce_w_bwd: rows must be >= 0");
    EGK_REQUIRE(aligned_to(4, {weight, offset}), "egk_ce_w_bwd: misaligned vector pointer -- weight and offset are read one float at a time and must be 4-byte aligned");
    EGK_REQUIRE(dtype == EGK_F32 || dtype == EGK_BF16, "egk_ce_w_bwd: unknown activation dtype %d", (int)dtype);
    if (rows == 0) return 0;
    hipStream_t s = (hipStream_t)stream;
    ProfScope prof(KID_CE_BALANCED, s, 0, 8.0 * rows * C);
    EGK_DISPATCH_T(dtype, hipLaunchKernelGGL(ce_w_bwd_kernel<T>, dim3(cew_row_grid(rows)), dim3(256), 0, s, logits, (long long)ld,
                                             (const long long*)y, (long long)y_stride, weight, offset, lse, gloss, (T*)dlogits,
                                             (long long)ldd, rows, C, smoothing));
    return check_launch("egk_ce_w_bwd");
}

int egk_ce_w_fused_multi(egk_stream_t stream, const egk_ce_w_task* tasks, int32_t count, float smoothing, int32_t dtype) {
    EGK_REQUIRE(tasks, "egk_ce_w_fused_multi: null pointer");
    EGK_REQUIRE(count >= 1 && count <= CEW_MAX_TASKS, "egk_ce_w_fused_multi: 1 .. %d tasks", CEW_MAX_TASKS);
    EGK_REQUIRE(dtype == EGK_F32 || dtype == EGK_BF16, "egk_ce_w_fused_multi: unknown activation dtype %d", (int)dtype);
    CEWTasks P;
    double bytes = 0;
    int max_rows = 0;
    for (int i = 0; i < CEW_MAX_TASKS; ++i) {  // (the slots behind ``count`` repeat the last task with no rows: no wild pointers in the argument)
        const egk_ce_w_task& wt = tasks[i < count ? i : count - 1];
        const egk_ce_task& t = wt.base;
        EGK_REQUIRE(t.n_heads >= 1 && t.n_heads <= CEW_MAX_HEADS, "egk_ce_w_fused_multi: 1 .. %d heads (task %d)", CEW_MAX_HEADS, i);
        EGK_REQUIRE(t.y && t.loss && t.dlogits, "egk_ce_w_fused_multi: null pointer in task %d", i);
        EGK_REQUIRE(t.rows >= 0, "egk_ce_w_fused_multi: rows must be >= 0 (task %d)", i);
        for (int h = 0; h < CEW_MAX_HEADS; ++h) {
            const int k = h < t.n_heads ? h : t.n_heads - 1;
            EGK_REQUIRE(t.logits[k], "egk_ce_w_fused_multi: null pointer (logits of head %d of task %d)", k, i);
            EGK_REQUIRE(t.C[k] >= 1, "egk_ce_w_fused_multi: C must be >= 1 (head %d of task %d)", k, i);
            EGK_REQUIRE(t.pad[k] >= t.C[k], "egk_ce_w_fused_multi: pad must be >= C (head %d of task %d)", k, i);
            EGK_REQUIRE(aligned_to(4, {wt.weight[k], wt.offset[k]}),
                        "egk_ce_w_fused_multi: misaligned vector pointer -- weight and offset are read one float at a time and must be 4-byte aligned (head %d of task %d)", k, i);
            CEWHeads& H = P.H[i];
            H.logits[h] = t.logits[k]; H.w[h] = wt.weight[k]; H.a[h] = wt.offset[k]; H.ld[h] = t.ld[k]; H.dcol[h] = t.dcol[k];
            H.C[h] = t.C[k]; H.pad[h] = t.pad[k];
            if (i < count && h < t.n_heads) bytes += 6.0 * t.rows * t.C[k];
        }
        P.n_heads[i] = t.n_heads; P.y[i] = (const long long*)t.y; P.ys[i] = t.y_stride; P.loss[i] = t.loss;
        P.dlogits[i] = t.dlogits; P.ldd[i] = t.ldd; P.rows[i] = i < count ? t.rows : 0; P.gscale[i] = t.gscale;
        if (i < count && t.rows > max_rows) max_rows = t.rows;
    }
    if (max_rows == 0) return 0;
    hipStream_t s = (hipStream_t)stream;
    ProfScope prof(KID_CE_BALANCED, s, 0, bytes);
    EGK_DISPATCH_T(dtype, hipLaunchKernelGGL(ce_w_fused_multi_kernel<T>, dim3(cew_row_grid(max_rows), count), dim3(256), 0, s, P, smoothing));
    return check_launch("egk_ce_w_fused_multi");
}

}  // extern "C"
