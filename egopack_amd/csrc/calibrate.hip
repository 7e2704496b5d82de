// Post-hoc temperature calibration of a head, fitted on the device (include/egopack_calibrate.h):
//   egk_temp_stats       the q24 integer sums of F, F' and F'' of one head at a beta = 1 / T read from device memory
//   egk_temp_newton      one safeguarded Newton step per head from those sums, the iterate rounded to f32 before it is stored
//   egk_temp_topk_prob   the probabilities of a GIVEN top-k order (egk_topk_softmax's) at a beta, and the scaled row's log-sum-exp
//   egk_temp_scale_rows  an f32 copy of the logits times beta
// Plain C++: one wave per row, four waves per workgroup, at most 2048 workgroups with a strided row loop (egk_class_report's walk),
// no LDS.  Every launcher refuses its argument errors on the host before it launches.
#include <math.h>

#include "common.h"
#include "temp_row.h"

namespace egk {

__device__ __forceinline__ void temp_add_i64(long long* p, long long v) { atomicAdd((unsigned long long*)p, (unsigned long long)v); }

// |v| < 2^39 and finite (a NaN fails the comparison): llrint(v * 2^24) then fits an int64 with room for 2^23 rows of the largest
__device__ __forceinline__ bool temp_fits(float v) { return fabsf(v) < 549755813888.f; }

template <typename T>
__global__ __launch_bounds__(256) void temp_stats_kernel(const T* __restrict__ logits, long long ld, const long long* __restrict__ labels,
                                                         long long label_stride, int rows, int C, const float* __restrict__ beta_p,
                                                         long long* __restrict__ acc) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const float beta = beta_p[0];
    const bool beta_ok = beta > 0.f && beta < INFINITY;
    const bool res = C <= TEMP_RES;
    long long s_nll = 0, s_d1 = 0, s_d2 = 0, n_valid = 0, n_ign = 0, n_left = 0;  // (the same value in every lane)
    for (int row = blockIdx.x * 4 + wave; row < rows; row += gridDim.x * 4) {
        const long long y = labels[(long long)row * label_stride];
        if (y < 0 || y >= C) {
            ++n_ign;
            continue;
        }
        ++n_valid;
        if (!beta_ok) {
            ++n_left;
            continue;
        }
        const T* __restrict__ r = logits + (long long)row * ld;
        float z[TEMP_SLOTS];
#pragma unroll
        for (int i = 0; i < TEMP_SLOTS; ++i) {
            const int c = lane + WAVE * i;
            z[i] = res && c < C ? ld1t(r + c) : 0.f;
        }
        const float lse = res ? temp_row_lse<T, true>(r, C, beta, z, lane) : temp_row_lse<T, false>(r, C, beta, z, lane);
        const float zy = ld1t(r + y);
        const float nll = lse - temp_scaled(beta, zy);
        // m = sum p z, then d2 = sum p (z - m)^2; a class of probability 0 adds nothing (0 * -inf is no number)
        float m = 0.f;
        if (res) {
#pragma unroll
            for (int i = 0; i < TEMP_SLOTS; ++i) {
                const float p = lane + WAVE * i < C ? expf(temp_scaled(beta, z[i]) - lse) : 0.f;
                if (p > 0.f) m += p * z[i];
            }
        } else {
            for (int c = lane; c < C; c += 64) {
                const float v = ld1t(r + c), p = expf(temp_scaled(beta, v) - lse);
                if (p > 0.f) m += p * v;
            }
        }
        m = wave_sum(m);
        float d2 = 0.f;
        if (res) {
#pragma unroll
            for (int i = 0; i < TEMP_SLOTS; ++i) {
                const float p = lane + WAVE * i < C ? expf(temp_scaled(beta, z[i]) - lse) : 0.f;
                const float d = z[i] - m;
                if (p > 0.f) d2 += p * (d * d);
            }
        } else {
            for (int c = lane; c < C; c += 64) {
                const float v = ld1t(r + c), p = expf(temp_scaled(beta, v) - lse), d = v - m;
                if (p > 0.f) d2 += p * (d * d);
            }
        }
        d2 = wave_sum(d2);
        const float d1 = m - zy;
        if (temp_fits(nll) && temp_fits(d1) && temp_fits(d2)) {
            s_nll += llrintf(nll * 16777216.f);  // (exact: a power of two)
            s_d1 += llrintf(d1 * 16777216.f);
            s_d2 += llrintf(d2 * 16777216.f);
        } else {
            ++n_left;
        }
    }
    if (lane == 0) {  // one 64-bit integer atomic per accumulator this wave has something for
        if (s_nll) temp_add_i64(acc + 0, s_nll);
        if (s_d1) temp_add_i64(acc + 1, s_d1);
        if (s_d2) temp_add_i64(acc + 2, s_d2);
        if (n_valid) temp_add_i64(acc + 3, n_valid);
        if (n_ign) temp_add_i64(acc + 4, n_ign);
        if (n_left) temp_add_i64(acc + 5, n_left);
    }
}

// one thread per head (include/egopack_calibrate.h has the rule; tests/calibration_common.py restates it in numpy, statement for
// statement).  f64, nothing fused.
__global__ __launch_bounds__(64) void temp_newton_kernel(const long long* __restrict__ acc, int n_heads, double* __restrict__ state,
                                                         float* __restrict__ beta, double bmin, double bmax, double stop) {
#pragma clang fp contract(off)
    const int h = threadIdx.x;
    if (h >= n_heads) return;
    double* st = state + 8 * h;
    const long long* a = acc + 8 * h;
    if (st[5] != 0.0) return;  // frozen
    const double b = st[0];
    double lo = st[1], hi = st[2], lo_seen = st[3], hi_seen = st[4];
    st[6] = st[6] + 1.0;
    if (a[3] - a[5] <= 0) {
        st[5] = 4.0;
        return;
    }
    const double F1 = (double)a[1] / 16777216.0, F2 = (double)a[2] / 16777216.0;
    if (F1 > 0.0) {
        hi = b;
        hi_seen = 1.0;
        st[2] = hi;
        st[4] = hi_seen;
        if (b <= bmin) {
            st[5] = 2.0;
            return;
        }
    } else {
        lo = b;
        lo_seen = 1.0;
        st[1] = lo;
        st[3] = lo_seen;
        if (b >= bmax) {
            st[5] = 3.0;
            return;
        }
    }
    double prop;
    if (F2 > 0.0)
        prop = b - F1 / F2;
    else
        prop = F1 > 0.0 ? -INFINITY : INFINITY;
    double nb = prop;
    if (prop >= hi)
        nb = hi_seen != 0.0 ? sqrt(lo * hi) : hi;
    else if (prop <= lo)
        nb = lo_seen != 0.0 ? sqrt(lo * hi) : lo;
    const float nbf = (float)nb;
    const double nbd = (double)nbf;
    const double rel = fabs(nbd - b) / b;
    st[0] = nbd;
    st[7] = rel;
    if (rel <= stop) st[5] = 1.0;
    beta[h] = nbf;
}

template <typename T>
__global__ __launch_bounds__(256) void temp_topk_prob_kernel(const T* __restrict__ logits, long long ld, int rows, int C,
                                                             const float* __restrict__ beta_p, const long long* __restrict__ idx,
                                                             long long idx_row_stride, int k, float* __restrict__ prob,
                                                             long long prob_row_stride, float* __restrict__ lse_out) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const float beta = beta_p[0];
    const float none[TEMP_SLOTS] = {};
    for (int row = blockIdx.x * 4 + wave; row < rows; row += gridDim.x * 4) {
        const T* __restrict__ r = logits + (long long)row * ld;
        const float lse = temp_row_lse<T, false>(r, C, beta, none, lane);
        if (lane < k) {
            const long long c = idx[(long long)row * idx_row_stride + lane];
            prob[(long long)row * prob_row_stride + lane] = c >= 0 && c < C ? expf(temp_scaled(beta, ld1t(r + c)) - lse) : 0.f;
        }
        if (lse_out && lane == 0) lse_out[row] = lse;
    }
}

template <typename T>
__global__ __launch_bounds__(256) void temp_scale_rows_kernel(const T* __restrict__ logits, long long ld, int rows, int C,
                                                              const float* __restrict__ beta_p, float* __restrict__ out, long long ldo) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const float beta = beta_p[0];
    for (int row = blockIdx.x * 4 + wave; row < rows; row += gridDim.x * 4) {
        const T* __restrict__ r = logits + (long long)row * ld;
        float* __restrict__ o = out + (long long)row * ldo;
        for (int c = lane; c < C; c += 64) o[c] = temp_scaled(beta, ld1t(r + c));
    }
}

static int temp_grid(int rows) {
    const int grid = cdiv(rows, 4);
    return grid > 2048 ? 2048 : grid;
}

template <typename T>
static void temp_stats_launch(hipStream_t s, const void* logits, long long ld, const int64_t* labels, long long label_stride, int rows, int C,
                              const float* beta, int64_t* acc) {
    hipLaunchKernelGGL(temp_stats_kernel<T>, dim3(temp_grid(rows)), dim3(256), 0, s, (const T*)logits, ld, (const long long*)labels,
                       label_stride, rows, C, beta, (long long*)acc);
}
template <typename T>
static void temp_topk_prob_launch(hipStream_t s, const void* logits, long long ld, int rows, int C, const float* beta, const int64_t* idx,
                                  long long idx_row_stride, int k, float* prob, long long prob_row_stride, float* lse) {
    hipLaunchKernelGGL(temp_topk_prob_kernel<T>, dim3(temp_grid(rows)), dim3(256), 0, s, (const T*)logits, ld, rows, C, beta,
                       (const long long*)idx, idx_row_stride, k, prob, prob_row_stride, lse);
}
template <typename T>
static void temp_scale_rows_launch(hipStream_t s, const void* logits, long long ld, int rows, int C, const float* beta, float* out,
                                   long long ldo) {
    hipLaunchKernelGGL(temp_scale_rows_kernel<T>, dim3(temp_grid(rows)), dim3(256), 0, s, (const T*)logits, ld, rows, C, beta, out, ldo);
}

}  // namespace egk

using namespace egk;

extern "C" {

int egk_temp_stats(egk_stream_t stream, const void* logits, int64_t ld, const int64_t* labels, int64_t label_stride, int32_t rows,
                   int32_t C, const float* beta, int64_t* acc, int32_t dtype) {
    EGK_REQUIRE(logits, "egk_temp_stats: null pointer (logits)");
    EGK_REQUIRE(labels, "egk_temp_stats: null pointer (labels)");
    EGK_REQUIRE(beta, "egk_temp_stats: null pointer (beta)");
    EGK_REQUIRE(acc, "egk_temp_stats: null pointer (acc)");
    EGK_REQUIRE(rows >= 0, "egk_temp_stats: rows >= 0 (got %d)", rows);
    EGK_REQUIRE(C >= 1, "egk_temp_stats: C >= 1 (got %d)", C);
    EGK_REQUIRE(ld >= C, "egk_temp_stats: ld >= C (ld %lld, C %d)", (long long)ld, C);
    EGK_REQUIRE(dtype == EGK_F32 || dtype == EGK_BF16, "egk_temp_stats: unknown logits dtype %d", dtype);
    EGK_REQUIRE(aligned_to(dtype == EGK_BF16 ? 2u : 4u, {logits}), "egk_temp_stats: misaligned logits (to their element)");
    EGK_REQUIRE(aligned_to(4u, {beta}), "egk_temp_stats: misaligned beta (4-byte)");
    EGK_REQUIRE(aligned_to(8u, {labels}), "egk_temp_stats: misaligned labels (8-byte)");
    EGK_REQUIRE(aligned_to(8u, {acc}), "egk_temp_stats: misaligned acc (8-byte)");
    if (rows == 0) return 0;
    hipStream_t s = (hipStream_t)stream;
    const double es = dtype == EGK_BF16 ? 2 : 4;
    ProfScope prof(KID_TEMP_STATS, s, 0, (double)rows * (C * es * (C > TEMP_RES ? 4 : 1) + 8.0));
    EGK_DISPATCH_T(dtype, (temp_stats_launch<T>(s, logits, (long long)ld, labels, (long long)label_stride, (int)rows, (int)C, beta, acc)));
    return check_launch("egk_temp_stats");
}

int egk_temp_newton(egk_stream_t stream, const int64_t* acc, int32_t n_heads, double* state, float* beta, float beta_min,
                    float beta_max, float stop) {
    EGK_REQUIRE(acc, "egk_temp_newton: null pointer (acc)");
    EGK_REQUIRE(state, "egk_temp_newton: null pointer (state)");
    EGK_REQUIRE(beta, "egk_temp_newton: null pointer (beta)");
    EGK_REQUIRE(n_heads >= 1 && n_heads <= EGK_TEMP_MAX_HEADS, "egk_temp_newton: n_heads in 1 .. %d (got %d)", EGK_TEMP_MAX_HEADS, n_heads);
    EGK_REQUIRE(aligned_to(8u, {acc}), "egk_temp_newton: misaligned acc (8-byte)");
    EGK_REQUIRE(aligned_to(8u, {state}), "egk_temp_newton: misaligned state (8-byte)");
    EGK_REQUIRE(aligned_to(4u, {beta}), "egk_temp_newton: misaligned beta (4-byte)");
    EGK_REQUIRE(beta_min > 0.f && beta_min < INFINITY, "egk_temp_newton: beta_min > 0 and finite (got %g)", (double)beta_min);
    EGK_REQUIRE(beta_max >= beta_min && beta_max < INFINITY, "egk_temp_newton: beta_max >= beta_min and finite (got %g, beta_min %g)",
                (double)beta_max, (double)beta_min);
    EGK_REQUIRE(stop >= 0.f, "egk_temp_newton: stop >= 0 (got %g)", (double)stop);
    hipStream_t s = (hipStream_t)stream;
    ProfScope prof(KID_TEMP_NEWTON, s, 0, 132.0 * n_heads);
    hipLaunchKernelGGL(temp_newton_kernel, dim3(1), dim3(64), 0, s, (const long long*)acc, (int)n_heads, state, beta, (double)beta_min,
                       (double)beta_max, (double)stop);
    return check_launch("egk_temp_newton");
}

int egk_temp_topk_prob(egk_stream_t stream, const void* logits, int64_t ld, int32_t rows, int32_t C, const float* beta,
                       const int64_t* idx, int64_t idx_row_stride, int32_t k, float* prob, int64_t prob_row_stride, float* lse,
                       int32_t dtype) {
    EGK_REQUIRE(logits, "egk_temp_topk_prob: null pointer (logits)");
    EGK_REQUIRE(beta, "egk_temp_topk_prob: null pointer (beta)");
    EGK_REQUIRE(idx, "egk_temp_topk_prob: null pointer (idx)");
    EGK_REQUIRE(prob, "egk_temp_topk_prob: null pointer (prob)");
    EGK_REQUIRE(rows >= 0, "egk_temp_topk_prob: rows >= 0 (got %d)", rows);
    EGK_REQUIRE(C >= 1, "egk_temp_topk_prob: C >= 1 (got %d)", C);
    EGK_REQUIRE(ld >= C, "egk_temp_topk_prob: ld >= C (ld %lld, C %d)", (long long)ld, C);
    EGK_REQUIRE(k >= 1 && k <= EGK_TEMP_MAX_K, "egk_temp_topk_prob: k in 1 .. %d (got %d)", EGK_TEMP_MAX_K, k);
    EGK_REQUIRE(idx_row_stride >= k, "egk_temp_topk_prob: idx row stride >= k (got %lld, k %d)", (long long)idx_row_stride, k);
    EGK_REQUIRE(prob_row_stride >= k, "egk_temp_topk_prob: prob row stride >= k (got %lld, k %d)", (long long)prob_row_stride, k);
    EGK_REQUIRE(dtype == EGK_F32 || dtype == EGK_BF16, "egk_temp_topk_prob: unknown logits dtype %d", dtype);
    EGK_REQUIRE(aligned_to(dtype == EGK_BF16 ? 2u : 4u, {logits}), "egk_temp_topk_prob: misaligned logits (to their element)");
    EGK_REQUIRE(aligned_to(8u, {idx}), "egk_temp_topk_prob: misaligned idx (8-byte)");
    EGK_REQUIRE(aligned_to(4u, {beta, prob, lse}), "egk_temp_topk_prob: misaligned beta, prob or lse (4-byte)");
    if (rows == 0) return 0;
    hipStream_t s = (hipStream_t)stream;
    const double es = dtype == EGK_BF16 ? 2 : 4;
    ProfScope prof(KID_TEMP_TOPK_PROB, s, 0, (double)rows * (C * es * 2 + (es + 12.0) * k + (lse ? 4 : 0)));
    EGK_DISPATCH_T(dtype, (temp_topk_prob_launch<T>(s, logits, (long long)ld, (int)rows, (int)C, beta, idx, (long long)idx_row_stride, (int)k,
                                                    prob, (long long)prob_row_stride, lse)));
    return check_launch("egk_temp_topk_prob");
}

int egk_temp_scale_rows(egk_stream_t stream, const void* logits, int64_t ld, int32_t rows, int32_t C, const float* beta, float* out,
                        int64_t ldo, int32_t dtype) {
    EGK_REQUIRE(logits, "egk_temp_scale_rows: null pointer (logits)");
    EGK_REQUIRE(beta, "egk_temp_scale_rows: null pointer (beta)");
    EGK_REQUIRE(out, "egk_temp_scale_rows: null pointer (out)");
    EGK_REQUIRE(rows >= 0, "egk_temp_scale_rows: rows >= 0 (got %d)", rows);
    EGK_REQUIRE(C >= 1, "egk_temp_scale_rows: C >= 1 (got %d)", C);
    EGK_REQUIRE(ld >= C, "egk_temp_scale_rows: ld >= C (ld %lld, C %d)", (long long)ld, C);
    EGK_REQUIRE(ldo >= C, "egk_temp_scale_rows: ldo >= C (ldo %lld, C %d)", (long long)ldo, C);
    EGK_REQUIRE(dtype == EGK_F32 || dtype == EGK_BF16, "egk_temp_scale_rows: unknown logits dtype %d", dtype);
    EGK_REQUIRE(aligned_to(dtype == EGK_BF16 ? 2u : 4u, {logits}), "egk_temp_scale_rows: misaligned logits (to their element)");
    EGK_REQUIRE(aligned_to(4u, {beta, out}), "egk_temp_scale_rows: misaligned beta or out (4-byte)");
    if (rows == 0) return 0;
    hipStream_t s = (hipStream_t)stream;
    const double es = dtype == EGK_BF16 ? 2 : 4;
    ProfScope prof(KID_TEMP_SCALE_ROWS, s, 0, (double)rows * C * (es + 4.0));
    EGK_DISPATCH_T(dtype, (temp_scale_rows_launch<T>(s, logits, (long long)ld, (int)rows, (int)C, beta, out, (long long)ldo)));
    return check_launch("egk_temp_scale_rows");
}

}  // extern "C"
