// Validation-side kernels: integer work on logits / predictions that are already resident in
// HBM, so that the validation loop needs no device->host copy of [N, C] logits per batch.
//   egk_label_rank    rank of the ground-truth class inside each logits row (top-k accuracy / recall are counts of
//                     rank < k: reference utils/meters/utils.py:6-28 topk_accuracy, torchmetrics MulticlassAccuracy)
//   egk_edit_distance Levenshtein distance of K sampled label sequences against the ground truth
//                     (reference utils/meters/ego4d.py:410-423 ``editdistance.eval(pred, label) / Z``, min over K on the host)
//   egk_class_report  confusion matrix, top-2 confusion matrix and per-class fixed-point loss sums of all heads of a task in one
//                     launch (include/egopack_class_report.h; reference utils/confusion.py, utils/meters/ego4d.py:125-170)
//   egk_topk_softmax  the best k classes of every row of every head in that same order, with their softmax probabilities and the
//                     row's log-sum-exp, in one launch (include/egopack_topk.h: what a prediction file holds)
#include "ce_row.h"
#include "common.h"
#include "rank_key.h"

namespace egk {

// one wave per row; rank = #{j : s_j > s_y} + #{j < y : s_j == s_y}  (ties go to the lower class index), -1 when the
// label is negative (ignore_index) or out of range.  NaN scores never outrank anything.
__global__ __launch_bounds__(256) void label_rank_kernel(const float* __restrict__ logits, long long ld,
                                                         const long long* __restrict__ labels, long long label_stride,
                                                         int* __restrict__ rank, int rows, int C) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int row = blockIdx.x * 4 + wave; row < rows; row += gridDim.x * 4) {
        const long long y = labels[(long long)row * label_stride];
        if (y < 0 || y >= C) {
            if (lane == 0) rank[row] = -1;
            continue;
        }
        const float* r = logits + (long long)row * ld;
        const float sy = r[y];
        int cnt = 0;
        for (int j = lane; j < C; j += 64) {
            const float v = r[j];
            cnt += (v > sy || (v == sy && j < (int)y)) ? 1 : 0;
        }
        for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o, 64);
        if (lane == 0) rank[row] = cnt;
    }
}

// one thread per (sequence n, sample k): single-row dynamic programme over Z <= 64 positions.
// pred [N, Z, K] (sample index fastest, as reference predictions.reshape(-1, 22, 5)[:, 2:] slices), label [N, Z]
__global__ __launch_bounds__(64) void edit_distance_kernel(const long long* __restrict__ pred, long long p_sn, long long p_sz,
                                                           long long p_sk, const long long* __restrict__ label,
                                                           long long l_sn, long long l_sz, int* __restrict__ out, int N,
                                                           int Z, int K) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= N * K) return;
    const int n = idx / K, k = idx % K;
    int prev[65];
    for (int j = 0; j <= Z; ++j) prev[j] = j;
    for (int i = 1; i <= Z; ++i) {
        const long long a = pred[n * p_sn + (long long)(i - 1) * p_sz + k * p_sk];
        int diag = prev[0];
        prev[0] = i;
        for (int j = 1; j <= Z; ++j) {
            const long long b = label[n * l_sn + (long long)(j - 1) * l_sz];
            const int sub = diag + (a == b ? 0 : 1);
            const int del = prev[j] + 1, ins = prev[j - 1] + 1;
            diag = prev[j];
            prev[j] = min(sub, min(del, ins));
        }
    }
    out[idx] = prev[Z];
}

// ---- the per-class report: one wave per (task, row) ---------------------------------------------------------------------------
// (the order of label_rank_kernel as ONE integer per class: rank_key of rank_key.h.)  top1 / top2 are the largest and the second
// largest key of the row.
__device__ __forceinline__ void add_i64(long long* p, long long v) { atomicAdd((unsigned long long*)p, (unsigned long long)v); }

struct ClassReportTasks {
    egk_class_report_task t[EGK_CLASS_REPORT_MAX_TASKS];
};
__global__ __launch_bounds__(256) void class_report_kernel(const ClassReportTasks P) {
    const egk_class_report_task& t = P.t[blockIdx.y];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int rows = t.rows, C = t.C;
    const long long* __restrict__ labels = (const long long*)t.labels;
    long long* __restrict__ counts = (long long*)t.counts;
    for (int row = blockIdx.x * 4 + wave; row < rows; row += gridDim.x * 4) {
        const long long y = labels[(long long)row * t.label_stride];
        if (y < 0 || y >= C) {
            if (lane == 0) add_i64(counts + 1, 1);
            continue;
        }
        const float* __restrict__ r = t.logits + (long long)row * t.ld;
        unsigned long long a1 = 0, a2 = 0;  // this lane's best and second best; then the wave's
        for (int c = lane; c < C; c += 64) {
            const unsigned long long k = rank_key(r[c], c);
            if (k > a1) {
                a2 = a1;
                a1 = k;
            } else if (k > a2) {
                a2 = k;
            }
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const unsigned long long b1 = __shfl_xor(a1, o, 64), b2 = __shfl_xor(a2, o, 64);
            const unsigned long long lo = a1 < b1 ? a1 : b1, hi2 = a2 > b2 ? a2 : b2;
            a1 = a1 > b1 ? a1 : b1;
            a2 = lo > hi2 ? lo : hi2;
        }
        float lse;
        const float loss = ce_row_plain<float, true, false>(r, C, 0, y, 0.f, 0.f, lse, nullptr, lane);
        if (lane == 0) {
            const long long top1 = (long long)(0xffffffffu - (unsigned)a1);
            const long long top2 = a2 ? (long long)(0xffffffffu - (unsigned)a2) : -1;
            add_i64(counts, 1);
            add_i64((long long*)t.confusion + y * C + top1, 1);
            if (t.top2 && top1 != y && top2 == y) add_i64((long long*)t.top2 + y * C + top1, 1);
            const float q = loss * 16777216.f;  // (exact: a power of two)
            if (fabsf(q) < 9.2233720368547758e18f) {  // finite, and llrint(q) fits: |q| < 2^63
                if (t.loss_q24) add_i64((long long*)t.loss_q24 + y, llrintf(q));
            } else {
                add_i64(counts + 2, 1);
            }
        }
    }
}

// ---- the best k classes of a row: one wave per (task, row) ---------------------------------------------------------------------
// Entry j of a row is the class with the j-th largest rank_key: pass j takes the wave-wide maximum of the keys BELOW the winner of
// pass j - 1 (no two classes of a row share a key, so "below" removes exactly the classes already taken) and lane j keeps it.  A
// row of at most TOPK_RES classes (the workload's 2, 115 and 478) holds its keys in registers, TOPK_SLOTS per lane, class
// c = lane + 64 * i in slot i (coalesced loads); a wider row forms the keys again from its logits in every pass.  k = 64 needs no
// register per entry (lane j holds entry j), so the budget is the 2 * TOPK_SLOTS key registers whatever k is: 71 VGPRs, no scratch,
// 7 of 8 waves per SIMD -- the passes are dependent wave reductions, so resident waves are what hides them.
// No LDS, no workspace, no atomics; lanes j < k store the outputs.
constexpr int TOPK_SLOTS = 8;
constexpr int TOPK_RES = WAVE * TOPK_SLOTS;

struct TopkTasks {
    egk_topk_task t[EGK_TOPK_MAX_TASKS];
};

template <typename T>
__global__ __launch_bounds__(256) void topk_softmax_kernel(const TopkTasks P, int count, int rows, int k) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long items = (long long)count * rows;
    for (long long item = (long long)blockIdx.x * 4 + wave; item < items; item += (long long)gridDim.x * 4) {
        const int ti = (int)(item / rows), row = (int)(item % rows);
        const egk_topk_task& t = P.t[ti];
        const int C = t.C;
        const T* __restrict__ r = reinterpret_cast<const T*>(t.logits) + (long long)row * t.ld;
        const bool res = C <= TOPK_RES;
        unsigned long long key[TOPK_SLOTS];
#pragma unroll
        for (int i = 0; i < TOPK_SLOTS; ++i) {  // (0: "no class" -- below every key, never taken)
            const int c = lane + WAVE * i;
            key[i] = res && c < C ? rank_key(ld1t(r + c), c) : 0ull;
        }
        unsigned long long prev = ~0ull;  // (above every key: the value part of a key is at most that of +inf)
        unsigned long long mine = 0ull;   // entry ``lane`` of the row
        for (int j = 0; j < k; ++j) {
            unsigned long long best = 0ull;
            if (res) {
#pragma unroll
                for (int i = 0; i < TOPK_SLOTS; ++i)
                    if (key[i] < prev && key[i] > best) best = key[i];
            } else {
                for (int c = lane; c < C; c += WAVE) {
                    const unsigned long long q = rank_key(ld1t(r + c), c);
                    if (q < prev && q > best) best = q;
                }
            }
            best = wave_max_u64(best);
            if (best == 0ull) break;  // the row has no more classes: entries j .. k - 1 stay "no class"
            if (lane == j) mine = best;
            prev = best;
        }
        float lse;
        ce_row_plain<float, true, false, T>(r, C, 0, -1, 0.f, 0.f, lse, nullptr, lane);
        if (lane < k) {
            const long long c = mine ? (long long)(0xffffffffu - (unsigned)mine) : -1;
            reinterpret_cast<long long*>(t.idx)[(long long)row * t.idx_row_stride + lane] = c;
            if (t.prob) t.prob[(long long)row * t.prob_row_stride + lane] = mine ? expf(ld1t(r + (mine ? c : 0)) - lse) : 0.f;
        }
        if (t.lse && lane == 0) t.lse[row] = lse;
    }
}

template <typename T>
static void topk_launch(hipStream_t s, int grid, const TopkTasks& P, int count, int rows, int k) {
    hipLaunchKernelGGL(topk_softmax_kernel<T>, dim3(grid), dim3(256), 0, s, P, count, rows, k);
}

}  // namespace egk

using namespace egk;

extern "C" {

int egk_label_rank(egk_stream_t stream, const float* logits, int64_t ld, const int64_t* labels, int64_t label_stride,
                   int32_t* rank, int32_t rows, int32_t C) {
    EGK_REQUIRE(logits && labels && rank, "egk_label_rank: null pointer");
    EGK_REQUIRE(C >= 1 && ld >= C, "egk_label_rank: bad class count / leading dimension");
    if (rows == 0) return 0;
    hipStream_t s = (hipStream_t)stream;
    int grid = cdiv(rows, 4);
    if (grid > 2048) grid = 2048;
    hipLaunchKernelGGL(label_rank_kernel, dim3(grid), dim3(256), 0, s, logits, (long long)ld, (const long long*)labels,
                       (long long)label_stride, rank, rows, C);
    return check_launch("egk_label_rank");
}

int egk_edit_distance(egk_stream_t stream, const int64_t* pred, int64_t p_sn, int64_t p_sz, int64_t p_sk, const int64_t* label,
                      int64_t l_sn, int64_t l_sz, int32_t* out, int32_t N, int32_t Z, int32_t K) {
    EGK_REQUIRE(pred && label && out, "egk_edit_distance: null pointer");
    EGK_REQUIRE(Z >= 0 && Z <= 64, "egk_edit_distance: sequence length %d > 64 unsupported", Z);
    if (N == 0 || K == 0) return 0;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(edit_distance_kernel, dim3(cdiv(N * K, 64)), dim3(64), 0, s, (const long long*)pred, (long long)p_sn,
                       (long long)p_sz, (long long)p_sk, (const long long*)label, (long long)l_sn, (long long)l_sz, out, N, Z, K);
    return check_launch("egk_edit_distance");
}

int egk_class_report(egk_stream_t stream, const egk_class_report_task* tasks, int32_t count) {
    EGK_REQUIRE(tasks, "egk_class_report: null task list");
    EGK_REQUIRE(count >= 1 && count <= EGK_CLASS_REPORT_MAX_TASKS, "egk_class_report: 1 .. %d tasks (got %d)",
                EGK_CLASS_REPORT_MAX_TASKS, count);
    ClassReportTasks P{};
    int max_rows = 0;
    double bytes = 0;
    for (int i = 0; i < count; ++i) {
        const egk_class_report_task& t = tasks[i];
        EGK_REQUIRE(t.logits && t.labels && t.confusion && t.counts, "egk_class_report: null pointer (task %d)", i);
        EGK_REQUIRE(t.C >= 1 && t.ld >= t.C, "egk_class_report: bad class count / leading dimension (task %d: C %d, ld %lld)", i, t.C,
                    (long long)t.ld);
        EGK_REQUIRE(t.rows >= 0, "egk_class_report: rows >= 0 (task %d: %d)", i, t.rows);
        EGK_REQUIRE(aligned_to(4u, {t.logits}) && aligned_to(8u, {t.labels, t.confusion, t.top2, t.loss_q24, t.counts}),
                    "egk_class_report: misaligned pointer (task %d: logits 4-byte, labels and the int64 accumulators 8-byte)", i);
        P.t[i] = t;
        if (t.rows > max_rows) max_rows = t.rows;
        bytes += 8.0 * t.rows * t.C + 8.0 * t.rows;
    }
    if (max_rows == 0) return 0;
    hipStream_t s = (hipStream_t)stream;
    ProfScope prof(KID_CLASS_REPORT, s, 0, bytes);
    int grid = cdiv(max_rows, 4);
    if (grid > 2048) grid = 2048;
    hipLaunchKernelGGL(class_report_kernel, dim3(grid, count), dim3(256), 0, s, P);
    return check_launch("egk_class_report");
}

int egk_topk_softmax(egk_stream_t stream, const egk_topk_task* tasks, int32_t count, int32_t rows, int32_t k, int32_t dtype) {
    EGK_REQUIRE(tasks, "egk_topk_softmax: null task list");
    EGK_REQUIRE(count >= 1 && count <= EGK_TOPK_MAX_TASKS, "egk_topk_softmax: 1 .. %d tasks (got %d)", EGK_TOPK_MAX_TASKS, count);
    EGK_REQUIRE(rows >= 0, "egk_topk_softmax: rows >= 0 (got %d)", rows);
    EGK_REQUIRE(k >= 1 && k <= EGK_TOPK_MAX_K, "egk_topk_softmax: k in 1 .. %d (got %d)", EGK_TOPK_MAX_K, k);
    EGK_REQUIRE(dtype == EGK_F32 || dtype == EGK_BF16, "egk_topk_softmax: unknown logits dtype %d", dtype);
    TopkTasks P{};
    double bytes = 0;
    for (int i = 0; i < count; ++i) {
        const egk_topk_task& t = tasks[i];
        EGK_REQUIRE(t.logits && t.idx, "egk_topk_softmax: null pointer (task %d)", i);
        EGK_REQUIRE(t.C >= 1 && t.ld >= t.C, "egk_topk_softmax: bad class count / leading dimension (task %d: C %d, ld %lld)", i, t.C,
                    (long long)t.ld);
        EGK_REQUIRE(t.reserved == 0, "egk_topk_softmax: the reserved field is 0 (task %d: %d)", i, t.reserved);
        EGK_REQUIRE(t.idx_row_stride >= k, "egk_topk_softmax: idx row stride >= k (task %d: %lld, k %d)", i, (long long)t.idx_row_stride, k);
        EGK_REQUIRE(!t.prob || t.prob_row_stride >= k, "egk_topk_softmax: prob row stride >= k (task %d: %lld, k %d)", i,
                    (long long)t.prob_row_stride, k);
        EGK_REQUIRE(aligned_to(dtype == EGK_BF16 ? 2u : 4u, {t.logits}) && aligned_to(8u, {t.idx}) && aligned_to(4u, {t.prob, t.lse}),
                    "egk_topk_softmax: misaligned pointer (task %d: logits to their element, idx 8-byte, prob and lse 4-byte)", i);
        P.t[i] = t;
        const double es = dtype == EGK_BF16 ? 2 : 4;
        const double passes = t.C > TOPK_RES ? (double)(k < t.C ? k : t.C) + 2 : 3;  // (the keys -- once, or once per entry --, the maximum, the sum)
        bytes += (double)rows * (t.C * es * passes + (t.prob ? (es + 4.0) * k : 0) + 8.0 * k + (t.lse ? 4 : 0));
    }
    if (rows == 0) return 0;
    hipStream_t s = (hipStream_t)stream;
    ProfScope prof(KID_TOPK_SOFTMAX, s, 0, bytes);
    int grid = cdiv((int64_t)count * rows, 4);
    if (grid > 2048) grid = 2048;
    EGK_DISPATCH_T(dtype, (topk_launch<T>(s, grid, P, (int)count, (int)rows, (int)k)));
    return check_launch("egk_topk_softmax");
}

}  // extern "C"
