// Seeded categorical sampling (include/egopack_sample.h): K class indices per logits row from softmax(row), every random bit a
// function of (seed, batch ordinal, row, head, sample index) through the library's Philox4x32-10 (common.h).
//   egk_categorical_sample   the K = 5 futures of the LTA heads (reference models/tasks/lta.py:60-66: Categorical(logits).sample()
//                            K times per head), all heads in one launch
// One wave per (task, row).  A lane owns 8 CONSECUTIVE classes of a 512-class chunk, so that the inclusive prefix sum is a serial
// sum inside the lane, one wave scan of the lane totals and a carry from chunk to chunk; a row of up to 512 classes (the workload's
// 115 and 478) is read once and stays in registers, a wider row is read once per pass.  No LDS, no workspace, no atomics.
#include "common.h"

namespace egk {

constexpr int SAMPLE_LANE = 8;                    // classes per lane
constexpr int SAMPLE_CHUNK = WAVE * SAMPLE_LANE;  // classes per chunk

struct SampleTasks {
    egk_sample_task t[EGK_SAMPLE_MAX_TASKS];
};

// the lane's 8 classes of chunk ``ch``; -inf beyond C (a dead class: e = 0 exactly), so columns >= C are never read
template <typename T>
__device__ __forceinline__ void sample_load(const T* __restrict__ r, int ch, int lane, int C, float (&x)[SAMPLE_LANE]) {
    const int c0 = ch * SAMPLE_CHUNK + lane * SAMPLE_LANE;
#pragma unroll
    for (int j = 0; j < SAMPLE_LANE; ++j) x[j] = c0 + j < C ? ld1t(r + c0 + j) : -INFINITY;
}

// e_j = expf(x_j - m) and the inclusive prefix sums P_j of the chunk on top of ``carry`` (the P of the class before the chunk).
// Called with the same arguments in the sum pass and in the selection pass of a multi-chunk row: the same bits both times.
__device__ __forceinline__ void sample_scan(const float (&x)[SAMPLE_LANE], float m, float carry, int lane, float (&e)[SAMPLE_LANE],
                                            float (&P)[SAMPLE_LANE]) {
    float l[SAMPLE_LANE];
    float run = 0.f;
#pragma unroll
    for (int j = 0; j < SAMPLE_LANE; ++j) {
        e[j] = expf(x[j] - m);
        run += e[j];
        l[j] = run;
    }
    float inc = run;  // inclusive scan of the lane totals
#pragma unroll
    for (int o = 1; o < WAVE; o <<= 1) {
        const float v = __shfl_up(inc, o, WAVE);
        if (lane >= o) inc += v;
    }
    float excl = __shfl_up(inc, 1, WAVE);
    if (lane == 0) excl = 0.f;
    const float base = carry + excl;
#pragma unroll
    for (int j = 0; j < SAMPLE_LANE; ++j) P[j] = base + l[j];
}

// P of the live class in front of class (lane L, slot j) -- L and j wave-uniform: the nearest live slot below j in lane L, else the
// last live class of the nearest lane below L that has one, else ``before`` (the last live P of the chunks in front; 0 at the start).
__device__ __forceinline__ float sample_prev_live(int L, int j, const float (&P)[SAMPLE_LANE], unsigned live, float lane_last_p,
                                                  float before) {
    const unsigned below = live & ((1u << j) - 1u);
    float mine = 0.f;  // (constant indices only: a register array that is indexed at run time is moved out of the registers)
#pragma unroll
    for (int i = 0; i < SAMPLE_LANE; ++i)
        if ((below >> i) & 1u) mine = P[i];
    const int has = __shfl((int)(below != 0u), L, WAVE);
    const float lo = __shfl(mine, L, WAVE);
    if (has) return lo;
    const unsigned long long lanes = __ballot(live != 0u) & ((1ull << L) - 1ull);
    const float other = __shfl(lane_last_p, lanes ? 63 - __clzll(lanes) : 0, WAVE);
    return lanes ? other : before;
}

__device__ __forceinline__ float sample_t(float u, float S) {
#pragma clang fp contract(off)  // t = fl32(u * S): the one product the host recomputes
    return u * S;
}

template <typename T>
__global__ __launch_bounds__(256) void categorical_sample_kernel(SampleTasks tasks, int count, int rows, int K, uint64_t seed,
                                                                 uint64_t ordinal, uint64_t row0) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long items = (long long)count * rows;
    for (long long item = (long long)blockIdx.x * 4 + wave; item < items; item += (long long)gridDim.x * 4) {
        const int ti = (int)(item / rows), row = (int)(item % rows);
        const egk_sample_task& tk = tasks.t[ti];
        const int C = tk.C;
        const T* r = reinterpret_cast<const T*>(tk.logits) + (long long)row * tk.ld;
        long long* out = reinterpret_cast<long long*>(tk.out) + (long long)row * tk.out_row_stride;
        const long long ks = tk.out_k_stride;
        const bool dbg = tk.total != nullptr;
        float* lo_o = dbg ? tk.lo + (long long)row * K : nullptr;
        float* hi_o = dbg ? tk.hi + (long long)row * K : nullptr;
        float* to_o = dbg ? tk.total + (long long)row * K : nullptr;
        const int nch = (C + SAMPLE_CHUNK - 1) / SAMPLE_CHUNK;

        // ---- pass 1: the maximum, and whether the row holds a NaN
        float x[SAMPLE_LANE];
        float m = -INFINITY;
        bool nan = false;
        for (int ch = 0; ch < nch; ++ch) {
            sample_load(r, ch, lane, C, x);
#pragma unroll
            for (int j = 0; j < SAMPLE_LANE; ++j) {
                m = fmaxf(m, x[j]);
                nan = nan || x[j] != x[j];
            }
        }
        m = wave_max(m);
        if (__ballot(nan) != 0ull || !(fabsf(m) < INFINITY)) {  // nothing to sample from: -1, and the row is not read again
            for (int k = lane; k < K; k += WAVE) {
                out[(long long)k * ks] = -1;
                if (dbg) lo_o[k] = hi_o[k] = to_o[k] = 0.f;
            }
            continue;
        }

        // ---- pass 2: S = P_{C-1} (a row of one chunk keeps x, e and P in registers for pass 3)
        float e[SAMPLE_LANE], P[SAMPLE_LANE];
        float carry = 0.f, S = 0.f;
        for (int ch = 0; ch < nch; ++ch) {
            if (nch > 1) sample_load(r, ch, lane, C, x);
            sample_scan(x, m, carry, lane, e, P);
            carry = __shfl(P[SAMPLE_LANE - 1], WAVE - 1, WAVE);
            if (ch == nch - 1) {
                const int last = C - 1 - ch * SAMPLE_CHUNK;
                float p_last = 0.f;
#pragma unroll
                for (int j = 0; j < SAMPLE_LANE; ++j)
                    if (j == last % SAMPLE_LANE) p_last = P[j];
                S = __shfl(p_last, last / SAMPLE_LANE, WAVE);
            }
        }

        // ---- pass 3: the K selections, chunk by chunk.  Sample k is settled in the first chunk that holds a live class with P > t;
        // its flag is bit (k >> 6) of lane (k & 63)'s ``found``.  (last_c, last_p, last2_p): the last live class seen so far, its P
        // and the P of the live class in front of it -- the fallback's answer, and the ``before`` of the next chunk.
        const uint64_t ctr0 = (ordinal << 40) | ((row0 + (uint64_t)row) << 16) | ((uint64_t)(unsigned)tk.head << 8);
        unsigned found = 0u;
        int last_c = -1;
        float last_p = 0.f, last2_p = 0.f;
        carry = 0.f;
        for (int ch = 0; ch < nch; ++ch) {
            if (nch > 1) {
                sample_load(r, ch, lane, C, x);
                sample_scan(x, m, carry, lane, e, P);
                carry = __shfl(P[SAMPLE_LANE - 1], WAVE - 1, WAVE);
            }
            unsigned live = 0u;
            float lane_last_p = 0.f;
#pragma unroll
            for (int j = 0; j < SAMPLE_LANE; ++j)
                if (e[j] > 0.f) {
                    live |= 1u << j;
                    lane_last_p = P[j];
                }
            uint4 w = make_uint4(0u, 0u, 0u, 0u);
            for (int k = 0; k < K; ++k) {
                if ((k & 3) == 0) w = philox4x32_10(ctr0 | (uint64_t)(k >> 2), seed);
                if ((__shfl((int)found, k & 63, WAVE) >> (k >> 6)) & 1) continue;
                const uint32_t word = (k & 3) == 0 ? w.x : (k & 3) == 1 ? w.y : (k & 3) == 2 ? w.z : w.w;
                const float t = sample_t(u01(word), S);
                int jsel = -1;
                float psel = 0.f;
#pragma unroll
                for (int j = SAMPLE_LANE - 1; j >= 0; --j)
                    if (((live >> j) & 1u) && P[j] > t) {
                        jsel = j;
                        psel = P[j];
                    }
                const unsigned long long hit = __ballot(jsel >= 0);
                if (hit == 0ull) continue;
                const int L = __ffsll((long long)hit) - 1;
                const int j = __shfl(jsel, L, WAVE);
                const float hi = __shfl(psel, L, WAVE);
                if (lane == (k & 63)) found |= 1u << (k >> 6);
                float lo = 0.f;
                if (dbg) lo = sample_prev_live(L, j, P, live, lane_last_p, last_p);
                if (lane == 0) {
                    out[(long long)k * ks] = (long long)ch * SAMPLE_CHUNK + L * SAMPLE_LANE + j;
                    if (dbg) {
                        lo_o[k] = lo;
                        hi_o[k] = hi;
                        to_o[k] = S;
                    }
                }
            }
            const unsigned long long lanes = __ballot(live != 0u);
            if (lanes) {
                const int L = 63 - __clzll(lanes);
                const int j = __shfl(live ? 31 - __clz(live) : 0, L, WAVE);
                last2_p = sample_prev_live(L, j, P, live, lane_last_p, last_p);
                last_p = __shfl(lane_last_p, L, WAVE);
                last_c = ch * SAMPLE_CHUNK + L * SAMPLE_LANE + j;
            }
        }
        // ---- the fallback: rounding left no live class with P > t (the class of the maximum is live: last_c >= 0)
        for (int k = 0; k < K; ++k) {
            if ((__shfl((int)found, k & 63, WAVE) >> (k >> 6)) & 1) continue;
            if (lane == 0) {
                out[(long long)k * ks] = last_c;
                if (dbg) {
                    lo_o[k] = last2_p;
                    hi_o[k] = last_p;
                    to_o[k] = S;
                }
            }
        }
    }
}

template <typename T>
static void sample_launch(hipStream_t s, int grid, const SampleTasks& st, int count, int rows, int K, uint64_t seed, uint64_t ordinal,
                          uint64_t row0) {
    hipLaunchKernelGGL(categorical_sample_kernel<T>, dim3(grid), dim3(256), 0, s, st, count, rows, K, seed, ordinal, row0);
}

}  // namespace egk

using namespace egk;

extern "C" {

int egk_categorical_sample(egk_stream_t stream, const egk_sample_task* tasks, int32_t count, int32_t rows, int32_t K, uint64_t seed,
                           int64_t ordinal, int64_t row0, int32_t dtype) {
    const int64_t lim = (int64_t)1 << 24;
    EGK_REQUIRE(tasks, "egk_categorical_sample: null task list");
    EGK_REQUIRE(count >= 1 && count <= EGK_SAMPLE_MAX_TASKS, "egk_categorical_sample: 1 .. %d tasks (got %d)", EGK_SAMPLE_MAX_TASKS, count);
    EGK_REQUIRE(rows >= 0, "egk_categorical_sample: rows >= 0 (got %d)", rows);
    EGK_REQUIRE(K >= 1 && K <= EGK_SAMPLE_MAX_K, "egk_categorical_sample: K in 1 .. %d (got %d)", EGK_SAMPLE_MAX_K, K);
    EGK_REQUIRE(ordinal >= 0 && ordinal < lim, "egk_categorical_sample: batch ordinal in [0, 2^24) (got %lld)", (long long)ordinal);
    EGK_REQUIRE(row0 >= 0 && row0 + rows <= lim, "egk_categorical_sample: rows [row0, row0 + rows) inside [0, 2^24) (got row0 %lld, rows %d)",
                (long long)row0, rows);
    EGK_REQUIRE(dtype == EGK_F32 || dtype == EGK_BF16, "egk_categorical_sample: unknown logits dtype %d", dtype);
    SampleTasks st{};
    for (int i = 0; i < count; ++i) {
        const egk_sample_task& t = tasks[i];
        EGK_REQUIRE(t.logits && t.out, "egk_categorical_sample: null pointer (task %d)", i);
        EGK_REQUIRE(t.C >= 1 && t.ld >= t.C, "egk_categorical_sample: bad class count / leading dimension (task %d: C %d, ld %lld)", i, t.C,
                    (long long)t.ld);
        EGK_REQUIRE(t.head >= 0 && t.head < 256, "egk_categorical_sample: head index in [0, 256) (task %d: %d)", i, t.head);
        EGK_REQUIRE(t.out_row_stride >= 0 && t.out_k_stride >= 0, "egk_categorical_sample: negative output stride (task %d)", i);
        EGK_REQUIRE((t.lo && t.hi && t.total) || (!t.lo && !t.hi && !t.total),
                    "egk_categorical_sample: lo / hi / total are given together or not at all (task %d)", i);
        EGK_REQUIRE(aligned_to(dtype == EGK_BF16 ? 2u : 4u, {t.logits}) && aligned_to(8u, {t.out}) && aligned_to(4u, {t.lo, t.hi, t.total}),
                    "egk_categorical_sample: misaligned pointer (task %d)", i);
        st.t[i] = t;
    }
    if (rows == 0) return 0;
    hipStream_t s = (hipStream_t)stream;
    double bytes = 0;
    for (int i = 0; i < count; ++i)
        bytes += (double)rows * ((double)tasks[i].C * (dtype == EGK_BF16 ? 2 : 4) * (tasks[i].C > SAMPLE_CHUNK ? 3 : 1) + 8.0 * K);
    ProfScope prof(KID_CATEGORICAL_SAMPLE, s, 0, bytes);
    int grid = cdiv((int64_t)count * rows, 4);
    if (grid > 2048) grid = 2048;
    EGK_DISPATCH_T(dtype, (sample_launch<T>(s, grid, st, (int)count, (int)rows, (int)K, seed, (uint64_t)ordinal, (uint64_t)row0)));
    return check_launch("egk_categorical_sample");
}

}  // extern "C"
