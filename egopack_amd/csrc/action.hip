// Action-level scores of the verb / noun heads (include/egopack_action.h): an action is the pair (verb, noun)
//   egk_action_topk          the best k pairs of every row under the product of the two heads' softmaxes, their scores, both
//                            log-sum-exps and the exact rank of the labelled pair, in one launch
//   egk_edit_distance_pairs  verb, noun and action Levenshtein distances of the K sampled futures in one launch
// Plain C++: one wave per row, four waves per workgroup, at most 2048 workgroups with a strided row loop (egk_topk_softmax's walk);
// no LDS, no workspace, no atomics.  The order of a head is rank_key's (rank_key.h), the log-sum-exp is the loss kernels' row
// function (ce_row.h) or, at a temperature, its sibling (temp_row.h): one definition of each.  Every launcher refuses its argument
// errors on the host before it launches.
#include "ce_row.h"
#include "common.h"
#include "rank_key.h"
#include "temp_row.h"

namespace egk {

struct ActionArgs {
    const void* zv;
    const void* zn;
    long long ld_v, ld_n;
    int Cv, Cn;
    const float* beta;
    const long long* yv;
    const long long* yn;
    long long syv, syn;
    int rows, k;
    long long* pair;
    long long pair_stride;
    float* logp;
    float* prob;
    long long out_stride;
    float* lse;
    int* rank;
};

// the value part of rank_key: the score's place in the order as one unsigned (NaN -> 0, below -inf; -0 and +0 share one)
__device__ __forceinline__ unsigned score_key(float s) { return (unsigned)(rank_key(s, 0) >> 32); }

// x = z, or fl(beta z) as ONE separately rounded product (temp_scaled)
__device__ __forceinline__ float action_x(bool scaled, float beta, float z) { return scaled ? temp_scaled(beta, z) : z; }

// Entry j of the order of N keys per lane (key_of(i): this lane's i-th key, 0 = none; no two keys of the wave are equal), kept by
// lane j, for j < k <= 64: pass j takes the wave-wide maximum of the keys below the winner of pass j - 1 (topk_softmax_kernel's
// passes).  0 where the wave has fewer than j + 1 keys.
template <int N, typename F>
__device__ __forceinline__ unsigned long long select_k(F key_of, int k, int lane) {
    unsigned long long prev = ~0ull, mine = 0ull;
    for (int j = 0; j < k; ++j) {
        unsigned long long best = 0ull;
#pragma unroll
        for (int i = 0; i < N; ++i) {
            const unsigned long long q = key_of(i);
            if (q < prev && q > best) best = q;
        }
        best = wave_max_u64(best);
        if (best == 0ull) break;
        if (lane == j) mine = best;
        prev = best;
    }
    return mine;
}

// SLOTS: registers per lane and head (class lane + 64 * i in slot i), so C <= 64 * SLOTS; CS: candidate pairs per lane, so
// min(k, Cv) * min(k, Cn) <= 64 * CS.  Positions inside the heads' best-k lists are below 32 (k <= EGK_ACTION_MAX_K), so a
// candidate's place in rules 2 and 3 is the integer 32 * (verb position) + (noun position), the smaller the better.
template <typename T, int SLOTS, int CS>
__global__ __launch_bounds__(256) void action_topk_kernel(const ActionArgs A) {
#pragma clang fp contract(off)
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int Cv = A.Cv, Cn = A.Cn, k = A.k;
    const bool scaled = A.beta != nullptr;
    const float bv = scaled ? A.beta[0] : 1.f, bn = scaled ? A.beta[1] : 1.f;
    const int Kv = k < Cv ? k : Cv, Kn = k < Cn ? k : Cn, ncand = Kv * Kn;
    const float none[TEMP_SLOTS] = {};
    for (int row = blockIdx.x * 4 + wave; row < A.rows; row += gridDim.x * 4) {
        const T* __restrict__ rv = reinterpret_cast<const T*>(A.zv) + (long long)row * A.ld_v;
        const T* __restrict__ rn = reinterpret_cast<const T*>(A.zn) + (long long)row * A.ld_n;
        float xv[SLOTS], xn[SLOTS];
#pragma unroll
        for (int i = 0; i < SLOTS; ++i) {
            const int c = lane + WAVE * i;
            xv[i] = c < Cv ? action_x(scaled, bv, ld1t(rv + c)) : 0.f;
            xn[i] = c < Cn ? action_x(scaled, bn, ld1t(rn + c)) : 0.f;
        }
        float lse_v, lse_n;
        if (scaled) {
            lse_v = temp_row_lse<T, false>(rv, Cv, bv, none, lane);
            lse_n = temp_row_lse<T, false>(rn, Cn, bn, none, lane);
        } else {
            ce_row_plain<float, true, false, T>(rv, Cv, 0, -1, 0.f, 0.f, lse_v, nullptr, lane);
            ce_row_plain<float, true, false, T>(rn, Cn, 0, -1, 0.f, 0.f, lse_n, nullptr, lane);
        }
        // the heads' best min(k, C) classes: lane j holds entry j of each head with its log-probability
        const unsigned long long hv = select_k<SLOTS>([&](int i) { const int c = lane + WAVE * i; return c < Cv ? rank_key(xv[i], c) : 0ull; }, Kv, lane);
        const unsigned long long hn = select_k<SLOTS>([&](int i) { const int c = lane + WAVE * i; return c < Cn ? rank_key(xn[i], c) : 0ull; }, Kn, lane);
        const int cv = hv ? (int)(0xffffffffu - (unsigned)hv) : -1, cn = hn ? (int)(0xffffffffu - (unsigned)hn) : -1;
        const float av = cv >= 0 ? action_x(scaled, bv, ld1t(rv + cv)) - lse_v : 0.f;
        const float an = cn >= 0 ? action_x(scaled, bn, ld1t(rn + cn)) - lse_n : 0.f;
        // the candidates: (verb position i, noun position j) for i < Kv, j < Kn, candidate q = i * Kn + j in lane q % 64
        unsigned long long cand[CS];
#pragma unroll
        for (int t = 0; t < CS; ++t) {
            const int q = lane + WAVE * t;
            const bool live = q < ncand;
            const int i = live ? q / Kn : 0, j = live ? q % Kn : 0;
            const float s = __shfl(av, i, 64) + __shfl(an, j, 64);
            cand[t] = live ? ((unsigned long long)score_key(s) << 32) | (unsigned long long)(0xffffffffu - (unsigned)(i * 32 + j)) : 0ull;
        }
        const unsigned long long mine = select_k<CS>([&](int t) { return cand[t]; }, k, lane);
        {
            const unsigned pos = mine ? 0xffffffffu - (unsigned)mine : 0u;
            const int i = (int)(pos >> 5), j = (int)(pos & 31u);
            const int pv = __shfl(cv, i, 64), pn = __shfl(cn, j, 64);
            const float s = __shfl(av, i, 64) + __shfl(an, j, 64);
            if (lane < k) {
                long long* __restrict__ p = A.pair + (long long)row * A.pair_stride + 2 * lane;
                p[0] = mine ? (long long)pv : -1;
                p[1] = mine ? (long long)pn : -1;
                if (A.logp) A.logp[(long long)row * A.out_stride + lane] = mine ? s : -INFINITY;
                if (A.prob) A.prob[(long long)row * A.out_stride + lane] = mine ? expf(s) : 0.f;
            }
        }
        if (A.lse && lane == 0) {
            A.lse[2 * (long long)row] = lse_v;
            A.lse[2 * (long long)row + 1] = lse_n;
        }
        if (!A.rank) continue;
        // the exact rank of the labelled pair: every pair is scored -- the verbs one after the other, broadcast from the lane that
        // holds them, against this lane's nouns -- and counted if it outranks the label's
        const long long yv = A.yv[(long long)row * A.syv], yn = A.yn[(long long)row * A.syn];
        if (yv < 0 || yv >= Cv || yn < 0 || yn >= Cn) {
            if (lane == 0) A.rank[row] = -1;
            continue;
        }
        const float xyv = action_x(scaled, bv, ld1t(rv + yv)), xyn = action_x(scaled, bn, ld1t(rn + yn));
        const unsigned ky = score_key((xyv - lse_v) + (xyn - lse_n));
        const unsigned long long kyv = rank_key(xyv, (int)yv), kyn = rank_key(xyn, (int)yn);
        float lpn[SLOTS];            // this lane's noun log-probabilities
        unsigned nlive = 0, ngt = 0;  // bit j: slot j holds a noun; that noun outranks the labelled noun in the head's order
#pragma unroll
        for (int j = 0; j < SLOTS; ++j) {
            const int c = lane + WAVE * j;
            lpn[j] = xn[j] - lse_n;
            if (c < Cn) {
                nlive |= 1u << j;
                if (rank_key(xn[j], c) > kyn) ngt |= 1u << j;
            }
        }
        int cnt = 0;
#pragma unroll
        for (int i = 0; i < SLOTS; ++i) {
            const int c = lane + WAVE * i;
            const float lpv = xv[i] - lse_v;
            const unsigned long long vgt = __ballot(c < Cv && rank_key(xv[i], c) > kyv);  // (wave-uniform)
            const int n = Cv - WAVE * i < WAVE ? Cv - WAVE * i : WAVE;  // (<= 0 beyond the row: no pass)
            for (int l = 0; l < n; ++l) {
                const float a = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(lpv), l));
                const bool vg = (vgt >> l) & 1ull, ve = WAVE * i + l == (int)yv;
#pragma unroll
                for (int j = 0; j < SLOTS; ++j) {
                    if (WAVE * j < Cn) {  // (wave-uniform)
                        const unsigned ks = score_key(a + lpn[j]);
                        const bool tie = vg || (ve && ((ngt >> j) & 1u));
                        cnt += (((nlive >> j) & 1u) && (ks > ky || (ks == ky && tie))) ? 1 : 0;
                    }
                }
            }
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o, 64);
        if (lane == 0) A.rank[row] = cnt;
    }
}

template <typename T>
static void action_topk_launch(hipStream_t s, int grid, const ActionArgs& A) {
    const bool wide = A.Cv > WAVE * 8 || A.Cn > WAVE * 8, many = A.k > 8;  // (k <= 8: at most 64 candidates, one per lane)
    if (!wide && !many) hipLaunchKernelGGL((action_topk_kernel<T, 8, 1>), dim3(grid), dim3(256), 0, s, A);
    else if (!wide) hipLaunchKernelGGL((action_topk_kernel<T, 8, 16>), dim3(grid), dim3(256), 0, s, A);
    else if (!many) hipLaunchKernelGGL((action_topk_kernel<T, 16, 1>), dim3(grid), dim3(256), 0, s, A);
    else hipLaunchKernelGGL((action_topk_kernel<T, 16, 16>), dim3(grid), dim3(256), 0, s, A);
}

// one thread per (sequence n, future k): three single-row dynamic programmes (edit_distance_kernel's, metrics.hip) over Z <= 64
// positions that share the loads of the prediction and of the labels
__global__ __launch_bounds__(64) void edit_distance_pairs_kernel(const long long* __restrict__ pred_v, const long long* __restrict__ pred_n,
                                                                 long long p_sn, long long p_sz, long long p_sk,
                                                                 const long long* __restrict__ label_v, const long long* __restrict__ label_n,
                                                                 long long l_sn, long long l_sz, int* __restrict__ out, int N, int Z, int K) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= N * K) return;
    const int n = idx / K, k = idx % K;
    int dv[65], dn[65], da[65];
    for (int j = 0; j <= Z; ++j) dv[j] = dn[j] = da[j] = j;
    for (int i = 1; i <= Z; ++i) {
        const long long po = n * p_sn + (long long)(i - 1) * p_sz + k * p_sk;
        const long long av = pred_v[po], an = pred_n[po];
        int gv = dv[0], gn = dn[0], ga = da[0];  // the diagonals
        dv[0] = dn[0] = da[0] = i;
        for (int j = 1; j <= Z; ++j) {
            const long long lo = n * l_sn + (long long)(j - 1) * l_sz;
            const bool ev = av == label_v[lo], en = an == label_n[lo];
            const int sv = gv + (ev ? 0 : 1), sn = gn + (en ? 0 : 1), sa = ga + (ev && en ? 0 : 1);
            gv = dv[j];
            gn = dn[j];
            ga = da[j];
            dv[j] = min(sv, min(dv[j] + 1, dv[j - 1] + 1));
            dn[j] = min(sn, min(dn[j] + 1, dn[j - 1] + 1));
            da[j] = min(sa, min(da[j] + 1, da[j - 1] + 1));
        }
    }
    out[3 * (long long)idx + 0] = dv[Z];
    out[3 * (long long)idx + 1] = dn[Z];
    out[3 * (long long)idx + 2] = da[Z];
}

}  // namespace egk

using namespace egk;

extern "C" {

int egk_action_topk(egk_stream_t stream, const void* verb_logits, int64_t ld_v, int32_t Cv, const void* noun_logits, int64_t ld_n,
                    int32_t Cn, const float* beta, const int64_t* verb_labels, int64_t verb_label_stride, const int64_t* noun_labels,
                    int64_t noun_label_stride, int32_t rows, int32_t k, int64_t* pair, int64_t pair_row_stride, float* logp, float* prob,
                    int64_t out_row_stride, float* lse, int32_t* rank, int32_t dtype) {
    EGK_REQUIRE(verb_logits, "egk_action_topk: null pointer (verb_logits)");
    EGK_REQUIRE(noun_logits, "egk_action_topk: null pointer (noun_logits)");
    EGK_REQUIRE(pair, "egk_action_topk: null pointer (pair)");
    EGK_REQUIRE(!verb_labels == !noun_labels, "egk_action_topk: verb_labels and noun_labels are both NULL or both given");
    EGK_REQUIRE(!rank || verb_labels, "egk_action_topk: rank requires the labels");
    EGK_REQUIRE(!verb_labels || rank, "egk_action_topk: the labels are given for rank, which is NULL");
    EGK_REQUIRE(rows >= 0, "egk_action_topk: rows >= 0 (got %d)", rows);
    EGK_REQUIRE(k >= 1 && k <= EGK_ACTION_MAX_K, "egk_action_topk: k in 1 .. %d (got %d)", EGK_ACTION_MAX_K, k);
    EGK_REQUIRE(Cv >= 1 && Cv <= EGK_ACTION_MAX_C, "egk_action_topk: Cv in 1 .. %d (got %d)", EGK_ACTION_MAX_C, Cv);
    EGK_REQUIRE(Cn >= 1 && Cn <= EGK_ACTION_MAX_C, "egk_action_topk: Cn in 1 .. %d (got %d)", EGK_ACTION_MAX_C, Cn);
    EGK_REQUIRE(ld_v >= Cv, "egk_action_topk: ld_v >= Cv (ld_v %lld, Cv %d)", (long long)ld_v, Cv);
    EGK_REQUIRE(ld_n >= Cn, "egk_action_topk: ld_n >= Cn (ld_n %lld, Cn %d)", (long long)ld_n, Cn);
    EGK_REQUIRE(pair_row_stride >= 2 * (int64_t)k, "egk_action_topk: pair row stride >= 2 k (got %lld, k %d)", (long long)pair_row_stride, k);
    EGK_REQUIRE(!(logp || prob) || out_row_stride >= k, "egk_action_topk: logp / prob row stride >= k (got %lld, k %d)",
                (long long)out_row_stride, k);
    EGK_REQUIRE(dtype == EGK_F32 || dtype == EGK_BF16, "egk_action_topk: unknown logits dtype %d", dtype);
    EGK_REQUIRE(aligned_to(dtype == EGK_BF16 ? 2u : 4u, {verb_logits, noun_logits}), "egk_action_topk: misaligned logits (to their element)");
    EGK_REQUIRE(aligned_to(8u, {pair}), "egk_action_topk: misaligned pair (8-byte)");
    EGK_REQUIRE(aligned_to(8u, {verb_labels, noun_labels}), "egk_action_topk: misaligned labels (8-byte)");
    EGK_REQUIRE(aligned_to(4u, {beta, logp, prob, lse, rank}), "egk_action_topk: misaligned beta, logp, prob, lse or rank (4-byte)");
    if (rows == 0) return 0;
    hipStream_t s = (hipStream_t)stream;
    ActionArgs A{verb_logits, noun_logits, (long long)ld_v, (long long)ld_n, (int)Cv, (int)Cn, beta, (const long long*)verb_labels,
                 (const long long*)noun_labels, (long long)verb_label_stride, (long long)noun_label_stride, (int)rows, (int)k,
                 (long long*)pair, (long long)pair_row_stride, logp, prob, (long long)out_row_stride, lse, rank};
    const double es = dtype == EGK_BF16 ? 2 : 4;
    ProfScope prof(KID_ACTION_TOPK, s, rank ? (double)rows * Cv * Cn : 0.0,
                   (double)rows * ((Cv + Cn) * es * 3 + 16.0 * k + (logp ? 4.0 * k : 0) + (prob ? 4.0 * k : 0) + (lse ? 8 : 0) + (rank ? 20 : 0)));
    int grid = cdiv(rows, 4);
    if (grid > 2048) grid = 2048;
    EGK_DISPATCH_T(dtype, (action_topk_launch<T>(s, grid, A)));
    return check_launch("egk_action_topk");
}

int egk_edit_distance_pairs(egk_stream_t stream, const int64_t* pred_v, const int64_t* pred_n, int64_t p_sn, int64_t p_sz, int64_t p_sk,
                            const int64_t* label_v, const int64_t* label_n, int64_t l_sn, int64_t l_sz, int32_t* out, int32_t N,
                            int32_t Z, int32_t K) {
    EGK_REQUIRE(pred_v, "egk_edit_distance_pairs: null pointer (pred_v)");
    EGK_REQUIRE(pred_n, "egk_edit_distance_pairs: null pointer (pred_n)");
    EGK_REQUIRE(label_v, "egk_edit_distance_pairs: null pointer (label_v)");
    EGK_REQUIRE(label_n, "egk_edit_distance_pairs: null pointer (label_n)");
    EGK_REQUIRE(out, "egk_edit_distance_pairs: null pointer (out)");
    EGK_REQUIRE(N >= 0 && K >= 0, "egk_edit_distance_pairs: N >= 0 and K >= 0 (got %d, %d)", N, K);
    EGK_REQUIRE(Z >= 0 && Z <= 64, "egk_edit_distance_pairs: sequence length %d outside 0 .. 64", Z);
    EGK_REQUIRE((int64_t)N * K <= 0x7fffffffLL / 3, "egk_edit_distance_pairs: N * K too large (%d, %d)", N, K);
    EGK_REQUIRE(aligned_to(8u, {pred_v, pred_n, label_v, label_n}), "egk_edit_distance_pairs: misaligned pred or label (8-byte)");
    EGK_REQUIRE(aligned_to(4u, {out}), "egk_edit_distance_pairs: misaligned out (4-byte)");
    if (N == 0 || K == 0) return 0;
    hipStream_t s = (hipStream_t)stream;
    ProfScope prof(KID_EDIT_DISTANCE_PAIRS, s, 0, (double)N * K * (16.0 * Z + 12.0) + 16.0 * N * Z);
    hipLaunchKernelGGL(edit_distance_pairs_kernel, dim3(cdiv((int64_t)N * K, 64)), dim3(64), 0, s, (const long long*)pred_v,
                       (const long long*)pred_n, (long long)p_sn, (long long)p_sz, (long long)p_sk, (const long long*)label_v,
                       (const long long*)label_n, (long long)l_sn, (long long)l_sz, out, (int)N, (int)Z, (int)K);
    return check_launch("egk_edit_distance_pairs");
}

}  // extern "C"
