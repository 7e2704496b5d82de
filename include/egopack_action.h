/*
 * egopack_action.h -- action-level scores of the verb / noun heads: an ACTION is the pair (verb, noun).
 *
 * Two heads over the same rows: verb logits z of width Cv, noun logits w of width Cn.  The model's distribution over the Cv * Cn
 * pairs is the product of the two softmaxes, so the log-probability of a pair is the sum of the heads' log-probabilities.
 *
 * Row arithmetic of egk_action_topk, in f32 (bf16 logits are widened as they are read), every operation rounded separately:
 *     x_v = z_v,  y_n = w_n                                        without beta
 *     x_v = fl(beta[0] * z_v),  y_n = fl(beta[1] * w_n)            with beta: one separately rounded product, never fused
 *     lse_v = fl(max + logf(sum_c expf(x_c - max)))                 the loss kernels' row function (csrc/ce_row.h; with beta its
 *                                                                   sibling at a temperature, csrc/temp_row.h): without beta, and at
 *                                                                   beta == 1, the bits of egk_topk_softmax's lse
 *     a_v = fl(x_v - lse_v),  b_n = fl(y_n - lse_n)                 the heads' log-probabilities
 *     s(v, n) = fl(a_v + b_n)                                       the score of the pair;  logp = s,  prob = expf(s)
 *
 * THE ORDER of the pairs of a row -- there is one definition.  The order of a head is the meters' (egk_label_rank,
 * egk_topk_softmax) over x (over y): the larger value first, ties to the lower class index, -0 == +0, a NaN below -inf.
 *     1. P outranks Q if s_P > s_Q  (-0 == +0);
 *     2. at equal scores, if P's verb outranks Q's verb in the verb head's order;
 *     3. with the same verb, if P's noun outranks Q's noun in the noun head's order;
 *     4. a NaN score never outranks by value: it is below -inf, and all NaN scores tie (rules 2 and 3 then decide).
 * Ties go through the heads' orders, not through class indices, because then this is exact under rounding: fl(x - lse) and
 * fl(a + b) are monotone (not strictly) in each argument, so replacing a pair's verb by a higher-ranked verb never lowers the score
 * and wins the tie.  Hence every one of the best k pairs lies in (the best min(k, Cv) verbs) x (the best min(k, Cn) nouns): the
 * launch selects k out of at most k * k candidates and never forms the Cv x Cn table.  (A row's scores are either all NaN or none
 * is: lse is finite or NaN, and a row with a NaN or +inf entry, or without a finite entry, has a NaN lse.)
 *
 * Part of the C ABI of libegopack_hip.so: egopack_hip.h includes this file, a C user includes that one.  The boundary rules of
 * egopack_hip.h hold here word for word (stream-ordered, no allocation, no synchronisation, capturable; 0 = ok, negative =
 * EGK_E*, positive = hipError_t; a launch touches only what its arguments name).  Scalars and pointers only: no struct.
 *
 * egopack_amd/_lib.py binds the prototypes below from its open third table, ADDON_HEADERS["action"]; tests/test_cabi_addons.py is
 * the ledger of that table (what it pins for this header: tests/cabi_addon_action.py) and tests/test_gpu_bounds_action.py holds
 * the guard-band cases.
 */
#ifndef EGOPACK_ACTION_H
#define EGOPACK_ACTION_H

#include "egopack_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define EGK_ACTION_MAX_K 32
#define EGK_ACTION_MAX_C 1024

/* The best k pairs of every row with their scores, both log-sum-exps and the exact rank of the labelled pair, in ONE launch.  One
 * wave per row, four waves per workgroup, at most 2048 workgroups with a strided row loop.  Both rows are read from memory once
 * into registers, class lane + 64 * i in slot i (one instance for C <= 512, one for C <= 1024); the row function re-reads them
 * from cache.  No atomics, no workspace, no LDS.
 *   verb_logits [rows, Cv], noun_logits [rows, Cn] of ``dtype`` (EGK_F32 / EGK_BF16), rows ld_v / ld_n elements apart; columns
 *   [C, ld) are never read.
 *   beta: NULL, or 2 f32 in device memory: 1 / T of the verbs, of the nouns.
 *   verb_labels, noun_labels: both NULL, or both given: int64, ``*_label_stride`` elements apart (a column view of a label matrix).
 *   pair: int64; entry j of row r is the verb at pair[r * pair_row_stride + 2 j] and the noun at [.. + 2 j + 1], j < k, in the
 *   order above; pair_row_stride >= 2 k.  Entries j >= Cv * Cn are (-1, -1) with prob 0 and logp -inf.
 *   logp, prob: each NULL or f32 [rows, k], rows out_row_stride >= k elements apart.
 *   lse: NULL or f32 [rows, 2]: lse_v, lse_n.
 *   rank: NULL or int32 [rows] (requires the labels, and the labels require it): the number of pairs among ALL Cv * Cn that
 *   outrank the labelled pair -- exact: every pair is scored and compared, Cv * Cn additions per row --, -1 when either label is
 *   outside [0, C).  Hence rank < k  <=>  the labelled pair is among the k exported ones, and one launch serves top-1 / 2 / 3 / 5.
 * A row with a NaN lse has NaN lse, logp and prob; its pairs and its rank still follow the order (rules 2 and 3).
 * Refused before any launch: a null verb_logits / noun_logits / pair; labels without rank, rank without labels, one label pointer
 * without the other; rows < 0; k outside 1 .. 32; Cv or Cn outside 1 .. 1024; ld < C; pair_row_stride < 2 k; out_row_stride < k
 * with logp or prob given; an unknown dtype; logits not aligned to their element, pair or labels not 8-byte aligned, beta / logp /
 * prob / lse / rank not 4-byte aligned.  rows == 0 launches nothing.  Profile id "action_topk". */
int egk_action_topk(egk_stream_t s, const void* verb_logits, int64_t ld_v, int32_t Cv, const void* noun_logits, int64_t ld_n,
                    int32_t Cn, const float* beta, const int64_t* verb_labels, int64_t verb_label_stride,
                    const int64_t* noun_labels, int64_t noun_label_stride, int32_t rows, int32_t k, int64_t* pair,
                    int64_t pair_row_stride, float* logp, float* prob, int64_t out_row_stride, float* lse, int32_t* rank,
                    int32_t dtype);

/* The Levenshtein distances of K sampled futures against the labelled sequence, per head and at ACTION level, in one launch: one
 * thread per (sequence n, future k), three single-row dynamic programmes over Z positions that share their loads.
 *   pred_v, pred_n: int64, element (n, z, k) at n * p_sn + z * p_sz + k * p_sk (both with the same strides);
 *   label_v, label_n: int64, element (n, z) at n * l_sn + z * l_sz.
 *   out: int32 [N, K, 3]: [n, k, 0] the verb distance and [n, k, 1] the noun distance -- the integers egk_edit_distance gives --,
 *   [n, k, 2] the action distance: position z of future k is the token (pred_v, pred_n), equal to a label token only if both parts
 *   are equal.  So [., ., 2] >= max([., ., 0], [., ., 1]).
 * Refused before any launch: a null pointer, N or K < 0, Z outside 0 .. 64, 3 * N * K beyond 2^31 - 1, pred / label pointers not
 * 8-byte aligned, out not 4-byte aligned.  N == 0 or K == 0 launches nothing.  Profile id "edit_distance_pairs". */
int egk_edit_distance_pairs(egk_stream_t s, const int64_t* pred_v, const int64_t* pred_n, int64_t p_sn, int64_t p_sz, int64_t p_sk,
                            const int64_t* label_v, const int64_t* label_n, int64_t l_sn, int64_t l_sz, int32_t* out, int32_t N,
                            int32_t Z, int32_t K);

#ifdef __cplusplus
}
#endif
#endif /* EGOPACK_ACTION_H */
