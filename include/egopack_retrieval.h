/*
 * egopack_retrieval.h -- what a GraphONE prediction rests on: for every node and every auxiliary task, in ONE launch, how far the
 * prototypes the node consulted were, and how much of the first stage's aggregated message each of them supplied.  The launch reads
 * the very tensors the interaction used (GraphONE.record_retrieval: the f32 features the search read, the [rows, k] list it produced,
 * the activation-type features the first stage's gather-max read) and the frozen bank; it searches nothing itself.
 *
 * dist[r, j]: the reference's distance (models/graphONE/graphONE.py, __compute_edges) between row r of ``f`` and prototype nn[r, j],
 * in f32 from the f32 operands:
 *     cosine (distance = 0):  1 - f.p / (|f| |p|)
 *     l2     (distance = 1):  sqrt(sum_c (f_c - p_c)^2) / 4096      (from the differences, not from expanded norms)
 * The launch forms f.p, |f|^2 and |p|^2 (or the sum of squared differences) itself, in one pass over the two rows; it takes no norm
 * vectors.  A zero row gives what the reference's division gives (NaN for cosine); nothing is special-cased.  Every sum has the lane
 * striding of egk_row_inv_norm: lane l adds the four-term groups of columns 4 l + 256 i .. 4 l + 256 i + 3 in the order of i, then one
 * butterfly over the 64 lanes.  A value is therefore a function of its row, its prototype and H alone -- not of the task's place in
 * the launch, of the leading dimensions, or of which outputs were asked for.
 *
 * wins[r, j]: the number of the H channels in which source j supplies the maximum of the first stage's gather-max.  Sources
 * 0 .. k - 1 are the prototypes nn[r, 0 .. k - 1] (their f32 bank rows), source k is the node's own row of ``f_act`` (widened to f32).
 * The rule is egk_gather_max_fwd's, word for word: prototype edges first, the self loop last; a source wins only with v > best,
 * starting from -inf; a column where no source exceeds -inf (all NaN, all -inf) counts for source 0.  So
 *     wins[r, j] == count_c(arg[r, c] == j)
 * for the ``arg`` egk_gather_max_fwd writes on the same f_act, bank and nn, and every row of wins sums to H.  The counts are integers
 * (wave ballots and population counts): exact in any order, no atomics.
 * wins says which source a channel of the FIRST stage's message came from.  It says nothing about later stages (they read features
 * nobody exports), nor how much the message then weighs in the stage's output.
 *
 * Part of the C ABI of libegopack_hip.so: egopack_hip.h includes this file, a C user includes that one.  The boundary rules
 * of egopack_hip.h hold here word for word (stream-ordered, no allocation, no workspace, no synchronisation, capturable; 0 = ok,
 * negative = EGK_E*, positive = hipError_t; a launch touches only what its arguments name).
 *
 * The entry points of THIS header have their guard-band cases in tests/test_gpu_bounds_retrieval.py; the one ledger of all
 * headers, tests/test_cabi.py, holds them under the key "retrieval" (egopack_amd/_lib.py binds them from the prototypes below).
 * Profile id "retrieval_report".
 */
#ifndef EGOPACK_RETRIEVAL_H
#define EGOPACK_RETRIEVAL_H

#include "egopack_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define EGK_RETRIEVAL_MAX_TASKS 8
#define EGK_RETRIEVAL_MAX_K 32

/* One auxiliary task of a launch.  Leading dimensions and row strides are in elements. */
typedef struct egk_retrieval_task {
    const float* f;          /* [rows, H] f32: the features the search read; 4-byte aligned */
    int64_t f_ld;            /* >= H */
    const void* f_act;       /* [rows, H] of the launch's dtype: what the first GraphONE stage's gather-max read (may alias f for EGK_F32) */
    int64_t f_act_ld;        /* >= H */
    const float* bank;       /* [K, H] f32; 4-byte aligned */
    int64_t bank_ld;         /* >= H */
    int32_t K;               /* >= 1 */
    int32_t reserved;        /* 0 */
    const int64_t* nn;       /* [rows, k], every entry in 0 .. K-1 (not checked, as in egk_gather_max_fwd); 8-byte aligned */
    int64_t nn_row_stride;   /* >= k */
    float* dist;             /* NULL, or entry j of row r at dist[r * dist_row_stride + j], j < k; 4-byte aligned */
    int64_t dist_row_stride; /* >= k when dist is given */
    int32_t* wins;           /* NULL, or entry j of row r at wins[r * wins_row_stride + j], j <= k; 4-byte aligned */
    int64_t wins_row_stride; /* >= k + 1 when wins is given */
} egk_retrieval_task;

/* The report of every row of every task: one wave per (task, row), four waves per workgroup, the row walk of the other row kernels
 * (a row stays with its XCD).  The k bank rows of a node are read once for the distances and once for the winners.  Rows whose
 * width, leading dimension and address allow it are read four elements at a time; the values read are the same either way.
 * tasks: HOST array of ``count`` entries (1 .. EGK_RETRIEVAL_MAX_TASKS), copied into the launch.  rows, H, k, distance and dtype
 * (EGK_F32 or EGK_BF16: the element type of every f_act) are shared by the tasks.
 * Refused with EGK_EINVAL before anything is launched: a null ``tasks``, count outside 1 .. 8, rows < 0, H < 1, k outside 1 .. 32,
 * an unknown distance or dtype; per task a null f / f_act / bank / nn, K < 1, a non-zero ``reserved``, a leading dimension < H, an
 * nn row stride < k, a dist given with a row stride < k, a wins given with a row stride < k + 1 (negative ones with them), dist and
 * wins both NULL, a misaligned pointer.  rows == 0 passes the same checks and launches nothing. */
int egk_retrieval_report(egk_stream_t s, const egk_retrieval_task* tasks, int32_t count, int32_t rows, int32_t H, int32_t k,
                         int32_t distance /* 0 cosine, 1 l2 */, int32_t dtype /* of f_act */);

#ifdef __cplusplus
}
#endif
#endif /* EGOPACK_RETRIEVAL_H */
