/*
 * egopack_topk.h -- what a trained head predicts: for every head of a task, in ONE launch, the best k classes of every logits row,
 * their softmax probabilities and the row's log-sum-exp, from the logits where they lie.  No [rows, C] probability tensor is formed
 * and nothing is sorted on the host: a prediction file (egopack_amd/predict.py) holds exactly these outputs.
 *
 * The order is the meters' order, the one of egk_label_rank and egk_class_report (csrc/metrics.hip: rank_key, one definition):
 * entry j of a row x_0 .. x_{C-1} is the class with the j-th largest key.  v outranks u if v > u, or if v == u and its class index
 * is lower (-0 == +0).  A NaN never outranks anything: it orders as the lowest value, below -inf, and ties between NaNs go to the
 * lower index.  So idx[., 0] and idx[., 1] are the top1 and top2 of egk_class_report, and egk_label_rank(logits, idx[., j]) == j for
 * every j < min(k, C).  Entries j >= C (k larger than the row) get index -1 and probability 0.
 *
 * bf16 logits are widened to f32 first; everything below is f32.
 *     lse     = what the row function of the loss kernels forms (csrc/ce_row.h: ce_row_plain, forward, no gradient):
 *               fl(max + logf(sum_c expf(x_c - max))), the same lane striding and wave reductions -- the bits of egk_ce_fwd's saved
 *               log-sum-exp and of egk_class_report's loss, so fl(lse - x_t) is egk_ce_fwd(smoothing = 0)'s loss of label t.
 *     prob[j] = expf(x_idx[j] - lse)
 * A -inf logit in an otherwise finite row gets exactly 0.  A row with a NaN gets NaN in lse and in all its probabilities (those of
 * entries j < C); its indices are still the order's.  Columns c >= C (between C and ld) are never read.
 *
 * Part of the C ABI of libegopack_hip.so: egopack_hip.h includes this file, a C user includes that one.  The boundary rules
 * of egopack_hip.h hold here word for word (stream-ordered, no allocation, no workspace, no synchronisation, capturable; 0 = ok,
 * negative = EGK_E*, positive = hipError_t; a launch touches only what its arguments name).
 *
 * The entry points of THIS header have their guard-band cases in tests/test_gpu_bounds_topk.py; the one ledger of all
 * headers, tests/test_cabi.py, holds them under the key "topk" (egopack_amd/_lib.py binds them from the prototypes below).
 * Profile id "topk_softmax".
 */
#ifndef EGOPACK_TOPK_H
#define EGOPACK_TOPK_H

#include "egopack_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define EGK_TOPK_MAX_TASKS 8
#define EGK_TOPK_MAX_K 64

/* One head of a launch. */
typedef struct egk_topk_task {
    const void* logits;      /* [rows, C] of the launch's dtype, rows ``ld`` elements apart (ld >= C), aligned to its element */
    int64_t ld;
    int32_t C;
    int32_t reserved;        /* 0 */
    int64_t* idx;            /* entry j of row r at idx[r * idx_row_stride + j], j < k; 8-byte aligned          (required) */
    int64_t idx_row_stride;  /* in elements, >= k */
    float* prob;             /* NULL, or entry j of row r at prob[r * prob_row_stride + j]; 4-byte aligned */
    int64_t prob_row_stride; /* in elements, >= k when prob is given */
    float* lse;              /* NULL, or [rows] contiguous; 4-byte aligned */
} egk_topk_task;

/* The best k classes of every row of every task: one wave per (task, row), four waves per workgroup, a grid-stride walk.  A row of
 * at most 512 classes is read once for the order (its keys stay in registers), a wider row once per entry; exact either way.
 * tasks: HOST array of ``count`` entries (1 .. EGK_TOPK_MAX_TASKS), copied into the launch.  rows, k and dtype (EGK_F32 or EGK_BF16)
 * are shared by the tasks.
 * Refused with EGK_EINVAL before anything is launched: a null ``tasks``, count outside 1 .. 8, rows < 0, k outside 1 .. 64, an
 * unknown dtype; per task a null logits / idx pointer, C < 1, ld < C, a non-zero ``reserved``, an idx row stride < k (negative
 * ones with it), a prob given with a row stride < k, a misaligned pointer.  rows == 0 passes the same checks and launches
 * nothing. */
int egk_topk_softmax(egk_stream_t s, const egk_topk_task* tasks, int32_t count, int32_t rows, int32_t k, int32_t dtype);

#ifdef __cplusplus
}
#endif
#endif /* EGOPACK_TOPK_H */
