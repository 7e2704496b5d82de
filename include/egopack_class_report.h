/*
 * egopack_class_report.h -- the per-class validation report: for every head of a task, in ONE launch, the confusion matrix, the
 * top-2 confusion matrix and the per-class sums of the plain cross entropy, accumulated into caller-owned int64 buffers from the
 * logits where they lie.  Every accumulator is an integer, so a validation split sharded over any number of ranks merges (by
 * integer addition) bit for bit to the single pass -- what a float sum cannot promise.
 *
 * The ranking of a row x_0 .. x_{C-1} is the order of egk_label_rank: v outranks u if v > u, or if v == u and its class index is
 * lower (-0 == +0).  A NaN never outranks anything: it orders as the lowest value, below -inf, and ties between NaNs go to the
 * lower index.  top1 is the first class of that order, top2 the second; a row of C == 1 has no top2 and makes no top-2 entry.
 *
 * The loss of a row with label t is the plain cross entropy lse - x_t (no smoothing, weight or offset: what validation scores),
 * formed by the row function of the loss kernels (csrc/ce_row.h: ce_row_plain, forward, no gradient), so it equals the per-row loss
 * of egk_ce_fwd(smoothing = 0) bit for bit: fl(fl(max + logf(sum exp)) - x_t).  It is accumulated in fixed point with 24
 * fractional bits: q = llrint(loss * 2^24) (the product is exact).  A loss that is not finite, or whose q would not fit an int64
 * (|loss| >= 2^39), is counted in counts[2] and added nowhere.
 *
 * Per row n of a task, label t = labels[n * label_stride]:
 *     t < 0 or t >= C :  counts[1] += 1, nothing else is touched (the row's logits are not read)
 *     otherwise       :  counts[0] += 1
 *                        confusion[t * C + top1] += 1
 *                        top2[t * C + top1] += 1          when top1 != t and top2 == t  (the label was the runner-up)
 *                        loss_q24[t] += q, or counts[2] += 1 when the loss is not finite
 * counts[3] is never touched.  The kernel ADDS (64-bit integer atomics, one lane per row): the caller zeroes the buffers once and
 * accumulates over the batches of a split.  Columns c >= C (between C and ld) are never read.
 *
 * Part of the C ABI of libegopack_hip.so: egopack_hip.h includes this file, a C user includes that one.  The boundary rules
 * of egopack_hip.h hold here word for word (stream-ordered, no allocation, no workspace, no synchronisation, capturable; 0 = ok,
 * negative = EGK_E*, positive = hipError_t; a launch touches only what its arguments name).
 *
 * The entry points of THIS header have their guard-band cases in tests/test_gpu_bounds_class_report.py; the one ledger of all
 * headers, tests/test_cabi.py, holds them under the key "class_report" (egopack_amd/_lib.py binds them from the prototypes below).
 * Profile id "class_report".
 */
#ifndef EGOPACK_CLASS_REPORT_H
#define EGOPACK_CLASS_REPORT_H

#include "egopack_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define EGK_CLASS_REPORT_MAX_TASKS 8

/* One head of a launch. */
typedef struct egk_class_report_task {
    const float* logits;    /* [rows, C] f32, rows ``ld`` elements apart (ld >= C), 4-byte aligned */
    int64_t ld;
    const int64_t* labels;  /* label of row n at labels[n * label_stride] (stride in elements), 8-byte aligned */
    int64_t label_stride;
    int32_t rows;
    int32_t C;
    int64_t* confusion;     /* [C, C] row-major, += 1 at [label, top1]                                             (required) */
    int64_t* top2;          /* [C, C] or NULL: += 1 at [label, top1] where top1 != label and top2 == label */
    int64_t* loss_q24;      /* [C]    or NULL: += llrint(loss * 2^24) at [label], finite losses only */
    int64_t* counts;        /* [4]: valid rows, ignored rows, valid rows with a non-finite loss, 0                  (required) */
} egk_class_report_task;

/* One wave per (task, row), four waves per workgroup, a capped grid and a row loop that strides.  tasks: HOST array of ``count``
 * entries (1 .. EGK_CLASS_REPORT_MAX_TASKS), copied into the launch; the tasks may differ in rows and C.
 * Refused with EGK_EINVAL before anything is launched: a null ``tasks``, count outside 1 .. 8; per task a null logits / labels /
 * confusion / counts pointer, C < 1, ld < C, rows < 0, a confusion / top2 / loss_q24 / counts pointer that is not 8-byte aligned
 * (or labels; logits 4-byte).  With rows == 0 in every task the same checks are made and nothing is launched. */
int egk_class_report(egk_stream_t s, const egk_class_report_task* tasks, int32_t count);

#ifdef __cplusplus
}
#endif
#endif /* EGOPACK_CLASS_REPORT_H */
