/*
 * egopack_task_scale.h -- the task factor of a head's backward seed read from DEVICE memory: adjustable and learned task weights
 * inside a captured multi-task step.
 *
 * The step's objective is sum_t w_t * mean(loss_t), and every head kernel that emits its gradient in the launch that computes the
 * loss takes the seed c = w_t / N_t by value: it is baked into a captured graph.  The _s entry points below take a device pointer
 * beside it and use
 *     c_eff = fl32(c * scale[0])
 * ONE separately rounded f32 product (compiled without contraction: never fused into what follows), formed once per wave from one
 * wave-uniform 4-byte load before anything else uses it.  Everything after it is the sibling's arithmetic, the rounding of the logit gradient to
 * the operand type in the row-dot heads included.  The contract that makes this testable without a tolerance:
 *     a launch with (c, scale) writes bit for bit what the sibling writes with c' = fl32(c * scale[0]) by value
 * -- loss, logits, dlogits, df, dw, db and workspaces, f32 and bf16.  The siblings are the same kernels with a null pointer (a
 * wave-uniform test, as the optimizer's gate pointer is): they compute what they computed.
 *
 * Two uses (egopack_amd.engine.MTLStep, ``task_weighting.mode``):
 *   manual       the host writes scale[t] between two replays; the next replay uses it without a re-capture.
 *   uncertainty  homoscedastic-uncertainty weighting (Kendall, Gal and Cipolla 2018): one learnable log-variance s_t per task,
 *                J = sum_t w_t (exp(-s_t) L_t + s_t),  L_t = mean(loss_t),  scale_t = exp(-s_t),  dJ/ds_t = w_t (1 - scale_t L_t).
 *                s = 0 gives scale = 1 exactly: the first step's losses and gradients are the fixed-weight step's.
 *
 * Part of the C ABI of libegopack_hip.so: egopack_hip.h includes this file, a C user includes that one.  The boundary rules
 * of egopack_hip.h hold here word for word (stream-ordered, no allocation, no synchronisation, capturable; 0 = ok, negative =
 * EGK_E*, positive = hipError_t; a launch touches only what its arguments name).  A scale pointer must be 4-byte aligned.
 *
 * The entry points of THIS header have their guard-band cases in tests/test_gpu_bounds_task_weighting.py; the one ledger of all
 * headers, tests/test_cabi.py, holds them under the key "task_scale" (egopack_amd/_lib.py binds them from the prototypes below).
 * Profile id "task_scale" counts all of them.
 */
#ifndef EGOPACK_TASK_SCALE_H
#define EGOPACK_TASK_SCALE_H

#include "egopack_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* egk_ce_fused_multi / egk_ce_w_fused_multi with a scale per task: scales is a HOST array of ``count`` device pointers, task i uses
 * fl32(tasks[i].gscale * scales[i][0]).  Grid, row ownership and every refusal of the sibling; refused too: null scales, a null or
 * misaligned scales[i]. */
int egk_ce_fused_multi_s(egk_stream_t s, const egk_ce_task* tasks, const float* const* scales, int32_t count, float smoothing,
                         int32_t dtype);
int egk_ce_w_fused_multi_s(egk_stream_t s, const egk_ce_w_task* tasks, const float* const* scales, int32_t count, float smoothing,
                           int32_t dtype);

/* egk_rowdot_bce / egk_rowdot_bce_w with seed_eff = fl32(seed * scale[0]): the same kernel, grid, ``ws`` layout
 * (float [egk_rowdot_ws_rows(rows)][cols + 4]) and the unchanged egk_rowdot_reduce behind it.  Every refusal of the sibling, and a
 * null or misaligned scale. */
int egk_rowdot_bce_s(egk_stream_t s, const void* f, const void* w, const float* bias, const int64_t* y, float* logits, float* loss,
                     void* df, float* ws, int32_t rows, int32_t cols, float seed, const float* scale, int32_t dtype);
int egk_rowdot_bce_w_s(egk_stream_t s, const void* f, const void* w, const float* bias, const int64_t* y, float* logits, float* loss,
                       void* df, float* ws, int32_t rows, int32_t cols, float seed, const float* scale, float pos, float neg,
                       float gamma, int32_t dtype);

/* egk_rowdot_ce2 / egk_rowdot_ce2_multi with seed_eff = fl32(seed * scale[0]), read by the row launch (phase 0 or 1; the column
 * launch reads the rounded gradients that launch left in ``gws`` and reads no scale).  Every refusal of the sibling, and a null or
 * misaligned scale. */
int egk_rowdot_ce2_s(egk_stream_t s, const void* f, const void* w, const float* bias, const int64_t* y, float* logits, float* loss,
                     void* df, float* dw, float* db, float* gws, int32_t rows, int32_t cols, float smoothing, float seed,
                     const float* scale, int32_t dtype);
int egk_rowdot_ce2_multi_s(egk_stream_t s, int32_t n_src, const void* const* f, const void* const* w, const float* const* bias,
                           const int64_t* y, float* logits, float* loss, void* const* df, float* const* dw, float* const* db,
                           float* gws, int32_t rows, int32_t cols, int32_t average, float smoothing, float seed, const float* scale,
                           int32_t dtype);

/* scale[t] = (float)exp(-(double)s[t]) for t < n (1 <= n <= 8): one launch of one wave at the head of the step.  s, scale: device
 * float [n].  Exactly 1 for s = 0. */
int egk_task_scale_prepare(egk_stream_t s, const float* log_var, float* scale, int32_t n);

/* The gradient of the log-variances, the reported objective and the running per-task loss sums in ONE launch of n workgroups
 * (1 <= n <= 8).  HOST arrays of n entries: loss (device pointers; NULL = the task is absent from this step -- a task that has no
 * loss element in this step is handed over the same way: it adds nothing to the objective and does not move its log-variance), ns
 * (elements of each vector), counts (what the task's mean divides by -- a compacted vector holds only its non-zero elements; <= 0: ns), w.
 * Device: log_var float [n] or NULL, scale float [n], ds float [n] (required with log_var), objective float [1], acc double [n] or NULL.
 * Workgroup t: S_t = sum(loss_t) in f64 in a fixed order (no atomics: the same bits on every launch), L_t = S_t / count_t,
 *     acc[t] += S_t                                    (the RAW loss sums, as egk_weighted_sums_acc feeds them)
 *     ds[t]   = (float)(w_t (1 - scale_t L_t))         (log_var given; one writer; 0 for an absent task)
 * and workgroup 0, which walks every task in order:
 *     objective[0] = (float) sum_t w_t (scale_t L_t + log_var_t)     (log_var given: J)
 *                  = (float) sum_t w_t  scale_t L_t                  (log_var NULL: fixed scales)
 * over the tasks present.  Refused: a null host array / scale / objective, log_var without ds, n outside 1..8, a negative length,
 * a misaligned pointer. */
int egk_task_scale_grad(egk_stream_t s, const float* const* loss, const int64_t* ns, const int64_t* counts, const float* w,
                        const float* log_var, const float* scale, float* ds, float* objective, double* acc, int32_t n);

/* out[i] = fl32(coef * scale[0]) for i < n: the tensor a head's backward starts from when the head runs off the announced-seed
 * paths.  Refused: null out / scale, n < 0, a misaligned pointer.  n == 0 launches nothing. */
int egk_fill_scaled_from(egk_stream_t s, float* out, int64_t n, float coef, const float* scale);

#ifdef __cplusplus
}
#endif
#endif /* EGOPACK_TASK_SCALE_H */
