/*
 * egopack_ce_balanced.h -- class-balanced cross entropy: egk_ce_fwd / egk_ce_bwd / egk_ce_fused_multi with two optional f32
 * vectors per head, applied INSIDE the row pass:
 *     weight[c]   torch's nn.CrossEntropyLoss(weight=...)            (class weighting, "effective number of samples")
 *     offset[c]   added to the logits inside the loss only           (logit adjustment, a_c = tau * log(prior_c))
 * In the captured step the loss and its gradient are one launch that writes dlogits into the classifier banks' operand buffers
 * with the backward seed baked in: there is no loss tensor to reweight and no logits gradient to scale from outside.
 *
 * For a live row (label t in [0, C)), x'_c = x_c + a_c, lse = logsumexp(x'), W = sum_c w_c, smoothing eps, p_j = exp(x'_j - lse):
 *     loss = (1 - eps) * w_t * (lse - x'_t)  +  (eps / C) * (W * lse - sum_c w_c x'_c)
 *     dx_j = g * [ (1 - eps) * w_t * (p_j - [j == t])  +  (eps / C) * (W * p_j - w_j) ]
 * = F.cross_entropy(x + a, y, weight=w, ignore_index=-1, reduction='none', label_smoothing=eps).  Ignored rows (t < 0 or t >= C)
 * give loss 0 and gradient 0.  A NULL weight means w = 1, a NULL offset a = 0.  W and sum_c w_c x'_c are reduced by the row's
 * wave in the pass that forms sum exp (shifted by the row maximum like it); the two vectors are at most a few hundred floats
 * that every row reads again, so they are served from L2: no host value of W, nothing synchronises.
 *
 * Part of the C ABI of libegopack_hip.so: egopack_hip.h includes this file, a C user includes that one.  The boundary rules
 * of egopack_hip.h hold here word for word (stream-ordered, no allocation, no synchronisation, capturable; 0 = ok, negative =
 * EGK_E*, positive = hipError_t; a launch touches only what its arguments name).  One wave per row, the row ownership and the
 * grid of the plain entry points, whose kernels these are with the vectors switched on by a template flag (csrc/loss.hip); a
 * caller that passes no vector runs the plain instantiation and gets the bits it always got.
 *
 * The entry points of THIS header have their guard-band cases in tests/test_gpu_bounds_class_balance.py; the one ledger of all
 * headers, tests/test_cabi.py, holds them under the key "ce_balanced" (egopack_amd/_lib.py binds them from the prototypes below).
 * Profile id "ce_balanced" counts all three.
 */
#ifndef EGOPACK_CE_BALANCED_H
#define EGOPACK_CE_BALANCED_H

#include "egopack_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* egk_ce_fwd with the vectors.  weight, offset: device, [C] f32, 4-byte aligned (read one float at a time), or NULL.  lse[n] = logsumexp of the ADJUSTED
 * logits (saved for egk_ce_w_bwd).  loss[n] (+)= the loss above.
 * Refused before any launch: null logits / y / loss / lse, C < 1, a vector pointer that is not 4-byte aligned.
 * rows == 0 launches nothing. */
int egk_ce_w_fwd(egk_stream_t s, const float* logits, int64_t ld, const int64_t* y, int64_t y_stride, const float* weight,
                 const float* offset, float* loss, float* lse, int32_t rows, int32_t C, float smoothing, int32_t accumulate);

/* egk_ce_bwd with the vectors: dlogits[n, j] = gloss[n] * [...] as above, element type ``dtype`` (EGK_F32 / EGK_BF16), 0 for
 * ignored rows.  lse: what egk_ce_w_fwd saved for the same logits and offset.  W is reduced again by the row's wave (in the
 * order of the forward pass).  Refusals as egk_ce_w_fwd (null gloss / dlogits included). */
int egk_ce_w_bwd(egk_stream_t s, const float* logits, int64_t ld, const int64_t* y, int64_t y_stride, const float* weight,
                 const float* offset, const float* lse, const float* gloss, void* dlogits, int64_t ldd, int32_t rows, int32_t C,
                 float smoothing, int32_t dtype);

/* egk_ce_fused_multi with the vectors: per task, loss[n] = sum_h loss_h(n) and dlogits[n, dcol[h] + c] = gscale * [...] for
 * c < C[h], 0 for C[h] <= c < pad[h], in ONE launch for ``count`` in 1..4 tasks (count == 1 is the single-task fused form).
 * weight[h] / offset[h]: the vectors of head h of the task, each [C[h]] f32, 4-byte aligned, or NULL.
 * Refused before any launch: null tasks, count outside 1..4, n_heads outside 1..4, null y / loss / dlogits / logits[h],
 * C[h] < 1, pad[h] < C[h], rows < 0, a vector pointer that is not 4-byte aligned.  No row in any task: nothing is launched. */
typedef struct {
    egk_ce_task base;
    const float* weight[4];
    const float* offset[4];
} egk_ce_w_task;
int egk_ce_w_fused_multi(egk_stream_t s, const egk_ce_w_task* tasks, int32_t count, float smoothing, int32_t dtype);

#ifdef __cplusplus
}
#endif
#endif /* EGOPACK_CE_BALANCED_H */
