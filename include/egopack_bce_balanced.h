/*
 * egopack_bce_balanced.h -- shaped BCE-with-logits for the PNR head: egk_bce_fwd / egk_bce_bwd / egk_rowdot_bce with three f32
 * scalars applied INSIDE the pass:
 *     pos, neg >= 0   the class factor c = (y != 0 ? pos : neg)          (nn.BCEWithLogitsLoss(pos_weight = pos / neg) times neg)
 *     gamma    >= 0   the focusing exponent of the sigmoid focal loss    (Lin et al. 2017; pos = alpha, neg = 1 - alpha)
 * In the captured step the PNR head is one row pass that computes the logit, the loss and df, dw, db from the backward seed
 * baked into the launch: there is no loss tensor to reweight and no logit gradient to scale from outside.
 *
 * For a node with logit z and label y in {0, 1}: t = (float)y, s = 2t - 1, u = s z, softplus(x) = max(x, 0) + log1p(exp(-|x|)),
 * sigma(x) = 1 / (1 + exp(-x)), g the upstream gradient (gloss[n], or the seed of the one-pass form):
 *   gamma == 0:  loss = c * [(1 - t) z + max(-z, 0) + log1p(exp(-|z|))]
 *                dz   = (c * (sigma(z) - t)) * g
 *   gamma  > 0:  ce = softplus(-u) (= -log p_t), mod = exp(-gamma * softplus(u)) (= (1 - p_t) ** gamma), p_t = sigma(u)
 *                loss = c * mod * ce
 *                dz   = (s * c * mod * (gamma * p_t * (-ce) - (1 - p_t))) * g
 * every product evaluated left to right in f32 without fused multiply-add, so the f32 and the bf16 gradient are one f32 value
 * and its rounding.  gamma == 0 is a branch on a kernel argument (wave-uniform): with pos = neg = 1 it is the arithmetic of the
 * plain kernels and gives their bits.  No 0 * inf and no overflow for |z| <= 100.  The scalars travel by value: the kernels read
 * no memory the plain ones do not read and add no launch.
 *
 * Part of the C ABI of libegopack_hip.so: egopack_hip.h includes this file, a C user includes that one.  The boundary rules
 * of egopack_hip.h hold here word for word (stream-ordered, no allocation, no synchronisation, capturable; 0 = ok, negative =
 * EGK_E*, positive = hipError_t; a launch touches only what its arguments name).  egk_bce_w_fwd / _bwd are the kernels of
 * egk_bce_fwd / _bwd with the loss expression switched by a template flag (csrc/loss.hip); the plain entry points compute what
 * they computed: a caller that passes no scalar runs them.
 *
 * The entry points of THIS header have their guard-band cases in tests/test_gpu_bounds_pnr_balance.py; the one ledger of all
 * headers, tests/test_cabi.py, holds them under the key "bce_balanced" (egopack_amd/_lib.py binds them from the prototypes below).
 * Profile id "bce_balanced" counts all three.
 */
#ifndef EGOPACK_BCE_BALANCED_H
#define EGOPACK_BCE_BALANCED_H

#include "egopack_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* egk_bce_fwd with the scalars: loss[i] = the loss above for i < n; one thread per node, the grid of egk_bce_fwd.
 * Refused before any launch: null logits / y / loss, n < 0, a negative or non-finite pos / neg / gamma.  n == 0 launches nothing. */
int egk_bce_w_fwd(egk_stream_t s, const float* logits, const int64_t* y, float* loss, int32_t n, float pos, float neg, float gamma);

/* egk_bce_bwd with the scalars: dlogits[i] = dz above with g = gloss[i], element type ``dtype`` (EGK_F32 / EGK_BF16).
 * Refusals as egk_bce_w_fwd (null gloss / dlogits and an unknown dtype included). */
int egk_bce_w_bwd(egk_stream_t s, const float* logits, const int64_t* y, const float* gloss, void* dlogits, int32_t n, float pos,
                  float neg, float gamma, int32_t dtype);

/* egk_rowdot_bce with the scalars: the one-logit classifier, the shaped loss and df / dw / db in ONE pass over the rows of f.
 * Its contract in every other respect: df == NULL is forward only (logits, loss); otherwise df = g w per row with g = dz above for
 * g = seed, ROUNDED to the element type ``dtype`` before it is used for df, dw and db, and ws = float
 * [egk_rowdot_ws_rows(rows)][cols + 4] receives the partial rows that the unchanged egk_rowdot_reduce accumulates into dw / db.
 * Refused before any launch: null f / w / y / logits / loss, df without ws, rows < 0, cols < 1 or > 4096, a negative or non-finite
 * pos / neg / gamma, an unknown dtype, and with cols a multiple of 4 an f / w / df that is not aligned to 4 elements.
 * rows == 0 launches nothing. */
int egk_rowdot_bce_w(egk_stream_t s, const void* f, const void* w, const float* bias, const int64_t* y, float* logits, float* loss,
                     void* df, float* ws, int32_t rows, int32_t cols, float seed, float pos, float neg, float gamma, int32_t dtype);

#ifdef __cplusplus
}
#endif
#endif /* EGOPACK_BCE_BALANCED_H */
