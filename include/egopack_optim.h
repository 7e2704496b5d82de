/*
 * egopack_optim.h -- the update rules of the flat-buffer optimizer behind ONE launch interface: torch.optim.Adam,
 * torch.optim.AdamW (= Adam with decoupled_weight_decay) and torch.optim.SGD, the single-tensor formulas of torch 2.10.
 *
 * Part of the C ABI of libegopack_hip.so: egopack_hip.h includes this file, a C user includes that one.  The boundary rules
 * of egopack_hip.h hold here word for word (stream-ordered, no allocation, no synchronisation, capturable; 0 = ok, negative =
 * EGK_E*, positive = hipError_t; a launch touches only what its arguments name).
 *
 * The entry points of THIS header have their guard-band cases in tests/test_gpu_bounds_optim.py; the one ledger of all
 * headers, tests/test_cabi.py, holds them under the key "optim" (egopack_amd/_lib.py binds them from the prototypes below).
 */
#ifndef EGOPACK_OPTIM_H
#define EGOPACK_OPTIM_H

#include "egopack_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

enum { EGK_OPT_ADAM = 0, EGK_OPT_ADAMW = 1, EGK_OPT_SGD = 2 };

/* One optimizer launch over n elements of the flat buffers.  s = hyper[3] (grad_scale, times the clip coefficient when
 * egk_grad_norm_finalize ran in front), lr = hyper[0]; hyper is what egk_adam_hyper writes (every rule is stepped behind it:
 * it counts the step in *t_dev).
 *   EGK_OPT_ADAM   g' = g*s + wd*p; m = m + (g' - m)*(1-b1); v = v*b2 + (1-b2)*g'*g';
 *                  p -= (lr/hyper[1]) * m / (sqrt(v)/hyper[2] + eps)      -- egk_adam_step_gated's bits
 *   EGK_OPT_ADAMW  p *= 1 - lr*wd; then the lines above with g' = g*s; 1-b1, 1-b2 and 1 - lr*wd are taken in double and rounded
 *                  once, as torch rounds the scalars it hands its kernels (EGK_OPT_ADAM keeps egk_adam_step's f32 1.f - b)
 *   EGK_OPT_SGD    g' = g*s + wd*p; momentum != 0: buf = g' when *t_dev == 1 (the first step that happens: a skipped step is
 *                  taken back out of the counter), else buf = momentum*buf + (1-dampening)*g'; step = g' + momentum*buf
 *                  (nesterov) or buf; momentum == 0: step = g'.  p -= lr*step
 * state0 / state1: exp_avg / exp_avg_sq (Adam, AdamW); the momentum buffer / unused (SGD with momentum); SGD without momentum
 * reads and writes NO state memory (both ignored, may be NULL).  t_dev: read by SGD with momentum only.
 * g_dtype: EGK_F32, or EGK_BF16 for the bf16 copy a compressed all-reduce summed.  bf16_shadow / bf16_lo_shadow (or NULL):
 * bf16(p) and bf16(p - bf16(p)) of the stored p -- egk_cast's and egk_split_bf16's bits.  *bump_word += bump (bump_word or
 * NULL) by one thread of the launch (n > 0).  gate (device int32 or NULL): *gate == 0 leaves p, the state and both copies
 * untouched, *bump_word still moves on.
 * p, g, state0, state1: 16-byte aligned; the bf16 copies 8-byte.  nesterov needs momentum > 0 and dampening == 0. */
typedef struct egk_optim_desc {
    int32_t rule, g_dtype;
    int64_t n;
    float* p;
    const void* g;
    float* state0;
    float* state1;
    const float* hyper;
    const int64_t* t_dev;
    double beta1, beta2;
    float eps, weight_decay, momentum, dampening;
    int32_t nesterov;
    void* bf16_shadow;
    void* bf16_lo_shadow;
    int64_t* bump_word;
    int64_t bump;
    const int32_t* gate;
} egk_optim_desc;

int egk_optim_step(egk_stream_t s, const egk_optim_desc* d);

#ifdef __cplusplus
}
#endif
#endif /* EGOPACK_OPTIM_H */
