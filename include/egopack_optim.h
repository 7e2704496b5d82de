/*
 * egopack_optim.h -- the update rules of the flat-buffer optimizer behind ONE launch interface: torch.optim.Adam,
 * torch.optim.AdamW (= Adam with decoupled_weight_decay) and torch.optim.SGD, the single-tensor formulas of torch 2.10.
 *
 * Part of the C ABI of libegopack_hip.so: egopack_hip.h includes this file, a C user includes that one.  The boundary rules
 * of egopack_hip.h hold here word for word (stream-ordered, no allocation, no synchronisation, capturable; 0 = ok, negative =
 * EGK_E*, positive = hipError_t; a launch touches only what its arguments name).
 *
 * The entry points of THIS header have their guard-band cases in tests/test_gpu_bounds_optim.py (a bf16 state:
 * tests/test_gpu_bounds_optim_state.py); the one ledger of all
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
 * p, g, state0, state1: 16-byte aligned; the bf16 copies 8-byte.  nesterov needs momentum > 0 and dampening == 0.
 *
 * The state in bf16 (state_dtype == EGK_BF16; the four fields at the end, all zero: the f32 launch as it always was, bit for bit).
 * state0 / state1 then hold bf16 elements, 8-byte aligned.  A launch reads them widened to f32 (exact), runs the lines above
 * unchanged and forms p, both bf16 copies and the moving average from the UNROUNDED new state: they are bit for bit those of the
 * f32-state launch started from the same (widened) state.  Only what is stored into state0 / state1 is rounded, so the one
 * effect on the arithmetic is the state the next step reads.  The rounding of one f32 value x with bits b:
 *     exponent all ones (inf / NaN)   f2bf(x): round to nearest even, the bits of egk_cast
 *     state_round == 0                f2bf(x)
 *     state_round == 1                (b + r) >> 16 with 16 random bits r: the magnitude grows with probability (b & 0xFFFF) / 2^16
 *                                     for either sign; a bf16-representable x is returned unchanged for every r; E[result] = x;
 *                                     a carry out of the largest finite value gives inf, as stated
 * Round to nearest stalls exp_avg_sq (beta2 = 0.999 moves v by 0.1 % of itself, under half a bf16 ulp: the store rounds it back);
 * it is there to be compared with.  The random bits of element i of the launch, with t = *t_dev (egk_adam_hyper has counted the
 * step) and e = elem0 + i:
 *     w = philox4x32_10(counter = (ctr_lo, ctr_hi, 0, 0), key = state_seed)[e & 3],  ctr = ((t & 0xFFFFFF) << 40) | (e >> 2)
 *     r(state0) = w >> 16,  r(state1) = w & 0xFFFF
 * One Philox call per 16-byte group of elements serves both buffers.  A draw is a function of (state_seed, counted step, absolute
 * element, buffer) and nothing else: not of how the flat buffers are cut into launches (elem0 = the absolute index of the launch's
 * first element), of the grid, of the group table or of the entry point.  *gate == 0 writes no state; the skipped step is taken
 * back out of the counter, so the next step that happens draws with the same t.  state_seed is the Philox KEY as given: a caller
 * that also runs the dropout kernels and the sampler of egopack_sample.h derives it from its seed so that no two consumers share a
 * (key, counter) pair (egopack_amd.ops.optim_state_key).
 * Refused behind every check above: an unknown state_dtype; state_round outside {0, 1}; state_round == 1 with f32 state or without
 * t_dev; elem0 negative, not a multiple of 4, or elem0 + n beyond 2^42; bf16 state pointers that are not 8-byte aligned.
 * egk_adam_step* (egopack_hip.h) take f32 state only. */
typedef struct egk_optim_desc {
    int32_t rule, g_dtype;
    int64_t n;
    float* p;
    const void* g;
    void* state0;
    void* state1;
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
    int32_t state_dtype;   /* EGK_F32 (0: the launch as it always was) | EGK_BF16: state0 / state1 hold bf16 */
    int32_t state_round;   /* 0: round to nearest even (f2bf's bits) | 1: stochastic; EGK_BF16 only */
    uint64_t state_seed;   /* the Philox KEY, as given */
    int64_t elem0;         /* absolute flat-buffer index of element 0 of this launch, a multiple of 4 */
} egk_optim_desc;

int egk_optim_step(egk_stream_t s, const egk_optim_desc* d);

#ifdef __cplusplus
}
#endif
#endif /* EGOPACK_OPTIM_H */
