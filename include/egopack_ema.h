/*
 * egopack_ema.h -- an exponential moving average of the weights (EMA, Polyak averaging) kept INSIDE the optimizer launch:
 * egk_optim_step / egk_optim_step_groups with one more f32 buffer, laid out like p, that follows the parameters the launch has
 * just formed.  The step is a replayed graph, the parameters have bf16 copies the launch keeps, a step may be skipped by the
 * gate and the step counter lives on the device: an average kept from outside would see none of that.  Inside the launch it is
 * 8 bytes per element on a 30-32 byte pass and no launch of its own.
 *
 * Part of the C ABI of libegopack_hip.so: egopack_hip.h includes this file, a C user includes that one.  The boundary rules
 * of egopack_hip.h hold here word for word (stream-ordered, no allocation, no synchronisation, capturable; 0 = ok, negative =
 * EGK_E*, positive = hipError_t; a launch touches only what its arguments name).
 *
 * The entry points of THIS header have their guard-band cases in tests/test_gpu_bounds_ema.py; the one ledger of all
 * headers, tests/test_cabi.py, holds them under the key "ema" (egopack_amd/_lib.py binds them from the prototypes below).
 */
#ifndef EGOPACK_EMA_H
#define EGOPACK_EMA_H

#include "egopack_optim_groups.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The average of one launch.  ema: device, [n] f32, 16-byte aligned, element i beside d->p[i].
 * decay in [0, 1).  warmup == 0: d_t = decay.  warmup != 0: d_t = min(decay, (1.0 + t) / (10.0 + t)) with t = *d->t_dev, the
 * step egk_adam_hyper has just counted -- read on the device, so a replayed graph needs no host value (t_dev must be given). */
typedef struct egk_ema_desc {
    float* ema;
    double decay;
    int32_t warmup;
} egk_ema_desc;

/* egk_optim_step(d) (g == NULL) or egk_optim_step_groups(d, g) with one addition: once element i's new p is formed, and before
 * it is stored, the same thread reads ema[i] and writes
 *     ema[i] = ema[i] + w * (p_new - ema[i]),   w = (float)(1.0 - d_t)
 * in f32, three separately rounded operations (no fused multiply-add); w is formed in double and rounded once.  The update
 * itself is the instruction sequence of the launch without the average: p, the state and both bf16 copies come out with its
 * bits.  All four kernel kinds, f32 and bf16 gradients, plain and grouped.  One writer per element, vector stores, no atomics.
 * The gate: as in every optimizer launch, d->gate is tested for NULL at run time (wave-uniform), there is no second
 * instantiation, and no device word holding 1 is needed when clipping is off.
 * A closed gate (*d->gate == 0) returns after that one load: ema, p, the state and the copies untouched, *bump_word moved on.
 * Refused before any launch: e or e->ema NULL, ema not 16-byte aligned, decay outside [0, 1), warmup with d->t_dev NULL, and
 * everything egk_optim_step / egk_optim_step_groups refuse.  Profile id "optim_ema": the rule's bytes + 8 per element. */
int egk_optim_step_ema(egk_stream_t s, const egk_optim_desc* d, const egk_optim_groups* g, const egk_ema_desc* e);

/* p[i] <-> ema[i] for i in [0, n): 16-byte accesses and a scalar tail, one writer per element.  Capturable.  Swapping twice
 * restores both buffers bit for bit.  Refused: NULL or not 16-byte aligned pointers, n < 0.  n == 0 launches nothing. */
int egk_ema_swap(egk_stream_t s, float* p, float* ema, int64_t n);

#ifdef __cplusplus
}
#endif
#endif /* EGOPACK_EMA_H */
