/*
 * egopack_optim_groups.h -- parameter groups of the flat-buffer optimizer: egk_optim_step with the learning rate and the weight
 * decay looked up PER ELEMENT from a segment table, in the one launch.  The flat layout is fixed by backward order, regions and
 * classifier banks, so the groups of a torch-style optimizer ("no decay on biases and LayerNorm rows", "a smaller lr for the
 * resumed backbone") interleave in it slot by slot; one launch per group would be one launch per slot.
 *
 * Part of the C ABI of libegopack_hip.so: egopack_hip.h includes this file, a C user includes that one.  The boundary rules
 * of egopack_hip.h hold here word for word (stream-ordered, no allocation, no synchronisation, capturable; 0 = ok, negative =
 * EGK_E*, positive = hipError_t; a launch touches only what its arguments name).
 *
 * The entry points of THIS header have their guard-band cases in tests/test_gpu_bounds_param_groups.py; the one ledger of all
 * headers, tests/test_cabi.py, holds them under the key "optim_groups" (egopack_amd/_lib.py binds them from the prototypes below).
 */
#ifndef EGOPACK_OPTIM_GROUPS_H
#define EGOPACK_OPTIM_GROUPS_H

#include "egopack_optim.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The segment table of one launch.  Segment k holds the absolute flat-buffer elements [seg_begin[k], seg_begin[k + 1]) and
 * belongs to group seg_group[k]; element i of the launch is the absolute element base + i.  Boundaries are multiples of 4, so
 * the 16-byte accesses of the kernel never straddle two groups; one table serves every slice of the flat buffers (the chunks of
 * the gradient exchange, the early and tail slices of the step) with base = the slice's first element.
 * A group id outside [0, n_groups) is clamped into it: no table content makes the kernel read outside the three tables.
 * Table pointers: seg_begin 8-byte aligned, seg_group 4-byte, group_hyper 16-byte. */
typedef struct egk_optim_groups {
    int64_t base;               /* absolute flat-buffer index of element 0 of this launch (multiple of 4) */
    int32_t n_seg, n_groups;    /* 1..4096, 1..64 */
    const int64_t* seg_begin;   /* device, [n_seg + 1], absolute element offsets, strictly increasing, multiples of 4,
                                   seg_begin[0] <= base, seg_begin[n_seg] >= base + n */
    const int32_t* seg_group;   /* device, [n_seg] */
    const float*   group_hyper; /* device, [n_groups][4] = {lr, weight_decay, 0, 0} */
} egk_optim_groups;

/* egk_optim_step(d) with two changes: element i takes lr and weight_decay from the group of the segment that holds base + i;
 * d->hyper[0] and d->weight_decay are ignored.  Everything else is egk_optim_step's: hyper[1..3] (bias corrections, grad scale
 * times clip coefficient), t_dev, the gate, the bump word, both bf16 copies, the gradient dtype, the four kernel kinds and
 * every refusal.  The per-group constants lr / hyper[1] and (float)(1.0 - (double)lr * (double)wd) are formed exactly as
 * egk_optim_step forms them, and the update is the same instruction sequence: a table of ONE group gives egk_optim_step's bits
 * for that lr / weight_decay, a table of several the bits of one egk_optim_step launch per segment. */
int egk_optim_step_groups(egk_stream_t s, const egk_optim_desc* d, const egk_optim_groups* g);

#ifdef __cplusplus
}
#endif
#endif /* EGOPACK_OPTIM_GROUPS_H */
