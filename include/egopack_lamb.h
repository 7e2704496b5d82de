/*
 * egopack_lamb.h -- LAMB (You et al. 2020), the layer-wise adaptive rule of the flat-buffer optimizer: Adam's moments, an update
 * u that carries the weight decay, and per SLOT of the flat layout (one parameter tensor with its alignment and 64-row padding)
 * a trust ratio ||p|| / ||u|| that rescales the learning rate.  No element of a slot may move before both norms of the whole
 * slot exist, so the rule is three launches: reduce (egk_lamb_moments), one ratio per slot (egk_lamb_trust), apply
 * (egk_lamb_apply).  No atomics: every word of device memory has one writer per step, every sum has a fixed order, and the same
 * inputs give the same bits on every run.
 *
 * With t the counted step, hyper = {lr, 1 - b1^t, sqrt(1 - b2^t), s} as egk_adam_hyper (and egk_grad_norm_finalize) write it,
 * lr and wd those of the slot's parameter group, every f32 operation rounded separately (no fused multiply-add):
 *     g' = g * s;  m += (g' - m) * (1 - b1);  v = v * b2 + (1 - b2) * g' * g'        (1 - b taken in double, rounded once)
 *     u  = (m / hyper[1]) / (sqrt(v) / hyper[2] + eps) + wd * p
 *     per slot S:  P = sum p^2,  U = sum u^2                                         (products and sums in f64)
 *     trust_S = 1                          if (wd == 0 and not always_adapt) or P == 0 or U == 0
 *             = (float)(sqrt(P) / sqrt(U)) otherwise;   trust_clip: min(trust_S, 1)
 *     p -= (lr * trust_S) * u
 * A slot's padding has p = m = v = g = 0, hence u = 0 (eps > 0): it adds nothing to either sum and stays zero.
 *
 * The tables (device memory, built once by the caller; n_slots >= 1):
 *     slot_begin   int64 [n_slots + 1]   first element of every slot, sorted, multiples of 4; slot_begin[n_slots] = the buffers' length
 *     slot_piece0  int32 [n_slots + 1]   first PIECE of every slot: a slot is cut into pieces of EGK_LAMB_PIECE elements, its last
 *                                        piece shorter; a piece never crosses a slot boundary; slot_piece0[n_slots] = the piece count
 *     slot_group   int32 [n_slots]       the slot's row of group_hyper (clamped into [0, n_groups))
 *     group_hyper  f32 [n_groups][4]     {lr, weight_decay, 0, 0} per parameter group, 16-byte aligned (include/egopack_optim_groups.h)
 *     part         f64 [pieces][2][2]    the partial sums {P, U} of every piece: half 0 is the part of the piece that starts at its
 *                                        first element, half 1 the part that ends at its last
 *
 * Part of the C ABI of libegopack_hip.so: egopack_hip.h includes this file, a C user includes that one.  The boundary rules of
 * egopack_hip.h hold here word for word (stream-ordered, no allocation, no synchronisation, capturable; 0 = ok, negative =
 * EGK_E*, positive = hipError_t; a launch touches only what its arguments name).  Scalars and pointers only: no struct.
 *
 * egopack_amd/_lib.py binds the prototypes below from its second table, EXTRA_HEADERS["lamb"]; tests/test_cabi_lamb.py is this
 * header's ledger and tests/test_gpu_bounds_lamb.py holds its guard-band cases.
 */
#ifndef EGOPACK_LAMB_H
#define EGOPACK_LAMB_H

#include "egopack_hip.h"

#define EGK_LAMB_PIECE 4096

#ifdef __cplusplus
extern "C" {
#endif

/* The moments and the partial sums over the ABSOLUTE element range [lo, hi) of the flat buffers p, g, m, v (base pointers, 16-byte
 * aligned; g: f32, or with g_dtype == EGK_BF16 the bf16 copy of a compressed exchange, 8-byte aligned).  lo and hi are multiples
 * of 8.  piece0 / n_pieces: the first piece that meets the range and how many do; one 256-thread workgroup per piece updates m and
 * v on piece /\ [lo, hi), forms u, adds p^2 and u^2 in f64 (per thread in element order, a shuffle tree per wave, the four waves
 * in order through LDS) and writes ONE half of part[piece]: a workgroup that covers its whole piece writes half 0 and zeroes half
 * 1; one that covers a front part writes half 0 alone, one that covers a back part half 1 alone.  A piece may therefore be cut
 * ONCE per step (a gradient-exchange chunk boundary), and whole pieces give the same bits however the buffer is sliced.  p is
 * read, never written.
 * The caller guarantees that [lo, hi) does not lie strictly inside one piece and that piece0 / n_pieces are those of the range.
 * meets_piece_bound != 0 is the caller's statement that [lo, hi] holds a piece boundary (a range of EGK_LAMB_PIECE elements always
 * does): the one thing that rules the forbidden case out and that the host cannot see without the table.
 * gate (NULL: none): *gate == 0 closes the launch -- m, v and part untouched.  bump_word (NULL: none): *bump_word += bump, gate
 * open or closed, as in every optimizer launch.
 * Refused before any launch: a NULL or misaligned pointer, an unknown g_dtype, lo < 0, lo >= hi, lo or hi no multiple of 8, a
 * range shorter than EGK_LAMB_PIECE without meets_piece_bound, piece0 < 0, n_pieces < 1, n_slots < 1, n_groups outside 1..64,
 * eps <= 0, a beta outside [0, 1).  Profile id "lamb_moments": 24 bytes per element (22 with a bf16 gradient). */
int egk_lamb_moments(egk_stream_t s, const float* p, const void* g, int32_t g_dtype, float* m, float* v, int64_t lo, int64_t hi,
                     int32_t piece0, int32_t n_pieces, int32_t meets_piece_bound, const int64_t* slot_begin, const int32_t* slot_piece0,
                     const int32_t* slot_group, int32_t n_slots, const float* group_hyper, int32_t n_groups, const float* hyper,
                     double beta1, double beta2, float eps, double* part, const int32_t* gate, int64_t* bump_word, int64_t bump);

/* One wave per slot: the lanes add the halves of the slot's pieces in a fixed strided order in f64 (lane l: pieces l, l + 64, ...,
 * half 0 then half 1; then the shuffle tree), lane 0 writes trust[slot] (f32) and norms[slot] = {sqrt(P), sqrt(U)} (f64, for
 * reporting).  A closed gate leaves both alone.  Refused: a NULL or misaligned pointer, n_slots < 1, n_groups outside 1..64.
 * Profile id "lamb_trust": 32 bytes per piece, which the host does not know and counts as 0. */
int egk_lamb_trust(egk_stream_t s, const double* part, const int32_t* slot_piece0, const int32_t* slot_group, int32_t n_slots,
                   const float* group_hyper, int32_t n_groups, int32_t trust_clip, int32_t always_adapt, float* trust, double* norms,
                   const int32_t* gate);

/* The update over the whole buffers, [0, n) with n = slot_begin[n_slots] and n_pieces = slot_piece0[n_slots]: one workgroup per
 * piece recomputes u from the stored m and v and the old p -- the function, and so the bits, the reduce launch summed -- and stores
 * p - (lr * trust[slot]) * u, bf16_shadow (egk_cast's bits of the stored p) and, if given, bf16_lo_shadow (egk_split_bf16's).
 * ema (NULL: none): the weight average of include/egopack_ema.h moved towards the new p inside the launch, with ema_decay and
 * ema_warmup as egk_ema_desc takes them (warmup needs t_dev).  A closed gate leaves everything untouched.
 * Refused: a NULL or misaligned pointer (p, m, v, ema 16-byte; the copies 8-byte), n < 1, n_pieces < 1, n_slots < 1, n_groups
 * outside 1..64, eps <= 0, ema_decay outside [0, 1), ema_warmup without t_dev.
 * Profile id "lamb_apply": 16 bytes per element + 2 per bf16 copy + 8 with the average. */
int egk_lamb_apply(egk_stream_t s, float* p, const float* m, const float* v, int64_t n, int32_t n_pieces, const int64_t* slot_begin,
                   const int32_t* slot_piece0, const int32_t* slot_group, int32_t n_slots, const float* group_hyper, int32_t n_groups,
                   const float* hyper, float eps, const float* trust, void* bf16_shadow, void* bf16_lo_shadow, float* ema,
                   double ema_decay, int32_t ema_warmup, const int64_t* t_dev, const int32_t* gate);

/* Knob of the measurements (profiles/lamb_cost.txt): key 0 = "m, v and p stay cacheable between the reduce and the apply launch"
 * (1, the default) or stream like everything else under the mask of egk_tune(9) (0).  Returns the previous value, -1 for an unknown
 * key; a value outside {0, 1} only queries.  Changes no arithmetic. */
int egk_lamb_tune(int32_t key, int32_t value);

#ifdef __cplusplus
}
#endif
#endif /* EGOPACK_LAMB_H */
