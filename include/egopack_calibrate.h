/*
 * egopack_calibrate.h -- post-hoc temperature calibration of a classification head (Guo et al. 2017), fitted on the device.
 *
 * One head: logits rows z_r of width C, labels y_r, beta = 1 / T > 0, p = softmax(beta z_r).  A row is VALID if 0 <= y_r < C.
 *     F(beta)   = sum_r  lse(beta z_r) - beta z_{r,y}              the NLL of the scaled logits
 *     F'(beta)  = sum_r  sum_c p_c z_c - z_{r,y}
 *     F''(beta) = sum_r  sum_c p_c (z_c - m_r)^2  >= 0,            m_r = sum_c p_c z_c
 * F is convex in beta, so the fit is a safeguarded Newton iteration on F' = 0 over [beta_min, beta_max]: per iteration one
 * egk_zero_fill of the accumulators, one egk_temp_stats per head and one egk_temp_newton, all on the stream; beta lives in device
 * memory, so no iteration needs the host.  The sums are INTEGERS (values times 2^24, rounded per row): integer addition is
 * associative, so launch order, batch order and the number of ranks whose accumulators are summed cannot change a bit.
 *
 * Row arithmetic of all launches, in f32 (bf16 logits are widened as they are read):
 *     x_c = fl(beta * z_c)                                          one separately rounded product, never fused
 *     lse = fl(max + logf(sum_c expf(x_c - max)))                   in the lane striding and reduction order of the loss kernels' row
 *                                                                   function (csrc/ce_row.h), so at beta = 1 it has egk_ce_fwd's bits
 *     nll = lse - x_y;   p_c = expf(x_c - lse);   m = sum_c p_c z_c;   d1 = m - z_y;   d2 = sum_c p_c (z_c - m)^2
 * A class with p_c == 0 adds nothing to m and d2 (a -inf logit in a finite row is a valid row).  Columns [C, ld) are never read.
 *
 * Part of the C ABI of libegopack_hip.so: egopack_hip.h includes this file, a C user includes that one.  The boundary rules of
 * egopack_hip.h hold here word for word (stream-ordered, no allocation, no synchronisation, capturable; 0 = ok, negative =
 * EGK_E*, positive = hipError_t; a launch touches only what its arguments name).  Scalars and pointers only: no struct.
 *
 * egopack_amd/_lib.py binds the prototypes below from its open third table, ADDON_HEADERS["calibrate"]; tests/test_cabi_addons.py
 * is the ledger of that table (what it pins for this header: tests/cabi_addon_calibrate.py) and
 * tests/test_gpu_bounds_calibration.py holds the guard-band cases.
 */
#ifndef EGOPACK_CALIBRATE_H
#define EGOPACK_CALIBRATE_H

#include "egopack_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define EGK_TEMP_MAX_HEADS 8
#define EGK_TEMP_MAX_K 64

/* The sums of one head at beta = *beta (ONE f32 read from device memory).  One wave per row, four waves per workgroup, at most 2048
 * workgroups with a strided row loop; a row of at most 512 classes is read once and kept in registers, a wider row is re-read.
 * logits: [rows, C] of ``dtype`` (EGK_F32 / EGK_BF16), rows ``ld`` elements apart; labels: int64, ``label_stride`` elements apart.
 * The launch ADDS to acc[8] (int64, 8-byte aligned):
 *     [0] += llrint(nll * 2^24)   [1] += llrint(d1 * 2^24)   [2] += llrint(d2 * 2^24)          of every valid row that is not left out
 *     [3] += valid rows           [4] += ignored rows (y < 0 or y >= C; they touch nothing else)
 *     [5] += valid rows left out: one of the three values is not finite or has magnitude >= 2^39, or beta itself is not a finite
 *            positive number
 *     [6], [7] are never touched.
 * Every wave sums its rows' integers in registers and issues one 64-bit integer atomic add per accumulator it has something for.
 * Refused before any launch: a null logits / labels / beta / acc, rows < 0, C < 1, ld < C, an unknown dtype, logits not aligned to
 * their element, beta not 4-byte aligned, labels or acc not 8-byte aligned.  rows == 0 launches nothing.  Profile id "temp_stats". */
int egk_temp_stats(egk_stream_t s, const void* logits, int64_t ld, const int64_t* labels, int64_t label_stride,
                   int32_t rows, int32_t C, const float* beta, int64_t* acc, int32_t dtype);

/* One safeguarded Newton step per head, one thread per head.  acc: [n_heads][8] as above, read only.  beta: f32 [n_heads], the
 * words egk_temp_stats reads.  state: [n_heads][8] doubles {beta, lo, hi, lo_seen, hi_seen, status, iterations, last relative step};
 * the caller starts a head at {b0, beta_min, beta_max, 0, 0, 0, 0, 0} with beta[h] = b0, an f32 value inside the bounds.
 * status: 0 running, 1 converged, 2 at beta_min, 3 at beta_max, 4 no valid rows.  A head whose status is not 0 is frozen: nothing of
 * it is written.  The rule of a running head, in f64, every operation rounded separately:
 *     iterations += 1;  acc[3] - acc[5] <= 0: status = 4, done
 *     F1 = acc[1] / 2^24,  F2 = acc[2] / 2^24
 *     F1 > 0:    hi = beta, hi_seen = 1;  beta <= beta_min: status = 2, done
 *     otherwise: lo = beta, lo_seen = 1;  beta >= beta_max: status = 3, done
 *     proposal = beta - F1 / F2  if F2 > 0,  else -inf if F1 > 0, else +inf
 *     proposal >= hi:  hi if hi was never evaluated (it is beta_max), else sqrt(lo * hi)
 *     proposal <= lo:  lo if lo was never evaluated (it is beta_min), else sqrt(lo * hi)
 *     the iterate is ROUNDED TO f32 before it is stored: state beta = (double)(float)new, beta[h] = that float -- the statistics
 *     are always taken at exactly the beta the state holds
 *     step = |new - beta| / beta is stored;  step <= stop: status = 1
 * Refused before any launch: a null pointer, n_heads outside 1 .. 8, acc or state not 8-byte aligned, beta not 4-byte aligned,
 * beta_min <= 0 (or not finite), beta_max < beta_min (or not finite), stop < 0 (or NaN).  Profile id "temp_newton". */
int egk_temp_newton(egk_stream_t s, const int64_t* acc, int32_t n_heads, double* state, float* beta,
                    float beta_min, float beta_max, float stop);

/* The probabilities of a GIVEN order at beta = *beta: prob[r * prob_row_stride + j] = expf(fl(beta z[r, idx[r, j]]) - lse_beta(r)),
 * j < k, and lse[r] = lse_beta(r) (NULL: not wanted).  idx is the raw order of egk_topk_softmax (include/egopack_topk.h): an INPUT,
 * never written and never recomputed -- fl(beta z) can merge two close logits into a tie, and a new ranking would then change what
 * is predicted.  An index outside [0, C) (egk_topk_softmax's -1 "no class") gives probability 0.  At beta == 1 the outputs have
 * egk_topk_softmax's bits.
 * Refused before any launch: a null logits / beta / idx / prob, rows < 0, C < 1, ld < C, k outside 1 .. 64, a row stride of idx or
 * prob below k, an unknown dtype, logits not aligned to their element, idx not 8-byte aligned, beta / prob / lse not 4-byte aligned.
 * rows == 0 launches nothing.  Profile id "temp_topk_prob". */
int egk_temp_topk_prob(egk_stream_t s, const void* logits, int64_t ld, int32_t rows, int32_t C, const float* beta,
                       const int64_t* idx, int64_t idx_row_stride, int32_t k, float* prob, int64_t prob_row_stride,
                       float* lse, int32_t dtype);

/* out[r * ldo + c] = fl(beta * z[r, c]) for c < C: one f32 product per element (what the LTA sampler draws from at a sampling
 * temperature).  Columns [C, ldo) of ``out`` are untouched.
 * Refused before any launch: a null logits / beta / out, rows < 0, C < 1, ld < C, ldo < C, an unknown dtype, logits not aligned to
 * their element, beta or out not 4-byte aligned.  rows == 0 launches nothing.  Profile id "temp_scale_rows". */
int egk_temp_scale_rows(egk_stream_t s, const void* logits, int64_t ld, int32_t rows, int32_t C, const float* beta,
                        float* out, int64_t ldo, int32_t dtype);

#ifdef __cplusplus
}
#endif
#endif /* EGOPACK_CALIBRATE_H */
