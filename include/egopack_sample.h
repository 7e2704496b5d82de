/*
 * egopack_sample.h -- K seeded categorical samples per logits row, for all heads of a task in ONE launch: the futures of the LTA
 * head (edit distance @ Z = 20, minimum over K = 5 futures) drawn from the library's counter-based Philox4x32-10 instead of torch's
 * device generator.  The sampler has no state: a draw is a function of (seed, batch ordinal, row, head, sample index) and nothing
 * else, so a set of weights has ONE edit distance -- the same in two runs, on one rank and on N, before and after a resume -- and
 * every draw can be predicted on the host (tests/lta_sampling_common.py over tests/philox_ref.py).
 *
 * The arithmetic of a row of C logits x_0 .. x_{C-1} (bf16 logits are widened to f32 first; everything below is f32):
 *     m   = max_c x_c
 *     e_c = expf(x_c - m)
 *     P_c = e_0 + ... + e_c      (inclusive prefix sum: serial inside a lane's 8 consecutive classes, a wave scan across the lanes,
 *                                 a carry across the 512-class chunks of a wider row)
 *     S   = P_{C-1}
 * Class c is LIVE when e_c > 0 (a -inf logit and an underflowed exponential are dead: never returned).
 *
 * The randomness of sample k of (batch ordinal b, row r, head h):
 *     ctr  = (b << 40) | (r << 16) | (h << 8) | (k >> 2)            b < 2^24, r < 2^24, h < 2^8, K <= 1024
 *     word = philox4x32_10(counter = (ctr_lo, ctr_hi, 0, 0), key = seed)[k & 3]
 *     u    = (float)(word >> 8) * 2^-24                             in [0, 1): the conversion of the dropout kernels
 * r = row0 + (the row's index in the launch).  ``seed`` is the Philox KEY as given: a caller that also runs the dropout kernels
 * derives it from its own seed so that the two consumers never share a (key, counter) pair (egopack_amd.ops.sampler_key).
 *
 * The selection:
 *     t      = u * S                                                (one f32 multiply)
 *     sample = the smallest live c with P_c > t
 *            = the largest live c when rounding leaves none         (the fallback: P of the last live class can sit an ulp under S)
 * A tree scan can leave P_c an ulp above P_{c-1} with e_c == 0, which is why dead classes are excluded by their e_c and not by
 * the scan.  A row with a NaN in it, or whose maximum is not finite (all -inf, a +inf), gets -1 in all K samples: it is read
 * once, for the maximum, and not again.  Columns c >= C (between C and ld) are never read.
 *
 * Optional outputs (tests): for every sample the bracket that selected it -- hi = P_c, lo = P of the live class before c (0 when
 * c is the first live class), total = S -- so that lo <= t < hi holds EXACTLY for every sample that did not take the fallback
 * (t recomputed on the host as fl32(u * total)) and lo / total, hi / total are the f32 CDF around the sample.  A -1 row writes
 * lo = hi = total = 0.  Null pointers: nothing is computed for them.
 *
 * Part of the C ABI of libegopack_hip.so: egopack_hip.h includes this file, a C user includes that one.  The boundary rules
 * of egopack_hip.h hold here word for word (stream-ordered, no allocation, no workspace, no synchronisation, capturable; 0 = ok,
 * negative = EGK_E*, positive = hipError_t; a launch touches only what its arguments name).
 *
 * The entry points of THIS header have their guard-band cases in tests/test_gpu_bounds_lta_sampling.py; the one ledger of all
 * headers, tests/test_cabi.py, holds them under the key "sample" (egopack_amd/_lib.py binds them from the prototypes below).
 * Profile id "categorical_sample".
 */
#ifndef EGOPACK_SAMPLE_H
#define EGOPACK_SAMPLE_H

#include "egopack_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define EGK_SAMPLE_MAX_TASKS 8
#define EGK_SAMPLE_MAX_K 1024

/* One head of a launch.  logits: [rows, C] of the launch's dtype, rows ``ld`` elements apart (ld >= C), aligned to its element.
 * out: int64, sample k of row r at out[r * out_row_stride + k * out_k_stride] (strides in elements, any sign-positive layout the
 * caller owns; 8-byte aligned).  head: the h of the counter.  lo / hi / total: all three NULL, or all three float [rows, K]
 * (row-major, contiguous). */
typedef struct egk_sample_task {
    const void* logits;
    int64_t ld;
    int32_t C;
    int32_t head;
    int64_t* out;
    int64_t out_row_stride;
    int64_t out_k_stride;
    float* lo;
    float* hi;
    float* total;
} egk_sample_task;

/* K samples of every row of every task: one wave per (task, row), four waves per workgroup, a grid-stride walk.  tasks: HOST
 * array of ``count`` entries (1 .. EGK_SAMPLE_MAX_TASKS), copied into the launch.  rows and K are shared by the tasks.
 * Refused with EGK_EINVAL before anything is launched: a null ``tasks``, count outside 1 .. 8, rows < 0, K outside 1 .. 1024,
 * ordinal outside [0, 2^24), row0 < 0 or row0 + rows > 2^24, an unknown dtype; per task a null logits / out pointer, C < 1,
 * ld < C, head outside [0, 256), negative strides, a misaligned pointer, lo / hi / total given in part.  rows == 0 passes the
 * same checks and launches nothing. */
int egk_categorical_sample(egk_stream_t s, const egk_sample_task* tasks, int32_t count, int32_t rows, int32_t K, uint64_t seed,
                           int64_t ordinal, int64_t row0, int32_t dtype);

#ifdef __cplusplus
}
#endif
#endif /* EGOPACK_SAMPLE_H */
