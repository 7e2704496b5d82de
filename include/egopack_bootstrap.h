/*
 * egopack_bootstrap.h -- a seeded cluster bootstrap of ratio metrics: R Poisson(1) replicates of integer (numerator, denominator) sums
 * over the rows of a validation batch, every row weighted by the weight of the CLUSTER (the sample: sequence or clip) it belongs to.
 *
 * WEIGHT (a row of the Philox contract).  Replicate r gives cluster c the integer weight
 *     ctr  = (c << 14) | (r >> 2)                                  0 <= c < 2^40, 0 <= r < R <= EGK_BOOT_MAX_R
 *     word = philox4x32_10(counter = (ctr_lo, ctr_hi, 0, 0), key)[r & 3]
 *     w    = #{ k in 0 .. 11 : word >= T[k] },  T[k] = floor(2^32 * sum_{j <= k} e^-1 / j!)          0 <= w <= 12
 *     T    = 1580030168, 3160060337, 3950075421, 4213413783, 4279248373, 4292415291, 4294609777, 4294923276, 4294962463, 4294966817,
 *            4294967252, 4294967292
 * Integer comparisons only: a host model has the same bits.  The weight is a function of (key, c, r) alone -- not of the row, the
 * batch, the launch or the rank.  A row with cluster < 0 has weight 0 in every replicate.  THE CALLER GUARANTEES cluster < 2^40:
 * device data, which the host cannot see.
 *
 * ACCUMULATE (egk_bootstrap_accumulate).  num / den: int64 [rows, M], rows ``ld`` elements apart.  For every replicate r and column m
 *     acc_num[r, m] += sum over the rows of w(cluster[row], r) * num[row, m]          acc_den likewise with den
 * and, with 0 <= class_col < M and y = label[row * label_stride], for the rows with 0 <= y < C
 *     cls_den[r, y] += w where den[row, class_col] != 0          cls_num[r, y] += w where num[row, class_col] != 0.
 * A label outside [0, C) leaves the class part alone; the row still counts in the column sums.  acc_*: int64 [R, M], cls_*: int64
 * [R, C], row-major; the launch ADDS into them.  class_col = -1: no class part; label, cls_num and cls_den may be NULL.
 * One workgroup owns four consecutive replicates and walks all rows: every word of acc_* and cls_* has one writer per launch, which
 * adds with a plain load and store.  No global atomics, integer sums only: the result does not depend on the grid, on the order of
 * the rows or on how the rows are split over launches.  int64 sums wrap silently; the class counts are int32 inside a launch, which
 * the bound on rows keeps from wrapping (12 * 2^24 < 2^31).
 *
 * WEIGHTS (egk_bootstrap_weights): w[row, r] = the weight above as uint8, [rows, R] row-major (0 where cluster[row] < 0): for tests
 * and for checking a host model.
 *
 * Refused before any launch, each with its own message (egk_last_error): a NULL cluster / num / den / acc_num / acc_den (cluster / w);
 * rows < 0 or rows > 2^24; M outside 1 .. EGK_BOOT_MAX_M; R outside 1 .. EGK_BOOT_MAX_R (R need not be a multiple of 4); ld < M;
 * class_col outside [-1, M); class_col >= 0 with a NULL label / cls_num / cls_den or C outside 1 .. EGK_BOOT_MAX_C; an int64 pointer
 * that is not 8-byte aligned.  rows == 0 passes the checks and launches nothing.  Profile id "bootstrap" (both launches).
 *
 * Part of the C ABI of libegopack_hip.so: egopack_hip.h includes this file, a C user includes that one.  The boundary rules of
 * egopack_hip.h hold here word for word (stream-ordered, no allocation, no workspace, no global atomics, no synchronisation, capturable;
 * 0 = ok, negative = EGK_E*, positive = hipError_t; a launch touches only what its arguments name).  Scalars and pointers only.
 *
 * egopack_amd/_lib.py binds the prototypes below from ADDON_HEADERS["bootstrap"]; tests/test_cabi_addons.py is the ledger (what it
 * pins for this header: tests/cabi_addon_bootstrap.py) and tests/test_gpu_bounds_bootstrap.py holds the guard-band cases.
 */
#ifndef EGOPACK_BOOTSTRAP_H
#define EGOPACK_BOOTSTRAP_H

#include "egopack_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define EGK_BOOT_MAX_R 65536
#define EGK_BOOT_MAX_M 8
#define EGK_BOOT_MAX_C 1024

int egk_bootstrap_accumulate(egk_stream_t s, const int64_t* cluster, const int64_t* num, const int64_t* den, int64_t ld,
                             int32_t rows, int32_t M, const int64_t* label, int64_t label_stride, int32_t class_col, int32_t C,
                             int64_t* acc_num, int64_t* acc_den, int64_t* cls_num, int64_t* cls_den, int32_t R, uint64_t key);
int egk_bootstrap_weights(egk_stream_t s, const int64_t* cluster, int32_t rows, int32_t R, uint64_t key, uint8_t* w /* [rows, R] */);

#ifdef __cplusplus
}
#endif
#endif /* EGOPACK_BOOTSTRAP_H */
