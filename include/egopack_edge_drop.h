/*
 * egopack_edge_drop.h -- DropEdge (Rong et al., ICLR 2020) for the SAGE mean: the neighbour mean of a CSR graph over a seeded random
 * subset of every row's in-edges, and its backward over the transposed CSR with the SAME subset, regenerated, not stored.
 *
 * KEEP DECISION (a row of the Philox contract).  The edge goes from source j to destination i:
 *     (a, b) = (min(i, j), max(i, j)) with EGK_EDGE_DROP_SYMMETRIC, (i, j) without
 *     r      = philox4x32_10(counter = offset + word[0] + a, key = seed ^ ((uint64)b << 32)).x        (64-bit counter arithmetic,
 *                                                                                                      word == NULL counts as 0)
 *     keep   = float32(r >> 8) * 2^-24 >= float32(p)                                                   (the rule of egk_dropout_fwd)
 *     keep   = true where i == j with EGK_EDGE_DROP_KEEP_SELF
 * The decision is a function of (i, j) alone: the forward CSR (row i lists its sources) and the transposed CSR (row j lists its
 * destinations) regenerate the same bit without an edge-id map, and in symmetric mode i -> j and j -> i share it.  DUPLICATE EDGES of
 * a CSR share one decision.  A launch draws from the counters [offset + word, offset + word + rows): the caller reserves rows + 64.
 *
 * FORWARD (egk_csr_mean_drop_fwd), row i:  cnt = kept in-edges;  inv_deg[i] = cnt ? 1.f / (float)cnt : 0.f;
 *     out[i, :] = (sum over the kept edges of x[col[e], :], in f32, in CSR edge order) * inv_deg[i], rounded once to the element type.
 * No 1 / (1 - p) rescale: the mean is normalised by the kept count.  A row without a kept edge is all +0.
 * BACKWARD (egk_csr_mean_drop_bwd), row j of the transposed CSR (t_col[e] = a destination i of j):
 *     dx[j, :] = sum over the kept edges, in transposed-CSR order, of acc += inv_deg[i] * dout[i, :]  (f32), then
 *     dx[j, c] = gate[j, c] > 0 ? dx[j, c] : 0 with a gate, rounded once to the element type.  No edge weights are read.
 * ORDER: every output element's additions happen in CSR order over the kept edges, whatever the work distribution: one wave sums a
 * row of at most 12 edges, the 4 waves of a workgroup take a quarter of the columns each of a heavier row (every wave walks all its
 * edges, in order; rows of more than 64 edges wrap the 64-edge batch inside the launch).  No element's sum is split over waves:
 * the sums of egk_csr_gather on the thinned graph, bit for bit, for every row that launch sums in one wave.  Only the kept neighbour
 * rows are requested from memory.
 *
 * keep_out (uint8 [E], E = rowptr[rows], or NULL) receives 1 / 0 per edge in the order of the CSR the launch walks: for tests.
 * 16-byte (f32) / 8-byte (bf16) accesses along the row where cols % 4 == 0, element accesses otherwise.  A pointer that is not
 * aligned for the vector path is REFUSED, as egk_csr_gather refuses it; there is no fall-back.
 * Refused before any launch, each with its own message (egk_last_error): p outside [0, 1] or NaN; cols < 1 or cols > 4096; rows < 0;
 * a NULL x / out / inv_deg / rowptr / col (dout / dx / inv_deg / t_rowptr / t_col); an unknown dtype; unknown flag bits; a matrix
 * pointer not aligned for the vector path, inv_deg / rowptr / col not 4-byte aligned, word not 8-byte aligned.  rows == 0 passes the
 * checks and launches nothing.  Profile id "csr_mean_drop" (both launches).
 * THE CALLER GUARANTEES 0 <= col[e] < rows and a monotone rowptr: device data.
 *
 * Part of the C ABI of libegopack_hip.so: egopack_hip.h includes this file, a C user includes that one.  The boundary rules of
 * egopack_hip.h hold here word for word (stream-ordered, no allocation, no workspace, no global atomics, no synchronisation, capturable;
 * 0 = ok, negative = EGK_E*, positive = hipError_t; a launch touches only what its arguments name).  Scalars and pointers only.
 *
 * egopack_amd/_lib.py binds the prototypes below from ADDON_HEADERS["edge_drop"]; tests/test_cabi_addons.py is the ledger (what it
 * pins for this header: tests/cabi_addon_edge_drop.py) and tests/test_gpu_bounds_edge_drop.py holds the guard-band cases.
 */
#ifndef EGOPACK_EDGE_DROP_H
#define EGOPACK_EDGE_DROP_H

#include "egopack_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define EGK_EDGE_DROP_SYMMETRIC 1 /* flags bit 0: i -> j and j -> i share one decision */
#define EGK_EDGE_DROP_KEEP_SELF 2 /* flags bit 1: an edge i -> i is always kept */

/* x, out: [rows, cols] of ``dtype`` (EGK_F32 / EGK_BF16), rows ``cols`` elements apart; inv_deg: f32 [rows], WRITTEN. */
int egk_csr_mean_drop_fwd(egk_stream_t s, const void* x, const int32_t* rowptr, const int32_t* col, void* out, float* inv_deg,
                          uint8_t* keep_out, int32_t rows, int32_t cols, int32_t dtype, float p, int32_t flags, uint64_t seed,
                          uint64_t offset, const uint64_t* word);

/* dout, gate (or NULL), dx: [rows, cols] of ``dtype``; inv_deg: f32 [rows], READ (what the forward launch wrote). */
int egk_csr_mean_drop_bwd(egk_stream_t s, const void* dout, const int32_t* t_rowptr, const int32_t* t_col, const float* inv_deg,
                          const void* gate, void* dx, uint8_t* keep_out, int32_t rows, int32_t cols, int32_t dtype, float p,
                          int32_t flags, uint64_t seed, uint64_t offset, const uint64_t* word);

#ifdef __cplusplus
}
#endif
#endif /* EGOPACK_EDGE_DROP_H */
