/*
 * egopack_mixup.h -- sequence mixup (Zhang et al. 2018) for the verb / noun heads: a convex combination of the rows of two
 * sequences in front of the backbone, and the cross entropy of one logits row against TWO labels behind it.
 *
 * The pairing (which row is mixed with which) and the coefficients are drawn on the host and travel with the batch
 * (egopack_amd.data: the fields mix_src, mix_lam, mix_y); the device does the two things that cost bytes and precision.
 *
 * ROW MIX (egk_mix_rows_multi), per element, in f32 (bf16 elements are widened as they are read), THREE operations, each rounded
 * once, never fused with anything else:
 *     u   = fl(1 - lam[r])
 *     t   = fl(lam[r] * in[r, c])
 *     out = fma(u, in[src[r], c], t)              one rounding of u * b + t; then ONE rounding to the element type
 * so |out - (lam a + (1 - lam) b)| <= 3 * 2^-24 * (|lam a| + |(1 - lam) b|) for an f32 output (one relative rounding each: u, t
 * and the fused sum).  Rows that need no arithmetic are COPIED, bit for bit (NaN payloads and -0 included):
 *     lam[r] == 1 or src[r] == r     out[r, :] = in[r, :]
 *     lam[r] == 0                    out[r, :] = in[src[r], :]
 *
 * TWO-TARGET CROSS ENTROPY (egk_ce_mix_fused_multi): the two-target form of egk_ce_fused_multi_s.  Row n of head h with labels
 * a = y[n, h], b = y_b[n, h] (live when in [0, C), ignored otherwise), eps = smoothing, g = fl(gscale * scale[0]) (gscale without a
 * scale: egopack_task_scale.h):
 *     la = lam[n] if a is live else 0,   lb = fl(1 - lam[n]) if b is live else 0,   W = fl(la + lb)
 *     lse, sum_c z_c                             formed ONCE per row and head, by the function the plain launch forms them with
 *     CE(t) = lse - (1 - eps) z_t - eps / C * sum_c z_c        the plain launch's own function (csrc/ce_row.h), 0 for an ignored t
 *     loss[n] = sum over the heads of  [la > 0] fl(la * CE(a))  +  [lb > 0] fl(lb * CE(b))
 *     p = expf(z_c - lse)
 *     dz_c = fl(g * fl(fl(fl(W * p) - fl((1 - eps) * fl(fl(la * [c == a]) + fl(lb * [c == b])))) - fl(W * fl(eps / C))))
 * every operation of the last line rounded separately (compiled without contraction).  W == 0 (both labels ignored, or the only
 * live label has coefficient 0): loss 0 and dz = +0.  Columns [C, pad) of a head's block are set to zero.
 * THE lam == 1 IDENTITY: with lam[n] == 1, la = 1, lb = 0, W = 1 (a live), every extra factor is an exact multiplication by 1 and
 * every extra term an exact 0: the row's loss and gradient are BIT FOR BIT those of egk_ce_fused_multi_s on (z, y), f32 and bf16,
 * whatever y_b holds.  With lam[n] == 0 they are those of the plain launch on (z, y_b).
 *
 * The row mix is csrc/mixup.hip; the two-target cross entropy is a mode of the fused cross-entropy kernel and shares its packer
 * (csrc/loss.hip, the row arithmetic in csrc/ce_row.h).
 *
 * Part of the C ABI of libegopack_hip.so: egopack_hip.h includes this file, a C user includes that one.  The boundary rules of
 * egopack_hip.h hold here word for word (stream-ordered, no allocation, no workspace, no synchronisation, capturable; 0 = ok,
 * negative = EGK_E*, positive = hipError_t; a launch touches only what its arguments name).  Scalars and pointers only: no struct.
 *
 * egopack_amd/_lib.py binds the prototypes below from its open third table, ADDON_HEADERS["mixup"]; tests/test_cabi_addons.py is
 * the ledger of that table (what it pins for this header: tests/cabi_addon_mixup.py) and tests/test_gpu_bounds_mixup.py holds the
 * guard-band cases.
 */
#ifndef EGOPACK_MIXUP_H
#define EGOPACK_MIXUP_H

#include "egopack_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define EGK_MIX_MAX_SEGMENTS 4
#define EGK_CE_MIX_MAX_TASKS 4
#define EGK_CE_MIX_MAX_HEADS 4

/* out[r, c] = lam[r] * in[r, c] + (1 - lam[r]) * in[src[r], c] for up to 4 SEGMENTS (the task batches of a merged input) in ONE
 * launch.  One wave per row, four waves per workgroup; the rows of all segments are walked as one list, XCD x owning a contiguous
 * eighth of it (the row kernels' rule), with ordinary stores: the contraction that reads the output next finds its rows in the L2
 * of the XCD that produced them.  16-byte accesses along the row where every segment's pointers are 16-byte aligned and its row
 * strides are multiples of 16 bytes, with a scalar tail for the columns behind the last whole vector; element accesses otherwise.
 *   HOST arrays of n_seg entries: x_in, x_out (device, [rows, cols] of ``dtype``, EGK_F32 / EGK_BF16, rows ld_in / ld_out elements
 *   apart; columns [cols, ld) are neither read nor written), ld_in, ld_out, rows, src (device int32 [rows] or NULL), lam (device
 *   f32 [rows] or NULL).  src and lam are both given or both NULL; both NULL: the segment is a plain copy -- how an unmixed task's
 *   rows of a merged buffer reach the output.  src[r] is the partner ROW OF THE SEGMENT.
 * THE CALLER GUARANTEES 0 <= src[r] < rows: it is device data and cannot be checked on the host (the loader's construction is a
 * permutation of the segment's rows).
 * OUT OF PLACE: an x_out range that overlaps any x_in range (of any segment) is refused -- an in-place mix would read partners
 * after they were written, and a replay over an input that was not restaged would mix the mix.
 * Refused before any launch: a null host array; n_seg outside 1 .. 4; cols < 1; an unknown dtype; per segment: rows < 0, a null
 * x_in / x_out (with rows > 0), ld_in < cols or ld_out < cols, src without lam or lam without src, a pointer not aligned to its
 * element (src, lam: 4 bytes), overlapping in / out ranges, output ranges of two segments that overlap.  Segments with rows == 0
 * pass the checks (for the overlap rule a segment without rows counts as one row: an in-place call is refused whatever its size);
 * nothing is launched when every segment is empty.  Profile id "mix_rows". */
int egk_mix_rows_multi(egk_stream_t s, int32_t n_seg, const void* const* x_in, void* const* x_out, const int64_t* ld_in,
                       const int64_t* ld_out, const int32_t* rows, const int32_t* const* src, const float* const* lam, int32_t cols,
                       int32_t dtype);

/* The fused cross entropy of up to 4 tasks x 4 heads against two labels per row: loss AND dlogits in one launch (the grid, the row
 * ownership and the layout of egk_ce_fused_multi: one wave per row, blockIdx.y = task).  The array form of egk_ce_fused, per task:
 *   HOST arrays of count * 4 entries, entry [4 * t + h] for head h < n_heads[t] of task t: logits (device f32 [rows, C], rows ld
 *   elements apart), ld, C, pad (columns [C, pad) of the head's gradient block are zero-filled), dcol (first column of the head's
 *   block in the task's gradient matrix).
 *   HOST arrays of count entries: n_heads, y and y_b (device int64, label of head h of row n at [n * y_stride + h], both with the
 *   same stride), y_stride, lam (device f32 [rows]), loss (device f32 [rows], overwritten with the sum over the heads), dlogits
 *   (device, ``dtype``, rows ldd elements apart), ldd, rows, gscale, scales (NULL: no task has a scale; else per task a device f32
 *   word or NULL).
 * lam[n] is expected in [0, 1] (device data, not checked).
 * Refused before any launch: a null host array (scales excepted); count outside 1 .. 4; n_heads outside 1 .. 4; a null logits / y /
 * y_b / lam / loss / dlogits pointer; rows < 0; C < 1; pad < C; an unknown dtype; lam or a scale not 4-byte aligned.  Tasks with
 * rows == 0 pass the checks; nothing is launched when every task is empty.  Profile id "ce_mix". */
int egk_ce_mix_fused_multi(egk_stream_t s, int32_t count, const float* const* logits, const int64_t* ld, const int32_t* C,
                           const int32_t* pad, const int64_t* dcol, const int32_t* n_heads, const int64_t* const* y,
                           const int64_t* const* y_b, const int64_t* y_stride, const float* const* lam, float* const* loss,
                           void* const* dlogits, const int64_t* ldd, const int32_t* rows, const float* gscale,
                           const float* const* scales, float smoothing, int32_t dtype);

#ifdef __cplusplus
}
#endif
#endif /* EGOPACK_MIXUP_H */
