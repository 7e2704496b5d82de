// Sequence mixup (include/egopack_mixup.h):
//   egk_mix_rows_multi       out[r] = lam[r] in[r] + (1 - lam[r]) in[src[r]] for the rows of up to 4 segments, out of place, one launch
//   egk_ce_mix_fused_multi   the fused cross entropy of up to 4 tasks x 4 heads against two labels per row: loss and dlogits
// Plain C++: one wave per row, four waves per workgroup, at most 2048 workgroups, the row walk of the other row kernels (common.h:
// XCD x owns a contiguous eighth of the rows); no LDS, no workspace, no atomics.  The mix is HBM-bound: 16-byte accesses along the
// row, ordinary stores (the first contraction reads the output next, from the L2 of the XCD that wrote it).  The forward pass of
// the loss is the plain row function's (ce_row.h), operation by operation, so that a row with lam == 1 has the plain launch's bits.
// Every launcher refuses its argument errors on the host before it launches.
#include <math.h>

#include "ce_row.h"
#include "common.h"

namespace egk {

constexpr int MIX_WPB = 4;
static inline int mix_row_grid(int rows) {
    int g = cdiv(rows, MIX_WPB);
    return g < 1 ? 1 : (g > 2048 ? 2048 : g);
}

// ---- the row mix ----------------------------------------------------------------------------------------------------------------
struct MixArgs {
    const void* in[EGK_MIX_MAX_SEGMENTS];
    void* out[EGK_MIX_MAX_SEGMENTS];
    const int* src[EGK_MIX_MAX_SEGMENTS];    // null: the segment is copied
    const float* lam[EGK_MIX_MAX_SEGMENTS];
    long long ld_in[EGK_MIX_MAX_SEGMENTS], ld_out[EGK_MIX_MAX_SEGMENTS];
    int row0[EGK_MIX_MAX_SEGMENTS];          // first row of the segment in the list of all rows; ``total`` behind the last segment
    int total, cols;
};

// the three operations of the header, each rounded once: u = fl(1 - lam) (per row), t = fl(lam * a), fma(u, b, t)
__device__ __forceinline__ float mix_u(float lam) {
#pragma clang fp contract(off)
    return 1.f - lam;
}
__device__ __forceinline__ float mix1(float lam, float u, float a, float b) {
#pragma clang fp contract(off)
    const float t = lam * a;
    return __builtin_fmaf(u, b, t);
}

template <typename T> struct MixVec;
template <> struct MixVec<float> {
    static constexpr int N = 4;
    __device__ static __forceinline__ uint4 mix(uint4 a, uint4 b, float lam, float u) {
        uint4 o;
        o.x = __float_as_uint(mix1(lam, u, __uint_as_float(a.x), __uint_as_float(b.x)));
        o.y = __float_as_uint(mix1(lam, u, __uint_as_float(a.y), __uint_as_float(b.y)));
        o.z = __float_as_uint(mix1(lam, u, __uint_as_float(a.z), __uint_as_float(b.z)));
        o.w = __float_as_uint(mix1(lam, u, __uint_as_float(a.w), __uint_as_float(b.w)));
        return o;
    }
};
template <> struct MixVec<bf16_t> {
    static constexpr int N = 8;
    __device__ static __forceinline__ unsigned mix2(unsigned a, unsigned b, float lam, float u) {
        const float lo = mix1(lam, u, __uint_as_float(a << 16), __uint_as_float(b << 16));
        const float hi = mix1(lam, u, __uint_as_float(a & 0xffff0000u), __uint_as_float(b & 0xffff0000u));
        return (unsigned)f2bf(lo) | ((unsigned)f2bf(hi) << 16);
    }
    __device__ static __forceinline__ uint4 mix(uint4 a, uint4 b, float lam, float u) {
        return make_uint4(mix2(a.x, b.x, lam, u), mix2(a.y, b.y, lam, u), mix2(a.z, b.z, lam, u), mix2(a.w, b.w, lam, u));
    }
};

// VEC: every segment's pointers and row strides admit 16-byte accesses (decided on the host); columns behind the last whole vector
// and, without VEC, all columns go one element at a time.
template <typename T, bool VEC>
__global__ __launch_bounds__(256) void mix_rows_kernel(const MixArgs A) {
    constexpr int NV = MixVec<T>::N;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int cols = A.cols, nvec = VEC ? cols / NV : 0;
    const RowWalk rw = row_walk(blockIdx.x, gridDim.x, 0, A.total, wave, MIX_WPB);  // (XCD x owns a contiguous eighth of the rows: common.h)
    for (int row = rw.first; row < rw.end; row += rw.step) {
        // the row's segment: the last one that begins at or before it (empty segments begin where the next one does)
        const T* in = (const T*)A.in[0];
        T* out = (T*)A.out[0];
        const int* srcp = A.src[0];
        const float* lamp = A.lam[0];
        long long ld_in = A.ld_in[0], ld_out = A.ld_out[0];
        int base = 0;
#pragma unroll
        for (int s = 1; s < EGK_MIX_MAX_SEGMENTS; ++s)
            if (row >= A.row0[s]) {
                in = (const T*)A.in[s]; out = (T*)A.out[s]; srcp = A.src[s]; lamp = A.lam[s];
                ld_in = A.ld_in[s]; ld_out = A.ld_out[s]; base = A.row0[s];
            }
        const int r = row - base;
        float lam = 1.f;
        int sr = r;
        if (srcp) {
            lam = lamp[r];
            sr = srcp[r];
        }
        const T* __restrict__ a = in + (long long)r * ld_in;
        const T* __restrict__ b = in + (long long)sr * ld_in;
        T* __restrict__ o = out + (long long)r * ld_out;
        if (lam == 1.f || sr == r || lam == 0.f) {  // no arithmetic: the bits of this row, or of the partner's
            const T* __restrict__ from = (lam == 1.f || sr == r) ? a : b;
            for (int v = lane; v < nvec; v += 64) reinterpret_cast<uint4*>(o)[v] = reinterpret_cast<const uint4*>(from)[v];
            for (int c = nvec * NV + lane; c < cols; c += 64) o[c] = from[c];
        } else {
            const float u = mix_u(lam);
            for (int v = lane; v < nvec; v += 64)
                reinterpret_cast<uint4*>(o)[v] = MixVec<T>::mix(reinterpret_cast<const uint4*>(a)[v], reinterpret_cast<const uint4*>(b)[v], lam, u);
            for (int c = nvec * NV + lane; c < cols; c += 64) st1t(o + c, mix1(lam, u, ld1t(a + c), ld1t(b + c)));
        }
    }
}

// ---- the two-target cross entropy ---------------------------------------------------------------------------------------------------
struct CEMixTasks {
    const float* logits[EGK_CE_MIX_MAX_TASKS][EGK_CE_MIX_MAX_HEADS];
    long long ld[EGK_CE_MIX_MAX_TASKS][EGK_CE_MIX_MAX_HEADS];
    long long dcol[EGK_CE_MIX_MAX_TASKS][EGK_CE_MIX_MAX_HEADS];
    int C[EGK_CE_MIX_MAX_TASKS][EGK_CE_MIX_MAX_HEADS];
    int pad[EGK_CE_MIX_MAX_TASKS][EGK_CE_MIX_MAX_HEADS];
    const long long* y[EGK_CE_MIX_MAX_TASKS];
    const long long* yb[EGK_CE_MIX_MAX_TASKS];
    const float* lam[EGK_CE_MIX_MAX_TASKS];
    float* loss[EGK_CE_MIX_MAX_TASKS];
    void* dlogits[EGK_CE_MIX_MAX_TASKS];
    const float* scale[EGK_CE_MIX_MAX_TASKS];
    long long ys[EGK_CE_MIX_MAX_TASKS], ldd[EGK_CE_MIX_MAX_TASKS];
    int n_heads[EGK_CE_MIX_MAX_TASKS], rows[EGK_CE_MIX_MAX_TASKS];
    float gscale[EGK_CE_MIX_MAX_TASKS];
};

// The plain launch's loss of a live label, WRITTEN AS ce_row_plain WRITES IT (ce_row.h) and compiled like it: no pragma here.
// The lam == 1 identity of the LOSS rests on the compiler contracting (or not) the multiply-adds of this expression here as it
// does there -- two inlinings of the same text under the same flags.  Nothing in the language promises that: it is pinned by
// tests/test_gpu_mixup.py::test_ce_mix_lam_one_is_the_plain_launch_bit_for_bit, which a compiler upgrade has to pass.  (The
// gradient needs no such luck: the plain form has no multiply-add to contract.)
__device__ __forceinline__ float ce_plain_loss(const float* __restrict__ lr, float l, long long t, float sx, float smoothing, int C) {
    return l - (1.f - smoothing) * ld1t(lr + t) - (smoothing > 0.f ? smoothing / C * sx : 0.f);
}

// What the two labels add to the plain row: every operation rounded separately (the header's order).  With la == 1, lb == 0 every
// extra factor is an exact 1 and every extra term an exact 0.
template <typename T>
__device__ __forceinline__ float ce_mix_tail(const float* __restrict__ lr, int C, int pad, long long a, long long b, bool alive,
                                             bool blive, float lam, float ca, float cb, float l, float smoothing, float g,
                                             T* __restrict__ dr, int lane) {
#pragma clang fp contract(off)  // (the f32 and the bf16 instantiation form the same f32 value: no fusing that depends on the code around)
    const float la = alive ? lam : 0.f, lb = blive ? 1.f - lam : 0.f, W = la + lb;
    float loss = la > 0.f ? la * ca : 0.f;
    if (lb > 0.f) loss = loss + lb * cb;
    const float sm = smoothing > 0.f ? smoothing / C : 0.f;
    const float hs = 1.f - smoothing, Wsm = W * sm;
    for (int c = lane; c < pad; c += 64) {
        float d = 0.f;
        if (W > 0.f && c < C) {
            const float p = expf(ld1t(lr + c) - l);
            const float oh = (c == a ? la : 0.f) + (c == b ? lb : 0.f);
            d = g * (W * p - hs * oh - Wsm);
        }
        st1t(dr + c, d);
    }
    return loss;
}

// One row of one head: the log-sum-exp and the sum of the logits ONCE, as ce_row_plain<FWD> forms them (the same lane striding, the
// same wave reductions, the same operations in the same order), then both labels' losses and the gradient.
template <typename T>
__device__ __forceinline__ float ce_row_mix(const float* __restrict__ lr, int C, int pad, long long a, long long b, float lam,
                                            float smoothing, float g, T* __restrict__ dr, int lane) {
    float mx = -INFINITY;
    for (int c = lane; c < C; c += 64) mx = fmaxf(mx, ld1t(lr + c));
    mx = wave_max(mx);
    float se = 0.f, sx = 0.f;
    for (int c = lane; c < C; c += 64) {
        const float v = ld1t(lr + c);
        se += expf(v - mx);
        sx += v;
    }
    se = wave_sum(se);
    sx = wave_sum(sx);
    const float l = mx + logf(se);
    const bool alive = a >= 0 && a < C, blive = b >= 0 && b < C;
    float ca = 0.f, cb = 0.f;
    if (alive) ca = ce_plain_loss(lr, l, a, sx, smoothing, C);
    if (blive) cb = ce_plain_loss(lr, l, b, sx, smoothing, C);
    return ce_mix_tail<T>(lr, C, pad, a, b, alive, blive, lam, ca, cb, l, smoothing, g, dr, lane);
}

template <typename T>
__global__ __launch_bounds__(256) void ce_mix_fused_multi_kernel(const CEMixTasks P, float smoothing) {
    const int k = blockIdx.y;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int n_heads = P.n_heads[k], rows = P.rows[k];
    const long long* __restrict__ y = P.y[k];
    const long long* __restrict__ yb = P.yb[k];
    const float* __restrict__ lamp = P.lam[k];
    const long long ys = P.ys[k], ldd = P.ldd[k];
    float* __restrict__ loss = P.loss[k];
    T* __restrict__ dlogits = (T*)P.dlogits[k];
    const float g = scaled_seed(P.gscale[k], P.scale[k]);  // (common.h: one rounded product, the seed itself without a scale)
    const RowWalk rw = row_walk(blockIdx.x, gridDim.x, 0, rows, wave, MIX_WPB);  // (XCD x owns a contiguous eighth of the rows: common.h)
    for (int row = rw.first; row < rw.end; row += rw.step) {
        const float lam = lamp[row];
        float total = 0.f;
        for (int h = 0; h < n_heads; ++h)
            total += ce_row_mix<T>(P.logits[k][h] + (long long)row * P.ld[k][h], P.C[k][h], P.pad[k][h], y[(long long)row * ys + h],
                                   yb[(long long)row * ys + h], lam, smoothing, g, dlogits + (long long)row * ldd + P.dcol[k][h], lane);
        if (lane == 0) loss[row] = total;
    }
}

// [lo, hi) in bytes of a [rows, cols] matrix with rows ``ld`` elements apart.  A matrix without rows counts as one row (an in-place
// call is refused whatever its size); a null pointer names nothing.
struct ByteRange {
    uintptr_t lo, hi;
};
static ByteRange byte_range(const void* p, int64_t rows, int64_t ld, int64_t cols, int64_t es) {
    const uintptr_t lo = reinterpret_cast<uintptr_t>(p);
    if (!p) return ByteRange{0, 0};
    return ByteRange{lo, lo + (uintptr_t)(((rows > 0 ? rows - 1 : 0) * ld + cols) * es)};
}
static bool overlap(const ByteRange& a, const ByteRange& b) { return a.lo < a.hi && b.lo < b.hi && a.lo < b.hi && b.lo < a.hi; }

}  // namespace egk

using namespace egk;

extern "C" {

int egk_mix_rows_multi(egk_stream_t stream, int32_t n_seg, const void* const* x_in, void* const* x_out, const int64_t* ld_in,
                       const int64_t* ld_out, const int32_t* rows, const int32_t* const* src, const float* const* lam, int32_t cols,
                       int32_t dtype) {
    EGK_REQUIRE(x_in && x_out && ld_in && ld_out && rows && src && lam, "egk_mix_rows_multi: null pointer (a host array)");
    EGK_REQUIRE(n_seg >= 1 && n_seg <= EGK_MIX_MAX_SEGMENTS, "egk_mix_rows_multi: 1 .. %d segments (got %d)", EGK_MIX_MAX_SEGMENTS, n_seg);
    EGK_REQUIRE(cols >= 1, "egk_mix_rows_multi: cols must be >= 1 (got %d)", cols);
    EGK_REQUIRE(dtype == EGK_F32 || dtype == EGK_BF16, "egk_mix_rows_multi: unknown element dtype %d", dtype);
    const int64_t es = dtype == EGK_BF16 ? 2 : 4;
    MixArgs A;
    ByteRange rin[EGK_MIX_MAX_SEGMENTS], rout[EGK_MIX_MAX_SEGMENTS];
    int64_t total = 0;
    bool vec = true;
    for (int i = 0; i < n_seg; ++i) {
        EGK_REQUIRE(rows[i] >= 0, "egk_mix_rows_multi: rows must be >= 0 (segment %d: %d)", i, rows[i]);
        EGK_REQUIRE(ld_in[i] >= cols, "egk_mix_rows_multi: ld_in >= cols (segment %d: ld_in %lld, cols %d)", i, (long long)ld_in[i], cols);
        EGK_REQUIRE(ld_out[i] >= cols, "egk_mix_rows_multi: ld_out >= cols (segment %d: ld_out %lld, cols %d)", i, (long long)ld_out[i], cols);
        EGK_REQUIRE(!src[i] || lam[i], "egk_mix_rows_multi: src is given without lam (segment %d)", i);
        EGK_REQUIRE(!lam[i] || src[i], "egk_mix_rows_multi: lam is given without src (segment %d)", i);
        EGK_REQUIRE(rows[i] == 0 || (x_in[i] && x_out[i]), "egk_mix_rows_multi: null pointer (x_in or x_out of segment %d)", i);
        EGK_REQUIRE(aligned_to((unsigned)es, {x_in[i], x_out[i]}), "egk_mix_rows_multi: x_in / x_out of segment %d are not aligned to their element", i);
        EGK_REQUIRE(aligned_to(4u, {src[i], lam[i]}), "egk_mix_rows_multi: src / lam of segment %d are not 4-byte aligned", i);
        rin[i] = byte_range(x_in[i], rows[i], ld_in[i], cols, es);
        rout[i] = byte_range(x_out[i], rows[i], ld_out[i], cols, es);
        if (rows[i] > 0)
            vec = vec && aligned_to(16u, {x_in[i], x_out[i]}) && (ld_in[i] * es) % 16 == 0 && (ld_out[i] * es) % 16 == 0;
        total += rows[i];
    }
    EGK_REQUIRE(total <= 0x7fffffffLL, "egk_mix_rows_multi: more than 2^31 - 1 rows in all");
    for (int i = 0; i < n_seg; ++i)
        for (int j = 0; j < n_seg; ++j) {
            EGK_REQUIRE(!overlap(rout[i], rin[j]), "egk_mix_rows_multi: x_out of segment %d overlaps x_in of segment %d -- the launch is "
                        "out of place", i, j);
            EGK_REQUIRE(i == j || !overlap(rout[i], rout[j]), "egk_mix_rows_multi: x_out of segment %d overlaps x_out of segment %d", i, j);
        }
    if (total == 0) return 0;
    int64_t row0 = 0;
    for (int i = 0; i < EGK_MIX_MAX_SEGMENTS; ++i) {
        const int j = i < n_seg ? i : n_seg - 1;  // (the slots behind n_seg repeat the last segment and begin behind every row)
        A.in[i] = x_in[j]; A.out[i] = x_out[j]; A.src[i] = (const int*)src[j]; A.lam[i] = lam[j];
        A.ld_in[i] = ld_in[j]; A.ld_out[i] = ld_out[j];
        A.row0[i] = (int)(i < n_seg ? row0 : total);
        if (i < n_seg) row0 += rows[i];
    }
    A.total = (int)total;
    A.cols = cols;
    hipStream_t s = (hipStream_t)stream;
    ProfScope prof(KID_MIX_ROWS, s, 0, 3.0 * (double)total * cols * es);
    if (vec) EGK_DISPATCH_T(dtype, hipLaunchKernelGGL((mix_rows_kernel<T, true>), dim3(mix_row_grid((int)total)), dim3(256), 0, s, A));
    else EGK_DISPATCH_T(dtype, hipLaunchKernelGGL((mix_rows_kernel<T, false>), dim3(mix_row_grid((int)total)), dim3(256), 0, s, A));
    return check_launch("egk_mix_rows_multi");
}

int egk_ce_mix_fused_multi(egk_stream_t stream, int32_t count, const float* const* logits, const int64_t* ld, const int32_t* C,
                           const int32_t* pad, const int64_t* dcol, const int32_t* n_heads, const int64_t* const* y,
                           const int64_t* const* y_b, const int64_t* y_stride, const float* const* lam, float* const* loss,
                           void* const* dlogits, const int64_t* ldd, const int32_t* rows, const float* gscale,
                           const float* const* scales, float smoothing, int32_t dtype) {
    EGK_REQUIRE(logits && ld && C && pad && dcol && n_heads && y && y_b && y_stride && lam && loss && dlogits && ldd && rows && gscale,
                "egk_ce_mix_fused_multi: null pointer (a host array)");
    EGK_REQUIRE(count >= 1 && count <= EGK_CE_MIX_MAX_TASKS, "egk_ce_mix_fused_multi: 1 .. %d tasks (got %d)", EGK_CE_MIX_MAX_TASKS, count);
    EGK_REQUIRE(dtype == EGK_F32 || dtype == EGK_BF16, "egk_ce_mix_fused_multi: unknown activation dtype %d", dtype);
    CEMixTasks P;
    double bytes = 0;
    int max_rows = 0;
    for (int i = 0; i < EGK_CE_MIX_MAX_TASKS; ++i) {
        const int j = i < count ? i : count - 1;  // (the slots behind count repeat the last task with no rows: no wild pointers)
        EGK_REQUIRE(n_heads[j] >= 1 && n_heads[j] <= EGK_CE_MIX_MAX_HEADS, "egk_ce_mix_fused_multi: 1 .. %d heads (task %d)",
                    EGK_CE_MIX_MAX_HEADS, j);
        EGK_REQUIRE(rows[j] >= 0, "egk_ce_mix_fused_multi: rows must be >= 0 (task %d)", j);
        EGK_REQUIRE(y[j] && y_b[j], "egk_ce_mix_fused_multi: null pointer (y or y_b of task %d)", j);
        EGK_REQUIRE(lam[j], "egk_ce_mix_fused_multi: null pointer (lam of task %d)", j);
        EGK_REQUIRE(loss[j] && dlogits[j], "egk_ce_mix_fused_multi: null pointer (loss or dlogits of task %d)", j);
        EGK_REQUIRE(aligned_to(8u, {y[j], y_b[j]}), "egk_ce_mix_fused_multi: y / y_b of task %d are not 8-byte aligned", j);
        EGK_REQUIRE(aligned_to(4u, {lam[j], loss[j]}), "egk_ce_mix_fused_multi: lam / loss of task %d are not 4-byte aligned", j);
        EGK_REQUIRE(aligned_to(dtype == EGK_BF16 ? 2u : 4u, {dlogits[j]}), "egk_ce_mix_fused_multi: dlogits of task %d is not aligned to its element", j);
        P.scale[i] = scales ? scales[j] : nullptr;
        EGK_REQUIRE(aligned_to(4u, {P.scale[i]}), "egk_ce_mix_fused_multi: the scale of task %d is not 4-byte aligned", j);
        for (int h = 0; h < EGK_CE_MIX_MAX_HEADS; ++h) {
            const int k = EGK_CE_MIX_MAX_HEADS * j + (h < n_heads[j] ? h : n_heads[j] - 1);
            EGK_REQUIRE(logits[k], "egk_ce_mix_fused_multi: null pointer (logits of head %d of task %d)", k % EGK_CE_MIX_MAX_HEADS, j);
            EGK_REQUIRE(aligned_to(4u, {logits[k]}), "egk_ce_mix_fused_multi: the logits of head %d of task %d are not 4-byte aligned",
                        k % EGK_CE_MIX_MAX_HEADS, j);
            EGK_REQUIRE(C[k] >= 1, "egk_ce_mix_fused_multi: C must be >= 1 (head %d of task %d)", k % EGK_CE_MIX_MAX_HEADS, j);
            EGK_REQUIRE(pad[k] >= C[k], "egk_ce_mix_fused_multi: pad must be >= C (head %d of task %d)", k % EGK_CE_MIX_MAX_HEADS, j);
            P.logits[i][h] = logits[k]; P.ld[i][h] = ld[k]; P.dcol[i][h] = dcol[k]; P.C[i][h] = C[k]; P.pad[i][h] = pad[k];
            if (i < count && h < n_heads[j]) bytes += 6.0 * rows[j] * C[k];
        }
        P.y[i] = (const long long*)y[j]; P.yb[i] = (const long long*)y_b[j]; P.lam[i] = lam[j]; P.loss[i] = loss[j];
        P.dlogits[i] = dlogits[j]; P.ys[i] = y_stride[j]; P.ldd[i] = ldd[j]; P.n_heads[i] = n_heads[j];
        P.rows[i] = i < count ? rows[j] : 0; P.gscale[i] = gscale[j];
        if (i < count && rows[j] > max_rows) max_rows = rows[j];
    }
    if (max_rows == 0) return 0;
    hipStream_t s = (hipStream_t)stream;
    ProfScope prof(KID_CE_MIX, s, 0, bytes);
    EGK_DISPATCH_T(dtype, hipLaunchKernelGGL((ce_mix_fused_multi_kernel<T>), dim3(mix_row_grid(max_rows), count), dim3(256), 0, s, P, smoothing));
    return check_launch("egk_ce_mix_fused_multi");
}

}  // extern "C"
