// Sequence mixup (include/egopack_mixup.h), the row mix:
//   egk_mix_rows_multi       out[r] = lam[r] in[r] + (1 - lam[r]) in[src[r]] for the rows of up to 4 segments, out of place, one launch
// (the header's other entry point, the two-target cross entropy egk_ce_mix_fused_multi, is a mode of the fused cross entropy: loss.hip).
// Plain C++: one wave per row, four waves per workgroup, at most 2048 workgroups, the row walk of the other row kernels (common.h:
// XCD x owns a contiguous eighth of the rows); no LDS, no workspace, no atomics.  The mix is HBM-bound: 16-byte accesses along the
// row, ordinary stores (the first contraction reads the output next, from the L2 of the XCD that wrote it).
// The launcher refuses its argument errors on the host before it launches.
#include <math.h>

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

}  // extern "C"
