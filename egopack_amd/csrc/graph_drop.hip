// DropEdge for the SAGE mean (include/egopack_edge_drop.h): the CSR neighbour mean over a seeded subset of every row's edges, forward
// and, over the transposed CSR with the regenerated subset, backward.
//
// One wave per output row, the row in NV float4 registers per lane (csr_gather_kernel's layout), rows walked with row_walk so that
// XCD x owns the rows the contractions on either side hand it.  Per batch of up to 64 edges every lane takes ONE edge: its column
// index, one Philox call keyed by the edge's two endpoints, the keep bit.  A ballot gives the kept set as a wave-uniform 64-bit mask;
// the wave then walks the SET bits in ascending order -- CSR order -- and requests only those neighbour rows, four in flight.  Rows
// of more than 12 edges are finished by the 4 waves of their workgroup, a column slice each.  No workspace, no global atomics, no
// partial sums; a row of any degree is finished inside the launch (the batch loop wraps past 64 edges).
#include "common.h"

namespace egk {

namespace {

constexpr int DROP_WPB = 4;

// keep bit of the edge source j -> destination i (the header's rule; ctr0 = offset + word)
__device__ __forceinline__ bool edge_keep(int i, int j, uint64_t ctr0, uint64_t seed, float p, int flags) {
    const bool sym = flags & EGK_EDGE_DROP_SYMMETRIC;
    const int a = sym ? min(i, j) : i, b = sym ? max(i, j) : j;
    const uint32_t r = philox4x32_10(ctr0 + (uint64_t)a, seed ^ ((uint64_t)(uint32_t)b << 32)).x;
    return u01(r) >= p || ((flags & EGK_EDGE_DROP_KEEP_SELF) && i == j);
}

// One row (or, with c0 / NVW, one column slice of it) by ONE wave.  BWD = false: row i of the forward CSR, col[e] = a source j;
// w = 1, the kept count is formed and, by the writer, inv_deg[row] written.  BWD = true: row j of the transposed CSR, col[e] = a
// destination i; w = inv_deg[i].  U neighbour rows are in flight; the additions of every element happen in CSR order over the kept
// edges whatever U and the slice are.  ``writer``: this wave also stores keep_out and inv_deg (one wave per row does).
template <int NVW, int U, typename T, bool BWD>
__device__ __forceinline__ void drop_row(const T* __restrict__ x, const int* __restrict__ rowptr, const int* __restrict__ col,
                                         const float* __restrict__ inv_in, float* __restrict__ inv_out, const T* __restrict__ gate,
                                         T* __restrict__ out, uint8_t* __restrict__ keep_out, int row, int cols, int c0, bool vec,
                                         float p, int flags, uint64_t seed, uint64_t ctr0, int lane, bool writer) {
    const int e0 = rowptr[row], e1 = rowptr[row + 1];
    float4 acc[NVW];
#pragma unroll
    for (int i = 0; i < NVW; ++i) acc[i] = make_float4(0.f, 0.f, 0.f, 0.f);
    int kept = 0;
    for (int base = e0; base < e1; base += 64) {
        const int e = base + lane;
        const bool valid = e < e1;
        const int c = valid ? col[e] : 0;
        const bool keep = valid && (BWD ? edge_keep(c, row, ctr0, seed, p, flags) : edge_keep(row, c, ctr0, seed, p, flags));
        if (keep_out && valid && writer) keep_out[e] = keep ? 1 : 0;
        float w = 1.f;
        if constexpr (BWD) w = keep ? inv_in[c] : 0.f;
        unsigned long long m = __ballot(keep);  // wave-uniform: bit l = lane l's edge is kept
        kept += __popcll(m);
        while (m) {
            int src[U];
            int n = 0;
#pragma unroll
            for (int u = 0; u < U; ++u) {
                src[u] = m ? __ffsll(m) - 1 : 0;
                n += m ? 1 : 0;
                m &= m - 1;  // (0 stays 0)
            }
            float4 v[U][NVW];
            float wu[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                if (u < n) {  // wave-uniform
                    const T* s = x + (long long)__shfl(c, src[u], 64) * cols;
                    wu[u] = __shfl(w, src[u], 64);
#pragma unroll
                    for (int i = 0; i < NVW; ++i) v[u][i] = ld4t(s, c0 + (i * 64 + lane) * 4, cols, vec);
                }
            }
#pragma unroll
            for (int u = 0; u < U; ++u) {
                if (u < n) {
#pragma unroll
                    for (int i = 0; i < NVW; ++i) {
                        acc[i].x += wu[u] * v[u][i].x; acc[i].y += wu[u] * v[u][i].y;
                        acc[i].z += wu[u] * v[u][i].z; acc[i].w += wu[u] * v[u][i].w;
                    }
                }
            }
        }
    }
    float mean_w = 1.f;
    if constexpr (!BWD) {
        mean_w = kept ? 1.f / (float)kept : 0.f;
        if (lane == 0 && writer) inv_out[row] = mean_w;
    }
#pragma unroll
    for (int i = 0; i < NVW; ++i) {
        const int cc = c0 + (i * 64 + lane) * 4;
        if constexpr (!BWD) {  // mean = sum / kept count (csr_finish's expression)
            acc[i].x *= mean_w; acc[i].y *= mean_w; acc[i].z *= mean_w; acc[i].w *= mean_w;
        }
        if (gate) {
            const float4 g = ld4t(gate + (long long)row * cols, cc, cols, vec);
            acc[i].x = g.x > 0.f ? acc[i].x : 0.f; acc[i].y = g.y > 0.f ? acc[i].y : 0.f;
            acc[i].z = g.z > 0.f ? acc[i].z : 0.f; acc[i].w = g.w > 0.f ? acc[i].w : 0.f;
        }
        st4t(out + (long long)row * cols, cc, cols, vec, acc[i]);
    }
}

// Rows of more than DROP_HEAVY edges (the LTA fan-out node: out-degree 31 in the backward orientation) are not walked by their wave
// alone, four neighbour rows per round trip: the wave lists the row, and after the workgroup's light rows its 4 waves take a
// quarter of the columns each (csr_gather_kernel's listed-row branch: every wave walks ALL the edges, in order, for its slice),
// sixteen neighbour rows in flight.  No element's sum is split over waves, so the bits do not depend on who sums a row.
constexpr int DROP_HEAVY = 12;

template <int NV, typename T, bool BWD>
__global__ __launch_bounds__(256) void csr_mean_drop_kernel(const T* __restrict__ x, const int* __restrict__ rowptr,
                                                            const int* __restrict__ col, const float* __restrict__ inv_in,
                                                            float* __restrict__ inv_out, const T* __restrict__ gate,
                                                            T* __restrict__ out, uint8_t* __restrict__ keep_out, int rows, int cols,
                                                            float p, int flags, uint64_t seed, uint64_t offset,
                                                            const uint64_t* __restrict__ word) {
    __shared__ int heavy[64];
    __shared__ int n_heavy;
    constexpr int U = NV <= 4 ? 4 : 1;         // neighbour rows in flight, a whole row per wave
    constexpr int NVW = NV >= 4 ? NV / 4 : 1;  // float4 per lane of a column slice
    constexpr int UW = NVW == 1 ? 16 : 4;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const bool vec = (cols & 3) == 0;
    const uint64_t ctr0 = offset + (word ? word[0] : 0ull);
    if (threadIdx.x == 0) n_heavy = 0;
    __syncthreads();
    const RowWalk rw = row_walk(blockIdx.x, gridDim.x, 0, rows, wave, DROP_WPB);  // (XCD x owns a contiguous eighth of the rows: common.h)
    for (int row = rw.first; row < rw.end; row += rw.step) {
        if (rowptr[row + 1] - rowptr[row] > DROP_HEAVY) {  // (wave-uniform) deferred while the list has room
            int slot = lane == 0 ? atomicAdd(&n_heavy, 1) : 0;
            slot = __shfl(slot, 0, 64);
            if (slot < 64) {
                if (lane == 0) heavy[slot] = row;
                continue;
            }
        }
        drop_row<NV, U, T, BWD>(x, rowptr, col, inv_in, inv_out, gate, out, keep_out, row, cols, 0, vec, p, flags, seed, ctr0, lane, true);
    }
    __syncthreads();
    const int nh = min(n_heavy, 64);
    const int c0 = wave * NVW * 256;
    if (c0 >= cols) return;  // (no barrier follows)
    for (int h = 0; h < nh; ++h)
        drop_row<NVW, UW, T, BWD>(x, rowptr, col, inv_in, inv_out, gate, out, keep_out, heavy[h], cols, c0, vec, p, flags, seed, ctr0, lane,
                                  wave == 0);
}

int drop_checks(const char* what, const void* x, const int32_t* rowptr, const int32_t* col, const void* out, const float* inv_deg,
                const void* gate, int32_t rows, int32_t cols, int32_t dtype, float p, int32_t flags, const uint64_t* word) {
    EGK_REQUIRE(p >= 0.f && p <= 1.f, "%s: p must lie in [0, 1] (and not be NaN)", what);
    EGK_REQUIRE(cols >= 1, "%s: cols must be >= 1", what);
    EGK_REQUIRE(cols <= 4096, "%s: rows wider than 4096 are unsupported", what);
    EGK_REQUIRE(rows >= 0, "%s: rows must be >= 0", what);
    EGK_REQUIRE(x, "%s: null input matrix", what);
    EGK_REQUIRE(out, "%s: null output matrix", what);
    EGK_REQUIRE(inv_deg, "%s: null inv_deg", what);
    EGK_REQUIRE(rowptr, "%s: null rowptr", what);
    EGK_REQUIRE(col, "%s: null col", what);
    EGK_REQUIRE(dtype == EGK_F32 || dtype == EGK_BF16, "%s: unknown element dtype %d", what, (int)dtype);
    EGK_REQUIRE((flags & ~(EGK_EDGE_DROP_SYMMETRIC | EGK_EDGE_DROP_KEEP_SELF)) == 0, "%s: unknown flag bits 0x%x", what, (unsigned)flags);
    EGK_REQUIRE_VEC_ALIGNED(what, (cols & 3) ? aligned_to(dtype == EGK_BF16 ? 2u : 4u, {x, out, gate}) : aligned_to(vec_bytes(dtype), {x, out, gate}));
    EGK_REQUIRE(aligned_to(4, {inv_deg, rowptr, col}) && aligned_to(8, {word}),
                "%s: inv_deg, rowptr and col must be 4-byte aligned, the device word 8-byte", what);
    return 0;
}

inline int drop_grid(int rows) {
    const int g = cdiv(rows, DROP_WPB);
    return g < 1 ? 1 : (g > 2048 ? 2048 : g);
}

}  // namespace

}  // namespace egk

using namespace egk;

#define EGK_DROP(NVV, BWDV, ...) hipLaunchKernelGGL((csr_mean_drop_kernel<NVV, T, BWDV>), dim3(drop_grid(rows)), dim3(256), 0, s, __VA_ARGS__)
#define EGK_DROP_NV(BWDV, ...)                                         \
    EGK_DISPATCH_T(dtype, {                                            \
        if (cols <= 256) EGK_DROP(1, BWDV, __VA_ARGS__);               \
        else if (cols <= 1024) EGK_DROP(4, BWDV, __VA_ARGS__);         \
        else EGK_DROP(16, BWDV, __VA_ARGS__);                          \
    })

extern "C" {

int egk_csr_mean_drop_fwd(egk_stream_t stream, const void* x, const int32_t* rowptr, const int32_t* col, void* out, float* inv_deg,
                          uint8_t* keep_out, int32_t rows, int32_t cols, int32_t dtype, float p, int32_t flags, uint64_t seed,
                          uint64_t offset, const uint64_t* word) {
    if (int rc = drop_checks("egk_csr_mean_drop_fwd", x, rowptr, col, out, inv_deg, nullptr, rows, cols, dtype, p, flags, word)) return rc;
    if (rows == 0) return 0;
    hipStream_t s = (hipStream_t)stream;
    ProfScope prof(KID_CSR_MEAN_DROP, s, 0, (dtype == EGK_BF16 ? 0.5 : 1.0) * 8.0 * rows * cols);
    EGK_DROP_NV(false, (const T*)x, rowptr, col, (const float*)nullptr, inv_deg, (const T*)nullptr, (T*)out, keep_out, rows, cols, p,
                flags, seed, offset, word);
    return check_launch("egk_csr_mean_drop_fwd");
}

int egk_csr_mean_drop_bwd(egk_stream_t stream, const void* dout, const int32_t* t_rowptr, const int32_t* t_col, const float* inv_deg,
                          const void* gate, void* dx, uint8_t* keep_out, int32_t rows, int32_t cols, int32_t dtype, float p,
                          int32_t flags, uint64_t seed, uint64_t offset, const uint64_t* word) {
    if (int rc = drop_checks("egk_csr_mean_drop_bwd", dout, t_rowptr, t_col, dx, inv_deg, gate, rows, cols, dtype, p, flags, word)) return rc;
    if (rows == 0) return 0;
    hipStream_t s = (hipStream_t)stream;
    ProfScope prof(KID_CSR_MEAN_DROP, s, 0, (dtype == EGK_BF16 ? 0.5 : 1.0) * (gate ? 12.0 : 8.0) * rows * cols);
    EGK_DROP_NV(true, (const T*)dout, t_rowptr, t_col, inv_deg, (float*)nullptr, (const T*)gate, (T*)dx, keep_out, rows, cols, p, flags,
                seed, offset, word);
    return check_launch("egk_csr_mean_drop_bwd");
}

}  // extern "C"
