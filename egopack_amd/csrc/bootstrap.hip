// The seeded cluster bootstrap of the validation metrics (include/egopack_bootstrap.h): R Poisson(1) replicates of integer
// (numerator, denominator) column sums and of a per-class (hit, support) pair, every row weighted by its cluster's weight.
//
// One 256-thread workgroup owns FOUR consecutive replicates -- the four words of one Philox call per cluster -- for the whole launch
// and walks all rows with a workgroup stride.  A thread keeps the 4 x M int64 partial sums of both sides in registers (the column
// loop is unrolled to EGK_BOOT_MAX_M under a wave-uniform predicate: no runtime-indexed array, no scratch); the class histograms of
// the four replicates sit in LDS as int32, 4 x 2 x C words, filled with LDS atomic adds (integer adds: the order is immaterial).  At
// the end the column sums go through a shuffle tree and LDS, and the workgroup adds both results into global memory with plain loads
// and stores: every word of acc_* and cls_* has exactly one writer per launch.  No global atomics, no workspace.
#include "common.h"

namespace egk {

namespace {

// T[k] = floor(2^32 * sum_{j <= k} e^-1 / j!): the Poisson(1) distribution function in 32-bit fixed point (tests/test_bootstrap_cpu.py
// recomputes the table in 60-digit decimals)
__device__ __forceinline__ int poisson1(uint32_t word) {
    constexpr uint32_t T[12] = {1580030168u, 3160060337u, 3950075421u, 4213413783u, 4279248373u, 4292415291u,
                                4294609777u, 4294923276u, 4294962463u, 4294966817u, 4294967252u, 4294967292u};
    int w = 0;
#pragma unroll
    for (int k = 0; k < 12; ++k) w += word >= T[k] ? 1 : 0;
    return w;
}

// the weights of cluster c >= 0 in the replicates 4 * group .. 4 * group + 3
__device__ __forceinline__ void boot_weights4(long long c, uint32_t group, uint64_t key, int (&w)[4]) {
    const uint4 q = philox4x32_10(((uint64_t)c << 14) | (uint64_t)group, key);
    w[0] = poisson1(q.x); w[1] = poisson1(q.y); w[2] = poisson1(q.z); w[3] = poisson1(q.w);
}

__device__ __forceinline__ long long wave_sum_i64(long long v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

constexpr int BOOT_M = EGK_BOOT_MAX_M, BOOT_C = EGK_BOOT_MAX_C;

__global__ __launch_bounds__(256) void bootstrap_accumulate_kernel(const long long* __restrict__ cluster, const long long* __restrict__ num,
                                                                   const long long* __restrict__ den, long long ld, int rows, int M,
                                                                   const long long* __restrict__ label, long long label_stride,
                                                                   int class_col, int C, long long* __restrict__ acc_num,
                                                                   long long* __restrict__ acc_den, long long* __restrict__ cls_num,
                                                                   long long* __restrict__ cls_den, int R, uint64_t key) {
    __shared__ int hist[4 * 2 * BOOT_C];         // [replicate of the four][num, den][C]
    __shared__ long long red[4][4 * 2 * BOOT_M]; // [wave][replicate of the four][num, den][column]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const bool cls = class_col >= 0;  // (a kernel argument: uniform)
    if (cls) {
        for (int i = tid; i < 4 * 2 * C; i += 256) hist[i] = 0;
        __syncthreads();
    }
    long long an[4][BOOT_M], ad[4][BOOT_M];
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int m = 0; m < BOOT_M; ++m) an[j][m] = ad[j][m] = 0;
    for (int row = tid; row < rows; row += 256) {
        const long long c = cluster[row];
        if (c < 0) continue;  // (the reductions follow the loop)
        int w[4];
        boot_weights4(c, blockIdx.x, key, w);
        const long long* nr = num + (long long)row * ld;
        const long long* dr = den + (long long)row * ld;
#pragma unroll
        for (int m = 0; m < BOOT_M; ++m) {
            if (m < M) {
                const long long n = nr[m], d = dr[m];
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    an[j][m] += (long long)w[j] * n;
                    ad[j][m] += (long long)w[j] * d;
                }
            }
        }
        if (cls) {
            const long long y = label[(long long)row * label_stride];
            if (y >= 0 && y < C) {
                const bool hn = nr[class_col] != 0, hd = dr[class_col] != 0;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    if (w[j] && hn) atomicAdd(&hist[(j * 2 + 0) * C + (int)y], w[j]);
                    if (w[j] && hd) atomicAdd(&hist[(j * 2 + 1) * C + (int)y], w[j]);
                }
            }
        }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
#pragma unroll
        for (int m = 0; m < BOOT_M; ++m) {
            if (m < M) {
                const long long sn = wave_sum_i64(an[j][m]), sd = wave_sum_i64(ad[j][m]);
                if (lane == 0) {
                    red[wave][(j * 2 + 0) * BOOT_M + m] = sn;
                    red[wave][(j * 2 + 1) * BOOT_M + m] = sd;
                }
            }
        }
    }
    __syncthreads();  // (red is complete, and so are the LDS atomics of every wave)
    if (tid < 4 * 2 * BOOT_M) {
        const int j = tid / (2 * BOOT_M), side = (tid / BOOT_M) & 1, m = tid % BOOT_M;
        const long long r = (long long)blockIdx.x * 4 + j;
        if (r < R && m < M) {
            const long long sum = red[0][tid] + red[1][tid] + red[2][tid] + red[3][tid];
            long long* dst = (side ? acc_den : acc_num) + r * M + m;
            *dst = *dst + sum;
        }
    }
    if (cls) {
        for (int i = tid; i < 4 * 2 * C; i += 256) {
            const int j = i / (2 * C), rem = i - j * 2 * C, side = rem >= C ? 1 : 0, y = rem - side * C;
            const long long r = (long long)blockIdx.x * 4 + j;
            const int h = hist[i];
            if (r < R && h) {  // (a class nobody drew: the word keeps its value without being read)
                long long* dst = (side ? cls_den : cls_num) + r * C + y;
                *dst = *dst + h;
            }
        }
    }
}

// one thread per (row, four replicates)
__global__ __launch_bounds__(256) void bootstrap_weights_kernel(const long long* __restrict__ cluster, int rows, int R, uint64_t key,
                                                                uint8_t* __restrict__ out) {
    const int groups = (R + 3) >> 2;
    const long long total = (long long)rows * groups;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        const int row = (int)(i / groups), g = (int)(i - (long long)row * groups);
        const long long c = cluster[row];
        int w[4] = {0, 0, 0, 0};
        if (c >= 0) boot_weights4(c, (uint32_t)g, key, w);
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (g * 4 + j < R) out[(long long)row * R + g * 4 + j] = (uint8_t)w[j];
    }
}

int boot_checks(const char* what, const int64_t* cluster, int32_t rows, int32_t R) {
    EGK_REQUIRE(cluster, "%s: null cluster", what);
    EGK_REQUIRE(rows >= 0, "%s: rows must be >= 0", what);
    EGK_REQUIRE(rows <= (1 << 24), "%s: more than 2^24 rows per launch are unsupported", what);
    EGK_REQUIRE(R >= 1 && R <= EGK_BOOT_MAX_R, "%s: R must lie in 1..%d (got %d)", what, EGK_BOOT_MAX_R, (int)R);
    return 0;
}

}  // namespace

}  // namespace egk

using namespace egk;

extern "C" {

int egk_bootstrap_accumulate(egk_stream_t stream, const int64_t* cluster, const int64_t* num, const int64_t* den, int64_t ld,
                             int32_t rows, int32_t M, const int64_t* label, int64_t label_stride, int32_t class_col, int32_t C,
                             int64_t* acc_num, int64_t* acc_den, int64_t* cls_num, int64_t* cls_den, int32_t R, uint64_t key) {
    const char* what = "egk_bootstrap_accumulate";
    if (int rc = boot_checks(what, cluster, rows, R)) return rc;
    EGK_REQUIRE(num && den, "%s: null num / den", what);
    EGK_REQUIRE(acc_num && acc_den, "%s: null acc_num / acc_den", what);
    EGK_REQUIRE(M >= 1 && M <= EGK_BOOT_MAX_M, "%s: M must lie in 1..%d (got %d)", what, EGK_BOOT_MAX_M, (int)M);
    EGK_REQUIRE(ld >= M, "%s: ld must be >= M", what);
    EGK_REQUIRE(class_col >= -1 && class_col < M, "%s: class_col must lie in [-1, M) (got %d)", what, (int)class_col);
    if (class_col >= 0) {
        EGK_REQUIRE(label && cls_num && cls_den, "%s: class_col >= 0 with a null label / cls_num / cls_den", what);
        EGK_REQUIRE(C >= 1 && C <= EGK_BOOT_MAX_C, "%s: C must lie in 1..%d (got %d)", what, EGK_BOOT_MAX_C, (int)C);
    }
    EGK_REQUIRE(aligned_to(8, {cluster, num, den, label, acc_num, acc_den, cls_num, cls_den}), "%s: int64 pointers must be 8-byte aligned", what);
    if (rows == 0) return 0;
    hipStream_t s = (hipStream_t)stream;
    const int groups = (R + 3) / 4;
    ProfScope prof(KID_BOOTSTRAP, s, 0, (double)groups * rows * (8.0 + 16.0 * M + (class_col >= 0 ? 8.0 : 0.0)));
    hipLaunchKernelGGL(bootstrap_accumulate_kernel, dim3(groups), dim3(256), 0, s, (const long long*)cluster, (const long long*)num,
                       (const long long*)den, (long long)ld, rows, M, (const long long*)label, (long long)label_stride, class_col, C,
                       (long long*)acc_num, (long long*)acc_den, (long long*)cls_num, (long long*)cls_den, R, key);
    return check_launch(what);
}

int egk_bootstrap_weights(egk_stream_t stream, const int64_t* cluster, int32_t rows, int32_t R, uint64_t key, uint8_t* w) {
    const char* what = "egk_bootstrap_weights";
    if (int rc = boot_checks(what, cluster, rows, R)) return rc;
    EGK_REQUIRE(w, "%s: null w", what);
    EGK_REQUIRE(aligned_to(8, {cluster}), "%s: int64 pointers must be 8-byte aligned", what);
    if (rows == 0) return 0;
    hipStream_t s = (hipStream_t)stream;
    const int64_t total = (int64_t)rows * ((R + 3) / 4);
    const int grid = total > 2048ll * 256 ? 2048 : cdiv(total, 256);  // (grid-stride beyond)
    ProfScope prof(KID_BOOTSTRAP, s, 0, 8.0 * rows + (double)rows * R);
    hipLaunchKernelGGL(bootstrap_weights_kernel, dim3(grid), dim3(256), 0, s, (const long long*)cluster, rows, R, key, w);
    return check_launch(what);
}

}  // extern "C"
