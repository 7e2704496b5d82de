// Small elementwise helpers (dropout, ReLU gate, axpby, scaled and weighted sums, block copies, zero fills), the step
// constants of the flat-buffer optimizer and the global gradient norm.  All HBM-bound / latency-bound.  (The loss kernels are in
// loss.hip, the optimizer's update kernels in optim_rules.hip.)
#include <math.h>

#include "common.h"

namespace egk {

// ---- dropout ---------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(256) void dropout_fwd_kernel(const T* __restrict__ x, T* __restrict__ y,
                                                          uint8_t* __restrict__ mask, long long n, float p, uint64_t seed,
                                                          uint64_t offset, const uint64_t* __restrict__ dev_offset) {
    if (dev_offset) offset += dev_offset[0];
    const float inv = 1.f / (1.f - p);
    for (long long q = (long long)blockIdx.x * blockDim.x + threadIdx.x; q * 4 < n; q += (long long)gridDim.x * blockDim.x) {
        const uint4 r = philox4x32_10(offset + (uint64_t)q, seed);
        const uint32_t rr[4] = {r.x, r.y, r.z, r.w};
        for (int t = 0; t < 4; ++t) {
            const long long i = q * 4 + t;
            if (i < n) {
                const bool keep = u01(rr[t]) >= p;
                mask[i] = keep;
                st1t(y + i, keep ? ld1t(x + i) * inv : 0.f);
            }
        }
    }
}
template <typename T>
__global__ __launch_bounds__(256) void dropout_bwd_kernel(const T* __restrict__ dy, const uint8_t* __restrict__ mask,
                                                          T* __restrict__ dx, long long n, float p) {
    const float inv = 1.f / (1.f - p);
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x)
        st1t(dx + i, mask[i] ? ld1t(dy + i) * inv : 0.f);
}

template <typename T>
__global__ __launch_bounds__(256) void relu_gate_kernel(const T* __restrict__ dy, const T* __restrict__ y,
                                                        T* __restrict__ dx, long long n, int vec) {
    for (long long i = ((long long)blockIdx.x * blockDim.x + threadIdx.x) * 4; i < n;
         i += (long long)gridDim.x * blockDim.x * 4) {
        if (vec && i + 4 <= n) {
            const float4 g = ld4t(dy + i, 0, 4, true);
            const float4 v = ld4t(y + i, 0, 4, true);
            st4t(dx + i, 0, 4, true,
                 make_float4(v.x > 0.f ? g.x : 0.f, v.y > 0.f ? g.y : 0.f, v.z > 0.f ? g.z : 0.f, v.w > 0.f ? g.w : 0.f));
        } else
            for (long long j = i; j < n && j < i + 4; ++j) st1t(dx + j, ld1t(y + j) > 0.f ? ld1t(dy + j) : 0.f);
    }
}

__global__ __launch_bounds__(256) void axpby_kernel(const float* __restrict__ x, const float* __restrict__ y,
                                                    float* __restrict__ out, long long n, float a, float b, int vec) {
    for (long long i = ((long long)blockIdx.x * blockDim.x + threadIdx.x) * 4; i < n;
         i += (long long)gridDim.x * blockDim.x * 4) {
        if (vec && i + 4 <= n) {
            const float4 xv = *reinterpret_cast<const float4*>(x + i);
            float4 o = make_float4(a * xv.x, a * xv.y, a * xv.z, a * xv.w);
            if (y) {
                const float4 yv = *reinterpret_cast<const float4*>(y + i);
                o.x += b * yv.x; o.y += b * yv.y; o.z += b * yv.z; o.w += b * yv.w;
            }
            *reinterpret_cast<float4*>(out + i) = o;
        } else
            for (long long j = i; j < n && j < i + 4; ++j) out[j] = a * x[j] + (y ? b * y[j] : 0.f);
    }
}

__global__ __launch_bounds__(256) void fill_scaled_kernel(const float* __restrict__ scalar, float coef,
                                                          float* __restrict__ out, long long n) {
    const float v = scalar[0] * coef;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x)
        out[i] = v;
}

// single workgroup, fixed-order tree: bitwise reproducible loss scalars
__global__ __launch_bounds__(1024) void sum_scale_kernel(const float* __restrict__ x, float* __restrict__ out, long long n,
                                                         float scale, int accumulate) {
    __shared__ float part[16];
    float s = 0.f;
    for (long long i = threadIdx.x; i < n; i += 1024) s += x[i];
    s = wave_sum(s);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        float t = 0.f;
        for (int i = 0; i < 16; ++i) t += part[i];
        t *= scale;
        out[0] = accumulate ? out[0] + t : t;
    }
}

// The objective of a multi-task step in ONE launch each way: out = sum_i coef_i * sum(x_i) (vectors reduced one after
// the other by the same fixed-order tree, terms added in vector order: the values of the per-vector launches), and
// its backward d x_i[:] = g * coef_i.  (Per task that was a chain of 1-workgroup launches separated by graph-node
// latencies: 7 nodes for three tasks.)
constexpr int MAXVEC = 8;
struct VecList {
    const float* x[MAXVEC];
    float* out[MAXVEC];
    long long n[MAXVEC];
    float coef[MAXVEC];
    int count;
};

__global__ __launch_bounds__(1024) void weighted_sums_kernel(const VecList v, float* __restrict__ out, double* __restrict__ acc) {
    __shared__ float part[16];
    float total = 0.f;
    for (int k = 0; k < v.count; ++k) {
        float s = 0.f;
        for (long long i = threadIdx.x; i < v.n[k]; i += 1024) s += v.x[k][i];
        s = wave_sum(s);
        __syncthreads();  // part[] free (previous vector consumed)
        if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = s;
        __syncthreads();
        if (threadIdx.x == 0) {
            float t = 0.f;
            for (int i = 0; i < 16; ++i) t += part[i];
            if (acc) acc[k] += (double)t;  // (running per-vector sums over the steps of a training loop: egk_weighted_sums_acc)
            t *= v.coef[k];
            total = k ? total + t : t;
        }
    }
    if (threadIdx.x == 0) out[0] = total;
}

__global__ __launch_bounds__(256) void fill_scaled_multi_kernel(const float* __restrict__ scalar, const VecList v) {
    const int k = blockIdx.y;
    const float val = scalar[0] * v.coef[k];
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < v.n[k]; i += (long long)gridDim.x * blockDim.x)
        v.out[k][i] = val;
}

// dst = srcs[0] | srcs[1] | ... (contiguous blocks, byte sizes; a NULL source fills its block with zeros) in one launch:
// the per-task feature gradients of the fused backbone pass go back into ONE buffer (ops._SplitRows.backward).
struct BlockList {
    const unsigned char* src[MAXVEC];
    long long off[MAXVEC], bytes[MAXVEC];
    int count;
};

__global__ __launch_bounds__(256) void copy_blocks_kernel(const BlockList b, unsigned char* __restrict__ dst) {
    const int k = blockIdx.y;
    const unsigned char* s = b.src[k];
    unsigned char* d = dst + b.off[k];
    const long long n = b.bytes[k];
    const bool vec = s == nullptr ? ((uintptr_t)d & 15) == 0 : (((uintptr_t)s | (uintptr_t)d) & 15) == 0;
    const long long n16 = vec ? n / 16 : 0;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n16; i += (long long)gridDim.x * blockDim.x)
        reinterpret_cast<uint4*>(d)[i] = s ? reinterpret_cast<const uint4*>(s)[i] : make_uint4(0, 0, 0, 0);
    for (long long i = n16 * 16 + (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x)
        d[i] = s ? s[i] : 0;
}

// The step's constants ON THE DEVICE: t = ++(*t_dev); hyper = {lr, 1 - b1^t, sqrt(1 - b2^t), grad_scale} in the host's
// arithmetic (double pow / sqrt, one rounding to f32).  A node of the captured step: a replay needs no host -> device copy
// in front of it (4 us of copy + the gap behind it, per step) and the step count advances with the replays.
__global__ void adam_hyper_kernel(const float* __restrict__ src, long long* __restrict__ t_dev, double b1, double b2,
                                  float* __restrict__ hyper) {
    if (threadIdx.x == 0 && blockIdx.x == 0) {
        const long long t = *t_dev + 1;
        *t_dev = t;
        hyper[0] = src[0];
        hyper[1] = (float)(1.0 - pow(b1, (double)t));
        hyper[2] = (float)sqrt(1.0 - pow(b2, (double)t));
        hyper[3] = src[1];
    }
}

// ---- global gradient norm (clipping inside the step) ---------------------------------------------------------------------
// Sum of squares of n gradient elements: 16-byte loads, grid-stride, products and sums in f64 (the product of two f32 or bf16
// values is exact in f64), ONE f64 partial per workgroup stored to partials[blockIdx.x].  The grid is a function of n alone
// (sumsq_grid) and every partial has one writer: no atomics, the same bits on every launch over the same data.
constexpr int SUMSQ_THREADS = 256;
constexpr long long SUMSQ_PER_WG = 16384;  // elements per workgroup until the grid reaches its cap
constexpr int SUMSQ_MAX_WG = 1024;
static inline int sumsq_grid(long long n) {
    const long long b = (n + SUMSQ_PER_WG - 1) / SUMSQ_PER_WG;
    return (int)(b < 1 ? 1 : b > SUMSQ_MAX_WG ? SUMSQ_MAX_WG : b);
}

__device__ __forceinline__ double sumsq16(const float* __restrict__ g) {
    const float4 v = *reinterpret_cast<const float4*>(g);
    return ((double)v.x * v.x + (double)v.y * v.y) + ((double)v.z * v.z + (double)v.w * v.w);
}
__device__ __forceinline__ double sumsq16(const bf16_t* __restrict__ g) {
    const uint4 r = *reinterpret_cast<const uint4*>(g);
    const unsigned w[4] = {r.x, r.y, r.z, r.w};
    double s = 0.0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const double a = (double)__uint_as_float(w[k] << 16), b = (double)__uint_as_float(w[k] & 0xffff0000u);
        s += a * a + b * b;
    }
    return s;
}

template <typename GT>
__global__ __launch_bounds__(SUMSQ_THREADS) void grad_sumsq_kernel(const GT* __restrict__ g, long long n, double* __restrict__ partials) {
    constexpr int V = 16 / (int)sizeof(GT);  // elements per 16-byte load
    __shared__ double part[SUMSQ_THREADS / 64];
    const long long stride = (long long)gridDim.x * SUMSQ_THREADS * V;
    const long long nv = n / V * V;
    double a0 = 0.0, a1 = 0.0;
    long long i = ((long long)blockIdx.x * SUMSQ_THREADS + threadIdx.x) * V;
    for (; i + stride < nv; i += 2 * stride) {  // two loads in flight per thread
        const double s0 = sumsq16(g + i), s1 = sumsq16(g + i + stride);
        a0 += s0;
        a1 += s1;
    }
    if (i < nv) a0 += sumsq16(g + i);
    if (blockIdx.x == 0 && threadIdx.x == 0)
        for (long long j = nv; j < n; ++j) {  // (a ragged end of fewer than V elements)
            const double x = (double)ld1t(g + j);
            a1 += x * x;
        }
    const double s = wave_sum(a0 + a1);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) partials[blockIdx.x] = (part[0] + part[1]) + (part[2] + part[3]);
}

// Device-side statistics of the clipped steps since the last reset (f64 words, FlatAdam.grad_norm_stats reads them)
enum { GN_STEPS = 0, GN_SUM, GN_MAX, GN_CLIPPED, GN_SKIPPED, GN_LAST, GN_WORDS };

// One workgroup: the partials added in a fixed order (thread t: slots t, t + 256, ... ; then a fixed tree), norm = grad_scale *
// sqrt(sum) -- the norm of the AVERAGED gradient on N ranks -- and torch.nn.utils.clip_grad_norm_'s arithmetic in f32:
// coef = min(1, max_norm / (norm + 1e-6)); hyper[3] = grad_scale * coef, EXACTLY grad_scale when coef clamps to 1.  A norm that
// is not finite closes the gate (the step's Adam launches leave everything untouched) and takes the step back out of t_dev.
__global__ __launch_bounds__(SUMSQ_THREADS) void grad_norm_finalize_kernel(const double* __restrict__ partials, int n_slots,
                                                                           const float* __restrict__ src, float max_norm,
                                                                           float* __restrict__ hyper, long long* __restrict__ t_dev,
                                                                           int* __restrict__ gate, double* __restrict__ stats) {
    __shared__ double part[SUMSQ_THREADS];
    double s = 0.0;
    for (int k = threadIdx.x; k < n_slots; k += SUMSQ_THREADS) s += partials[k];
    part[threadIdx.x] = s;
    __syncthreads();
    for (int w = SUMSQ_THREADS / 2; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) part[threadIdx.x] += part[threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
#pragma clang fp contract(off)
        const float gs = src[1];
        const float norm = (float)((double)gs * sqrt(part[0]));
        const bool finite = norm - norm == 0.f;  // (false for inf and NaN)
        stats[GN_STEPS] += 1.0;
        stats[GN_LAST] = (double)norm;
        if (finite) {
            const float coef = max_norm / (norm + 1e-6f);
            const bool clip = coef < 1.f;
            hyper[3] = clip ? gs * coef : gs;
            *gate = 1;
            stats[GN_SUM] += (double)norm;
            if ((double)norm > stats[GN_MAX]) stats[GN_MAX] = (double)norm;
            if (clip) stats[GN_CLIPPED] += 1.0;
        } else {
            hyper[3] = gs;
            *gate = 0;
            *t_dev -= 1;  // (egk_adam_hyper counted this step: it does not happen)
            stats[GN_SKIPPED] += 1.0;
        }
    }
}

// ---- task weights in device memory (include/egopack_task_scale.h) ---------------------------------------------------------------
// scale[t] = exp(-s[t]) in f64, rounded to f32 once: exactly 1 for s = 0
__global__ __launch_bounds__(64) void task_scale_prepare_kernel(const float* __restrict__ s, float* __restrict__ scale, int n) {
    const int t = threadIdx.x;
    if (t < n) scale[t] = (float)exp(-(double)s[t]);
}

// out[i] = fl32(coef * scale[0]): the seed of a head that runs off the announced-seed paths, as the tensor its backward starts from
__global__ __launch_bounds__(256) void fill_scaled_from_kernel(float* __restrict__ out, long long n, float coef,
                                                               const float* __restrict__ scale) {
    const float v = scaled_seed(coef, scale);
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) out[i] = v;
}

struct TaskGrad {
    const float* x[MAXVEC];   // loss vectors (null: the task is absent from this step)
    long long n[MAXVEC];      // their elements
    double count[MAXVEC];     // what the task's mean divides by (>= 1)
    double w[MAXVEC];
    int tasks;
};
// sum of x[0 .. n) in f64 by the 1024 threads of a workgroup, in a fixed order (strided per thread, the wave's butterfly, the 16
// waves in wave order): the same bits on every launch.  Valid in thread 0; every thread of the workgroup must call it.
__device__ __forceinline__ double block_sum_f64(const float* __restrict__ x, long long n, double* part) {
    double a = 0.0;
    for (long long i = threadIdx.x; i < n; i += 1024) a += (double)x[i];
    a = wave_sum(a);
    __syncthreads();  // part[] free (the previous vector consumed)
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = a;
    __syncthreads();
    double t = 0.0;
    if (threadIdx.x == 0)
        for (int i = 0; i < 16; ++i) t += part[i];
    return t;
}
// Workgroup t owns task t: L_t = sum(loss_t) / count_t, acc[t] += sum(loss_t), ds[t] = w_t (1 - scale_t L_t) -- one writer each.
// Workgroup 0 also walks every task in order for the reported objective (the same sums, so the same bits): no atomics, no workspace.
// s == null: fixed scales (the ``manual`` mode) -- no ds, objective = sum_t w_t scale_t L_t.
__global__ __launch_bounds__(1024) void task_scale_grad_kernel(const TaskGrad v, const float* __restrict__ s,
                                                               const float* __restrict__ scale, float* __restrict__ ds,
                                                               float* __restrict__ objective, double* __restrict__ acc) {
    __shared__ double part[16];
    const int me = blockIdx.x;
    double J = 0.0;
    for (int k = me == 0 ? 0 : me; k < (me == 0 ? v.tasks : me + 1); ++k) {
        const bool present = v.x[k] != nullptr;
        const double S = block_sum_f64(v.x[k], present ? v.n[k] : 0, part);
        if (threadIdx.x == 0) {
            const double L = S / v.count[k], sc = (double)scale[k];
            if (k == me) {
                if (acc) acc[k] += S;
                if (s) ds[k] = present ? (float)(v.w[k] * (1.0 - sc * L)) : 0.f;
            }
            if (present) J += v.w[k] * (sc * L + (s ? (double)s[k] : 0.0));
        }
    }
    if (me == 0 && threadIdx.x == 0) objective[0] = (float)J;
}

static inline unsigned ew_grid(long long n, int per_thread) {
    long long b = (n / per_thread + 255) / 256;
    return (unsigned)(b < 1 ? 1 : b > 4096 ? 4096 : b);
}

}  // namespace egk

using namespace egk;


extern "C" {

int egk_dropout_fwd(egk_stream_t stream, const void* x, void* y, uint8_t* mask, int64_t n, float p, uint64_t seed,
                    uint64_t offset, const uint64_t* dev_offset, int32_t dtype) {
    EGK_REQUIRE(x && y && mask, "egk_dropout_fwd: null pointer");
    EGK_REQUIRE(p >= 0.f && p < 1.f, "egk_dropout_fwd: p out of range");
    if (n == 0) return 0;
    hipStream_t s = (hipStream_t)stream;
    ProfScope prof(KID_DROPOUT_FWD, s, 0, 9.0 * n);
    EGK_DISPATCH_T(dtype, hipLaunchKernelGGL(dropout_fwd_kernel<T>, dim3(ew_grid(n, 4)), dim3(256), 0, s, (const T*)x, (T*)y, mask,
                                             (long long)n, p, seed, offset, dev_offset));
    return check_launch("egk_dropout_fwd");
}

int egk_dropout_bwd(egk_stream_t stream, const void* dy, const uint8_t* mask, void* dx, int64_t n, float p, int32_t dtype) {
    EGK_REQUIRE(dy && mask && dx, "egk_dropout_bwd: null pointer");
    if (n == 0) return 0;
    hipStream_t s = (hipStream_t)stream;
    ProfScope prof(KID_DROPOUT_BWD, s, 0, 9.0 * n);
    EGK_DISPATCH_T(dtype, hipLaunchKernelGGL(dropout_bwd_kernel<T>, dim3(ew_grid(n, 1)), dim3(256), 0, s, (const T*)dy, mask,
                                             (T*)dx, (long long)n, p));
    return check_launch("egk_dropout_bwd");
}

int egk_relu_gate(egk_stream_t stream, const void* dy, const void* y, void* dx, int64_t n, int32_t dtype) {
    EGK_REQUIRE(dy && y && dx, "egk_relu_gate: null pointer");
    if (n == 0) return 0;
    const int vec = (((uintptr_t)dy | (uintptr_t)y | (uintptr_t)dx) & 15) == 0;
    hipStream_t s = (hipStream_t)stream;
    ProfScope prof(KID_RELU_GATE, s, 0, 12.0 * n);
    EGK_DISPATCH_T(dtype, hipLaunchKernelGGL(relu_gate_kernel<T>, dim3(ew_grid(n, 4)), dim3(256), 0, s, (const T*)dy, (const T*)y,
                                             (T*)dx, (long long)n, vec));
    return check_launch("egk_relu_gate");
}

int egk_axpby(egk_stream_t stream, const float* x, const float* y, float* out, int64_t n, float a, float b) {
    EGK_REQUIRE(x && out, "egk_axpby: null pointer");
    if (n == 0) return 0;
    const int vec = ((uintptr_t)x & 15) == 0 && ((uintptr_t)out & 15) == 0 && (!y || ((uintptr_t)y & 15) == 0);
    hipStream_t s = (hipStream_t)stream;
    ProfScope prof(KID_AXPBY, s, 0, (y ? 12.0 : 8.0) * n);
    hipLaunchKernelGGL(axpby_kernel, dim3(ew_grid(n, 4)), dim3(256), 0, s, x, y, out, (long long)n, a, b, vec);
    return check_launch("egk_axpby");
}

int egk_fill_scaled(egk_stream_t stream, const float* scalar, float coef, float* out, int64_t n) {
    EGK_REQUIRE(scalar && out, "egk_fill_scaled: null pointer");
    if (n == 0) return 0;
    hipStream_t s = (hipStream_t)stream;
    ProfScope prof(KID_AXPBY, s, 0, 4.0 * n);
    hipLaunchKernelGGL(fill_scaled_kernel, dim3(ew_grid(n, 1)), dim3(256), 0, s, scalar, coef, out, (long long)n);
    return check_launch("egk_fill_scaled");
}

int egk_sum_scale(egk_stream_t stream, const float* x, float* out, int64_t n, float scale, int32_t accumulate) {
    EGK_REQUIRE(x && out, "egk_sum_scale: null pointer");
    hipStream_t s = (hipStream_t)stream;
    ProfScope prof(KID_SUM_SCALE, s, 0, 4.0 * n);
    hipLaunchKernelGGL(sum_scale_kernel, dim3(1), dim3(1024), 0, s, x, out, (long long)n, scale, accumulate);
    return check_launch("egk_sum_scale");
}

int egk_weighted_sums(egk_stream_t stream, const float* const* xs, const int64_t* ns, const float* coefs, int32_t count,
                      float* out) {
    return egk_weighted_sums_acc(stream, xs, ns, coefs, count, out, nullptr);
}

int egk_weighted_sums_acc(egk_stream_t stream, const float* const* xs, const int64_t* ns, const float* coefs, int32_t count,
                          float* out, double* acc) {
    EGK_REQUIRE(xs && ns && coefs && out, "egk_weighted_sums: null pointer");
    EGK_REQUIRE(count >= 1 && count <= MAXVEC, "egk_weighted_sums: 1..%d vectors", MAXVEC);
    VecList v{};
    double bytes = 0;
    for (int k = 0; k < count; ++k) {
        EGK_REQUIRE(xs[k] || ns[k] == 0, "egk_weighted_sums: null vector");
        v.x[k] = xs[k]; v.n[k] = ns[k]; v.coef[k] = coefs[k];
        bytes += 4.0 * ns[k];
    }
    v.count = count;
    hipStream_t s = (hipStream_t)stream;
    ProfScope prof(KID_SUM_SCALE, s, 0, bytes);
    hipLaunchKernelGGL(weighted_sums_kernel, dim3(1), dim3(1024), 0, s, v, out, acc);
    return check_launch("egk_weighted_sums");
}

int egk_fill_scaled_multi(egk_stream_t stream, const float* scalar, const float* coefs, float* const* outs, const int64_t* ns,
                          int32_t count) {
    EGK_REQUIRE(scalar && coefs && outs && ns, "egk_fill_scaled_multi: null pointer");
    EGK_REQUIRE(count >= 1 && count <= MAXVEC, "egk_fill_scaled_multi: 1..%d vectors", MAXVEC);
    VecList v{};
    long long nmax = 0;
    for (int k = 0; k < count; ++k) {
        EGK_REQUIRE(outs[k] || ns[k] == 0, "egk_fill_scaled_multi: null vector");
        v.out[k] = outs[k]; v.n[k] = ns[k]; v.coef[k] = coefs[k];
        nmax = ns[k] > nmax ? ns[k] : nmax;
    }
    v.count = count;
    if (nmax == 0) return 0;
    hipStream_t s = (hipStream_t)stream;
    const long long blocks = (nmax + 255) / 256;
    hipLaunchKernelGGL(fill_scaled_multi_kernel, dim3((unsigned)(blocks > 1024 ? 1024 : blocks), count), dim3(256), 0, s, scalar, v);
    return check_launch("egk_fill_scaled_multi");
}

int egk_task_scale_prepare(egk_stream_t stream, const float* s_, float* scale, int32_t n) {
    EGK_REQUIRE(s_ && scale, "egk_task_scale_prepare: null pointer");
    EGK_REQUIRE(n >= 1 && n <= MAXVEC, "egk_task_scale_prepare: 1..%d tasks", MAXVEC);
    EGK_REQUIRE(aligned_to(4, {s_, scale}), "egk_task_scale_prepare: s and scale must be 4-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    ProfScope prof(KID_TASK_SCALE, s, 0, 8.0 * n);
    hipLaunchKernelGGL(task_scale_prepare_kernel, dim3(1), dim3(64), 0, s, s_, scale, n);
    return check_launch("egk_task_scale_prepare");
}

int egk_task_scale_grad(egk_stream_t stream, const float* const* loss, const int64_t* ns, const int64_t* counts, const float* w,
                        const float* s_, const float* scale, float* ds, float* objective, double* acc, int32_t n) {
    EGK_REQUIRE(loss && ns && counts && w && scale && objective, "egk_task_scale_grad: null pointer");
    EGK_REQUIRE(!s_ || ds, "egk_task_scale_grad: null pointer (ds: the gradient of s)");
    EGK_REQUIRE(n >= 1 && n <= MAXVEC, "egk_task_scale_grad: 1..%d tasks", MAXVEC);
    EGK_REQUIRE(aligned_to(4, {s_, scale, ds, objective}) && aligned_to(8, {acc}), "egk_task_scale_grad: misaligned pointer");
    TaskGrad v{};
    double bytes = 0;
    for (int k = 0; k < n; ++k) {
        EGK_REQUIRE(ns[k] >= 0, "egk_task_scale_grad: negative length (task %d)", k);
        EGK_REQUIRE(aligned_to(4, {loss[k]}), "egk_task_scale_grad: misaligned loss vector (task %d)", k);
        v.x[k] = loss[k]; v.n[k] = ns[k]; v.w[k] = (double)w[k];
        v.count[k] = (double)(counts[k] > 0 ? counts[k] : (ns[k] > 0 ? ns[k] : 1));
        if (loss[k]) bytes += 8.0 * ns[k];  // (workgroup 0 reads every vector again)
    }
    v.tasks = n;
    hipStream_t s = (hipStream_t)stream;
    ProfScope prof(KID_TASK_SCALE, s, 0, bytes);
    hipLaunchKernelGGL(task_scale_grad_kernel, dim3(n), dim3(1024), 0, s, v, s_, scale, ds, objective, acc);
    return check_launch("egk_task_scale_grad");
}

int egk_fill_scaled_from(egk_stream_t stream, float* out, int64_t n, float coef, const float* scale) {
    EGK_REQUIRE(out && scale, "egk_fill_scaled_from: null pointer");
    EGK_REQUIRE(n >= 0, "egk_fill_scaled_from: n must be >= 0");
    EGK_REQUIRE(aligned_to(4, {out, scale}), "egk_fill_scaled_from: out and scale must be 4-byte aligned");
    if (n == 0) return 0;
    hipStream_t s = (hipStream_t)stream;
    ProfScope prof(KID_TASK_SCALE, s, 0, 4.0 * n);
    hipLaunchKernelGGL(fill_scaled_from_kernel, dim3(ew_grid(n, 1)), dim3(256), 0, s, out, (long long)n, coef, scale);
    return check_launch("egk_fill_scaled_from");
}

int egk_copy_blocks(egk_stream_t stream, const void* const* srcs, const int64_t* nbytes, void* dst, int32_t count) {
    EGK_REQUIRE(srcs && nbytes && dst, "egk_copy_blocks: null pointer");
    EGK_REQUIRE(count >= 1 && count <= MAXVEC, "egk_copy_blocks: 1..%d blocks", MAXVEC);
    BlockList b{};
    long long off = 0, nmax = 0;
    for (int k = 0; k < count; ++k) {
        b.src[k] = (const unsigned char*)srcs[k]; b.off[k] = off; b.bytes[k] = nbytes[k];
        off += nbytes[k];
        nmax = nbytes[k] > nmax ? nbytes[k] : nmax;
    }
    b.count = count;
    if (nmax == 0) return 0;
    hipStream_t s = (hipStream_t)stream;
    const long long blocks = (nmax / 16 + 255) / 256 + 1;
    hipLaunchKernelGGL(copy_blocks_kernel, dim3((unsigned)(blocks > 2048 ? 2048 : blocks), count), dim3(256), 0, s, b, (unsigned char*)dst);
    return check_launch("egk_copy_blocks");
}

// the flat gradient buffer cleared by a launch of the library (16-byte stores; the buffer is 16-byte aligned and padded)
__global__ __launch_bounds__(256) void zero_fill_kernel(uint4* __restrict__ p, long long n16) {
    const uint4 z = make_uint4(0u, 0u, 0u, 0u);
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n16; i += (long long)gridDim.x * blockDim.x) p[i] = z;
}

int egk_zero_fill(egk_stream_t stream, void* p, int64_t bytes) {
    EGK_REQUIRE(p || bytes == 0, "egk_zero_fill: null pointer");
    EGK_REQUIRE(((uintptr_t)p & 15) == 0 && (bytes & 15) == 0 && bytes >= 0, "egk_zero_fill: 16-byte aligned buffer of whole 16-byte groups");
    if (bytes == 0) return 0;
    hipStream_t s = (hipStream_t)stream;
    const long long n16 = bytes / 16;
    const long long blocks = (n16 + 255) / 256;
    // A GENTLE fill: the captured step clears the gradient buffer beside its forward pass, with ~0.4 ms to spare -- at full
    // rate (4096 workgroups, 5 TB/s) the 100 MB burst doubled the HBM-bound row kernel it ran beside (positional-encoding add
    // 7.2 -> 15.7 us, profiles/r05_c3_replay_timeline.txt at 141 us): at most 64 workgroups.
    // Same box, three alternating rounds of the headline step: 4096 workgroups 1.407-1.417 ms, 192: 1.399-1.413, 64: 1.401-1.408
    const long long cap = 64;
    hipLaunchKernelGGL(zero_fill_kernel, dim3((unsigned)(blocks > cap ? cap : blocks)), dim3(256), 0, s, (uint4*)p, n16);
    return check_launch("egk_zero_fill");
}

// up to ZERO_MAX_RANGES byte ranges of one buffer cleared by ONE launch (blockIdx.y = range): the gradient slots that are still
// accumulated into once the matrices whose ONE weight-gradient launch stores its result are left alone (FlatAdam.store_slots)
constexpr int ZERO_MAX_RANGES = 48;
struct ByteRanges {
    long long begin[ZERO_MAX_RANGES], len[ZERO_MAX_RANGES];
};
__global__ __launch_bounds__(256) void zero_ranges_kernel(unsigned char* __restrict__ base, const ByteRanges R) {
    uint4* p = reinterpret_cast<uint4*>(base + R.begin[blockIdx.y]);
    const long long n16 = R.len[blockIdx.y] >> 4;
    const uint4 z = make_uint4(0u, 0u, 0u, 0u);
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n16; i += (long long)gridDim.x * blockDim.x) p[i] = z;
}

int egk_zero_fill_ranges(egk_stream_t stream, void* base, const int64_t* begin, const int64_t* bytes, int32_t n_ranges) {
    EGK_REQUIRE(base && begin && bytes, "egk_zero_fill_ranges: null pointer");
    EGK_REQUIRE(n_ranges >= 1 && n_ranges <= ZERO_MAX_RANGES, "egk_zero_fill_ranges: 1 .. %d ranges per launch", ZERO_MAX_RANGES);
    EGK_REQUIRE(((uintptr_t)base & 15) == 0, "egk_zero_fill_ranges: 16-byte aligned buffer");
    ByteRanges R;
    long long longest = 0;
    for (int i = 0; i < ZERO_MAX_RANGES; ++i) {
        R.begin[i] = i < n_ranges ? begin[i] : 0;
        R.len[i] = i < n_ranges ? bytes[i] : 0;
        if (i < n_ranges) {
            EGK_REQUIRE(begin[i] >= 0 && bytes[i] >= 0 && begin[i] % 16 == 0 && bytes[i] % 16 == 0,
                        "egk_zero_fill_ranges: ranges of whole 16-byte groups");
            longest = bytes[i] > longest ? bytes[i] : longest;
        }
    }
    if (longest == 0) return 0;
    long long gx = (longest / 16 + 255) / 256;
    if (gx > 16) gx = 16;  // (gentle, as egk_zero_fill: it runs beside the forward pass)
    hipLaunchKernelGGL(zero_ranges_kernel, dim3((unsigned)gx, n_ranges), dim3(256), 0, (hipStream_t)stream, (unsigned char*)base, R);
    return check_launch("egk_zero_fill_ranges");
}

int egk_adam_hyper(egk_stream_t stream, const float* src, int64_t* t_dev, double beta1, double beta2, float* hyper) {
    EGK_REQUIRE(src && t_dev && hyper, "egk_adam_hyper: null pointer");
    hipLaunchKernelGGL(adam_hyper_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, src, (long long*)t_dev, beta1, beta2, hyper);
    return check_launch("egk_adam_hyper");
}

int egk_grad_sumsq_slots(int64_t n) { return n > 0 ? sumsq_grid((long long)n) : 0; }

int egk_grad_sumsq(egk_stream_t stream, const void* g, int32_t g_dtype, int64_t n, double* partials, int32_t n_slots) {
    EGK_REQUIRE(g && partials, "egk_grad_sumsq: null pointer");
    EGK_REQUIRE(((uintptr_t)g & 15) == 0, "egk_grad_sumsq: the gradient slice must be 16-byte aligned");
    EGK_REQUIRE(((uintptr_t)partials & 7) == 0, "egk_grad_sumsq: the partial sums must be 8-byte aligned");
    EGK_REQUIRE(n > 0, "egk_grad_sumsq: n >= 1 (got %lld)", (long long)n);
    const int grid = sumsq_grid((long long)n);
    EGK_REQUIRE(n_slots == grid, "egk_grad_sumsq: %lld elements write %d partial sums (egk_grad_sumsq_slots), the caller gave %d slots",
                (long long)n, grid, (int)n_slots);
    hipStream_t s = (hipStream_t)stream;
    EGK_DISPATCH_T(g_dtype, hipLaunchKernelGGL(grad_sumsq_kernel<T>, dim3(grid), dim3(SUMSQ_THREADS), 0, s, (const T*)g, (long long)n, partials));
    return check_launch("egk_grad_sumsq");
}

int egk_grad_norm_finalize(egk_stream_t stream, const double* partials, int32_t n_slots, const float* src, float max_norm,
                           float* hyper, int64_t* t_dev, int32_t* gate, double* stats) {
    EGK_REQUIRE(partials && src && hyper && t_dev && gate && stats, "egk_grad_norm_finalize: null pointer");
    EGK_REQUIRE(n_slots >= 1, "egk_grad_norm_finalize: at least one partial sum (got %d)", (int)n_slots);
    EGK_REQUIRE(max_norm > 0.f, "egk_grad_norm_finalize: max_norm > 0 (got %g)", (double)max_norm);
    hipLaunchKernelGGL(grad_norm_finalize_kernel, dim3(1), dim3(SUMSQ_THREADS), 0, (hipStream_t)stream, partials, (int)n_slots, src,
                       max_norm, hyper, (long long*)t_dev, (int*)gate, stats);
    return check_launch("egk_grad_norm_finalize");
}
}
