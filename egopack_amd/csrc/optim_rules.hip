// The update rules of the flat-buffer optimizer behind one launch interface (include/egopack_optim.h): Adam, AdamW and SGD, the
// single-tensor formulas of torch 2.10.  ONE kernel family in the shape of adam_span / adam_kernel (loss_optim.hip): 16-byte
// accesses on p, g and the state, a scalar tail for n % 4, the bf16 copy and the low half of the stored p, the offset word moved on
// by workgroup 0, one wave-uniform load of the gate.  No atomics; every element has one writer.
// The same family with an exponential moving average of the stored p kept beside it (include/egopack_ema.h): the bottom of the file.
#include "common.h"

namespace egk {

// what a kernel of the family does per element; the rule codes of the ABI map onto these (SGD: by its momentum)
enum { K_ADAM = 0, K_ADAMW, K_SGD, K_SGD_MOMENTUM };
template <int KIND> struct StateCount { static constexpr int value = KIND == K_SGD ? 0 : KIND == K_SGD_MOMENTUM ? 1 : 2; };

struct OptimConsts {
    AdamConsts adam;    // (K_ADAM: adam_update itself, the shipped kernel's bits; K_ADAMW: its step, bc2s, gs, b2, eps; wd through ``decay``)
    float lr, decay;    // decay = 1 - lr * wd
    float omb1, omb2;   // K_ADAMW: 1 - beta1, 1 - beta2 taken in double, rounded once (torch hands its kernels these scalars)
    float wd, gs, mu, damp1;  // damp1 = 1 - dampening
    bool first, nesterov;     // first: no momentum buffer yet (*t_dev == 1)
};

template <int KIND>
__device__ __forceinline__ void optim_update(float& p, float g, float& a, float& b, const OptimConsts& c) {
#pragma clang fp contract(off)  // (no fused multiply-adds: as adam_update)
    if constexpr (KIND == K_ADAM) {
        adam_update(p, g, a, b, c.adam);
    } else if constexpr (KIND == K_ADAMW) {
        p = p * c.decay;                                      // param.mul_(1 - lr * weight_decay)
        const float gg = g * c.gs;
        a = a + (gg - a) * c.omb1;                            // exp_avg.lerp_(grad, 1 - beta1)
        b = b * c.adam.b2 + c.omb2 * gg * gg;                 // mul_(beta2).addcmul_(g, g, 1 - beta2)
        const float denom = sqrtf(b) / c.adam.bc2s + c.adam.eps;
        p = p - c.adam.step * (a / denom);
    } else {
        const float gg = g * c.gs + c.wd * p;                 // grad.add(param, alpha=weight_decay)
        float step = gg;
        if constexpr (KIND == K_SGD_MOMENTUM) {
            a = c.first ? gg : c.mu * a + c.damp1 * gg;       // buf = clone(grad) | buf.mul_(momentum).add_(grad, alpha=1 - dampening)
            step = c.nesterov ? gg + c.mu * a : a;            // grad.add(buf, alpha=momentum) | buf
        }
        p = p - c.lr * step;                                  // param.add_(grad, alpha=-lr)
    }
}

// the moving average of the weights (include/egopack_ema.h): e += w * (p_new - e), three separately rounded f32 operations
__device__ __forceinline__ void ema_update(float& e, float p_new, float w) {
#pragma clang fp contract(off)
    const float diff = p_new - e;
    const float move = w * diff;
    e = e + move;
}

// the four elements [i, i + 4) of a span in 16-byte accesses; ``consts()`` is asked for the constants once the loads are issued.
// EMA: ``ema`` follows the new p with weight ``w`` before p is stored (read with the other loads, one 16-byte store).
template <int KIND, typename GT, bool EMA = false, typename CF>
__device__ __forceinline__ void optim_quad(float* __restrict__ p, const GT* __restrict__ g, float* __restrict__ s0, float* __restrict__ s1,
                                           long long i, CF consts, bf16_t* __restrict__ shadow, bf16_t* __restrict__ shadow_lo,
                                           float* __restrict__ ema = nullptr, float w = 0.f) {
    constexpr int NS = StateCount<KIND>::value;
    float4 pv = *reinterpret_cast<float4*>(p + i);
    const float4 gv = ld4t(g + i, 0, 4, true);
    float4 av = make_float4(0.f, 0.f, 0.f, 0.f), bv = av, ev = av;
    if constexpr (NS >= 1) av = *reinterpret_cast<float4*>(s0 + i);
    if constexpr (NS >= 2) bv = *reinterpret_cast<float4*>(s1 + i);
    if constexpr (EMA) ev = *reinterpret_cast<float4*>(ema + i);
    const OptimConsts c = consts();
    float* pp = &pv.x; const float* gp = &gv.x; float* ap = &av.x; float* bp = &bv.x;
#pragma unroll
    for (int t = 0; t < 4; ++t) optim_update<KIND>(pp[t], gp[t], ap[t], bp[t], c);
    if constexpr (EMA) {
        float* ep = &ev.x;
#pragma unroll
        for (int t = 0; t < 4; ++t) ema_update(ep[t], pp[t], w);
        *reinterpret_cast<float4*>(ema + i) = ev;
    }
    *reinterpret_cast<float4*>(p + i) = pv;
    if constexpr (NS >= 1) *reinterpret_cast<float4*>(s0 + i) = av;
    if constexpr (NS >= 2) *reinterpret_cast<float4*>(s1 + i) = bv;
    if (shadow) st4t(shadow + i, 0, 4, true, pv);
    if (shadow_lo) {  // bf16(p - bf16(p)): egk_split_bf16's bits
        const float lo4[4] = {pp[0] - bf2f(f2bf(pp[0])), pp[1] - bf2f(f2bf(pp[1])), pp[2] - bf2f(f2bf(pp[2])), pp[3] - bf2f(f2bf(pp[3]))};
        st4t(shadow_lo + i, 0, 4, true, make_float4(lo4[0], lo4[1], lo4[2], lo4[3]));
    }
}

// the scalar tail [i, n) of a span (n - i < 4)
template <int KIND, typename GT, bool EMA = false>
__device__ __forceinline__ void optim_tail(float* __restrict__ p, const GT* __restrict__ g, float* __restrict__ s0, float* __restrict__ s1,
                                           long long i, long long n, const OptimConsts& c, bf16_t* __restrict__ shadow,
                                           bf16_t* __restrict__ shadow_lo, float* __restrict__ ema = nullptr, float w = 0.f) {
    constexpr int NS = StateCount<KIND>::value;
    for (long long j = i; j < n; ++j) {
        float a = 0.f, b = 0.f;
        if constexpr (NS >= 1) a = s0[j];
        if constexpr (NS >= 2) b = s1[j];
        optim_update<KIND>(p[j], ld1t(g + j), a, b, c);
        if constexpr (EMA) {
            float e = ema[j];
            ema_update(e, p[j], w);
            ema[j] = e;
        }
        if constexpr (NS >= 1) s0[j] = a;
        if constexpr (NS >= 2) s1[j] = b;
        if (shadow) shadow[j] = f2bf(p[j]);
        if (shadow_lo) shadow_lo[j] = f2bf(p[j] - bf2f(f2bf(p[j])));
    }
}

// the elements [0, n) of one span, grid-stride over ``nblk`` workgroups
template <int KIND, typename GT, bool EMA = false>
__device__ __forceinline__ void optim_span(float* __restrict__ p, const GT* __restrict__ g, float* __restrict__ s0, float* __restrict__ s1,
                                           long long n, const OptimConsts& c, bf16_t* __restrict__ shadow, bf16_t* __restrict__ shadow_lo,
                                           int blk, int nblk, float* __restrict__ ema = nullptr, float w = 0.f) {
    for (long long i = ((long long)blk * blockDim.x + threadIdx.x) * 4; i < n; i += (long long)nblk * blockDim.x * 4) {
        if (i + 4 <= n)
            optim_quad<KIND, GT, EMA>(p, g, s0, s1, i, [&]() -> const OptimConsts& { return c; }, shadow, shadow_lo, ema, w);
        else
            optim_tail<KIND, GT, EMA>(p, g, s0, s1, i, n, c, shadow, shadow_lo, ema, w);
    }
}

struct OptimHyper {  // the host's scalars of a launch
    float b1, b2, omb1, omb2, eps, wd, mu, damp1;
    int nesterov;
};

// the constants of a launch from its learning rate and weight decay (of the launch: optim_kernel; of a group: optim_groups_kernel)
template <int KIND>
__device__ __forceinline__ OptimConsts optim_consts(float lr, float wd, const float* __restrict__ hyper, const long long* __restrict__ t_dev,
                                                    const OptimHyper& h) {
#pragma clang fp contract(off)
    OptimConsts c;
    c.adam = AdamConsts{lr / hyper[1], hyper[2], hyper[3], h.b1, h.b2, h.eps, wd};
    c.lr = lr;
    c.decay = (float)(1.0 - (double)lr * (double)wd);  // (torch takes 1 - lr * weight_decay in double and rounds it once)
    c.wd = wd;
    c.gs = hyper[3];
    c.omb1 = h.omb1;
    c.omb2 = h.omb2;
    c.mu = h.mu;
    c.damp1 = h.damp1;
    c.nesterov = h.nesterov != 0;
    c.first = KIND == K_SGD_MOMENTUM ? *t_dev == 1 : false;  // (egk_adam_hyper has counted this step)
    return c;
}

template <int KIND, typename GT, bool GATED>  // GT: element type of the gradient buffer (f32, or bf16 after a compressed all-reduce)
__global__ __launch_bounds__(256) void optim_kernel(float* __restrict__ p, const GT* __restrict__ g, float* __restrict__ s0,
                                                    float* __restrict__ s1, long long n, const float* __restrict__ hyper,
                                                    const long long* __restrict__ t_dev, const OptimHyper h, bf16_t* __restrict__ shadow,
                                                    bf16_t* __restrict__ shadow_lo, long long* __restrict__ bump_word, long long bump,
                                                    const int* __restrict__ gate) {
    // (the step's dropout offset word moves on inside this launch, whether the step happens or not: adam_kernel)
    if (bump_word && blockIdx.x == 0 && threadIdx.x == 0) *bump_word += bump;
    // (a closed gate -- the gradient norm was not finite -- skips the step: one wave-uniform load, nothing else is touched)
    if (GATED && *gate == 0) return;
    const OptimConsts c = optim_consts<KIND>(hyper[0], h.wd, hyper, t_dev, h);
    optim_span<KIND, GT>(p, g, s0, s1, n, c, shadow, shadow_lo, blockIdx.x, gridDim.x);
}

template <int KIND, typename GT>
static void optim_launch(hipStream_t s, unsigned grid, const egk_optim_desc& d, const OptimHyper& h) {
    if (d.gate)
        hipLaunchKernelGGL((optim_kernel<KIND, GT, true>), dim3(grid), dim3(256), 0, s, d.p, (const GT*)d.g, d.state0, d.state1,
                           (long long)d.n, d.hyper, (const long long*)d.t_dev, h, (bf16_t*)d.bf16_shadow, (bf16_t*)d.bf16_lo_shadow,
                           (long long*)d.bump_word, (long long)d.bump, (const int*)d.gate);
    else
        hipLaunchKernelGGL((optim_kernel<KIND, GT, false>), dim3(grid), dim3(256), 0, s, d.p, (const GT*)d.g, d.state0, d.state1,
                           (long long)d.n, d.hyper, (const long long*)d.t_dev, h, (bf16_t*)d.bf16_shadow, (bf16_t*)d.bf16_lo_shadow,
                           (long long*)d.bump_word, (long long)d.bump, (const int*)nullptr);
}

// ---- parameter groups: lr and weight decay per element from a segment table (include/egopack_optim_groups.h) ----------------------
struct GroupTable {
    long long base;
    int n_seg, n_groups;
    const long long* __restrict__ seg_begin;
    const int* __restrict__ seg_group;
    const float* __restrict__ group_hyper;
};

// the largest s in [lo, hi] with seg_begin[s] <= e (lo when there is none): every index read lies in [lo + 1, hi], whatever the table holds
__device__ __forceinline__ int seg_find(const long long* __restrict__ seg_begin, int lo, int hi, long long e) {
    while (lo < hi) {
        const int mid = lo + ((hi - lo + 1) >> 1);
        if (seg_begin[mid] <= e) lo = mid; else hi = mid - 1;
    }
    return lo;
}

// the constants of the group that holds element i of the 1024-element block at b0 (the lookup optim_groups_kernel describes)
template <int KIND>
__device__ __forceinline__ OptimConsts group_consts(const GroupTable& t, long long b0, long long i, long long n,
                                                    const float* __restrict__ hyper, const long long* __restrict__ t_dev,
                                                    const OptimHyper& h) {
    const long long first = t.base + b0, last = t.base + (b0 + 1024 < n ? b0 + 1024 : n) - 1;
    int s = seg_find(t.seg_begin, 0, t.n_seg - 1, first);
    if (t.seg_begin[s + 1] <= last) {  // (s + 1 <= n_seg: the table has n_seg + 1 entries)
        const int hi = s + (int)threadIdx.x < t.n_seg - 1 ? s + (int)threadIdx.x : t.n_seg - 1;
        s = seg_find(t.seg_begin, s, hi, t.base + i);
    }
    int grp = t.seg_group[s];
    grp = grp < 0 ? 0 : grp >= t.n_groups ? t.n_groups - 1 : grp;
    const float2 lw = *reinterpret_cast<const float2*>(t.group_hyper + 4 * grp);
    return optim_consts<KIND>(lw.x, lw.y, hyper, t_dev, h);
}

// optim_kernel with the constants of the group that holds the element.  The lookup: ONE search per workgroup and 1024-element block
// for the segment of the block's first element -- workgroup-uniform, so it runs on the scalar unit while the block's vector loads are
// in flight -- and one comparison that tells whether the block ends inside that segment.  Only the lanes of a block that straddles
// a boundary search for themselves, over the at most 256 segments a block can touch.  A 16-byte group of elements never
// straddles (boundaries and base are multiples of 4), so the scalar tail shares the segment of its first element.
template <int KIND, typename GT, bool GATED>
__global__ __launch_bounds__(256) void optim_groups_kernel(float* __restrict__ p, const GT* __restrict__ g, float* __restrict__ s0,
                                                           float* __restrict__ s1, long long n, const float* __restrict__ hyper,
                                                           const long long* __restrict__ t_dev, const OptimHyper h,
                                                           bf16_t* __restrict__ shadow, bf16_t* __restrict__ shadow_lo,
                                                           long long* __restrict__ bump_word, long long bump, const int* __restrict__ gate,
                                                           const GroupTable t) {
    if (bump_word && blockIdx.x == 0 && threadIdx.x == 0) *bump_word += bump;
    if (GATED && *gate == 0) return;
    for (long long b0 = (long long)blockIdx.x * 1024; b0 < n; b0 += (long long)gridDim.x * 1024) {
        const long long i = b0 + (long long)threadIdx.x * 4;
        if (i >= n) continue;
        auto consts = [&]() -> OptimConsts { return group_consts<KIND>(t, b0, i, n, hyper, t_dev, h); };
        if (i + 4 <= n)
            optim_quad<KIND, GT>(p, g, s0, s1, i, consts, shadow, shadow_lo);
        else
            optim_tail<KIND, GT>(p, g, s0, s1, i, n, consts(), shadow, shadow_lo);
    }
}

template <int KIND, typename GT>
static void optim_groups_launch(hipStream_t s, unsigned grid, const egk_optim_desc& d, const OptimHyper& h, const GroupTable& t) {
    if (d.gate)
        hipLaunchKernelGGL((optim_groups_kernel<KIND, GT, true>), dim3(grid), dim3(256), 0, s, d.p, (const GT*)d.g, d.state0, d.state1,
                           (long long)d.n, d.hyper, (const long long*)d.t_dev, h, (bf16_t*)d.bf16_shadow, (bf16_t*)d.bf16_lo_shadow,
                           (long long*)d.bump_word, (long long)d.bump, (const int*)d.gate, t);
    else
        hipLaunchKernelGGL((optim_groups_kernel<KIND, GT, false>), dim3(grid), dim3(256), 0, s, d.p, (const GT*)d.g, d.state0, d.state1,
                           (long long)d.n, d.hyper, (const long long*)d.t_dev, h, (bf16_t*)d.bf16_shadow, (bf16_t*)d.bf16_lo_shadow,
                           (long long*)d.bump_word, (long long)d.bump, (const int*)nullptr, t);
}

// ---- the moving average of the weights inside the launch (include/egopack_ema.h) ----------------------------------------------------
struct EmaArgs {
    float* __restrict__ ema;
    double decay;   // warmup: d_t = min(decay, (1 + t) / (10 + t)) from the device step counter
    float w;        // no warmup: (float)(1.0 - decay), rounded on the host
    int warmup;
};

__device__ __forceinline__ float ema_weight(const EmaArgs& e, const long long* __restrict__ t_dev) {
    if (!e.warmup) return e.w;
    const double t = (double)*t_dev;  // (egk_adam_hyper has counted this step)
    const double ramp = (1.0 + t) / (10.0 + t);
    return (float)(1.0 - (e.decay < ramp ? e.decay : ramp));
}

// optim_kernel (GROUPED = false) / optim_groups_kernel (GROUPED = true) with the average: optim_update, optim_quad and optim_tail
// are theirs.  The gate pointer is tested at run time (wave-uniform), so the family has one kernel per (kind, gradient type, table).
template <int KIND, typename GT, bool GROUPED>
__global__ __launch_bounds__(256) void optim_ema_kernel(float* __restrict__ p, const GT* __restrict__ g, float* __restrict__ s0,
                                                        float* __restrict__ s1, long long n, const float* __restrict__ hyper,
                                                        const long long* __restrict__ t_dev, const OptimHyper h,
                                                        bf16_t* __restrict__ shadow, bf16_t* __restrict__ shadow_lo,
                                                        long long* __restrict__ bump_word, long long bump, const int* __restrict__ gate,
                                                        const GroupTable t, const EmaArgs e) {
    if (bump_word && blockIdx.x == 0 && threadIdx.x == 0) *bump_word += bump;
    if (gate && *gate == 0) return;  // (a closed gate: ema, p, the state and the copies stay as they are)
    const float w = ema_weight(e, t_dev);
    if constexpr (!GROUPED) {
        const OptimConsts c = optim_consts<KIND>(hyper[0], h.wd, hyper, t_dev, h);
        optim_span<KIND, GT, true>(p, g, s0, s1, n, c, shadow, shadow_lo, blockIdx.x, gridDim.x, e.ema, w);
    } else {
        for (long long b0 = (long long)blockIdx.x * 1024; b0 < n; b0 += (long long)gridDim.x * 1024) {
            const long long i = b0 + (long long)threadIdx.x * 4;
            if (i >= n) continue;
            auto consts = [&]() -> OptimConsts { return group_consts<KIND>(t, b0, i, n, hyper, t_dev, h); };
            if (i + 4 <= n)
                optim_quad<KIND, GT, true>(p, g, s0, s1, i, consts, shadow, shadow_lo, e.ema, w);
            else
                optim_tail<KIND, GT, true>(p, g, s0, s1, i, n, consts(), shadow, shadow_lo, e.ema, w);
        }
    }
}

template <int KIND, typename GT>
static void optim_ema_launch(hipStream_t s, unsigned grid, const egk_optim_desc& d, const OptimHyper& h, const GroupTable* t, const EmaArgs& e) {
    if (t)
        hipLaunchKernelGGL((optim_ema_kernel<KIND, GT, true>), dim3(grid), dim3(256), 0, s, d.p, (const GT*)d.g, d.state0, d.state1,
                           (long long)d.n, d.hyper, (const long long*)d.t_dev, h, (bf16_t*)d.bf16_shadow, (bf16_t*)d.bf16_lo_shadow,
                           (long long*)d.bump_word, (long long)d.bump, (const int*)d.gate, *t, e);
    else
        hipLaunchKernelGGL((optim_ema_kernel<KIND, GT, false>), dim3(grid), dim3(256), 0, s, d.p, (const GT*)d.g, d.state0, d.state1,
                           (long long)d.n, d.hyper, (const long long*)d.t_dev, h, (bf16_t*)d.bf16_shadow, (bf16_t*)d.bf16_lo_shadow,
                           (long long*)d.bump_word, (long long)d.bump, (const int*)d.gate, GroupTable{}, e);
}

// p[i] <-> ema[i]: 16-byte accesses, a scalar tail for n % 4, grid-stride
__global__ __launch_bounds__(256) void ema_swap_kernel(float* __restrict__ p, float* __restrict__ ema, long long n) {
    for (long long i = ((long long)blockIdx.x * blockDim.x + threadIdx.x) * 4; i < n; i += (long long)gridDim.x * blockDim.x * 4) {
        if (i + 4 <= n) {
            const float4 pv = *reinterpret_cast<float4*>(p + i), ev = *reinterpret_cast<float4*>(ema + i);
            *reinterpret_cast<float4*>(p + i) = ev;
            *reinterpret_cast<float4*>(ema + i) = pv;
        } else {
            for (long long j = i; j < n; ++j) {
                const float a = p[j], b = ema[j];
                p[j] = b;
                ema[j] = a;
            }
        }
    }
}

// what both entry points refuse, before any launch; ``a``: the descriptor without the state the rule does not have, ``kind``: its kernel
static int optim_check(const char* who, const egk_optim_desc* d, egk_optim_desc& a, int& kind) {
    EGK_REQUIRE(d, "%s: null descriptor", who);
    EGK_REQUIRE(d->rule == EGK_OPT_ADAM || d->rule == EGK_OPT_ADAMW || d->rule == EGK_OPT_SGD,
                "%s: unknown rule %d (EGK_OPT_ADAM = 0, EGK_OPT_ADAMW = 1, EGK_OPT_SGD = 2)", who, (int)d->rule);
    EGK_REQUIRE(d->g_dtype == EGK_F32 || d->g_dtype == EGK_BF16, "%s: unknown gradient dtype %d", who, (int)d->g_dtype);
    EGK_REQUIRE(d->p && d->g && d->hyper, "%s: null pointer", who);
    EGK_REQUIRE(d->n >= 0, "%s: n >= 0 (got %lld)", who, (long long)d->n);
    const bool sgd = d->rule == EGK_OPT_SGD;
    kind = !sgd ? (d->rule == EGK_OPT_ADAM ? K_ADAM : K_ADAMW) : d->momentum != 0.f ? K_SGD_MOMENTUM : K_SGD;
    if (kind == K_ADAM || kind == K_ADAMW)
        EGK_REQUIRE(d->state0 && d->state1, "%s: missing state pointer -- Adam and AdamW need state0 (exp_avg) and state1 (exp_avg_sq)", who);
    if (kind == K_SGD_MOMENTUM)
        EGK_REQUIRE(d->state0 && d->t_dev, "%s: missing state pointer -- SGD with momentum needs state0 (the momentum buffer) "
                                           "and t_dev (the step counter)", who);
    if (sgd) {
        EGK_REQUIRE(d->momentum >= 0.f, "%s: momentum >= 0 (got %g)", who, (double)d->momentum);
        EGK_REQUIRE(!d->nesterov || (d->momentum > 0.f && d->dampening == 0.f),
                    "%s: nesterov momentum requires a momentum and zero dampening", who);
    }
    // (state the rule does not have is neither checked nor handed to the kernel)
    a = *d;
    if (kind == K_SGD) a.state0 = nullptr;
    if (kind == K_SGD || kind == K_SGD_MOMENTUM) a.state1 = nullptr;
    EGK_REQUIRE((((uintptr_t)a.p | (uintptr_t)a.g | (uintptr_t)a.state0 | (uintptr_t)a.state1) & 15) == 0,
                "%s: buffers must be 16-byte aligned", who);
    EGK_REQUIRE(((uintptr_t)a.bf16_shadow & 7) == 0, "%s: shadow must be 8-byte aligned", who);
    EGK_REQUIRE(((uintptr_t)a.bf16_lo_shadow & 7) == 0, "%s: low-half shadow must be 8-byte aligned", who);
    return 0;
}

// what the grouped entry points refuse in their table
static int groups_check(const char* who, const egk_optim_groups* g) {
    EGK_REQUIRE(g, "%s: null group table", who);
    EGK_REQUIRE(g->n_seg >= 1 && g->n_seg <= 4096, "%s: n_seg in 1..4096 (got %d)", who, (int)g->n_seg);
    EGK_REQUIRE(g->n_groups >= 1 && g->n_groups <= 64, "%s: n_groups in 1..64 (got %d)", who, (int)g->n_groups);
    EGK_REQUIRE(g->seg_begin && g->seg_group && g->group_hyper, "%s: null table pointer", who);
    EGK_REQUIRE(g->base >= 0 && g->base % 4 == 0, "%s: base must be a non-negative multiple of 4 (got %lld)", who, (long long)g->base);
    EGK_REQUIRE(((uintptr_t)g->seg_begin & 7) == 0 && ((uintptr_t)g->seg_group & 3) == 0 && ((uintptr_t)g->group_hyper & 15) == 0,
                "%s: misaligned table pointer (seg_begin 8-byte, seg_group 4-byte, group_hyper 16-byte)", who);
    return 0;
}

// bytes per parameter: p read + written, each state buffer read + written, the gradient read, the bf16 copies written
static double optim_bytes(const egk_optim_desc& a, int kind) {
    const double state_bytes = kind == K_SGD ? 0.0 : kind == K_SGD_MOMENTUM ? 8.0 : 16.0;
    return (8.0 + state_bytes + (a.g_dtype == EGK_BF16 ? 2.0 : 4.0) + (a.bf16_shadow ? 2.0 : 0.0) + (a.bf16_lo_shadow ? 2.0 : 0.0)) * (double)a.n;
}

// the grid of egk_adam_step*: one 1024-element group per workgroup up to 32768 of them (measured there)
static unsigned optim_grid(long long n) {
    const long long want = (n / 4 + 255) / 256;
    const long long cap = 32768;
    return (unsigned)(want < 1 ? 1 : want > cap ? cap : want);
}

static GroupTable group_table(const egk_optim_groups& g) {
    return GroupTable{(long long)g.base, (int)g.n_seg, (int)g.n_groups, (const long long*)g.seg_begin, (const int*)g.seg_group, g.group_hyper};
}

static OptimHyper optim_hyper(const egk_optim_desc& a) {
    return OptimHyper{(float)a.beta1, (float)a.beta2, (float)(1.0 - a.beta1), (float)(1.0 - a.beta2), a.eps, a.weight_decay, a.momentum,
                      (float)(1.0 - (double)a.dampening), a.nesterov ? 1 : 0};
}

}  // namespace egk

using namespace egk;

extern "C" int egk_optim_step(egk_stream_t stream, const egk_optim_desc* d) {
    egk_optim_desc a;
    int kind = 0;
    if (const int rc = optim_check("egk_optim_step", d, a, kind)) return rc;
    if (a.n == 0) return 0;
    hipStream_t s = (hipStream_t)stream;
    ProfScope prof(KID_OPTIM, s, 0, optim_bytes(a, kind));
    const unsigned grid = optim_grid(a.n);
    const OptimHyper h = optim_hyper(a);
    switch (kind) {
        case K_ADAM: EGK_DISPATCH_T(a.g_dtype, (optim_launch<K_ADAM, T>(s, grid, a, h))); break;
        case K_ADAMW: EGK_DISPATCH_T(a.g_dtype, (optim_launch<K_ADAMW, T>(s, grid, a, h))); break;
        case K_SGD: EGK_DISPATCH_T(a.g_dtype, (optim_launch<K_SGD, T>(s, grid, a, h))); break;
        default: EGK_DISPATCH_T(a.g_dtype, (optim_launch<K_SGD_MOMENTUM, T>(s, grid, a, h))); break;
    }
    return check_launch("egk_optim_step");
}

extern "C" int egk_optim_step_groups(egk_stream_t stream, const egk_optim_desc* d, const egk_optim_groups* g) {
    egk_optim_desc a;
    int kind = 0;
    if (const int rc = optim_check("egk_optim_step_groups", d, a, kind)) return rc;
    if (const int rc = groups_check("egk_optim_step_groups", g)) return rc;
    if (a.n == 0) return 0;
    hipStream_t s = (hipStream_t)stream;
    ProfScope prof(KID_OPTIM_GROUPS, s, 0, optim_bytes(a, kind));
    const unsigned grid = optim_grid(a.n);
    const OptimHyper h = optim_hyper(a);
    const GroupTable t = group_table(*g);
    switch (kind) {
        case K_ADAM: EGK_DISPATCH_T(a.g_dtype, (optim_groups_launch<K_ADAM, T>(s, grid, a, h, t))); break;
        case K_ADAMW: EGK_DISPATCH_T(a.g_dtype, (optim_groups_launch<K_ADAMW, T>(s, grid, a, h, t))); break;
        case K_SGD: EGK_DISPATCH_T(a.g_dtype, (optim_groups_launch<K_SGD, T>(s, grid, a, h, t))); break;
        default: EGK_DISPATCH_T(a.g_dtype, (optim_groups_launch<K_SGD_MOMENTUM, T>(s, grid, a, h, t))); break;
    }
    return check_launch("egk_optim_step_groups");
}

extern "C" int egk_optim_step_ema(egk_stream_t stream, const egk_optim_desc* d, const egk_optim_groups* g, const egk_ema_desc* e) {
    egk_optim_desc a;
    int kind = 0;
    if (const int rc = optim_check("egk_optim_step_ema", d, a, kind)) return rc;
    if (g)
        if (const int rc = groups_check("egk_optim_step_ema", g)) return rc;
    EGK_REQUIRE(e, "egk_optim_step_ema: null ema descriptor");
    EGK_REQUIRE(e->ema, "egk_optim_step_ema: null ema pointer");
    EGK_REQUIRE(((uintptr_t)e->ema & 15) == 0, "egk_optim_step_ema: ema must be 16-byte aligned");
    EGK_REQUIRE(e->decay >= 0.0 && e->decay < 1.0, "egk_optim_step_ema: decay in [0, 1) (got %g)", e->decay);
    EGK_REQUIRE(!e->warmup || a.t_dev, "egk_optim_step_ema: warmup needs t_dev (the device step counter)");
    if (a.n == 0) return 0;
    hipStream_t s = (hipStream_t)stream;
    ProfScope prof(KID_OPTIM_EMA, s, 0, optim_bytes(a, kind) + 8.0 * (double)a.n);
    const unsigned grid = optim_grid(a.n);
    const OptimHyper h = optim_hyper(a);
    GroupTable table{};
    if (g) table = group_table(*g);
    const GroupTable* t = g ? &table : nullptr;
    const EmaArgs ea{e->ema, e->decay, (float)(1.0 - e->decay), e->warmup ? 1 : 0};
    switch (kind) {
        case K_ADAM: EGK_DISPATCH_T(a.g_dtype, (optim_ema_launch<K_ADAM, T>(s, grid, a, h, t, ea))); break;
        case K_ADAMW: EGK_DISPATCH_T(a.g_dtype, (optim_ema_launch<K_ADAMW, T>(s, grid, a, h, t, ea))); break;
        case K_SGD: EGK_DISPATCH_T(a.g_dtype, (optim_ema_launch<K_SGD, T>(s, grid, a, h, t, ea))); break;
        default: EGK_DISPATCH_T(a.g_dtype, (optim_ema_launch<K_SGD_MOMENTUM, T>(s, grid, a, h, t, ea))); break;
    }
    return check_launch("egk_optim_step_ema");
}

extern "C" int egk_ema_swap(egk_stream_t stream, float* p, float* ema, int64_t n) {
    EGK_REQUIRE(p && ema, "egk_ema_swap: null pointer");
    EGK_REQUIRE((((uintptr_t)p | (uintptr_t)ema) & 15) == 0, "egk_ema_swap: buffers must be 16-byte aligned");
    EGK_REQUIRE(n >= 0, "egk_ema_swap: n >= 0 (got %lld)", (long long)n);
    if (n == 0) return 0;
    hipStream_t s = (hipStream_t)stream;
    ProfScope prof(KID_EMA_SWAP, s, 0, 16.0 * (double)n);
    hipLaunchKernelGGL(ema_swap_kernel, dim3(optim_grid(n)), dim3(256), 0, s, p, ema, (long long)n);
    return check_launch("egk_ema_swap");
}
