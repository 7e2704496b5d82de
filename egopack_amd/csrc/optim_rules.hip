// The update rules of the flat-buffer optimizer: Adam, AdamW and SGD, the single-tensor formulas of torch 2.10, behind every
// optimizer entry point of the ABI (egk_adam_step*, include/egopack_hip.h; egk_optim_step, include/egopack_optim.h; the segment
// table of include/egopack_optim_groups.h; the moving average of include/egopack_ema.h).  ONE body (optim_body) and one kernel
// family over it: 16-byte accesses on p, g and the state, a scalar tail for n % 4, the bf16 copy and the low half of the stored p,
// the offset word moved on by workgroup 0, one wave-uniform load of the gate.  No atomics; every element has one writer.
// ONE dispatcher (optim_dispatch) behind the entry points: the refusals, the grid, the bytes and the launch line.
#include "common.h"
#include "optim_stream.h"  // ema_update, ema_weight, the NT_* cache policy and its loads and stores

namespace egk {

// ---- Adam on one element (torch.optim.Adam single-tensor formulas, L2 weight decay) -------------------------------------------------
struct AdamConsts {
    float step, bc2s, gs, b1, b2, eps, wd;  // step = lr / (1 - b1^t), bc2s = sqrt(1 - b2^t), gs = gradient scale
};
__device__ __forceinline__ void adam_update(float& p, float g, float& m, float& v, const AdamConsts& c) {
#pragma clang fp contract(off)  // (no fused multiply-adds: which products the compiler fuses depends on the code around the inlined body)
    const float gg = g * c.gs + c.wd * p;
    m = m + (gg - m) * (1.f - c.b1);          // exp_avg.lerp_(grad, 1 - beta1)
    v = v * c.b2 + (1.f - c.b2) * gg * gg;    // mul_(beta2).addcmul_(g, g, 1 - beta2)
    const float denom = sqrtf(v) / c.bc2s + c.eps;
    p = p - c.step * (m / denom);
}

// what a kernel of the family does per element; the rule codes of the ABI map onto these (SGD: by its momentum)
enum { K_ADAM = 0, K_ADAMW, K_SGD, K_SGD_MOMENTUM };
template <int KIND> struct StateCount { static constexpr int value = KIND == K_SGD ? 0 : KIND == K_SGD_MOMENTUM ? 1 : 2; };

struct OptimConsts {
    AdamConsts adam;    // (K_ADAM: adam_update itself; K_ADAMW: its step, bc2s, gs, b2, eps; wd through ``decay``)
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

// ---- the state's element type (include/egopack_optim.h: state_dtype) ------------------------------------------------------------------
// ST = float: the 16-byte loads and stores the family has always issued.  ST = bf16_t: one 8-byte access per buffer and quad, the
// elements widened to f32 on the way in and rounded on the way out -- to nearest (f2bf), or by adding 16 random bits under the bits
// that are dropped.  The body between the load and the store never sees which: it computes on f32 and uses the unrounded result.
struct StateRound {      // wave-uniform: the launch's mode and what its Philox counters start from
    int stochastic;      // state_round
    uint64_t seed;       // state_seed, the key
    uint64_t ctr_hi;     // (t & 0xFFFFFF) << 40, t = *t_dev, read once per workgroup
    long long elem0;     // the absolute index of element 0 of the launch, a multiple of 4
};

// the four words of the 16-byte group that holds absolute element e = elem0 + i (i a multiple of 4): word k serves element e + k,
// its high half state0, its low half state1
__device__ __forceinline__ uint4 state_words(const StateRound& r, long long i) {
    return philox4x32_10(r.ctr_hi | ((uint64_t)(r.elem0 + i) >> 2), r.seed);
}

// one f32 value to the bf16 bits that are stored; r16: 16 random bits, used when ``stochastic``
__device__ __forceinline__ bf16_t round_state(float x, unsigned r16, bool stochastic) {
    const unsigned b = __float_as_uint(x);
    if (!stochastic || (b & 0x7f800000u) == 0x7f800000u) return f2bf(x);  // (inf / NaN keep f2bf's bits)
    return (bf16_t)((b + r16) >> 16);  // (no carry into the sign: the exponent is not all ones)
}

__device__ __forceinline__ float4 ld_state4(const float* __restrict__ s, bool nt) { return ld_quad(s, nt); }
__device__ __forceinline__ float4 ld_state4(const bf16_t* __restrict__ s, bool nt) { return ld_quad(s, nt); }
// ``high``: this buffer draws the high halves of the words (state0), otherwise the low halves (state1)
__device__ __forceinline__ void st_state4(float* __restrict__ s, const float4& v, const uint4&, bool, bool, bool nt) { st_quad(s, v, nt); }
__device__ __forceinline__ void st_state4(bf16_t* __restrict__ s, const float4& v, const uint4& w, bool high, bool stochastic, bool nt) {
    const unsigned sh = high ? 16u : 0u;
    uint2 pk;
    pk.x = (unsigned)round_state(v.x, (w.x >> sh) & 0xffffu, stochastic) | ((unsigned)round_state(v.y, (w.y >> sh) & 0xffffu, stochastic) << 16);
    pk.y = (unsigned)round_state(v.z, (w.z >> sh) & 0xffffu, stochastic) | ((unsigned)round_state(v.w, (w.w >> sh) & 0xffffu, stochastic) << 16);
    if (nt) {
        const nt_u2 q = {pk.x, pk.y};
        __builtin_nontemporal_store(q, reinterpret_cast<nt_u2*>(s));
        return;
    }
    *reinterpret_cast<uint2*>(s) = pk;
}

// the four elements [i, i + 4) of a span in 16-byte accesses (8-byte on a bf16 state); ``consts()`` is asked for the constants, and
// the Philox call of a stochastic store issued, once the loads are on their way.
// EMA: ``ema`` follows the new p with weight ``w`` before p is stored (read with the other loads, one 16-byte store).
// NT: the launch's cache policy, an NT_* mask (0: the default policy on every stream, the accesses the family has always issued).
template <int KIND, typename GT, typename ST, bool EMA = false, int NT = 0, typename CF>
__device__ __forceinline__ void optim_quad(float* __restrict__ p, const GT* __restrict__ g, ST* __restrict__ s0, ST* __restrict__ s1,
                                           long long i, CF consts, const StateRound& sr, bf16_t* __restrict__ shadow,
                                           bf16_t* __restrict__ shadow_lo, float* __restrict__ ema = nullptr, float w = 0.f) {
    constexpr int NS = StateCount<KIND>::value;
    constexpr bool NARROW = !__is_same(ST, float);
    constexpr bool nt_ld = NT & NT_LOAD, nt_st = NT & NT_STORE, nt_ema = NT & NT_EMA;
    float4 pv = ld_quad(p + i, nt_ld);
    const float4 gv = ld_quad(g + i, NT & NT_G);
    float4 av = make_float4(0.f, 0.f, 0.f, 0.f), bv = av, ev = av;
    if constexpr (NS >= 1) av = ld_state4(s0 + i, nt_ld);
    if constexpr (NS >= 2) bv = ld_state4(s1 + i, nt_ld);
    if constexpr (EMA) ev = ld_quad(ema + i, nt_ema);
    const OptimConsts c = consts();
    uint4 rw = make_uint4(0u, 0u, 0u, 0u);
    if constexpr (NARROW && NS >= 1)
        if (sr.stochastic) rw = state_words(sr, i);
    float* pp = &pv.x; const float* gp = &gv.x; float* ap = &av.x; float* bp = &bv.x;
#pragma unroll
    for (int t = 0; t < 4; ++t) optim_update<KIND>(pp[t], gp[t], ap[t], bp[t], c);
    if constexpr (EMA) {
        float* ep = &ev.x;
#pragma unroll
        for (int t = 0; t < 4; ++t) ema_update(ep[t], pp[t], w);
        st_quad(ema + i, ev, nt_ema);
    }
    st_quad(p + i, pv, nt_st);
    if constexpr (NS >= 1) st_state4(s0 + i, av, rw, true, sr.stochastic != 0, nt_st);
    if constexpr (NS >= 2) st_state4(s1 + i, bv, rw, false, sr.stochastic != 0, nt_st);
    if (shadow) st4t(shadow + i, 0, 4, true, pv);
    if (shadow_lo) {  // bf16(p - bf16(p)): egk_split_bf16's bits
        const float lo4[4] = {pp[0] - bf2f(f2bf(pp[0])), pp[1] - bf2f(f2bf(pp[1])), pp[2] - bf2f(f2bf(pp[2])), pp[3] - bf2f(f2bf(pp[3]))};
        st4t(shadow_lo + i, 0, 4, true, make_float4(lo4[0], lo4[1], lo4[2], lo4[3]));
    }
}

// the scalar tail [i, n) of a span (n - i < 4)
template <int KIND, typename GT, typename ST, bool EMA = false, int NT = 0>
__device__ __forceinline__ void optim_tail(float* __restrict__ p, const GT* __restrict__ g, ST* __restrict__ s0, ST* __restrict__ s1,
                                           long long i, long long n, const OptimConsts& c, const StateRound& sr,
                                           bf16_t* __restrict__ shadow, bf16_t* __restrict__ shadow_lo,
                                           float* __restrict__ ema = nullptr, float w = 0.f) {
    constexpr int NS = StateCount<KIND>::value;
    constexpr bool NARROW = !__is_same(ST, float);
    constexpr bool nt_ld = NT & NT_LOAD, nt_st = NT & NT_STORE, nt_ema = NT & NT_EMA;
    uint4 q = make_uint4(0u, 0u, 0u, 0u);  // (the tail's group starts at i, a multiple of 4: one call, word j - i for element j)
    if constexpr (NARROW && NS >= 1)
        if (sr.stochastic) q = state_words(sr, i);
    for (long long j = i; j < n; ++j) {
        const unsigned rw = j == i ? q.x : j == i + 1 ? q.y : q.z;
        (void)rw;
        float a = 0.f, b = 0.f;
        if constexpr (NS >= 1) a = ld_one_f(s0 + j, nt_ld);
        if constexpr (NS >= 2) b = ld_one_f(s1 + j, nt_ld);
        float pj = ld_one(p + j, nt_ld);
        optim_update<KIND>(pj, ld_one_f(g + j, NT & NT_G), a, b, c);
        if constexpr (EMA) {
            float e = ld_one(ema + j, nt_ema);
            ema_update(e, pj, w);
            st_one(ema + j, e, nt_ema);
        }
        st_one(p + j, pj, nt_st);
        if constexpr (NARROW) {
            if constexpr (NS >= 1) st_one(s0 + j, round_state(a, rw >> 16, sr.stochastic != 0), nt_st);
            if constexpr (NS >= 2) st_one(s1 + j, round_state(b, rw & 0xffffu, sr.stochastic != 0), nt_st);
        } else {
            if constexpr (NS >= 1) st_one(s0 + j, a, nt_st);
            if constexpr (NS >= 2) st_one(s1 + j, b, nt_st);
        }
        if (shadow) shadow[j] = f2bf(pj);
        if (shadow_lo) shadow_lo[j] = f2bf(pj - bf2f(f2bf(pj)));
    }
}

struct OptimHyper {  // the host's scalars of a launch
    float b1, b2, omb1, omb2, eps, wd, mu, damp1;
    int nesterov;
};

// the constants of a launch from its learning rate and weight decay (of the launch, or of a group: group_consts)
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

// The constants of the group that holds element i of the 1024-element block at b0.  The lookup: ONE search per workgroup and
// 1024-element block for the segment of the block's first element -- workgroup-uniform, so it runs on the scalar unit while the
// block's vector loads are in flight -- and one comparison that tells whether the block ends inside that segment.  Only the lanes of
// a block that straddles a boundary search for themselves, over the at most 256 segments a block can touch.  A 16-byte group of
// elements never straddles (boundaries and base are multiples of 4), so the scalar tail shares the segment of its first element.
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

// ---- the one body and the kernels over it --------------------------------------------------------------------------------------------
struct OptimArgs {  // what a launch of the family is handed; ``t`` without a table and ``e`` without an average stay empty
    float* p;
    const void* g;  // f32, or bf16 after a compressed all-reduce (the kernel's GT)
    void* s0;       // f32, or bf16 with state_dtype == EGK_BF16 (the kernel's ST)
    void* s1;
    long long n;
    const float* hyper;
    const long long* t_dev;
    bf16_t* shadow;
    bf16_t* shadow_lo;
    long long* bump_word;
    long long bump;
    const int* gate;
    OptimHyper h;
    GroupTable t;
    EmaArgs e;
    int st_round;             // bf16 state: state_round, state_seed, elem0 of the descriptor
    unsigned long long st_seed;
    long long elem0;
};

// One launch over [0, n): workgroup b takes the 1024-element blocks b, b + gridDim.x, ... (256 threads x 4 elements).  The constants
// come from the launch's lr and weight decay, formed once, or with GROUPED from the block's group (group_consts).
// The buffers the launch writes arrive as __restrict__ PARAMETERS (optim_body unpacks them): a qualifier on a struct member tells
// the compiler nothing, and without it every store may change hyper, the gate and the segment table, whose workgroup-uniform loads
// then leave the scalar unit (the grouped kernel: 20 vector loads instead of 14).
template <int KIND, typename GT, typename ST, bool GROUPED, bool EMA, int NT>
__device__ __forceinline__ void optim_walk(float* __restrict__ p, const GT* __restrict__ g, ST* __restrict__ s0, ST* __restrict__ s1,
                                           bf16_t* __restrict__ shadow, bf16_t* __restrict__ shadow_lo, float* __restrict__ ema,
                                           long long* __restrict__ bump_word, const OptimArgs& a) {
    // (a device-side counter that moves on once per step -- the Philox offset word of the step's dropout launches -- rides in this
    //  launch instead of costing one of its own, whether the step happens or not)
    if (bump_word && blockIdx.x == 0 && threadIdx.x == 0) *bump_word += a.bump;
    // (the step's gate word, written by egk_grad_norm_finalize -- 0 = the gradient norm was not finite, the step is skipped: one
    //  wave-uniform load, nothing of p / the state / the average / the bf16 copies is touched)
    if (a.gate && *a.gate == 0) return;
    const float w = EMA ? ema_weight(a.e, a.t_dev) : 0.f;
    // (the counted step of a stochastic store: one wave-uniform load per workgroup, like the gate; the f32 state never asks)
    StateRound sr{0, 0, 0, 0};
    if constexpr (!__is_same(ST, float))
        if (a.st_round) sr = StateRound{1, a.st_seed, ((uint64_t)*a.t_dev & 0xFFFFFFull) << 40, a.elem0};
    OptimConsts launch{};
    if constexpr (!GROUPED) launch = optim_consts<KIND>(a.hyper[0], a.h.wd, a.hyper, a.t_dev, a.h);
    for (long long b0 = (long long)blockIdx.x * 1024; b0 < a.n; b0 += (long long)gridDim.x * 1024) {
        const long long i = b0 + (long long)threadIdx.x * 4;
        if (i >= a.n) continue;
        auto consts = [&]() -> OptimConsts {
            if constexpr (GROUPED) return group_consts<KIND>(a.t, b0, i, a.n, a.hyper, a.t_dev, a.h);
            else return launch;
        };
        if (i + 4 <= a.n)
            optim_quad<KIND, GT, ST, EMA, NT>(p, g, s0, s1, i, consts, sr, shadow, shadow_lo, ema, w);
        else
            optim_tail<KIND, GT, ST, EMA, NT>(p, g, s0, s1, i, a.n, consts(), sr, shadow, shadow_lo, ema, w);
    }
}

template <int KIND, typename GT, typename ST, bool GROUPED, bool EMA, int NT>
__device__ __forceinline__ void optim_body(const OptimArgs& a) {
    optim_walk<KIND, GT, ST, GROUPED, EMA, NT>(a.p, static_cast<const GT*>(a.g), static_cast<ST*>(a.s0), static_cast<ST*>(a.s1), a.shadow,
                                               a.shadow_lo, a.e.ema, a.bump_word, a);
}

template <int KIND, typename GT, bool GROUPED, bool EMA, int NT = 0>
__global__ __launch_bounds__(256) void optim_kernel(const OptimArgs a) {
    optim_body<KIND, GT, float, GROUPED, EMA, NT>(a);
}

// The same body on a bf16 state.  Left alone the compiler keeps the ten round keys of the Philox call and the counter's uniform half
// in scalar registers for the whole walk and ends at the scalar file's cap (106), which admits 7 waves per SIMD where the f32-state
// kernels run 8; told to aim for 8 it keeps what does not fit in lanes of a vector register instead.
template <int KIND, typename GT, bool GROUPED, bool EMA, int NT = 0>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(8))) void optim_kernel_bf16_state(const OptimArgs a) {
    optim_body<KIND, GT, bf16_t, GROUPED, EMA, NT>(a);
}

// what egk_adam_step* launch: the body for Adam under the name the profiles, bench.py and the timeline tools know the step's
// optimizer launch by
template <typename GT, int NT = 0>
__global__ __launch_bounds__(256) void adam_kernel(const OptimArgs a) {
    optim_body<K_ADAM, GT, float, false, false, NT>(a);
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

// what every entry point refuses, before any launch; ``a``: the descriptor without the state the rule does not have, ``kind``: its kernel
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
    const bool narrow = a.state_dtype == EGK_BF16;  // (a bf16 state is accessed 8 bytes at a time: its own refusal, below)
    const uintptr_t state_ptrs = narrow ? 0 : (uintptr_t)a.state0 | (uintptr_t)a.state1;
    EGK_REQUIRE((((uintptr_t)a.p | (uintptr_t)a.g | state_ptrs) & 15) == 0, "%s: buffers must be 16-byte aligned", who);
    EGK_REQUIRE(((uintptr_t)a.bf16_shadow & 7) == 0, "%s: shadow must be 8-byte aligned", who);
    EGK_REQUIRE(((uintptr_t)a.bf16_lo_shadow & 7) == 0, "%s: low-half shadow must be 8-byte aligned", who);
    return 0;
}

// what every entry point refuses in the four state fields at the descriptor's end, behind everything else it refuses (a zeroed
// tail passes: the f32 launch)
static int state_check(const char* who, const egk_optim_desc& a) {
    EGK_REQUIRE(a.state_dtype == EGK_F32 || a.state_dtype == EGK_BF16, "%s: unknown state dtype %d (EGK_F32 = 0, EGK_BF16 = 1)", who,
                (int)a.state_dtype);
    EGK_REQUIRE(a.state_round == 0 || a.state_round == 1, "%s: state_round in {0 (nearest), 1 (stochastic)} (got %d)", who, (int)a.state_round);
    EGK_REQUIRE(!a.state_round || a.state_dtype == EGK_BF16, "%s: stochastic rounding (state_round = 1) needs a bf16 state (state_dtype = EGK_BF16)", who);
    EGK_REQUIRE(!a.state_round || a.t_dev,"%s: stochastic rounding (state_round = 1) needs t_dev (the device step counter)", who);
    EGK_REQUIRE(a.elem0 >= 0 && a.elem0 % 4 == 0 && a.elem0 <= (1ll << 42) - a.n,
                "%s: elem0 must be a non-negative multiple of 4 with elem0 + n <= 2^42 (got %lld)", who, (long long)a.elem0);
    if (a.state_dtype == EGK_BF16)
        EGK_REQUIRE((((uintptr_t)a.state0 | (uintptr_t)a.state1) & 7) == 0, "%s: bf16 state must be 8-byte aligned", who);
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

// what the entry point with the average refuses in its descriptor
static int ema_check(const char* who, const egk_ema_desc* e, const egk_optim_desc& a) {
    EGK_REQUIRE(e, "%s: null ema descriptor", who);
    EGK_REQUIRE(e->ema, "%s: null ema pointer", who);
    EGK_REQUIRE(((uintptr_t)e->ema & 15) == 0, "%s: ema must be 16-byte aligned", who);
    EGK_REQUIRE(e->decay >= 0.0 && e->decay < 1.0, "%s: decay in [0, 1) (got %g)", who, e->decay);
    EGK_REQUIRE(!e->warmup || a.t_dev, "%s: warmup needs t_dev (the device step counter)", who);
    return 0;
}

// bytes per parameter: p read + written, each state buffer read + written (4 B an access, 2 B on a bf16 state), the gradient read,
// the bf16 copies written, the average read + written
static double optim_bytes(const egk_optim_desc& a, int kind, bool ema) {
    const double state_bytes = (kind == K_SGD ? 0.0 : kind == K_SGD_MOMENTUM ? 8.0 : 16.0) * (a.state_dtype == EGK_BF16 ? 0.5 : 1.0);
    return (8.0 + state_bytes + (a.g_dtype == EGK_BF16 ? 2.0 : 4.0) + (a.bf16_shadow ? 2.0 : 0.0) + (a.bf16_lo_shadow ? 2.0 : 0.0) +
            (ema ? 8.0 : 0.0)) * (double)a.n;
}

// Workgroups: one 1024-element group per workgroup up to 32768 of them (egk_tune(6, n) sets the cap: the tests lower it so that a
// small launch walks several laps).  An optimizer slice runs
// BESIDE weight-gradient launches in every captured step's tail; round 5 first capped it at 4096 (a 8 us reduction queued beside
// it had waited 135 us for wave slots) and, once the gradient buffer was no longer cleared and read back, measured the wide grid
// ahead again: headline 1.365-1.379 against 1.374-1.386 ms, config 4 2.180-2.182 against 2.191-2.206, Hp = 4096 2.722 against
// 2.751 (narrower is clearly worse: 1024 workgroups 1.405-1.414, 512 1.447)
int g_optim_grid_cap = 32768;  // egk_tune 6 (norm_ops.hip)
static unsigned optim_grid(long long n) {
    const long long want = (n / 4 + 255) / 256;
    const long long cap = g_optim_grid_cap;
    return (unsigned)(want < 1 ? 1 : want > cap ? cap : want);
}

// the kernel of a launch: adam_kernel for egk_adam_step* (KID_ADAM), otherwise the member of the family
template <int KIND, typename GT, typename ST, int NT>
static auto optim_pick(int kid, bool grouped, bool ema) -> void (*)(OptimArgs) {
    if constexpr (__is_same(ST, float)) {
        if (kid == KID_ADAM) return adam_kernel<GT, NT>;
        if (grouped) return ema ? optim_kernel<KIND, GT, true, true, NT> : optim_kernel<KIND, GT, true, false, NT>;
        return ema ? optim_kernel<KIND, GT, false, true, NT> : optim_kernel<KIND, GT, false, false, NT>;
    } else {
        if (grouped) return ema ? optim_kernel_bf16_state<KIND, GT, true, true, NT> : optim_kernel_bf16_state<KIND, GT, true, false, NT>;
        return ema ? optim_kernel_bf16_state<KIND, GT, false, true, NT> : optim_kernel_bf16_state<KIND, GT, false, false, NT>;
    }
}
// ... by the state's element type too (K_SGD has no state: its one instantiation serves either)
template <int KIND, typename GT, int NT>
static auto optim_pick(int kid, bool grouped, bool ema, bool narrow) -> void (*)(OptimArgs) {
    if constexpr (StateCount<KIND>::value > 0)
        if (narrow) return optim_pick<KIND, GT, bf16_t, NT>(kid, grouped, ema);
    return optim_pick<KIND, GT, float, NT>(kid, grouped, ema);
}
// ... and by the cache policy of the launch's streams (egk_tune 9): the masks that are instantiated
// Default: the three stores and every load non-temporal, the average left alone (NT_G | NT_LOAD | NT_STORE).  Same box, alternating
// runs of the headline step: masks 0 / 1 / 3 within noise of each other, 7 ahead in every round (HISTORY.md section 21).
int g_optim_stream_policy = NT_G | NT_LOAD | NT_STORE;
bool optim_stream_policy_ok(int mask) { return mask == 0 || mask == 1 || mask == 2 || mask == 3 || mask == 4 || mask == 7 || mask == 8 || mask == 15; }
template <int KIND, typename GT>
static auto optim_pick(int kid, bool grouped, bool ema, bool narrow) -> void (*)(OptimArgs) {
    switch (g_optim_stream_policy) {
        case 1: return optim_pick<KIND, GT, 1>(kid, grouped, ema, narrow);
        case 2: return optim_pick<KIND, GT, 2>(kid, grouped, ema, narrow);
        case 3: return optim_pick<KIND, GT, 3>(kid, grouped, ema, narrow);
        case 4: return optim_pick<KIND, GT, 4>(kid, grouped, ema, narrow);
        case 7: return optim_pick<KIND, GT, 7>(kid, grouped, ema, narrow);
        case 8: return optim_pick<KIND, GT, 8>(kid, grouped, ema, narrow);
        case 15: return optim_pick<KIND, GT, 15>(kid, grouped, ema, narrow);
        default: return optim_pick<KIND, GT, 0>(kid, grouped, ema, narrow);
    }
}

// Every optimizer entry point: the refusals, then one launch.  ``who``: the name the messages carry; ``kid``: the entry point's
// profile id -- KID_OPTIM_GROUPS requires the table ``g``, KID_OPTIM_EMA the average ``e`` (and takes a table or none).
static int optim_dispatch(const char* who, int kid, egk_stream_t stream, const egk_optim_desc* d, const egk_optim_groups* g,
                          const egk_ema_desc* e) {
    egk_optim_desc a;
    int kind = 0;
    if (const int rc = optim_check(who, d, a, kind)) return rc;
    if (g || kid == KID_OPTIM_GROUPS)
        if (const int rc = groups_check(who, g)) return rc;
    if (kid == KID_OPTIM_EMA)
        if (const int rc = ema_check(who, e, a)) return rc;
    if (const int rc = state_check(who, a)) return rc;
    if (a.n == 0) return 0;
    hipStream_t s = (hipStream_t)stream;
    ProfScope prof(kid, s, 0, optim_bytes(a, kind, e != nullptr));
    OptimArgs k{a.p, a.g, a.state0, a.state1, (long long)a.n, a.hyper, (const long long*)a.t_dev, (bf16_t*)a.bf16_shadow,
                (bf16_t*)a.bf16_lo_shadow, (long long*)a.bump_word, (long long)a.bump, (const int*)a.gate,
                OptimHyper{(float)a.beta1, (float)a.beta2, (float)(1.0 - a.beta1), (float)(1.0 - a.beta2), a.eps, a.weight_decay,
                           a.momentum, (float)(1.0 - (double)a.dampening), a.nesterov ? 1 : 0},
                GroupTable{}, EmaArgs{}, (int)a.state_round, (unsigned long long)a.state_seed, (long long)a.elem0};
    if (g) k.t = GroupTable{(long long)g->base, (int)g->n_seg, (int)g->n_groups, (const long long*)g->seg_begin, (const int*)g->seg_group, g->group_hyper};
    if (e) k.e = EmaArgs{e->ema, e->decay, (float)(1.0 - e->decay), e->warmup ? 1 : 0};
    void (*kernel)(OptimArgs) = nullptr;
    const bool narrow = a.state_dtype == EGK_BF16;
    switch (kind) {
        case K_ADAM: EGK_DISPATCH_T(a.g_dtype, (kernel = optim_pick<K_ADAM, T>(kid, g, e, narrow))); break;
        case K_ADAMW: EGK_DISPATCH_T(a.g_dtype, (kernel = optim_pick<K_ADAMW, T>(kid, g, e, narrow))); break;
        case K_SGD: EGK_DISPATCH_T(a.g_dtype, (kernel = optim_pick<K_SGD, T>(kid, g, e, narrow))); break;
        default: EGK_DISPATCH_T(a.g_dtype, (kernel = optim_pick<K_SGD_MOMENTUM, T>(kid, g, e, narrow))); break;
    }
    hipLaunchKernelGGL(kernel, dim3(optim_grid(a.n)), dim3(256), 0, s, k);
    return check_launch(who);
}

}  // namespace egk

using namespace egk;

extern "C" int egk_optim_step(egk_stream_t stream, const egk_optim_desc* d) {
    return optim_dispatch("egk_optim_step", KID_OPTIM, stream, d, nullptr, nullptr);
}

extern "C" int egk_optim_step_groups(egk_stream_t stream, const egk_optim_desc* d, const egk_optim_groups* g) {
    return optim_dispatch("egk_optim_step_groups", KID_OPTIM_GROUPS, stream, d, g, nullptr);
}

extern "C" int egk_optim_step_ema(egk_stream_t stream, const egk_optim_desc* d, const egk_optim_groups* g, const egk_ema_desc* e) {
    return optim_dispatch("egk_optim_step_ema", KID_OPTIM_EMA, stream, d, g, e);
}

// egk_adam_step*: EGK_OPT_ADAM from scalar arguments, under its own profile id and kernel name
extern "C" int egk_adam_step_gated(egk_stream_t stream, float* p, const void* g, int32_t g_dtype, float* m, float* v, int64_t n,
                                   const float* hyper, float beta1, float beta2, float eps, float weight_decay, void* bf16_shadow,
                                   void* bf16_lo_shadow, int64_t* bump_word, int64_t bump, const int32_t* gate) {
    egk_optim_desc d{};
    d.rule = EGK_OPT_ADAM, d.g_dtype = g_dtype, d.n = n;
    d.p = p, d.g = g, d.state0 = m, d.state1 = v, d.hyper = hyper;
    d.beta1 = beta1, d.beta2 = beta2, d.eps = eps, d.weight_decay = weight_decay;
    d.bf16_shadow = bf16_shadow, d.bf16_lo_shadow = bf16_lo_shadow, d.bump_word = bump_word, d.bump = bump, d.gate = gate;
    return optim_dispatch("egk_adam_step", KID_ADAM, stream, &d, nullptr, nullptr);
}

extern "C" int egk_adam_step_bump(egk_stream_t stream, float* p, const void* g, int32_t g_dtype, float* m, float* v, int64_t n,
                                  const float* hyper, float beta1, float beta2, float eps, float weight_decay, void* bf16_shadow,
                                  void* bf16_lo_shadow, int64_t* bump_word, int64_t bump) {
    return egk_adam_step_gated(stream, p, g, g_dtype, m, v, n, hyper, beta1, beta2, eps, weight_decay, bf16_shadow, bf16_lo_shadow,
                               bump_word, bump, nullptr);
}

extern "C" int egk_adam_step(egk_stream_t stream, float* p, const void* g, int32_t g_dtype, float* m, float* v, int64_t n,
                             const float* hyper, float beta1, float beta2, float eps, float weight_decay, void* bf16_shadow) {
    return egk_adam_step_bump(stream, p, g, g_dtype, m, v, n, hyper, beta1, beta2, eps, weight_decay, bf16_shadow, nullptr, nullptr, 0);
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
