// What the optimizer launches of optim_rules.hip and optim_lamb.hip share: the cache policy of their single-use streams and the
// moving average of the weights.  One definition each, so that a launch of either file stores the same bits.
#pragma once
#include "common.h"

namespace egk {

// the moving average of the weights (include/egopack_ema.h): e += w * (p_new - e), three separately rounded f32 operations
__device__ __forceinline__ void ema_update(float& e, float p_new, float w) {
#pragma clang fp contract(off)
    const float diff = p_new - e;
    const float move = w * diff;
    e = e + move;
}

// ---- cache policy of the single-use streams (egk_tune 9) ---------------------------------------------------------------------------
// A launch reads g, p and the state and writes p and the state once per step; nothing reads those lines again before the next
// step's launch, while the bf16 copies it writes are the next step's contraction operands.  A mask, the kernels' template argument NT,
// marks accesses as non-temporal, per stream; the copies always keep the default policy.  The policy changes no arithmetic.
enum { NT_G = 1, NT_LOAD = 2, NT_STORE = 4, NT_EMA = 8 };  // loads of g | loads of p and the state | their stores | the average, both ways
typedef float nt_f4 __attribute__((ext_vector_type(4)));
typedef unsigned nt_u2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ float4 ld_quad(const float* __restrict__ p, bool nt) {
    if (nt) {
        const nt_f4 v = __builtin_nontemporal_load(reinterpret_cast<const nt_f4*>(p));
        return make_float4(v.x, v.y, v.z, v.w);
    }
    return *reinterpret_cast<const float4*>(p);
}
__device__ __forceinline__ float4 ld_quad(const bf16_t* __restrict__ p, bool nt) {
    if (nt) {
        const nt_u2 r = __builtin_nontemporal_load(reinterpret_cast<const nt_u2*>(p));
        return make_float4(__uint_as_float(r.x << 16), __uint_as_float(r.x & 0xffff0000u), __uint_as_float(r.y << 16),
                           __uint_as_float(r.y & 0xffff0000u));
    }
    return ld4t(p, 0, 4, true);
}
__device__ __forceinline__ void st_quad(float* __restrict__ p, const float4& v, bool nt) {
    if (nt) {
        const nt_f4 w = {v.x, v.y, v.z, v.w};
        __builtin_nontemporal_store(w, reinterpret_cast<nt_f4*>(p));
        return;
    }
    *reinterpret_cast<float4*>(p) = v;
}
template <typename T> __device__ __forceinline__ T ld_one(const T* p, bool nt) { return nt ? __builtin_nontemporal_load(p) : *p; }
template <typename T> __device__ __forceinline__ void st_one(T* p, T v, bool nt) {
    if (nt) __builtin_nontemporal_store(v, p);
    else *p = v;
}
__device__ __forceinline__ float ld_one_f(const float* p, bool nt) { return ld_one(p, nt); }
__device__ __forceinline__ float ld_one_f(const bf16_t* p, bool nt) { return bf2f(ld_one(p, nt)); }

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

}  // namespace egk
