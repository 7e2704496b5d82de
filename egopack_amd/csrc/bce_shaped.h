// The shaped BCE-with-logits of include/egopack_bce_balanced.h for ONE node: a class factor (pos for y != 0, neg otherwise) and a
// focal exponent gamma.  Written once for the three kernels that use it (bce_fwd_kernel / bce_bwd_kernel<SHAPED> in loss.hip,
// rowdot_bce_kernel<SHAPED> in norm_ops.hip).  The three scalars are kernel arguments: ``gamma == 0`` is a wave-uniform branch
// whose arithmetic is the plain instantiations' times the class factor, so pos = neg = 1 gives their bits.
#pragma once

#include <math.h>

#include <hip/hip_runtime.h>

namespace egk {

struct BceShape {
    float pos, neg, gamma;
};

__device__ __forceinline__ float bce_softplus(float x) { return fmaxf(x, 0.f) + log1pf(expf(-fabsf(x))); }

// loss of a node with logit z and label y
__device__ __forceinline__ float bce_shaped_loss(float z, long long y, const BceShape sh) {
#pragma clang fp contract(off)  // (no fusing that depends on the code around: every kernel forms the same f32 value)
    const float t = (float)y;
    const float c = y != 0 ? sh.pos : sh.neg;
    if (sh.gamma == 0.f) return c * ((1.f - t) * z + fmaxf(-z, 0.f) + log1pf(expf(-fabsf(z))));
    const float u = (2.f * t - 1.f) * z;
    const float ce = bce_softplus(-u);                   // -log p_t
    const float mod = expf(-sh.gamma * bce_softplus(u));  // (1 - p_t) ** gamma
    return c * mod * ce;
}

// d loss / d z times the upstream gradient g, evaluated left to right
__device__ __forceinline__ float bce_shaped_grad(float z, long long y, float g, const BceShape sh) {
#pragma clang fp contract(off)
    const float t = (float)y;
    const float c = y != 0 ? sh.pos : sh.neg;
    if (sh.gamma == 0.f) return (c * (1.f / (1.f + expf(-z)) - t)) * g;
    const float s = 2.f * t - 1.f;
    const float u = s * z;
    const float ce = bce_softplus(-u);
    const float mod = expf(-sh.gamma * bce_softplus(u));
    const float pt = 1.f / (1.f + expf(-u));
    return (s * c * mod * (sh.gamma * pt * (-ce) - (1.f - pt))) * g;
}

// what the entry points refuse on the host: a negative or non-finite scalar
inline bool bce_shape_ok(float pos, float neg, float gamma) {
    return isfinite(pos) && isfinite(neg) && isfinite(gamma) && pos >= 0.f && neg >= 0.f && gamma >= 0.f;
}

}  // namespace egk
