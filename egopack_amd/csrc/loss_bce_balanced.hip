// Shaped BCE-with-logits (include/egopack_bce_balanced.h): loss_optim.hip's bce_fwd_kernel / bce_bwd_kernel with a class factor
// and a focal exponent applied inside them (bce_shaped.h).  One thread per node, the grids and the access pattern of the plain
// kernels, which this unit leaves alone: a caller that passes no scalar never comes here.  The one-pass form (egk_rowdot_bce_w)
// sits beside rowdot_bce_kernel in norm_ops.hip, whose row helpers it shares.
#include "bce_shaped.h"
#include "common.h"

namespace egk {

namespace {

__global__ __launch_bounds__(256) void bce_w_fwd_kernel(const float* __restrict__ x, const long long* __restrict__ y,
                                                        float* __restrict__ loss, int n, const BceShape sh) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    loss[i] = bce_shaped_loss(x[i], y[i], sh);
}

template <typename T>
__global__ __launch_bounds__(256) void bce_w_bwd_kernel(const float* __restrict__ x, const long long* __restrict__ y,
                                                        const float* __restrict__ gloss, T* __restrict__ dx, int n, const BceShape sh) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    st1t(dx + i, bce_shaped_grad(x[i], y[i], gloss[i], sh));
}

}  // namespace

}  // namespace egk

using namespace egk;

extern "C" {

int egk_bce_w_fwd(egk_stream_t stream, const float* logits, const int64_t* y, float* loss, int32_t n, float pos, float neg,
                  float gamma) {
    EGK_REQUIRE(logits && y && loss, "egk_bce_w_fwd: null pointer");
    EGK_REQUIRE(n >= 0, "egk_bce_w_fwd: n must be >= 0");
    EGK_REQUIRE(bce_shape_ok(pos, neg, gamma), "egk_bce_w_fwd: pos, neg and gamma must be finite and >= 0 (got %g, %g, %g)", (double)pos,
                (double)neg, (double)gamma);
    if (n == 0) return 0;
    hipStream_t s = (hipStream_t)stream;
    ProfScope prof(KID_BCE_BALANCED, s, 0, 16.0 * n);
    hipLaunchKernelGGL(bce_w_fwd_kernel, dim3(cdiv(n, 256)), dim3(256), 0, s, logits, (const long long*)y, loss, n,
                       BceShape{pos, neg, gamma});
    return check_launch("egk_bce_w_fwd");
}

int egk_bce_w_bwd(egk_stream_t stream, const float* logits, const int64_t* y, const float* gloss, void* dlogits, int32_t n, float pos,
                  float neg, float gamma, int32_t dtype) {
    EGK_REQUIRE(logits && y && gloss && dlogits, "egk_bce_w_bwd: null pointer");
    EGK_REQUIRE(n >= 0, "egk_bce_w_bwd: n must be >= 0");
    EGK_REQUIRE(bce_shape_ok(pos, neg, gamma), "egk_bce_w_bwd: pos, neg and gamma must be finite and >= 0 (got %g, %g, %g)", (double)pos,
                (double)neg, (double)gamma);
    EGK_REQUIRE(dtype == EGK_F32 || dtype == EGK_BF16, "egk_bce_w_bwd: unknown activation dtype %d", (int)dtype);
    if (n == 0) return 0;
    hipStream_t s = (hipStream_t)stream;
    ProfScope prof(KID_BCE_BALANCED, s, 0, 20.0 * n);
    EGK_DISPATCH_T(dtype, hipLaunchKernelGGL(bce_w_bwd_kernel<T>, dim3(cdiv(n, 256)), dim3(256), 0, s, logits, (const long long*)y,
                                             gloss, (T*)dlogits, n, BceShape{pos, neg, gamma}));
    return check_launch("egk_bce_w_bwd");
}

}  // extern "C"
