// LAMB for the flat-buffer optimizer (include/egopack_lamb.h): reduce, one trust ratio per slot, apply.  Every slot of the flat
// layout is cut into pieces of EGK_LAMB_PIECE elements; one 256-thread workgroup owns a piece in the reduce launch and in the apply
// launch, so the slot, its group's lr and weight decay and its trust ratio are workgroup-uniform (scalar loads, one binary search
// per workgroup as seg_find does for the group table).  No atomics: the reduce launch stores per-piece partial sums with one
// writer each, the trust launch adds them in a fixed order.  16-byte accesses; a scalar tail only in a slot's last quad.
#include "common.h"
#include "optim_stream.h"

namespace egk {

constexpr int LAMB_PIECE = EGK_LAMB_PIECE;
constexpr int LAMB_THREADS = 256;
constexpr int LAMB_QUADS = LAMB_PIECE / (4 * LAMB_THREADS);  // 16-byte groups per thread and piece
static_assert(LAMB_QUADS * 4 * LAMB_THREADS == LAMB_PIECE, "a piece is whole rounds of the workgroup");

struct LambTables {
    const long long* slot_begin;
    const int* slot_piece0;
    const int* slot_group;
    const float* group_hyper;
    int n_slots, n_groups;
};

struct PieceSpan {
    int slot;
    long long begin, end;  // the piece's elements
};

// piece q of the layout: the largest slot with slot_piece0[slot] <= q (every index read lies in [1, n_slots - 1]), then the q-th
// run of LAMB_PIECE elements of that slot, cut at the slot's end
__device__ __forceinline__ PieceSpan piece_span(const LambTables& t, int q) {
    int lo = 0, hi = t.n_slots - 1;
    while (lo < hi) {
        const int mid = lo + ((hi - lo + 1) >> 1);
        if (t.slot_piece0[mid] <= q) lo = mid; else hi = mid - 1;
    }
    const long long b = t.slot_begin[lo] + (long long)(q - t.slot_piece0[lo]) * LAMB_PIECE, e = t.slot_begin[lo + 1];
    return PieceSpan{lo, b, b + LAMB_PIECE < e ? b + LAMB_PIECE : e};
}

// {lr, weight_decay} of a slot's parameter group
__device__ __forceinline__ float2 slot_hyper(const LambTables& t, int slot) {
    int grp = t.slot_group[slot];
    grp = grp < 0 ? 0 : grp >= t.n_groups ? t.n_groups - 1 : grp;
    return *reinterpret_cast<const float2*>(t.group_hyper + 4 * grp);
}

struct LambConsts {
    float bc1, bc2s, eps, wd;  // 1 - b1^t, sqrt(1 - b2^t): hyper[1], hyper[2]
};

// u of one element: the ONE definition -- the reduce launch sums its square, the apply launch steps by it
__device__ __forceinline__ float lamb_u(float p, float m, float v, const LambConsts& c) {
#pragma clang fp contract(off)
    const float mh = m / c.bc1;
    const float denom = sqrtf(v) / c.bc2s + c.eps;
    const float r = mh / denom;
    const float d = c.wd * p;
    return r + d;
}

__device__ __forceinline__ void lamb_moments(float g, float& m, float& v, float gs, float omb1, float b2, float omb2) {
#pragma clang fp contract(off)
    const float gg = g * gs;
    m = m + (gg - m) * omb1;
    v = v * b2 + omb2 * gg * gg;
}

// ---- cache policy (egk_tune 9, egk_lamb_tune 0) -----------------------------------------------------------------------------------
// NT: 0 = the default policy everywhere, NT_G = the gradient's loads stream, 7 = every single-use stream does.  KEEP: what the apply
// launch reads again within the step -- p, and the m and v the reduce launch stores -- stays cacheable in the reduce launch (the
// old m and v, read once, still stream); the apply launch's loads and its store of p are the step's last use and stream.
int g_lamb_keep = 1;
extern int g_optim_stream_policy;

struct LambMomentsArgs {
    long long lo, hi;
    int piece0, n_pieces;
    LambTables t;
    const float* hyper;
    float omb1, b2, omb2, eps;
    const int* gate;
    long long* bump_word;
    long long bump;
};

template <typename GT, int NT, bool KEEP>
__global__ __launch_bounds__(LAMB_THREADS) void lamb_moments_kernel(const float* __restrict__ p, const GT* __restrict__ g,
                                                                    float* __restrict__ m, float* __restrict__ v,
                                                                    double* __restrict__ part, const LambMomentsArgs a) {
    constexpr bool nt_g = NT & NT_G, nt_old = NT & NT_LOAD, nt_p = (NT & NT_LOAD) && !KEEP, nt_st = (NT & NT_STORE) && !KEEP;
    __shared__ double red[LAMB_THREADS / WAVE][2];
    if (a.bump_word && blockIdx.x == 0 && threadIdx.x == 0) *a.bump_word += a.bump;
    if (a.gate && *a.gate == 0) return;
    const int q = a.piece0 + (int)blockIdx.x;
    if ((int)blockIdx.x >= a.n_pieces || q >= a.t.slot_piece0[a.t.n_slots]) return;
    const PieceSpan sp = piece_span(a.t, q);
    const long long b = sp.begin > a.lo ? sp.begin : a.lo, e = sp.end < a.hi ? sp.end : a.hi;
    if (e <= b) return;  // (the piece does not meet the range: nothing of it is this launch's)
    const LambConsts c{a.hyper[1], a.hyper[2], a.eps, slot_hyper(a.t, sp.slot).y};
    const float gs = a.hyper[3];
    double P = 0.0, U = 0.0;
#pragma unroll
    for (int k = 0; k < LAMB_QUADS; ++k) {
        const long long i = sp.begin + ((long long)k * LAMB_THREADS + threadIdx.x) * 4;
        if (i < b || i >= e) continue;  // (b and the piece's begin are multiples of 4: a quad lies on one side of b)
        if (i + 4 <= e) {
            const float4 pv = ld_quad(p + i, nt_p);
            const float4 gv = ld_quad(g + i, nt_g);
            float4 mv = ld_quad(m + i, nt_old), vv = ld_quad(v + i, nt_old);
            const float* pp = &pv.x; const float* gp = &gv.x; float* mp = &mv.x; float* vp = &vv.x;
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                lamb_moments(gp[t], mp[t], vp[t], gs, a.omb1, a.b2, a.omb2);
                const double u = (double)lamb_u(pp[t], mp[t], vp[t], c), x = (double)pp[t];
                P += x * x;
                U += u * u;
            }
            st_quad(m + i, mv, nt_st);
            st_quad(v + i, vv, nt_st);
        } else {
            for (long long j = i; j < e; ++j) {
                const float pj = p[j];
                float mj = m[j], vj = v[j];
                lamb_moments(ld1t(g + j), mj, vj, gs, a.omb1, a.b2, a.omb2);
                const double u = (double)lamb_u(pj, mj, vj, c), x = (double)pj;
                P += x * x;
                U += u * u;
                m[j] = mj;
                v[j] = vj;
            }
        }
    }
    P = wave_sum(P);
    U = wave_sum(U);
    const int wave = threadIdx.x / WAVE;
    if ((threadIdx.x & (WAVE - 1)) == 0) red[wave][0] = P, red[wave][1] = U;
    __syncthreads();
    if (threadIdx.x == 0) {
        double Ps = 0.0, Us = 0.0;
        for (int w = 0; w < LAMB_THREADS / WAVE; ++w) Ps += red[w][0], Us += red[w][1];
        double* out = part + 4ll * q;
        const bool front = b == sp.begin, back = e == sp.end;
        if (front) out[0] = Ps, out[1] = Us;  // half 0: the part that starts at the piece's first element
        else out[2] = Ps, out[3] = Us;        // half 1: the part that ends at its last
        if (front && back) out[2] = 0.0, out[3] = 0.0;
    }
}

// one wave per slot
__global__ __launch_bounds__(LAMB_THREADS) void lamb_trust_kernel(const double* __restrict__ part, const LambTables t, int trust_clip,
                                                                  int always_adapt, float* __restrict__ trust,
                                                                  double* __restrict__ norms, const int* __restrict__ gate) {
    if (gate && *gate == 0) return;
    const int slot = (int)blockIdx.x * (LAMB_THREADS / WAVE) + (int)threadIdx.x / WAVE, lane = threadIdx.x & (WAVE - 1);
    if (slot >= t.n_slots) return;
    const int q0 = t.slot_piece0[slot], q1 = t.slot_piece0[slot + 1];
    double P = 0.0, U = 0.0;
    for (int q = q0 + lane; q < q1; q += WAVE) {
        const double* h = part + 4ll * q;
        P += h[0]; U += h[1];
        P += h[2]; U += h[3];
    }
    P = wave_sum(P);
    U = wave_sum(U);
    if (lane == 0) {
        const float wd = slot_hyper(t, slot).y;
        const double np = sqrt(P), nu = sqrt(U);
        float tr = 1.f;
        if (!((wd == 0.f && !always_adapt) || P == 0.0 || U == 0.0)) tr = (float)(np / nu);
        if (trust_clip && tr > 1.f) tr = 1.f;
        trust[slot] = tr;
        norms[2 * slot] = np;
        norms[2 * slot + 1] = nu;
    }
}

struct LambApplyArgs {
    long long n;
    int n_pieces;
    LambTables t;
    const float* hyper;
    float eps;
    const float* trust;
    EmaArgs e;
    const long long* t_dev;
    const int* gate;
};

template <bool EMA, int NT>
__global__ __launch_bounds__(LAMB_THREADS) void lamb_apply_kernel(float* __restrict__ p, const float* __restrict__ m,
                                                                  const float* __restrict__ v, bf16_t* __restrict__ shadow,
                                                                  bf16_t* __restrict__ shadow_lo, float* __restrict__ ema,
                                                                  const LambApplyArgs a) {
#pragma clang fp contract(off)
    constexpr bool nt_ld = NT & NT_LOAD, nt_st = NT & NT_STORE;
    if (a.gate && *a.gate == 0) return;
    const int q = (int)blockIdx.x;
    if (q >= a.n_pieces || q >= a.t.slot_piece0[a.t.n_slots]) return;
    const PieceSpan sp = piece_span(a.t, q);
    const long long e = sp.end < a.n ? sp.end : a.n;
    const float2 lw = slot_hyper(a.t, sp.slot);
    const LambConsts c{a.hyper[1], a.hyper[2], a.eps, lw.y};
    const float step = lw.x * a.trust[sp.slot];
    const float w = EMA ? ema_weight(a.e, a.t_dev) : 0.f;
#pragma unroll
    for (int k = 0; k < LAMB_QUADS; ++k) {
        const long long i = sp.begin + ((long long)k * LAMB_THREADS + threadIdx.x) * 4;
        if (i >= e) continue;
        if (i + 4 <= e) {
            float4 pv = ld_quad(p + i, nt_ld);
            const float4 mv = ld_quad(m + i, nt_ld), vv = ld_quad(v + i, nt_ld);
            float4 ev = make_float4(0.f, 0.f, 0.f, 0.f);
            if constexpr (EMA) ev = ld_quad(ema + i, false);
            float* pp = &pv.x; const float* mp = &mv.x; const float* vp = &vv.x; float* ep = &ev.x;
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                const float u = lamb_u(pp[t], mp[t], vp[t], c);
                const float move = step * u;
                pp[t] = pp[t] - move;
                if constexpr (EMA) ema_update(ep[t], pp[t], w);
            }
            if constexpr (EMA) st_quad(ema + i, ev, false);
            st_quad(p + i, pv, nt_st);
            st4t(shadow + i, 0, 4, true, pv);
            if (shadow_lo)  // bf16(p - bf16(p)): egk_split_bf16's bits
                st4t(shadow_lo + i, 0, 4, true, make_float4(pp[0] - bf2f(f2bf(pp[0])), pp[1] - bf2f(f2bf(pp[1])),
                                                            pp[2] - bf2f(f2bf(pp[2])), pp[3] - bf2f(f2bf(pp[3]))));
        } else {
            for (long long j = i; j < e; ++j) {
                float pj = p[j];
                const float u = lamb_u(pj, m[j], v[j], c);
                const float move = step * u;
                pj = pj - move;
                if constexpr (EMA) {
                    float ej = ema[j];
                    ema_update(ej, pj, w);
                    ema[j] = ej;
                }
                p[j] = pj;
                shadow[j] = f2bf(pj);
                if (shadow_lo) shadow_lo[j] = f2bf(pj - bf2f(f2bf(pj)));
            }
        }
    }
}

// the policy of a launch from the family's mask: anything that streams p or the state streams all of LAMB's single-use streams
static int lamb_policy() {
    const int mask = g_optim_stream_policy;
    return (mask & (NT_LOAD | NT_STORE)) ? (NT_G | NT_LOAD | NT_STORE) : (mask & NT_G);
}

static int tables_check(const char* who, const int64_t* slot_begin, const int32_t* slot_piece0, const int32_t* slot_group, int32_t n_slots,
                        const float* group_hyper, int32_t n_groups) {
    EGK_REQUIRE(slot_piece0 && slot_group && group_hyper && slot_begin, "%s: null table pointer", who);
    EGK_REQUIRE(n_slots >= 1, "%s: n_slots >= 1 (got %d)", who, (int)n_slots);
    EGK_REQUIRE(n_groups >= 1 && n_groups <= 64, "%s: n_groups in 1..64 (got %d)", who, (int)n_groups);
    EGK_REQUIRE(aligned_to(8, {slot_begin}) && aligned_to(4, {slot_piece0, slot_group}) && aligned_to(16, {group_hyper}),
                "%s: misaligned table pointer (slot_begin 8-byte, slot_piece0 and slot_group 4-byte, group_hyper 16-byte)", who);
    return 0;
}

}  // namespace egk

using namespace egk;

extern "C" int egk_lamb_moments(egk_stream_t stream, const float* p, const void* g, int32_t g_dtype, float* m, float* v, int64_t lo,
                                int64_t hi, int32_t piece0, int32_t n_pieces, int32_t meets_piece_bound, const int64_t* slot_begin,
                                const int32_t* slot_piece0, const int32_t* slot_group, int32_t n_slots, const float* group_hyper,
                                int32_t n_groups, const float* hyper, double beta1, double beta2, float eps, double* part,
                                const int32_t* gate, int64_t* bump_word, int64_t bump) {
    const char* who = "egk_lamb_moments";
    EGK_REQUIRE(p && g && m && v && hyper && part, "%s: null pointer", who);
    EGK_REQUIRE(g_dtype == EGK_F32 || g_dtype == EGK_BF16, "%s: unknown gradient dtype %d", who, (int)g_dtype);
    EGK_REQUIRE(aligned_to(16, {p, m, v}) && aligned_to(g_dtype == EGK_BF16 ? 8 : 16, {g}),
                "%s: buffers must be 16-byte aligned (a bf16 gradient 8-byte)", who);
    EGK_REQUIRE(aligned_to(8, {part, bump_word}) && aligned_to(4, {gate, hyper}), "%s: misaligned part, bump_word, gate or hyper", who);
    if (const int rc = tables_check(who, slot_begin, slot_piece0, slot_group, n_slots, group_hyper, n_groups)) return rc;
    EGK_REQUIRE(lo >= 0 && lo < hi, "%s: an empty or negative range [%lld, %lld)", who, (long long)lo, (long long)hi);
    EGK_REQUIRE(lo % 8 == 0 && hi % 8 == 0, "%s: lo and hi must be multiples of 8 (got [%lld, %lld))", who, (long long)lo, (long long)hi);
    EGK_REQUIRE(meets_piece_bound || hi - lo >= LAMB_PIECE,
                "%s: a range of %lld elements is shorter than a piece (%d) and is not stated to hold a piece boundary: it may lie "
                "strictly inside one piece", who, (long long)(hi - lo), LAMB_PIECE);
    EGK_REQUIRE(piece0 >= 0 && n_pieces >= 1, "%s: piece0 >= 0 and n_pieces >= 1 (got %d, %d)", who, (int)piece0, (int)n_pieces);
    EGK_REQUIRE(eps > 0.f, "%s: eps > 0 (got %g): the padding of a slot has v = 0", who, (double)eps);
    EGK_REQUIRE(beta1 >= 0.0 && beta1 < 1.0 && beta2 >= 0.0 && beta2 < 1.0, "%s: betas in [0, 1) (got %g, %g)", who, beta1, beta2);
    hipStream_t s = (hipStream_t)stream;
    ProfScope prof(KID_LAMB_MOMENTS, s, 0, (g_dtype == EGK_BF16 ? 22.0 : 24.0) * (double)(hi - lo));
    const LambMomentsArgs a{(long long)lo, (long long)hi, (int)piece0, (int)n_pieces,
                            LambTables{(const long long*)slot_begin, slot_piece0, slot_group, group_hyper, (int)n_slots, (int)n_groups},
                            hyper, (float)(1.0 - beta1), (float)beta2, (float)(1.0 - beta2), eps, gate, (long long*)bump_word, (long long)bump};
    const int nt = lamb_policy();
    const bool keep = g_lamb_keep != 0;
#define EGK_LAMB_MOMENTS(NT, KEEP) \
    EGK_DISPATCH_T(g_dtype, hipLaunchKernelGGL((lamb_moments_kernel<T, NT, KEEP>), dim3((unsigned)n_pieces), dim3(LAMB_THREADS), 0, s, p, \
                                               (const T*)g, m, v, part, a))
    if (nt == 0) EGK_LAMB_MOMENTS(0, true);
    else if (nt == NT_G) EGK_LAMB_MOMENTS(1, true);
    else if (keep) EGK_LAMB_MOMENTS(7, true);
    else EGK_LAMB_MOMENTS(7, false);
#undef EGK_LAMB_MOMENTS
    return check_launch(who);
}

extern "C" int egk_lamb_trust(egk_stream_t stream, const double* part, const int32_t* slot_piece0, const int32_t* slot_group, int32_t n_slots,
                              const float* group_hyper, int32_t n_groups, int32_t trust_clip, int32_t always_adapt, float* trust,
                              double* norms, const int32_t* gate) {
    const char* who = "egk_lamb_trust";
    EGK_REQUIRE(part && trust && norms, "%s: null pointer", who);
    EGK_REQUIRE(aligned_to(8, {part, norms}) && aligned_to(4, {trust, gate}), "%s: misaligned part, norms, trust or gate", who);
    const int64_t some = 8;  // (this launch reads no slot_begin: any aligned non-null value passes the shared check)
    if (const int rc = tables_check(who, &some, slot_piece0, slot_group, n_slots, group_hyper, n_groups)) return rc;
    hipStream_t s = (hipStream_t)stream;
    ProfScope prof(KID_LAMB_TRUST, s, 0, 0.0);
    const LambTables t{nullptr, slot_piece0, slot_group, group_hyper, (int)n_slots, (int)n_groups};
    const int per = LAMB_THREADS / WAVE;
    hipLaunchKernelGGL(lamb_trust_kernel, dim3((unsigned)((n_slots + per - 1) / per)), dim3(LAMB_THREADS), 0, s, part, t, (int)trust_clip,
                       (int)always_adapt, trust, norms, gate);
    return check_launch(who);
}

extern "C" int egk_lamb_apply(egk_stream_t stream, float* p, const float* m, const float* v, int64_t n, int32_t n_pieces,
                              const int64_t* slot_begin, const int32_t* slot_piece0, const int32_t* slot_group, int32_t n_slots,
                              const float* group_hyper, int32_t n_groups, const float* hyper, float eps, const float* trust,
                              void* bf16_shadow, void* bf16_lo_shadow, float* ema, double ema_decay, int32_t ema_warmup,
                              const int64_t* t_dev, const int32_t* gate) {
    const char* who = "egk_lamb_apply";
    EGK_REQUIRE(p && m && v && hyper && trust && bf16_shadow, "%s: null pointer", who);
    EGK_REQUIRE(aligned_to(16, {p, m, v, ema}), "%s: buffers must be 16-byte aligned", who);
    EGK_REQUIRE(aligned_to(8, {bf16_shadow, bf16_lo_shadow, t_dev}), "%s: the bf16 copies must be 8-byte aligned", who);
    EGK_REQUIRE(aligned_to(4, {hyper, trust, gate}), "%s: misaligned hyper, trust or gate", who);
    if (const int rc = tables_check(who, slot_begin, slot_piece0, slot_group, n_slots, group_hyper, n_groups)) return rc;
    EGK_REQUIRE(n >= 1 && n_pieces >= 1, "%s: n >= 1 and n_pieces >= 1 (got %lld, %d)", who, (long long)n, (int)n_pieces);
    EGK_REQUIRE(eps > 0.f, "%s: eps > 0 (got %g): the padding of a slot has v = 0", who, (double)eps);
    if (ema) {
        EGK_REQUIRE(ema_decay >= 0.0 && ema_decay < 1.0, "%s: ema_decay in [0, 1) (got %g)", who, ema_decay);
        EGK_REQUIRE(!ema_warmup || t_dev, "%s: ema_warmup needs t_dev (the device step counter)", who);
    }
    hipStream_t s = (hipStream_t)stream;
    ProfScope prof(KID_LAMB_APPLY, s, 0, (16.0 + 2.0 + (bf16_lo_shadow ? 2.0 : 0.0) + (ema ? 8.0 : 0.0)) * (double)n);
    const LambApplyArgs a{(long long)n, (int)n_pieces,
                          LambTables{(const long long*)slot_begin, slot_piece0, slot_group, group_hyper, (int)n_slots, (int)n_groups},
                          hyper, eps, trust, EmaArgs{ema, ema_decay, (float)(1.0 - ema_decay), ema_warmup ? 1 : 0}, (const long long*)t_dev, gate};
    const int nt = lamb_policy() & (NT_LOAD | NT_STORE);
#define EGK_LAMB_APPLY(EMA, NT) \
    hipLaunchKernelGGL((lamb_apply_kernel<EMA, NT>), dim3((unsigned)n_pieces), dim3(LAMB_THREADS), 0, s, p, m, v, (bf16_t*)bf16_shadow, \
                       (bf16_t*)bf16_lo_shadow, ema, a)
    if (ema) { if (nt) EGK_LAMB_APPLY(true, 6); else EGK_LAMB_APPLY(true, 0); }
    else { if (nt) EGK_LAMB_APPLY(false, 6); else EGK_LAMB_APPLY(false, 0); }
#undef EGK_LAMB_APPLY
    return check_launch(who);
}

extern "C" int egk_lamb_tune(int32_t key, int32_t value) {
    if (key != 0) return -1;
    const int prev = g_lamb_keep;
    if (value == 0 || value == 1) g_lamb_keep = value;
    return prev;
}
