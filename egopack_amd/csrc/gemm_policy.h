// Tile variants of the contraction kernels (gemm.hip): their geometry, their launch numbers and the host-side policy that picks
// one for a launch.  Plain C++17 without HIP: a host compiler alone builds it (tests/test_gemm_policy_cpu.py drives the policy
// through tests/gemm_policy_driver.cpp without launching anything).
#pragma once

namespace egk {
namespace policy {

constexpr int MAX_PROBLEMS = 8;  // problems of a grouped launch (MAX_GROUPS of gemm.hip)

// Tile variants.  The values are the public codes of egk_gemm_set_pipeline.
enum Variant : int {
    V_128 = 3,        // 128 x 128, 4 waves, 2-stage ring: two workgroups per CU
    V_G2 = 5,         // 128 x 128, two wave groups that walk alternate K tiles
    V_T256 = 7,       // 256 x 256, the big-tile kernel (single launches)
    V_R96 = 8,        // 96 x 128 (row-major A)
    V_R64 = 11,       // 64 x 128 (row-major A)
    V_R64_G2 = 12,    // 64 x 128 with two wave groups (row-major A, single launches, forced only)
    V_TALL = 13,      // 256 x 128, 8 waves, 3-stage ring (tt groups)
    V_R192_T256 = 15, // 192 x 256, the big-tile kernel (row-major A, single launches)
    V_R192 = 16,      // 192 x 128, 8 waves, 3-stage ring, optionally with loader waves (row-major A)
};

// Profile id bases (the nn entry of each four- or two-layout run of common.h's KID_GEMM_* list; gemm.hip asserts the match).
constexpr int PROF_NN = 0, PROF_G2 = 8, PROF_R96 = 12, PROF_R64 = 14, PROF_R192 = 16, PROF_T256 = 18;

// One record per variant: what the kernel templates take (gemm_pipe_kernel<stages, TA, TB, kg, mb, ni, F16, LW>, gemm_big_kernel<TA, TB,
// 8, ni>) and what the host needs to know about the tile.
struct Shape {
    int variant;
    int rows, cols;   // tile
    int kg, mb, ni;   // wave groups, 4-wave blocks per group (tile height), MFMA row fragments per wave
    int stages, lw;   // LDS ring depth; loader waves the variant CAN run with (0: none)
    bool big;         // the big-tile kernel family (fixed block and LDS size)
    bool stats;       // carries the segment-statistics epilogue
    int prof;         // profile id base
};
constexpr Shape SHAPES[] = {
    {V_128, 128, 128, 1, 1, 4, 2, 0, false, true, PROF_NN},
    {V_G2, 128, 128, 2, 1, 4, 2, 0, false, false, PROF_G2},
    {V_T256, 256, 256, 1, 2, 8, 2, 0, true, false, PROF_T256},
    {V_R96, 96, 128, 1, 1, 3, 2, 0, false, true, PROF_R96},
    {V_R64, 64, 128, 1, 1, 2, 2, 0, false, true, PROF_R64},
    {V_R64_G2, 64, 128, 2, 1, 2, 2, 0, false, false, PROF_G2},
    {V_TALL, 256, 128, 1, 2, 4, 3, 0, false, false, PROF_NN},
    {V_R192_T256, 192, 256, 1, 2, 6, 2, 0, true, false, PROF_T256},
    {V_R192, 192, 128, 1, 2, 3, 3, 4, false, true, PROF_R192},
};
constexpr bool is_variant(int v) {
    for (const Shape& s : SHAPES)
        if (s.variant == v) return true;
    return false;
}
constexpr Shape shape(int v) {  // (a code that names no variant: the 128 x 128 record)
    for (const Shape& s : SHAPES)
        if (s.variant == v) return s;
    return SHAPES[0];
}

// Block size and dynamic LDS bytes, by the kernels' own formulas: __launch_bounds__(NTHREADS * KG * MB + 64 * LW) and NSTAGE * KG
// stages of an A image of MB * NI * 4096 bytes plus a 16 KiB B image.  The big-tile kernels are 8 waves on 128 KiB.  The exact-f32
// kernels (gemm_pipe_f32_kernel<TA, TB, NI>) are the V_128 / V_R96 records: 4 waves, two stages of the same images.
constexpr int threads(const Shape& s, bool loaders) { return s.big ? 512 : 256 * s.kg * s.mb + 64 * (loaders ? s.lw : 0); }
constexpr int lds_bytes(const Shape& s) { return s.big ? 131072 : s.stages * s.kg * (s.mb * s.ni * 4096 + 16384); }

static_assert(lds_bytes(shape(V_128)) == 2 * 32768 && threads(shape(V_128), false) == 256, "128 x 128");
static_assert(lds_bytes(shape(V_G2)) == 4 * 32768 && threads(shape(V_G2), false) == 512, "two wave groups");
static_assert(lds_bytes(shape(V_R96)) == 2 * 28672 && threads(shape(V_R96), false) == 256, "96-row tile");
static_assert(lds_bytes(shape(V_R64)) == 2 * 24576 && threads(shape(V_R64), false) == 256, "64-row tile");
static_assert(lds_bytes(shape(V_R64_G2)) == 4 * 24576 && threads(shape(V_R64_G2), false) == 512, "64-row tile, two wave groups");
static_assert(lds_bytes(shape(V_TALL)) == 3 * 49152 && threads(shape(V_TALL), false) == 512, "256 x 128 tile");
static_assert(lds_bytes(shape(V_R192)) == 3 * 40960 && threads(shape(V_R192), true) == 768 && threads(shape(V_R192), false) == 512,
              "192-row tile");
static_assert(lds_bytes(shape(V_T256)) == 131072 && threads(shape(V_T256), false) == 512, "256 x 256 tile");
static_assert(lds_bytes(shape(V_R192_T256)) == 131072 && threads(shape(V_R192_T256), false) == 512, "192 x 256 tile");
static_assert(lds_bytes(shape(V_128)) == 65536 && lds_bytes(shape(V_R96)) == 2 * 28672, "the exact-f32 kernels");

enum Layout : int { NN = 0, NT = 1, TT = 2, TN = 3 };
constexpr int layout_of(bool transA, bool transB) { return transA ? (transB ? TT : TN) : (transB ? NT : NN); }

// Every launched instantiation, once: X(family, variant, transA, transB, flavour).  gemm.hip expands the list into its launch table
// (kernel address, block size and LDS bytes of each row); what is not listed here cannot be launched.
//   PIPE / GROUP   gemm_pipe_kernel / gemm_pipe_group_kernel and their _e0 twins (bf16 operands)
//   BIG            gemm_big_kernel
//   F32 / F32_GROUP  gemm_pipe_f32_kernel / gemm_pipe_f32_group_kernel (exact f32)
//   GEN_F32 / GEN_BF16 / GEN_MIXED  gemm_kernel, the generic register-staged kernel: f32; bf16 MFMA on bf16 / on f32 operands
enum Family : int { PIPE, GROUP, BIG, F32, F32_GROUP, GEN_F32, GEN_BF16, GEN_MIXED };
enum Flavour : int { PLAIN, LOADERS, F16 };  // LOADERS: with the variant's loader waves; F16: IEEE half operands
#define EGK_GEMM_ROWS_4(X, FAM, V, FL) X(FAM, V, false, false, FL) X(FAM, V, false, true, FL) X(FAM, V, true, true, FL) X(FAM, V, true, false, FL)
#define EGK_GEMM_ROWS_3(X, FAM, V, FL) X(FAM, V, false, false, FL) X(FAM, V, false, true, FL) X(FAM, V, true, true, FL)
#define EGK_GEMM_ROWS_2(X, FAM, V, FL) X(FAM, V, false, false, FL) X(FAM, V, false, true, FL)
#define EGK_GEMM_LAUNCH_ROWS(X)                                                                  \
    EGK_GEMM_ROWS_4(X, PIPE, V_128, PLAIN) EGK_GEMM_ROWS_4(X, PIPE, V_G2, PLAIN)                 \
    EGK_GEMM_ROWS_2(X, PIPE, V_R96, PLAIN) EGK_GEMM_ROWS_2(X, PIPE, V_R64, PLAIN)                \
    EGK_GEMM_ROWS_2(X, PIPE, V_R64_G2, PLAIN)                                                    \
    EGK_GEMM_ROWS_2(X, PIPE, V_R192, PLAIN) EGK_GEMM_ROWS_2(X, PIPE, V_R192, LOADERS)            \
    EGK_GEMM_ROWS_4(X, BIG, V_T256, PLAIN) EGK_GEMM_ROWS_2(X, BIG, V_R192_T256, PLAIN)           \
    EGK_GEMM_ROWS_3(X, GROUP, V_128, PLAIN) EGK_GEMM_ROWS_3(X, GROUP, V_G2, PLAIN)               \
    EGK_GEMM_ROWS_2(X, GROUP, V_R96, PLAIN) EGK_GEMM_ROWS_2(X, GROUP, V_R64, PLAIN)              \
    X(GROUP, V_TALL, true, true, PLAIN) EGK_GEMM_ROWS_2(X, GROUP, V_R192, LOADERS)               \
    X(GROUP, V_128, false, false, F16)                                                           \
    EGK_GEMM_ROWS_4(X, F32, V_128, PLAIN) EGK_GEMM_ROWS_2(X, F32, V_R96, PLAIN)                  \
    EGK_GEMM_ROWS_3(X, F32_GROUP, V_128, PLAIN)                                                  \
    EGK_GEMM_ROWS_4(X, GEN_F32, V_128, PLAIN) EGK_GEMM_ROWS_4(X, GEN_BF16, V_128, PLAIN)         \
    EGK_GEMM_ROWS_4(X, GEN_MIXED, V_128, PLAIN)
// block size and dynamic LDS bytes of a row
constexpr int row_threads(int family, int variant, int flavour) {
    return family >= GEN_F32 ? 256 : threads(shape(variant), flavour == LOADERS);
}
constexpr int row_lds_bytes(int family, int variant) { return family >= GEN_F32 ? 0 : lds_bytes(shape(variant)); }

// The development switches of egk_gemm_set_pipeline that the policy reads.
struct Knobs {
    int pipe = 1;          // 0 .. 19: 1 the policy, else a forced variant (a code that names none: V_128)
    int tt_tall = 1;       // 850 / 851
    int r192_loaders = 1;  // 870 / 871
};

constexpr long long ceil_div(long long a, long long b) { return (a + b - 1) / b; }

// near-square XCD patches: group_m ~ sqrt(workgroups per XCD), inside one slab (single launches: launch_wgs = tiles * split-K) or inside
// one problem (grouped launches -- near-square patches of what ONE XCD works on: its share of the whole launch, launch_wgs = total)
inline int xcd_patch_height(int tiles_m, int tiles_n, int launch_wgs) {
    const int tiles = tiles_m * tiles_n;
    int per_xcd = (int)ceil_div(launch_wgs, 8);
    if (per_xcd > tiles) per_xcd = tiles;
    int gm = 1;
    while ((gm + 1) * (gm + 1) <= per_xcd) ++gm;
    return gm < tiles_m ? gm : tiles_m;
}
// ... of a single launch.
// Row-major A (forward / dX forms: the output rows ARE the rows of the chain's activations): XCD x takes the tile rows
// [x * tiles_m / 8, (x + 1) * tiles_m / 8) with ALL their tile columns -- the contiguous eighth of the rows that the row
// kernels in front of and behind this launch give to XCD x (common.h, row_walk): its A strips were written, and its output
// rows will be read, by workgroups of the SAME XCD, i.e. through that XCD's own L2 instead of across the fabric
// (tools/exp/xcd_affinity.hip: 4.0-4.4 us against 8.3-11.2 us for a 12.6 MB hand-off).  Every XCD then streams the whole
// B operand (weights: 2-9 MB, shared by its 32 workgroups K tile by K tile).
inline int single_patch_height(int tiles_m, int tiles_n, int splitk, bool transA) {
    if (!transA && splitk == 1 && tiles_m % 8 == 0) return tiles_m / 8;
    return xcd_patch_height(tiles_m, tiles_n, tiles_m * tiles_n * splitk);
}

struct Choice {
    int variant;
    bool loaders;  // the variant's loader waves run
    int tiles_m, tiles_n, group_m;
};

// Variant of a single bf16 pipelined launch.  K: the sum of the K sources; nkt_slab: 64-deep K tiles per split-K slab; dbias: the FUSED
// bias gradient is on; st_mode: the caller asks for the segment-statistics epilogue.
inline Choice pick_single(int M, int N, long long K, int nkt_slab, int layout, int splitk, bool dbias, bool st_mode, const Knobs& kn) {
    const bool transA = layout >= TT;
    const int tiles_n = (int)ceil_div(N, 128);
    // Variant policy (g_use_pipe == 1), by the number of 128 x 128 workgroups the launch would have:
    //   <= 256 : one workgroup (one wave per SIMD) per CU would walk K at a fifth of the MFMA rate (DMA issue, LDS
    //            reads and MFMAs of the lone wave serialise): two wave groups per workgroup instead (5);
    //   >  256 : 128 x 128 tiles, two 4-wave workgroups per CU (3).
    // The 256 x 128 tile (6) is kept as a measured alternative: it fetches a third fewer bytes per flop, but the
    // rate of this loop is set by LDS fragment reads + MFMA issue per 64 x 64 wave patch, not by the bytes a CU
    // takes in -- it is 3-10 % slower than (3) up to 4096^3 and 5 % faster at 8192^3 (tools/gemm_bench.py --layouts).
    const int nwg128 = (int)ceil_div(M, 128) * tiles_n * splitk;
    int variant = kn.pipe;
    if (variant == 1) {
        variant = nwg128 > 256 ? V_128 : (nkt_slab >= 4 ? V_G2 : V_128);
        if (!transA && splitk == 1) {  // row-major A: the tile height is free (MFMA row fragments per wave)
            const long long t128 = ceil_div(M, 128) * tiles_n, t96 = ceil_div(M, 96) * tiles_n;
            const long long t64 = ceil_div(M, 64) * tiles_n;
            if (nwg128 > 256) {
                // a CU runs its share of the tiles two at a time at a fixed intake: the launch ends after
                // ceil(tiles / 256) tiles' worth of bytes on the fullest CU (6144 x 1024: 2 x 32 KiB per K tile with
                // 384 tiles of 128 rows, 2 x 28 KiB with 512 tiles of 96 rows)
                if (((t96 + 255) / 256) * 28 < ((t128 + 255) / 256) * 32) variant = V_R96;
                // ... or ONE 8-wave workgroup per CU on 192 x 128 tiles with a 3-stage ring (two K tiles = 80 KiB in flight
                // per CU): 40 KiB per K tile and round of 256 tiles -- 6144 x 1024 is exactly one round (256 tiles) where the
                // 96-row tiles are two co-resident workgroups of 28 KiB each
                const long long t192 = ceil_div(M, 192) * tiles_n;
                const long long cur = variant == V_R96 ? ((t96 + 255) / 256) * 28 : ((t128 + 255) / 256) * 32;
                // (ONE round only: 8192 x 1024 -- 344 tiles, two rounds of which the second is a third full -- measured 32.6 us
                //  against 22.3 on 128-row tiles; BASELINE config 5's 16384 rows 3.08 against 2.92 ms per step)
                if (t192 > 192 && t192 <= 256 && 40 < cur) variant = V_R192;
                // (several rounds of this tile with its loader waves -- 16384 x 1024: 688 tiles, 2.7 rounds -- measured 2.938 -> 2.901 ms
                //  for BASELINE config 5 on one box and 2.93 -> 3.03 on two others: one round only)
            } else if (t64 <= 256 && t64 > t128) {
                // at most 128 tiles: 64-row tiles put one 4-wave workgroup on twice as many CUs instead of one
                // 8-wave (two wave groups) workgroup on half of them (2048 x 1024 x 1024: 10.6 vs 12.4 us)
                variant = V_R64;
            }
        }
        // large outputs with a long K walk: 256 x 256 tiles, one 8-wave workgroup per CU, when whole tiles fill at least
        // 90 % of the CU slots of the rounds they take.  Measured against the 128 x 128 kernel (tools/gemm_big.py):
        // 16384 x 1024 x 4608: 126 vs 145 us; 4096^3: 113 vs 128; 8192^3: 836 vs 1178; but 16384 x 1024 x 2048: 76 vs 74
        // and x 1024: 45 vs 45 (16 K tiles: prologue and epilogue of the big tile weigh as much as its loop saves),
        // 24576 x 1024 (384 tiles, 1.5 rounds): 78 vs 65.  6144 x 1024 (96 tiles) never qualifies.
        const long long t256 = ceil_div(M, 256) * ceil_div(N, 256);
        if (splitk == 1 && !dbias && M % 256 == 0 && N % 256 == 0 && t256 >= 192 && K >= 3072 &&
            10 * t256 >= 9 * 256 * ((t256 + 255) / 256))
            variant = V_T256;
        // ... and 192 x 256 tiles (row-major A) where THEY fill their rounds and the 256-row tiles do not: 6144 x 4096 is 384
        // tiles of 256 rows (1.5 rounds: the makespan of two) but 512 of 192 rows (two whole rounds of 3/4 the height)
        const long long t192 = ceil_div(M, 192) * ceil_div(N, 256);
        // (round 5, HISTORY.md; us: 6144 x 4096 x 4608 199 vs 211-263 on 128-row tiles, x 4096 180 vs 190, the dX form 185 vs
        //  190, 6144 x 4096 x 1024 63.3 vs 66.7; 6144 x 1024 outputs are 128 such tiles and stay on 96-row tiles)
        if (variant != V_T256 && !transA && splitk == 1 && !dbias && M % 192 == 0 && N % 256 == 0 && t192 >= 192 && K >= 1024 &&
            10 * t192 >= 9 * 256 * ((t192 + 255) / 256))
            variant = V_R192_T256;
    } else if ((variant == V_R96 || variant == V_R64 || variant == V_R64_G2 || variant == V_R192) &&
               (transA || (variant == V_R192 && splitk > 1))) {
        variant = V_128;  // the forced variants exist for row-major A only (16: unsplit)
    } else if (variant == V_T256 && (dbias || M % 256 != 0 || N % 256 != 0)) {
        variant = V_128;  // whole 256 x 256 tiles only, no fused bias gradient
    } else if (variant == V_R192_T256 && (transA || dbias || M % 192 != 0 || N % 256 != 0)) {
        variant = V_128;  // whole 192 x 256 tiles of a row-major A only
    }
    if (!is_variant(variant) || variant == V_TALL)
        variant = V_128;  // (a forced value that names no tile variant of a single launch: the 2-stage 128 x 128 kernel)
    if (variant == V_R64_G2 && st_mode) variant = V_R64;  // (forced by the knob: the epilogue statistics win)
    const Shape s = shape(variant);
    Choice c;
    c.variant = variant;
    c.loaders = s.lw > 0 && kn.r192_loaders && nkt_slab >= 4;
    c.tiles_m = (int)ceil_div(M, s.rows);
    c.tiles_n = (int)ceil_div(N, s.cols);
    c.group_m = single_patch_height(c.tiles_m, c.tiles_n, splitk, transA);
    return c;
}

// ... of a single exact-f32 pipelined launch: V_128 or V_R96.
inline Choice pick_single_f32(int M, int N, int layout, int splitk, const Knobs& kn) {
    const bool transA = layout >= TT;
    const int tiles_n = (int)ceil_div(N, 128);
    // 96-row tiles (row-major A) when they load the CUs more evenly: the matrix pipes of a CU are shared by its co-resident
    // workgroups, so a launch lasts as long as the ROWS on its fullest CU
    bool r96 = false;
    if (!transA && kn.pipe != 3) {
        const long long t128 = ceil_div(M, 128) * tiles_n * splitk, t96 = ceil_div(M, 96) * tiles_n * splitk;
        r96 = kn.pipe == 8 || ((t96 + 255) / 256) * 96 < ((t128 + 255) / 256) * 128;
    }
    Choice c;
    c.variant = r96 ? V_R96 : V_128;
    c.loaders = false;
    c.tiles_m = (int)ceil_div(M, r96 ? 96 : 128);
    c.tiles_n = tiles_n;
    c.group_m = single_patch_height(c.tiles_m, c.tiles_n, splitk, transA);
    return c;
}

struct GroupChoice {
    int variant;
    bool loaders;
    int total;  // tiles of the whole launch
    int tiles_m[MAX_PROBLEMS], tiles_n[MAX_PROBLEMS], group_m[MAX_PROBLEMS];
};

// One tile variant for the whole grouped launch of ``count`` problems M[i] x N[i], by the policy of egk_gemm applied to the TOTAL tile
// count.  min_nkt: the fewest 64-deep K tiles of a problem; any_extra: a problem has extra K sources (the three-product groups of the
// precise pass); f16: IEEE half operands; f32: exact-f32 problems (128 x 128 tiles, XCD-packed placement).
inline GroupChoice pick_group(const int* M, const int* N, int count, int layout, int min_nkt, bool any_extra, bool f16, bool f32,
                              const Knobs& kn) {
    const bool ta = layout >= TT, tb = layout == NT || layout == TT;
    long long t128 = 0, t96 = 0, t64 = 0, t256 = 0, t192 = 0;
    for (int i = 0; i < count; ++i) {
        const long long tn = ceil_div(N[i], 128);
        t128 += ceil_div(M[i], 128) * tn; t96 += ceil_div(M[i], 96) * tn; t64 += ceil_div(M[i], 64) * tn;
        t256 += ceil_div(M[i], 256) * tn;
        t192 += ceil_div(M[i], 192) * tn;
    }
    int variant = t128 > 256 ? V_128 : (min_nkt >= 4 ? V_G2 : V_128);
    if (!ta) {
        if (t128 > 256) {
            if (((t96 + 255) / 256) * 28 < ((t128 + 255) / 256) * 32) variant = V_R96;
        } else if (t64 <= 256 && t64 > t128) {
            variant = V_R64;
        }
    }
    // weight-gradient groups (A^T B): a CU works on one 128 x 128 workgroup at a time (272 registers per lane), so a launch of 257 ..
    // 512 tiles takes two rounds whatever its tile count; when that count leaves many CUs idle in the second round (the pooling's
    // three weight gradients: 416 tiles) and the 256 x 128 tiling fits one workgroup per CU, the tall tile (8 waves, 3-stage ring,
    // 48 KiB per K tile for twice the flops) is one round instead.  Long K walks only: same box, alternating, 6144 rows 1.291 -> 1.284 ms, 16384 rows
    // 2.947 -> 2.934, 2048 rows 0.842 -> 0.863 (its 3-stage fill and 256-row epilogue outweigh 32 K tiles).
    if (ta && tb && kn.tt_tall && t128 > 256 && t128 <= 448 && t256 <= 256 && min_nkt >= 64) variant = V_TALL;
    // row-major A: the 192 x 128 tile with loader waves (egk_gemm's variant 16) when the group is ONE round of such tiles that more
    // than half fills the chip and 128- / 96-row tiles would take more than one (the projection heads of three task batches:
    // 64 + 2048 + 2048 rows = 184 tiles against 264 / 360)
    // (not for the three-product groups of the precise pass: BASELINE config 4 2.113 -> 2.124 ms with them)
    if (!ta && !f16 && !any_extra && kn.r192_loaders && t192 > 128 && t192 <= 256 && t128 > 256 && min_nkt >= 8) variant = V_R192;
    if (kn.pipe == V_128 || kn.pipe == V_G2) variant = kn.pipe;
    if (kn.pipe == V_TALL && ta && tb) variant = V_TALL;
    if ((kn.pipe == V_R96 || kn.pipe == V_R64) && !ta) variant = kn.pipe;
    if (f16) variant = V_128;  // (one instantiation: 128 x 128 tiles, one wave group)
    if (f32) variant = V_128;  // (exact-f32 problems: 128 x 128 tiles)
    const Shape s = shape(variant);
    GroupChoice c;
    c.variant = variant;
    c.loaders = s.lw > 0;  // (a grouped launch on the 192-row tile always runs its loader waves)
    c.total = 0;
    for (int i = 0; i < count; ++i) {
        c.tiles_m[i] = (int)ceil_div(M[i], s.rows);
        c.tiles_n[i] = (int)ceil_div(N[i], 128);
        c.total += c.tiles_m[i] * c.tiles_n[i];
    }
    for (int i = 0; i < count; ++i) c.group_m[i] = xcd_patch_height(c.tiles_m[i], c.tiles_n[i], c.total);
    return c;
}

}  // namespace policy
}  // namespace egk
