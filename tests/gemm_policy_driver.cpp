// Command-line face of egopack_amd/csrc/gemm_policy.h for tests/test_gemm_policy_cpu.py (host compiler only, nothing is launched).
// One query per input line, one answer per output line:
//   single M N K layout splitk dbias st_mode pipe tt_tall r192_loaders        -> variant loaders tiles_m tiles_n group_m
//   single_f32 M N layout splitk pipe                                         -> variant loaders tiles_m tiles_n group_m
//   group layout min_nkt any_extra f16 f32 pipe tt_tall r192_loaders count M0 N0 M1 N1 ...
//                                                                             -> variant loaders total, then tiles_m tiles_n group_m per problem
//   rows                                                                      -> family variant layout flavour threads lds, one line per launch row
// layout: 0 nn, 1 nt, 2 tt, 3 tn.  K: the sum of the K sources (a multiple of 64); the K tiles of a slab are derived as gemm.hip does.
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>

#include "gemm_policy.h"

using namespace egk::policy;

int main() {
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string what;
        if (!(in >> what)) continue;
        Knobs kn;
        if (what == "single") {
            int M, N, layout, splitk, dbias, st;
            long long K;
            in >> M >> N >> K >> layout >> splitk >> dbias >> st >> kn.pipe >> kn.tt_tall >> kn.r192_loaders;
            const Choice c = pick_single(M, N, K, (int)ceil_div(K / 64, splitk), layout, splitk, dbias != 0, st != 0, kn);
            std::printf("%d %d %d %d %d\n", c.variant, (int)c.loaders, c.tiles_m, c.tiles_n, c.group_m);
        } else if (what == "single_f32") {
            int M, N, layout, splitk;
            in >> M >> N >> layout >> splitk >> kn.pipe;
            const Choice c = pick_single_f32(M, N, layout, splitk, kn);
            std::printf("%d %d %d %d %d\n", c.variant, (int)c.loaders, c.tiles_m, c.tiles_n, c.group_m);
        } else if (what == "group") {
            int layout, min_nkt, any_extra, f16, f32, count, M[MAX_PROBLEMS], N[MAX_PROBLEMS];
            in >> layout >> min_nkt >> any_extra >> f16 >> f32 >> kn.pipe >> kn.tt_tall >> kn.r192_loaders >> count;
            if (count < 1 || count > MAX_PROBLEMS) return 2;
            for (int i = 0; i < count; ++i) in >> M[i] >> N[i];
            const GroupChoice c = pick_group(M, N, count, layout, min_nkt, any_extra != 0, f16 != 0, f32 != 0, kn);
            std::printf("%d %d %d", c.variant, (int)c.loaders, c.total);
            for (int i = 0; i < count; ++i) std::printf(" %d %d %d", c.tiles_m[i], c.tiles_n[i], c.group_m[i]);
            std::printf("\n");
        } else if (what == "rows") {
#define PRINT_ROW(FAM, V, TA, TB, FL) \
    std::printf("%d %d %d %d %d %d\n", (int)FAM, (int)V, layout_of(TA, TB), (int)FL, row_threads(FAM, V, FL), row_lds_bytes(FAM, V));
            EGK_GEMM_LAUNCH_ROWS(PRINT_ROW)
#undef PRINT_ROW
        } else {
            return 2;
        }
        if (!in) return 2;
    }
    return 0;
}
