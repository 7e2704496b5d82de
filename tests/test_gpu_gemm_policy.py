"""The launch side of the contraction policy on the GPU: every single-launch row of tests/gemm_policy_expected.json (the table
tests/test_gemm_policy_cpu.py checks against egopack_amd/csrc/gemm_policy.h) runs once on ``torch.empty`` operands with the
library's profiling on, outside any capture, and must show up under the profile name of the kernel family its expected variant
belongs to -- ``gemm_bf16_<layout>`` (128-row tiles), ``..._g2``, ``..._r96``, ``..._r64``, ``..._r192``, ``..._t256``, the generic
kernel, ``gemm_f32_<layout>`` -- once, plus one ``gemm_splitk_reduce`` behind a split launch and nothing else of the contraction
family.  ``egk_gemm_stats_blocks`` is asked twice per row, with one row segment of M rows and with segments of at least 100 rows
(between the 96- and the 128-row tile), and must answer what the library answered before the policy moved into gemm_policy.h
(``stats_blocks`` in the table, recorded on an MI355X with that library).

Group variants are not visible through the profile names: tests/test_gemm_policy_cpu.py covers them.  The variant a row expects
comes from the table; the map from variant to profile suffix below is the one of common.h's kernel id list."""
import ctypes as C
import json
from pathlib import Path

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"
TABLE = json.loads((Path(__file__).resolve().parent / "gemm_policy_expected.json").read_text())
SUFFIX = {3: "", 5: "_g2", 12: "_g2", 8: "_r96", 11: "_r64", 16: "_r192", 7: "_t256", 15: "_t256"}
# launches that never reach the pipelined kernels: bf16 with a K that is no multiple of 64, f32 with one that is no multiple of 32
GENERIC = [dict(name="bf16 nn 256x256 K96: the generic kernel", layout="nn", M=256, N=256, K=96, splitk=1, dtype="bf16", profile="gemm_bf16_generic"),
           dict(name="bf16 tt 256x256 K96 split-K 2: the generic kernel", layout="tt", M=256, N=256, K=96, splitk=2, dtype="bf16", profile="gemm_bf16_generic"),
           dict(name="f32 nt 256x256 K48: the generic kernel", layout="nt", M=256, N=256, K=48, splitk=1, dtype="f32", profile="gemm_f32_nt")]


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from egopack_amd import ops as _ops
    return _ops


@pytest.fixture(scope="module")
def lib(ops):
    from egopack_amd import _lib
    return _lib.load()


class knobs:
    """The row's egk_gemm_set_pipeline settings -- defaults restored on exit."""

    def __init__(self, lib, row):
        self.lib, self.row = lib, row

    def __enter__(self):
        self.prev = self.lib.egk_gemm_set_pipeline(self.row.get("pipe", 1))
        self.lib.egk_gemm_set_pipeline(850 + self.row.get("tt_tall", 1))
        self.lib.egk_gemm_set_pipeline(870 + self.row.get("r192_loaders", 1))

    def __exit__(self, *exc):
        self.lib.egk_gemm_set_pipeline(851)
        self.lib.egk_gemm_set_pipeline(871)
        self.lib.egk_gemm_set_pipeline(self.prev)


def operands(row, dtype):
    M, N, K = row["M"], row["N"], row["K"]
    ta, tb = row["layout"][0] == "t", row["layout"][1] == "t"
    A = torch.empty((K, M) if ta else (M, K), device=DEV, dtype=dtype)
    B = torch.empty((K, N) if tb else (N, K), device=DEV, dtype=dtype)
    out = torch.empty(M, N, device=DEV, dtype=torch.float32)
    kw = dict(transA=ta, transB=tb)
    if row.get("dbias"):
        kw.update(dbias=torch.empty(M, device=DEV, dtype=torch.float32))
    return (M, N, A, A.shape[1], B, B.shape[1], K, out, N), kw


def launch_profile(ops, lib, row, dtype, compute):
    """{profile name: launches} of the contraction family for one launch of ``row`` (a row with st_mode: the launch carries the
    statistics epilogue over one row segment)."""
    args, kw = operands(row, dtype)
    with knobs(lib, row):
        ops.prof_reset()
        ops.prof_enable(True)
        try:
            if row.get("st_mode"):
                seg = torch.tensor([0, row["M"]], device=DEV, dtype=torch.int32)
                got = ops._gemm_with_stats(args, dict(compute=compute, **kw), dict(mode=1, n_seg=1, min_rows=row["M"], seg_ptr=seg))
                assert got is not None, "the launch took no statistics epilogue"
            else:
                ops.gemm(*args, compute=compute, splitk=row["splitk"], **kw)
            torch.cuda.synchronize()
            rep = ops.prof_report()
        finally:
            ops.prof_enable(False)
            ops.prof_reset()
    return {k: v["launches"] for k, v in rep.items() if k.startswith("gemm_")}


def stats_blocks(ops, lib, row, dtype, compute):
    """[egk_gemm_stats_blocks with one segment of M rows, ... with segments of at least 100 rows] (nothing is launched)."""
    args, kw = operands(row, dtype)
    kw.pop("dbias", None)
    seg = torch.tensor([0, row["M"]], device=DEV, dtype=torch.int32)
    out = []
    with knobs(lib, row):
        for min_rows in (row["M"], 100):
            d = ops._gemm_desc(*args, compute=compute, stats=dict(mode=1, n_seg=1, min_rows=min_rows, seg_ptr=seg), **kw)
            d.splitk = row["splitk"]
            out.append(int(lib.egk_gemm_stats_blocks(C.byref(d))))
    return out


def expected_profile(row, base):
    want = {base: 1}
    if row["splitk"] > 1:
        want["gemm_splitk_reduce"] = 1
    return want


@pytest.mark.parametrize("row", TABLE["single"], ids=lambda r: r["name"])
def test_single_bf16_rows(ops, lib, row):
    got = launch_profile(ops, lib, row, torch.bfloat16, ops.BF16)
    assert got == expected_profile(row, f"gemm_bf16_{row['layout']}{SUFFIX[row['expect']['variant']]}"), row["name"]
    assert stats_blocks(ops, lib, row, torch.bfloat16, ops.BF16) == row["stats_blocks"], row["name"]


@pytest.mark.parametrize("row", TABLE["single_f32"], ids=lambda r: r["name"])
def test_single_f32_rows(ops, lib, row):
    got = launch_profile(ops, lib, row, torch.float32, ops.F32)
    assert got == expected_profile(row, f"gemm_f32_{row['layout']}"), row["name"]
    assert stats_blocks(ops, lib, row, torch.float32, ops.F32) == row["stats_blocks"], row["name"]


@pytest.mark.parametrize("row", GENERIC, ids=lambda r: r["name"])
def test_generic_rows(ops, lib, row):
    dtype, compute = (torch.bfloat16, ops.BF16) if row["dtype"] == "bf16" else (torch.float32, ops.F32)
    assert launch_profile(ops, lib, row, dtype, compute) == expected_profile(row, row["profile"]), row["name"]
    assert stats_blocks(ops, lib, row, dtype, compute) == [0, 0], row["name"]
