"""The contraction launch policy without a GPU: egopack_amd/csrc/gemm_policy.h is plain C++17, so the system C++ compiler builds
tests/gemm_policy_driver.cpp around it and the named shapes of tests/gemm_policy_expected.json are asked one by one: tile variant,
loader waves, tiles_m, tiles_n and the XCD patch height (group_m) of single bf16 launches, single exact-f32 launches and grouped
launches.  Every expected value was produced by the variant ladders gemm.hip had before the policy moved into the header; the
shapes sit on both sides of every boundary of the policy (tile counts around 256, K tiles around 4 / 8 / 64, whole and partial big
tiles, every forced code that falls back).

The launch table's rows (the list gemm.hip expands into kernel addresses) must fit the hardware: at most 1024 threads and 160 KiB
of LDS, and the pinned sizes of the pipelined bf16 family."""
import json
import shutil
import subprocess
from pathlib import Path

import pytest

HERE = Path(__file__).resolve().parent
CSRC = HERE.parent / "egopack_amd" / "csrc"
TABLE = json.loads((HERE / "gemm_policy_expected.json").read_text())
LAYOUT = {"nn": 0, "nt": 1, "tt": 2, "tn": 3}
PIPE, GROUP, BIG, F32, F32_GROUP, GEN_F32 = range(6)  # (enum Family of gemm_policy.h)


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx is not None, "the policy test needs the system C++ compiler"
    exe = tmp_path_factory.mktemp("gemm_policy") / "driver"
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", f"-I{CSRC}", str(HERE / "gemm_policy_driver.cpp"), "-o", str(exe)],
                   check=True, capture_output=True, text=True)

    def ask(line: str):
        r = subprocess.run([str(exe)], input=line + "\n", capture_output=True, text=True, check=True)
        return [list(map(int, ln.split())) for ln in r.stdout.splitlines()]

    return ask


def knob_fields(r):
    return f"{r['pipe']} {r.get('tt_tall', 1)} {r.get('r192_loaders', 1)}"


@pytest.mark.parametrize("row", TABLE["single"], ids=lambda r: r["name"])
def test_single_launch_policy(driver, row):
    (v,) = driver(f"single {row['M']} {row['N']} {row['K']} {LAYOUT[row['layout']]} {row['splitk']} {row['dbias']} {row['st_mode']} "
                  + knob_fields(row))
    assert dict(zip(("variant", "loaders", "tiles_m", "tiles_n", "group_m"), v)) == row["expect"]


@pytest.mark.parametrize("row", TABLE["single_f32"], ids=lambda r: r["name"])
def test_single_f32_launch_policy(driver, row):
    (v,) = driver(f"single_f32 {row['M']} {row['N']} {LAYOUT[row['layout']]} {row['splitk']} {row['pipe']}")
    assert dict(zip(("variant", "loaders", "tiles_m", "tiles_n", "group_m"), v)) == row["expect"]


@pytest.mark.parametrize("row", TABLE["group"], ids=lambda r: r["name"])
def test_grouped_launch_policy(driver, row):
    (v,) = driver(f"group {LAYOUT[row['layout']]} {row['min_nkt']} {row['any_extra']} {row['f16']} {row['f32']} {knob_fields(row)} "
                  f"{len(row['problems'])} " + " ".join(f"{m} {n}" for m, n in row["problems"]))
    got = dict(variant=v[0], loaders=v[1], total=v[2], tiles_m=v[3::3], tiles_n=v[4::3], group_m=v[5::3])
    assert got == row["expect"]


def test_table_names_the_shapes_of_the_policy():
    """The shapes the policy's comments and the step rely on, by their expected variant (the table itself is data).
    4096 x 3072 x 3072 stays on 128-row tiles: its 192 tiles of 256 x 256 fill 75 % of a round of 256 CUs, under the 90 % the
    big tile asks for; 4096 x 3840 (240 tiles) is the nearest whole-tile output of that height that takes it."""
    by_name = {r["name"]: r["expect"] for kind in ("single", "single_f32", "group") for r in TABLE[kind]}
    want = {"tt 1024x1024 K512: two wave groups": 5, "tt 1024x1024 K128": 3, "nn 2048x1024x1024: 64-row tiles": 11,
            "nn 4608x1024x1024: 96-row tiles": 8, "nn 8192x1024x1024: 128-row tiles (192-row tiles would take two rounds)": 3,
            "nn 6144x1024 K1024: 192-row tile with loader waves": 16, "nn 6144x1024 K128: no loader waves": 16,
            "nn 4096x3840 K3072: 240 tiles of 256 x 256": 7, "nn 3072x4096 K1024: 192 x 256 tiles": 15,
            "nn 1024x1024x2048 split-K 4: two wave groups and a reduce launch": 5,
            "tt 416 tiles, 64 K tiles: the tall tile": 13, "nn projection group, 184 tiles of 192 rows: loader-wave tile": 16,
            "f16 group: 128-row tiles, one wave group": 3}
    for name, variant in want.items():
        assert by_name[name]["variant"] == variant, name
    assert by_name["nn 64x128 K256: one tile either way, not 64-row tiles"]["variant"] != 11
    assert by_name["nn 6144x1024 K1024: 192-row tile with loader waves"]["loaders"] == 1
    assert by_name["nn 6144x1024 K128: no loader waves"]["loaders"] == 0
    assert by_name["tt 416 tiles, 32 K tiles: 128-row tiles"]["variant"] != 13
    assert by_name["nn projection group with extra K sources: 96-row tiles"]["variant"] != 16
    assert by_name["tt 4096x3840 K3072 with the fused bias gradient: not the 256 x 256 tiles"]["variant"] != 7


def test_launch_rows_fit_the_hardware(driver):
    rows = driver("rows")
    assert len(rows) == 59 and len({tuple(r[:4]) for r in rows}) == 59  # (18 + 14 with an _e0 twin each, 6 + 6 + 3 + 12 without: 91 kernels)
    for family, variant, layout, flavour, threads, lds in rows:
        assert 64 <= threads <= 1024 and threads % 64 == 0, (family, variant, layout, flavour)
        assert 0 <= lds <= 160 * 1024, (family, variant, layout, flavour)
        assert (lds == 0) == (family >= GEN_F32)
    size = {(f, v, fl): (t, l) for f, v, _, fl, t, l in rows}
    assert size[(PIPE, 3, 0)] == (256, 2 * 32768) and size[(PIPE, 5, 0)] == (512, 4 * 32768)
    assert size[(PIPE, 8, 0)] == (256, 2 * 28672) and size[(PIPE, 11, 0)] == (256, 2 * 24576) and size[(PIPE, 12, 0)] == (512, 4 * 24576)
    assert size[(GROUP, 13, 0)] == (512, 3 * 49152)
    assert size[(PIPE, 16, 1)] == (768, 3 * 40960) and size[(PIPE, 16, 0)] == (512, 3 * 40960) and size[(GROUP, 16, 1)] == (768, 3 * 40960)
    assert size[(BIG, 7, 0)] == (512, 131072) and size[(BIG, 15, 0)] == (512, 131072)
    assert size[(F32, 3, 0)] == (256, 65536) and size[(F32, 8, 0)] == (256, 2 * 28672) and size[(F32_GROUP, 3, 0)] == (256, 65536)
