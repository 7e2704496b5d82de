"""The cache policy of the optimizer launches' single-use streams (egk_tune 9, egopack_amd/csrc/optim_rules.hip: NT_*) changes no bit.

Every mask bit alone, the shipped mask (7) and all bits together against mask 0: Adam / AdamW / SGD with momentum, f32 and bf16 state,
the plain, grouped and moving-average entry points and egk_adam_step, on n = 1024 + 3 elements (one block of 16-byte accesses and a
scalar tail) and on a slice that starts at an odd multiple of four elements.  Every buffer a launch writes is compared bit for bit."""
import ctypes as C

import pytest
import torch

from tests import test_gpu_optim_state as OSG

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF = torch.bfloat16
N = 1024 + 3
MASKS = [1, 2, 4, 8, 7, 15]


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


@pytest.fixture
def lib():
    from egopack_amd import _lib
    lib = _lib.load()
    shipped = lib.egk_tune(9, 0)
    lib.egk_tune(9, shipped)
    yield lib
    lib.egk_tune(9, shipped)


def _tables(elem0, three):
    """The segment table over absolute elements [0, elem0 + N): one group, or three whose two boundaries (elements 500 and 900 of the
    launch) lie inside its one 1024-element block, so that lanes of one workgroup take their constants from different groups."""
    ends = [elem0 + 500, elem0 + 900, elem0 + N] if three else [elem0 + N]
    begin = torch.tensor([0, *ends], dtype=torch.int64, device=DEV)
    group = torch.tensor([2, 0, 1] if three else [0], dtype=torch.int32, device=DEV)
    rows = [(1e-2, 1e-2), (3e-3, 0.0), (1e-3, 2e-2)] if three else [(1e-2, 1e-2)]
    hyper = torch.zeros(len(rows), 4, device=DEV)
    hyper[:, :2] = torch.tensor(rows)
    return begin, group, hyper


def _run(lib, mask, rule, sd, door, three, lo, gdt=torch.float32):
    prev = lib.egk_tune(9, mask)
    try:
        assert lib.egk_tune(9, mask) == mask, "the mask is one of the instantiated ones"
        prob = OSG.Problem(rule, N, gdt)
        elem0 = 4096
        table = _tables(elem0, three) if door != "plain" or three else None
        entry = "ema" if door == "ema" else "groups" if table is not None else "plain"
        side = OSG.Side(prob, sd, ema=entry == "ema")
        side.launch(lo, N, elem0=elem0, mode=1, door=entry, table=table if (entry != "ema" or three) else None)
        return side.out()
    finally:
        lib.egk_tune(9, prev)


# "odd base": the launch starts 12 elements into the buffers, so the group table's ``base`` is 4108 = 4 x 1027, an ODD multiple of the
# four elements every base must be a multiple of (16-byte accesses), and every element sits in another lane than in the whole launch
@pytest.mark.parametrize("lo", [0, 12], ids=["whole", "odd_base"])
@pytest.mark.parametrize("door,three", [("plain", False), ("groups", True), ("ema", False), ("ema", True)],
                         ids=["plain", "groups3", "ema", "ema_groups3"])
@pytest.mark.parametrize("sd", [torch.float32, BF], ids=["state_f32", "state_bf16"])
@pytest.mark.parametrize("rule", list(OSG.RULES))
def test_every_stream_policy_stores_the_bits_of_the_default(lib, rule, sd, door, three, lo):
    want = _run(lib, 0, rule, sd, door, three, lo)
    for mask in MASKS:
        got = _run(lib, mask, rule, sd, door, three, lo)
        assert got.keys() == want.keys()
        for k in want:
            OSG.same(got[k], want[k], f"{rule} mask {mask}: {k}")


def test_a_bf16_gradient_and_the_adam_entry_point(lib):
    """egk_optim_step on a bf16 gradient, and egk_adam_step_bump (the launch of the flagship step) with both gradient types."""
    want = _run(lib, 0, "adam", torch.float32, "plain", False, 0, gdt=BF)
    for mask in MASKS:
        got = _run(lib, mask, "adam", torch.float32, "plain", False, 0, gdt=BF)
        for k in want:
            OSG.same(got[k], want[k], f"bf16 gradient, mask {mask}: {k}")

    def adam(mask, gdt):
        prev = lib.egk_tune(9, mask)
        try:
            prob = OSG.Problem("adam", N, gdt)
            s = OSG.Side(prob, torch.float32)
            rc = lib.egk_adam_step_bump(OSG.S(), s.p.data_ptr(), s.g.data_ptr(), 1 if gdt == BF else 0, s.s0.data_ptr(), s.s1.data_ptr(), N,
                                        s.hyper.data_ptr(), 0.9, 0.999, 1e-8, 1e-2, s.hi.data_ptr(), s.lo.data_ptr(), s.word.data_ptr(), 7)
            assert rc == 0
            return s.out()
        finally:
            lib.egk_tune(9, prev)
    for gdt in (torch.float32, BF):
        want = adam(0, gdt)
        for mask in MASKS:
            got = adam(mask, gdt)
            for k in want:
                OSG.same(got[k], want[k], f"egk_adam_step_bump {gdt} mask {mask}: {k}")


def test_a_mask_that_is_not_instantiated_leaves_the_policy(lib):
    shipped = lib.egk_tune(9, 3)
    assert shipped == 7, "the shipped policy: loads of g, p and the state and their stores non-temporal, the average left alone"
    assert lib.egk_tune(9, 5) == 3 and lib.egk_tune(9, 16) == 3 and lib.egk_tune(9, -1) == 3
    assert lib.egk_tune(9, shipped) == 3
