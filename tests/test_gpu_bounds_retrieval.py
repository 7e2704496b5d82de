"""Guard-band tests of include/egopack_retrieval.h: egk_retrieval_report touches only what its task list names.

The form of tests/test_gpu_bounds_topk.py (helpers and ``Guards`` of tests/test_gpu_bounds.py are imported; nothing is registered
there): every device argument -- the searched features, the activation features, the bank, the index lists, the distances, the
wins -- sits in a sentinel-filled window: NaN in the guard rows and in the padding columns of the three matrices (ld = H + one
16-byte vector; a read beyond a window puts a NaN into a distance, and into a channel's comparison), the banks carry one poison row
of NaN (number K) that the sentinel of ``nn`` names (row stride k + 3; every entry of the window itself stays in 0 .. K - 1), NaN
around and between the rows of ``dist`` (row stride k + 2), a poison count around and between the rows of ``wins`` (row stride
k + 1 + 3).  ``dist`` and ``wins`` are each absent once.  The results must equal the host model (tests/retrieval_common.py),
everything outside the windows must keep the sentinel bits -- the gap between k and a wider row stride included --, every refused
call must leave the outputs alone, and a second run on plain buffers must give the same bits.  The ledger of this header is in
tests/test_retrieval_cpu.py; the module imports without a GPU."""
import numpy as np
import pytest
import torch

from tests import retrieval_common as RC
from tests import test_gpu_bounds as B
from tests.test_gpu_bounds import Guards, S, bf16, f32, gen, i32, i64, ok, refused

CASES = []  # (id, function, variant dict, covers, second run on plain buffers?) -- this header's own list
POISON = -7  # around and between the rows of wins


def case(*covers, variants=None, plain=True):
    def deco(fn):
        for v in variants or [dict()]:
            v = dict(v)
            second = v.pop("plain", plain)
            vid = v.pop("id", None) or "-".join(f"{k}={B._fmt(x)}" for k, x in v.items())
            CASES.append((fn.__name__ + ("-" + vid if vid else ""), fn, v, covers, second))
        fn.covers = covers
        return fn
    return deco


def covered():
    """Every entry point some case declares it covers (the ledger in tests/test_retrieval_cpu.py)."""
    return sorted({name for _, _, _, cov, _ in CASES for name in cov})


@case("egk_retrieval_report",
      variants=[dict(rows=67, H=200, k=4, Ks=(37, 500, 4), dt=bf16, distance=0, dist=True, wins=True),
                dict(rows=5, H=1024, k=32, Ks=(32,), dt=f32, distance=1, dist=True, wins=True),
                dict(rows=44, H=64, k=4, Ks=(37, 57), dt=f32, distance=0, dist=False, wins=True),
                dict(rows=44, H=64, k=4, Ks=(37, 57), dt=bf16, distance=1, dist=True, wins=False),
                dict(rows=1, H=8, k=1, Ks=(1,), dt=f32, distance=0, dist=True, wins=True),
                dict(rows=3, H=7, k=2, Ks=(5, 9), dt=bf16, distance=0, dist=True, wins=True),
                dict(rows=0, H=64, k=4, Ks=(37, 57), dt=f32, distance=0, dist=True, wins=True, plain=False)])
def retrieval_report(lib, ops, G, rows, H, k, Ks, dt, distance, dist, wins):
    """Padded leading dimensions (one 16-byte vector of NaN behind every row), index lists with a row stride of k + 3, distances with
    one of k + 2, wins with one of k + 4.  ``rows = 0``: nothing is launched and nothing is touched."""
    from egopack_amd import _lib
    g = gen(rows * 31 + H + sum(Ks) + k)
    n = len(Ks)
    f = [torch.randn(rows, H, generator=g) for _ in Ks]
    fa = [torch.randn(rows, H, generator=g).to(dt) for _ in Ks]
    bank = [torch.randn(K, H, generator=g) for K in Ks]
    nn = [RC.lists(rows, K, k, g) for K in Ks]
    nan_row = torch.full((1, H), float("nan"))
    Fm = [G.m(f"f{i}", rows, H, f32, pad=B.pad_cols(f32), init=f[i]) for i in range(n)]
    Am = [G.m(f"f_act{i}", rows, H, dt, pad=B.pad_cols(dt), init=fa[i]) for i in range(n)]
    Bm = [G.m(f"bank{i} (+ poison row)", K + 1, H, f32, pad=B.pad_cols(f32), init=torch.cat([bank[i], nan_row])) for i, K in enumerate(Ks)]
    Nm = [G.m(f"nn{i}", rows, k, i64, pad=3, init=nn[i], poison=K) for i, K in enumerate(Ks)]
    Dm = [G.m(f"dist{i}", rows, k, f32, pad=2) for i in range(n)] if dist else [None] * n
    Wm = [G.m(f"wins{i}", rows, k + 1, i32, pad=3, poison=POISON) for i in range(n)] if wins else [None] * n
    tasks = (_lib.RetrievalTask * n)()
    for i, t in enumerate(tasks):
        t.f, t.f_ld, t.f_act, t.f_act_ld, t.bank, t.bank_ld = Fm[i].ptr, Fm[i].ld, Am[i].ptr, Am[i].ld, Bm[i].ptr, Bm[i].ld
        t.K, t.reserved, t.nn, t.nn_row_stride = Ks[i], 0, Nm[i].ptr, Nm[i].ld
        if dist:
            t.dist, t.dist_row_stride = Dm[i].ptr, Dm[i].ld
        if wins:
            t.wins, t.wins_row_stride = Wm[i].ptr, Wm[i].ld
    call = lambda **kw: lib.egk_retrieval_report(S(), tasks, kw.get("count", n), kw.get("rows", rows), kw.get("H", H), kw.get("k", k),
                                                 kw.get("distance", distance), kw.get("dtype", B.edt(dt)))
    ok(call(), "egk_retrieval_report")
    G.check()
    name = ("cosine", "l2")[distance]
    for i in range(n):
        if wins:
            B.same(Wm[i].view, torch.from_numpy(RC.wins_model(RC.widen(fa[i]), RC.widen(bank[i]), nn[i].numpy())), f"wins{i}")
        if dist and rows:
            ref = RC.dist_model(RC.widen(f[i]), RC.widen(bank[i]), nn[i].numpy(), name)
            err = np.abs(Dm[i].view.cpu().numpy().astype(np.float64) - ref) / (ref if distance else 1.0)
            assert float(err.max()) <= RC.dist_bound(H), (f"dist{i}", float(err.max()), RC.dist_bound(H))
    # refused on the host, nothing launched: the windows and the guards keep their bits
    outs = [o for o in (*Dm, *Wm) if o is not None]
    before = [o.bits() for o in outs]
    refused(call(count=0), "1 .. 8 tasks")
    refused(call(count=9), "1 .. 8 tasks")
    refused(call(rows=-1), "rows >= 0")
    refused(call(H=0), "H >= 1")
    refused(call(k=0), "k in 1 .. 32")
    refused(call(k=33), "k in 1 .. 32")
    refused(call(distance=2), "unknown distance")
    refused(call(dtype=5), "unknown f_act dtype")
    t0 = tasks[0]

    def with_field(field, value, needle):
        keep = getattr(t0, field)
        setattr(t0, field, value)
        try:
            refused(call(), needle)
        finally:
            setattr(t0, field, keep)

    for field in ("f", "f_act", "bank", "nn"):
        with_field(field, None, "null pointer")
    with_field("K", 0, "bank rows")
    with_field("reserved", 3, "reserved")
    for field in ("f_ld", "f_act_ld", "bank_ld"):
        with_field(field, H - 1, "leading dimension")
    with_field("nn_row_stride", k - 1, "nn row stride")
    with_field("nn", Nm[0].ptr + 4, "misaligned pointer")
    with_field("f", Fm[0].ptr + 2, "misaligned pointer")
    with_field("bank", Bm[0].ptr + 2, "misaligned pointer")
    with_field("f_act", Am[0].ptr + 1, "misaligned pointer")
    if dist:
        with_field("dist_row_stride", k - 1, "dist row stride")
        with_field("dist", Dm[0].ptr + 2, "misaligned pointer")
    if wins:
        with_field("wins_row_stride", k, "wins row stride")
        with_field("wins", Wm[0].ptr + 2, "misaligned pointer")
    keep = (t0.dist, t0.wins)
    t0.dist, t0.wins = None, None
    try:
        refused(call(), "both null")
    finally:
        t0.dist, t0.wins = keep
    G.check()
    assert all(torch.equal(a, o.bits()) for a, o in zip(before, outs)), "a refused call wrote an output"
    out = {}
    if dist:
        out.update({f"dist{i}": o for i, o in enumerate(Dm)})
    if wins:
        out.update({f"wins{i}": o for i, o in enumerate(Wm)})
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("name,fn,variant,covers,plain", CASES, ids=[c[0] for c in CASES])
def test_bounds_retrieval(name, fn, variant, covers, plain):
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from egopack_amd import _lib, ops
    lib = _lib.load()
    try:
        G = Guards()
        out = fn(lib, ops, G, **variant)
        G.check()
        if plain and out:
            got = {k: B._bits(v) for k, v in out.items()}
            H = Guards(plain=True)
            base = fn(lib, ops, H, **variant)
            torch.cuda.synchronize()
            for k, v in base.items():
                b = B._bits(v)
                assert got[k].shape == b.shape and torch.equal(got[k], b), f"{k}: the guarded call and the contiguous call differ in bits"
    finally:
        torch.cuda.synchronize()
