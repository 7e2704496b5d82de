"""Guard-band tests of include/egopack_topk.h: egk_topk_softmax touches only what its task list names.

The form of tests/test_gpu_bounds_class_report.py (helpers and ``Guards`` of tests/test_gpu_bounds.py are imported; nothing is
registered there): every device argument -- the logits of every head, the int64 entries, the probabilities, the log-sum-exp --
sits in a sentinel-filled window: NaN in the guard rows and in the padding columns of the logits (ld = C + one 16-byte vector; a
read beyond a window puts a NaN into the order and into the log-sum-exp), a poison index around and between the rows of ``idx``
(row stride k + 3), NaN around and between the rows of ``prob`` (row stride k + 2) and around ``lse``.  ``prob`` and ``lse`` are
each absent once.  The results must equal the host model (tests/topk_common.py), everything outside the windows must keep the
sentinel bits, and a second run on plain buffers must give the same bits.  The ledger of this header is in
tests/test_topk_cpu.py; the module imports without a GPU."""
import numpy as np
import pytest
import torch

from tests import class_report_common as CR
from tests import test_gpu_bounds as B
from tests import topk_common as TK
from tests.test_gpu_bounds import Guards, S, bf16, f32, gen, i64, ok, refused

CASES = []  # (id, function, variant dict, covers, second run on plain buffers?) -- this header's own list
POISON = -7  # around and between the rows of idx


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
    """Every entry point some case declares it covers (the ledger in tests/test_topk_cpu.py)."""
    return sorted({name for _, _, _, cov, _ in CASES for name in cov})


@case("egk_topk_softmax",
      variants=[dict(rows=44, Cs=(115, 478), k=5, dt=f32, prob=True, lse=True), dict(rows=44, Cs=(115, 478), k=5, dt=bf16, prob=False, lse=True),
                dict(rows=5, Cs=(513, 7), k=16, dt=f32, prob=True, lse=False), dict(rows=3, Cs=(1, 65, 1030), k=64, dt=bf16, prob=True, lse=True),
                dict(rows=1, Cs=(64,), k=1, dt=f32, prob=True, lse=True),
                dict(rows=0, Cs=(115, 478), k=5, dt=f32, prob=True, lse=True, plain=False)])
def topk_softmax(lib, ops, G, rows, Cs, k, dt, prob, lse):
    """Padded leading dimensions (one 16-byte vector of NaN behind every row), entries with a row stride of k + 3, probabilities
    with one of k + 2; the second head holds tie rows.  ``rows = 0``: nothing is launched and nothing is touched."""
    from egopack_amd import _lib
    g = gen(rows * 31 + sum(Cs) + k)
    n = len(Cs)
    x = [CR.logits(rows, c, g, ties=(i == 1)).to(dt) for i, c in enumerate(Cs)]
    L = [G.m(f"logits{i}", rows, c, dt, pad=B.pad_cols(dt), init=x[i]) for i, c in enumerate(Cs)]
    I = [G.m(f"idx{i}", rows, k, i64, pad=3, poison=POISON) for i in range(n)]
    P = [G.m(f"prob{i}", rows, k, f32, pad=2) for i in range(n)] if prob else [None] * n
    E = [G.v(f"lse{i}", rows, f32) for i in range(n)] if lse else [None] * n
    tasks = (_lib.TopkTask * n)()
    for i, t in enumerate(tasks):
        t.logits, t.ld, t.C, t.reserved = L[i].ptr, L[i].ld, Cs[i], 0
        t.idx, t.idx_row_stride = I[i].ptr, I[i].ld
        if prob:
            t.prob, t.prob_row_stride = P[i].ptr, P[i].ld
        if lse:
            t.lse = E[i].ptr
    call = lambda **kw: lib.egk_topk_softmax(S(), tasks, kw.get("count", n), rows, kw.get("k", k), kw.get("dtype", B.edt(dt)))
    ok(call(), "egk_topk_softmax")
    G.check()
    for i, c in enumerate(Cs):
        idx, p64, lse64 = TK.model(TK.widen(x[i]), k)
        B.same(I[i].view, torch.from_numpy(idx), f"idx{i}")
        if prob:
            B.close(P[i].view, torch.from_numpy(p64), f"prob{i}", **TK.PROB_TOL)
        if lse:
            B.close(E[i].view, torch.from_numpy(lse64), f"lse{i}", **TK.PROB_TOL)
    # refused on the host, nothing launched: the windows and the guards keep their bits
    outs = [o for o in (*I, *P, *E) if o is not None]
    before = [o.bits() for o in outs]
    refused(call(count=0), "1 .. 8 tasks")
    refused(call(count=9), "1 .. 8 tasks")
    refused(call(k=65), "k in 1 .. 64")
    refused(call(dtype=5), "unknown logits dtype")
    for name in ("logits", "idx"):
        keep = getattr(tasks[0], name)
        setattr(tasks[0], name, None)
        refused(call(), "null pointer")
        setattr(tasks[0], name, keep)
    tasks[0].C = 0
    refused(call(), "class count")
    tasks[0].C = Cs[0]
    tasks[0].ld = Cs[0] - 1
    refused(call(), "leading dimension")
    tasks[0].ld = L[0].ld
    tasks[0].idx_row_stride = k - 1
    refused(call(), "idx row stride")
    tasks[0].idx_row_stride = I[0].ld
    tasks[0].idx = I[0].ptr + 4
    refused(call(), "misaligned pointer")
    tasks[0].idx = I[0].ptr
    tasks[0].reserved = 3
    refused(call(), "reserved")
    tasks[0].reserved = 0
    G.check()
    assert all(torch.equal(a, o.bits()) for a, o in zip(before, outs)), "a refused call wrote an output"
    out = {f"idx{i}": o for i, o in enumerate(I)}
    if prob:
        out.update({f"prob{i}": o for i, o in enumerate(P)})
    if lse:
        out.update({f"lse{i}": o for i, o in enumerate(E)})
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("name,fn,variant,covers,plain", CASES, ids=[c[0] for c in CASES])
def test_bounds_topk(name, fn, variant, covers, plain):
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
