"""Guard-band tests of include/egopack_class_report.h: egk_class_report touches only what its task list names.

The form of tests/test_gpu_bounds_lta_sampling.py (helpers and ``Guards`` of tests/test_gpu_bounds.py are imported; nothing is
registered there): every device argument -- the logits of every head, the labels read at stride 2, the four int64 accumulators
-- sits in a sentinel-filled window: NaN in the guard rows and in the padding columns of the logits (a read beyond a window
changes the ranking or makes the loss non-finite), a poison label (-5: a row that reads it counts as ignored) around and between
the labels, a poison value around the accumulators.  The accumulators are pre-filled with a known non-zero pattern, since the
kernel ADDS: the results must equal the host model (tests/class_report_common.py) plus the pre-fill, everything outside the
windows must keep the sentinel bits, and a second run on plain buffers must give the same bits.  The ledger of this header is in
tests/test_class_report_cpu.py; the module imports without a GPU."""
import numpy as np
import pytest
import torch

from tests import class_report_common as CR
from tests import test_gpu_bounds as B
from tests.test_gpu_bounds import Guards, S, f32, gen, i64, ok, refused

CASES = []  # (id, function, variant dict, covers, second run on plain buffers?) -- this header's own list
POISON = -7      # around the int64 accumulators
BAD_LABEL = -5   # around and between the labels: an ignored row
FILL = 1000003   # what the accumulators hold before the call


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
    """Every entry point some case declares it covers (the ledger in tests/test_class_report_cpu.py)."""
    return sorted({name for _, _, _, cov, _ in CASES for name in cov})


@case("egk_class_report",
      variants=[dict(rows=(44, 44), Cs=(115, 478), opt=True), dict(rows=(3,), Cs=(1,), opt=True), dict(rows=(7,), Cs=(65,), opt=True),
                dict(rows=(0, 0), Cs=(115, 478), opt=True, plain=False), dict(rows=(44, 5), Cs=(115, 513), opt=False)])
def class_report(lib, ops, G, rows, Cs, opt):
    """Padded leading dimensions (one 16-byte vector of NaN behind every row), labels in column 0 of an [N, 2] table.  ``opt``:
    with the optional top2 / loss_q24 outputs; without them the two pointers are null.  ``rows = 0``: nothing is launched and
    nothing is touched."""
    from egopack_amd import _lib
    g = gen(sum(rows) * 31 + sum(Cs))
    n = len(Cs)
    x = [CR.logits(r, c, g, ties=(i == 1)) for i, (r, c) in enumerate(zip(rows, Cs))]
    y = [CR.labels(r, c, g) for r, c in zip(rows, Cs)]
    L = [G.m(f"logits{i}", rows[i], Cs[i], f32, pad=B.pad_cols(f32), init=x[i]) for i in range(n)]
    Y = [G.v(f"labels{i}", rows[i] * 2, i64, init=y[i], poison=BAD_LABEL) for i in range(n)]
    fill = lambda *shape: torch.full(shape, FILL, dtype=i64)
    CF = [G.m(f"confusion{i}", c, c, i64, init=fill(c, c), poison=POISON) for i, c in enumerate(Cs)]
    T2 = [G.m(f"top2_{i}", c, c, i64, init=fill(c, c), poison=POISON) for i, c in enumerate(Cs)] if opt else [None] * n
    LQ = [G.v(f"loss_q24_{i}", c, i64, init=fill(c), poison=POISON) for i, c in enumerate(Cs)] if opt else [None] * n
    CN = [G.v(f"counts{i}", 4, i64, init=fill(4), poison=POISON) for i in range(n)]
    tasks = (_lib.ClassReportTask * n)()
    for i, t in enumerate(tasks):
        t.logits, t.ld, t.labels, t.label_stride, t.rows, t.C = L[i].ptr, L[i].ld, Y[i].ptr, 2, rows[i], Cs[i]
        t.confusion, t.counts = CF[i].ptr, CN[i].ptr
        t.top2, t.loss_q24 = (T2[i].ptr, LQ[i].ptr) if opt else (None, None)
    call = lambda **kw: lib.egk_class_report(S(), tasks, kw.get("count", n))
    ok(call(), "egk_class_report")
    G.check()
    for i in range(n):
        loss = None
        if rows[i]:  # the per-row loss of the library's cross entropy on the same window
            with torch.no_grad():
                loss = ops.cross_entropy(L[i].view, Y[i].view.view(rows[i], 2)[:, 0]).cpu().numpy()
        conf, top2, q24, counts = CR.model(x[i].numpy(), y[i][:, 0].numpy(), loss)
        B.same(CF[i].view, torch.from_numpy(conf) + FILL, f"confusion{i}")
        B.same(CN[i].view, torch.from_numpy(counts) + FILL, f"counts{i}")
        if opt:
            B.same(T2[i].view, torch.from_numpy(top2) + FILL, f"top2_{i}")
            B.same(LQ[i].view, torch.from_numpy(q24) + FILL, f"loss_q24_{i}")
    # refused on the host, nothing launched: the windows and the guards keep their bits
    outs = [o for o in (*CF, *T2, *LQ, *CN) if o is not None]
    before = [o.bits() for o in outs]
    refused(call(count=0), "1 .. 8 tasks")
    refused(call(count=9), "1 .. 8 tasks")
    for name in ("logits", "labels", "confusion", "counts"):
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
    tasks[0].confusion = CF[0].ptr + 4
    refused(call(), "misaligned pointer")
    tasks[0].confusion = CF[0].ptr
    G.check()
    assert all(torch.equal(a, o.bits()) for a, o in zip(before, outs)), "a refused call changed an accumulator"
    out = {f"confusion{i}": o for i, o in enumerate(CF)}
    out.update({f"counts{i}": o for i, o in enumerate(CN)})
    if opt:
        out.update({f"top2_{i}": o for i, o in enumerate(T2)})
        out.update({f"loss_q24_{i}": o for i, o in enumerate(LQ)})
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("name,fn,variant,covers,plain", CASES, ids=[c[0] for c in CASES])
def test_bounds_class_report(name, fn, variant, covers, plain):
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
