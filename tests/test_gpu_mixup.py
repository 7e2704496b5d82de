"""The two launches of include/egopack_mixup.h against the float64 models of tests/mixup_common.py.

``egk_mix_rows_multi``: f32 within 3 * 2^-24 * (|lam a| + |(1 - lam) b|) of the exact value (the three f32 roundings of the header);
rows with lam == 1, src == r or lam == 0 bit for bit; bf16 = the f32 twin's output rounded to nearest-even, bit for bit (the two
instantiations run the same three operations: round-once without a cap); every refusal, with rows == 0 too.
``egk_ce_mix_fused_multi``: loss and gradient against F.cross_entropy / autograd in float64 at the tolerances of
tests/test_gpu_kernels.py::test_cross_entropy_heads_ignore_index (the result is a convex combination of what that test bounds);
both-ignored rows and pad columns exactly 0; bf16 dlogits against the f32 twin (tests/round_once_common.py); lam == 1 bit for bit
the plain launch egk_ce_fused_multi_s on (z, a), whatever b holds."""
import ctypes as C

import pytest
import torch

from tests import mixup_common as MC
from tests import round_once_common as RO

pytestmark = pytest.mark.gpu

DEV = "cuda"
BF, F32T = torch.bfloat16, torch.float32


@pytest.fixture(scope="module")
def lib():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from egopack_amd import _lib
    return _lib.load()


def S():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def ok(rc):
    from egopack_amd import _lib
    assert rc == 0, _lib.last_error()


def refused(rc, needle):
    from egopack_amd import _lib
    assert rc == -1 and needle in _lib.last_error(), (rc, _lib.last_error())


def edt(dt):
    return MC.BF16 if dt == BF else MC.F32


def bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == F32T else torch.int16).cpu()


# ---- egk_mix_rows_multi ------------------------------------------------------------------------------------------------------------
def mix_segment(rows, cols, pad, kind, g, copy=False):
    """One segment on the host: x (bf16-representable f32), src with fixed points, lam of ``kind``."""
    x = RO.r16(torch.randn(rows, cols, generator=g) * 2)
    if copy:
        return dict(x=x, src=None, lam=None, pad=pad)
    src = torch.randperm(rows, generator=g).to(torch.int32)
    src[::4] = torch.arange(rows, dtype=torch.int32)[::4]  # fixed points
    lam = MC.lam_vector(kind, rows, g)
    if kind == "random" and rows > 2:
        lam[1], lam[2] = 1.0, 0.0
    return dict(x=x, src=src, lam=lam, pad=pad)


def run_mix(lib, segs, cols, dt):
    """The launch over ``segs`` in ``dt`` with ld = cols + pad; returns the outputs ([rows, cols] views) and the padded buffers."""
    call, outs, keep = [], [], []
    for s in segs:
        rows, ld = s["x"].shape[0], cols + s["pad"]
        xin = torch.full((max(rows, 1), ld), float("nan"), dtype=dt, device=DEV)
        xin[:rows, :cols] = s["x"].to(DEV).to(dt)
        out = torch.full((max(rows, 1), ld), 7.0, dtype=dt, device=DEV)
        src = None if s["src"] is None else s["src"].to(DEV)
        lam = None if s["lam"] is None else s["lam"].to(DEV)
        keep += [xin, src, lam]
        call.append((xin.data_ptr(), out.data_ptr(), ld, ld, rows, None if src is None else src.data_ptr(), None if lam is None else lam.data_ptr()))
        outs.append(out)
    ok(MC.call_mix_rows(lib, call, cols, edt(dt), S()))
    torch.cuda.synchronize()
    return [o[:s["x"].shape[0], :cols] for o, s in zip(outs, segs)], outs


@pytest.mark.parametrize("cols", [1, 40, 43, 1536])  # (43: whole vectors and a scalar tail)
@pytest.mark.parametrize("rows", [1, 5, 67])
@pytest.mark.parametrize("kind", [0.0, 1.0, 0.5, "random"])
def test_mix_rows_one_segment(lib, rows, cols, kind):
    g = MC.gen(1000 * rows + cols)
    for pad in (0, 8, 3):  # ld == cols; ld > cols with vector rows; ld that only guarantees element alignment
        seg = mix_segment(rows, cols, pad, kind, g)
        (o32,), (full32,) = run_mix(lib, [seg], cols, F32T)
        (o16,), _ = run_mix(lib, [seg], cols, BF)
        exact, bound = MC.mix_model(seg["x"], seg["src"], seg["lam"]), MC.mix_bound(seg["x"], seg["src"], seg["lam"])
        err = (o32.double().cpu() - exact).abs()
        assert bool((err <= bound).all()), f"pad {pad}: |out - exact| exceeds 3 * 2^-24 (|lam a| + |(1 - lam) b|) by {float((err - bound).max())}"
        own, partner = MC.copied_rows(seg["src"], seg["lam"])
        assert torch.equal(bits(o32)[own], bits(seg["x"])[own]), "lam == 1 / src == r rows are this row's bits"
        assert torch.equal(bits(o32)[partner], bits(seg["x"][seg["src"].long()])[partner]), "lam == 0 rows are the partner's bits"
        assert torch.equal(bits(o16), bits(o32.to(BF))), "bf16 = the f32 twin rounded once, bit for bit"
        assert bool((full32[:rows, cols:] == 7.0).all()), "columns [cols, ld) of x_out are not written"


@pytest.mark.parametrize("dt", [F32T, BF])
def test_mix_rows_three_segments_one_of_them_a_copy(lib, dt):
    g = MC.gen(7)
    cols = 40
    segs = [mix_segment(67, cols, 8, "random", g), mix_segment(5, cols, 8, None, g, copy=True), mix_segment(9, cols, 0, 0.5, g),
            mix_segment(0, cols, 0, 0.5, g)]
    outs, _ = run_mix(lib, segs, cols, dt)
    for i, (o, s) in enumerate(zip(outs, segs)):
        if s["src"] is None:
            assert torch.equal(bits(o), bits(s["x"].to(dt))), "a segment without src / lam is a copy"
            continue
        (alone,), _ = run_mix(lib, [s], cols, dt)
        assert torch.equal(bits(o), bits(alone)), f"segment {i}: the bits of the launch with that segment alone"
        if dt == F32T:
            err = (o.double().cpu() - MC.mix_model(s["x"], s["src"], s["lam"])).abs()
            assert bool((err <= MC.mix_bound(s["x"], s["src"], s["lam"])).all())


@pytest.mark.parametrize("rows", [0, 5])
def test_mix_rows_refusals(lib, rows):
    cols = 8
    x = torch.zeros(max(rows, 1) * 2, cols, device=DEV)
    o = torch.zeros(max(rows, 1), cols, device=DEV)
    src = torch.zeros(max(rows, 1), dtype=torch.int32, device=DEV)
    lam = torch.ones(max(rows, 1), device=DEV)
    seg = lambda **kw: (kw.get("xin", x.data_ptr()), kw.get("out", o.data_ptr()), kw.get("ld_in", cols), kw.get("ld_out", cols), kw.get("rows", rows),
                        kw.get("src", src.data_ptr()), kw.get("lam", lam.data_ptr()))
    call = lambda segs, cols_=cols, dt=MC.F32: MC.call_mix_rows(lib, segs, cols_, dt, S())
    before = bits(o).clone()
    refused(call([seg()], cols_=0), "cols must be >= 1")
    refused(call([seg(ld_in=cols - 1)]), "ld_in >= cols")
    refused(call([seg(ld_out=cols - 1)]), "ld_out >= cols")
    refused(call([seg()] * 5), "1 .. 4 segments")
    refused(call([]), "1 .. 4 segments")
    refused(call([seg()], dt=5), "unknown element dtype")
    refused(call([seg(lam=None)]), "src is given without lam")
    refused(call([seg(src=None)]), "lam is given without src")
    refused(call([seg(rows=-1)]), "rows must be >= 0")
    refused(call([seg(out=x.data_ptr())]), "out of place")                           # in place
    if rows:
        refused(call([seg(out=x.data_ptr() + 4 * cols * (rows - 1))]), "out of place")  # the last input row
        refused(call([seg(), seg(xin=o.data_ptr(), out=x.data_ptr() + 4 * cols * rows)]), "overlaps x_in of segment 1")
        refused(call([seg(), seg()]), "overlaps x_out of segment")
        refused(call([seg(xin=None)]), "null pointer")
    ok(call([seg()]))
    torch.cuda.synchronize()
    assert rows or torch.equal(bits(o), before), "rows == 0 launches nothing"


# ---- egk_ce_mix_fused_multi -------------------------------------------------------------------------------------------------------
def ce_case(rows, Cs, g, kind):
    logits = [RO.r16(torch.randn(rows, c, generator=g) * 3) for c in Cs]
    y, yb = MC.mix_labels(rows, Cs, g)
    lam = MC.lam_vector(kind, rows, g)
    if kind == "random" and rows > 2:
        lam[1], lam[2] = 1.0, 0.0
    return logits, y, yb, lam


def run_ce(lib, logits, y, yb, lam, sm, dt, gscale, scale=None, plain=False):
    """The two-target launch (``plain``: egk_ce_fused_multi_s / egk_ce_fused_multi on (z, y)) with pad = C + 3 per head, the heads'
    blocks side by side behind a spare column, logits rows 5 elements apart from the next; returns loss [rows] and dlogits."""
    from egopack_amd import _lib
    rows, Cs = y.shape[0], [l.shape[1] for l in logits]
    pads = [c + 3 for c in Cs]
    dcol = [1 + sum(pads[:h]) for h in range(len(Cs))]
    L = []
    for l in logits:
        buf = torch.full((max(rows, 1), l.shape[1] + 5), float("nan"), device=DEV)
        buf[:rows, :l.shape[1]] = l.to(DEV)
        L.append(buf)
    yd, ybd, lamd = y.to(DEV), yb.to(DEV), lam.to(DEV)
    loss = torch.full((max(rows, 1),), float("nan"), device=DEV)
    D = torch.full((max(rows, 1), 1 + sum(pads) + 2), 7.0, dtype=dt, device=DEV)
    sc = None if scale is None else torch.tensor([scale], device=DEV)
    if plain:
        arr = (_lib.CETask * 1)()
        t = arr[0]
        for h, l in enumerate(L):
            t.logits[h], t.ld[h], t.C[h], t.pad[h], t.dcol[h] = l.data_ptr(), l.stride(0), Cs[h], pads[h], dcol[h]
        t.n_heads, t.y, t.y_stride, t.loss, t.dlogits, t.ldd, t.rows, t.gscale = len(L), yd.data_ptr(), y.shape[1], loss.data_ptr(), D.data_ptr(), D.stride(0), rows, gscale
        if sc is None:
            ok(lib.egk_ce_fused_multi(S(), arr, 1, sm, edt(dt)))
        else:
            ok(lib.egk_ce_fused_multi_s(S(), arr, (C.c_void_p * 1)(sc.data_ptr()), 1, sm, edt(dt)))
    else:
        task = dict(logits=[(l.data_ptr(), l.stride(0), Cs[h], pads[h], dcol[h]) for h, l in enumerate(L)], y=yd.data_ptr(), y_b=ybd.data_ptr(),
                    y_stride=y.shape[1], lam=lamd.data_ptr(), loss=loss.data_ptr(), dlogits=D.data_ptr(), ldd=D.stride(0), rows=rows,
                    gscale=gscale, scale=None if sc is None else sc.data_ptr())
        ok(MC.call_ce_mix(lib, [task], sm, edt(dt), S()))
    torch.cuda.synchronize()
    return loss[:rows].cpu(), D[:rows].cpu(), dcol, pads


CE_CLASSES = [(2, 115), (478, 513)]  # two heads each; 513 crosses a 512-class chunk of the lane walk


@pytest.mark.parametrize("scale", [None, 0.7])
@pytest.mark.parametrize("kind", [0.0, 1.0, 0.3, "random"])
@pytest.mark.parametrize("sm", [0.0, 0.1])
@pytest.mark.parametrize("rows", [1, 5, 67])
@pytest.mark.parametrize("Cs", CE_CLASSES)
def test_ce_mix_against_float64(lib, Cs, rows, sm, kind, scale):
    g = MC.gen(rows * 31 + Cs[1])
    logits, y, yb, lam = ce_case(rows, Cs, g, kind)
    gscale = 0.37
    geff = gscale if scale is None else float(torch.tensor(gscale) * torch.tensor(scale))
    ref_loss, ref_grad = MC.ce_mix_model(logits, y, yb, lam, sm, geff)
    loss, D, dcol, pads = run_ce(lib, logits, y, yb, lam, sm, F32T, gscale, scale)
    # tests/test_gpu_kernels.py::test_cross_entropy_heads_ignore_index
    torch.testing.assert_close(loss.double(), ref_loss, rtol=1e-5, atol=1e-5)
    for h, c in enumerate(Cs):
        torch.testing.assert_close(D[:, dcol[h]:dcol[h] + c].double(), ref_grad[h], rtol=1e-4, atol=1e-6)
        assert not bool(D[:, dcol[h] + c:dcol[h] + pads[h]].ne(0).any()), "pad columns [C, pad) are exactly 0"
    assert bool((D[:, 0] == 7.0).all()) and bool((D[:, dcol[-1] + pads[-1]:] == 7.0).all()), "columns outside the heads' blocks are not written"
    dead = torch.tensor([all(not (0 <= int(v[n, h]) < Cs[h]) for h in range(2) for v in (y, yb)) for n in range(rows)])
    if bool(dead.any()):
        assert not bool(loss[dead].ne(0).any()), "both labels ignored in every head: loss exactly 0"
        assert not bool(D[dead][:, dcol[0]:dcol[-1] + pads[-1]].ne(0).any()), "both labels ignored: gradient exactly 0"
    # bf16 dlogits: one of the two bf16 neighbours of the f32 twin, at most 1 % not the nearest (tests/test_gpu_round_once.py)
    loss16, D16, _, _ = run_ce(lib, logits, y, yb, lam, sm, BF, gscale, scale)
    assert torch.equal(bits(loss16), bits(loss)), "the loss is f32 in both instantiations"
    for h, c in enumerate(Cs):
        RO.check_round_once(D16[:, dcol[h]:dcol[h] + pads[h]].contiguous(), D[:, dcol[h]:dcol[h] + pads[h]].contiguous(), f"dlogits head {h}")


@pytest.mark.parametrize("dt", [F32T, BF])
@pytest.mark.parametrize("scale", [None, 0.7])
@pytest.mark.parametrize("sm", [0.0, 0.1])
@pytest.mark.parametrize("rows", [1, 5, 67])
@pytest.mark.parametrize("Cs", CE_CLASSES)
def test_ce_mix_lam_one_is_the_plain_launch_bit_for_bit(lib, Cs, rows, sm, scale, dt):
    g = MC.gen(rows * 17 + Cs[0])
    logits, y, yb, _ = ce_case(rows, Cs, g, 1.0)
    lam = torch.ones(rows)
    for gscale in (0.37, -0.01):
        loss, D, _, _ = run_ce(lib, logits, y, yb, lam, sm, dt, gscale, scale)
        ploss, PD, _, _ = run_ce(lib, logits, y, yb, lam, sm, dt, gscale, scale, plain=True)
        assert torch.equal(bits(loss), bits(ploss)), "loss: lam == 1 is egk_ce_fused_multi_s on (z, a)"
        assert torch.equal(bits(D), bits(PD)), "dlogits: lam == 1 is egk_ce_fused_multi_s on (z, a)"
        # and lam == 0 is the plain launch on (z, b)
        loss0, D0, _, _ = run_ce(lib, logits, y, yb, torch.zeros(rows), sm, dt, gscale, scale)
        bloss, BD, _, _ = run_ce(lib, logits, yb, y, lam, sm, dt, gscale, scale, plain=True)
        assert torch.equal(bits(loss0), bits(bloss)) and torch.equal(bits(D0), bits(BD)), "lam == 0 is the plain launch on (z, b)"


def test_ce_mix_two_tasks_in_one_launch_and_refusals(lib):
    g = MC.gen(3)
    A, B = ce_case(67, (115, 478), g, "random"), ce_case(5, (20,), g, 0.3)
    # one launch with both tasks gives each task's bits alone
    keep, tasks, outs = [], [], []
    for logits, y, yb, lam in (A, B):
        rows = y.shape[0]
        L = [l.to(DEV).contiguous() for l in logits]
        yd, ybd, lamd = y.to(DEV), yb.to(DEV), lam.to(DEV)
        loss = torch.empty(rows, device=DEV)
        width = sum(l.shape[1] for l in L)
        D = torch.empty(rows, width, device=DEV)
        dcol = [sum(l.shape[1] for l in L[:h]) for h in range(len(L))]
        keep += [L, yd, ybd, lamd]
        tasks.append(dict(logits=[(l.data_ptr(), l.stride(0), l.shape[1], l.shape[1], dcol[h]) for h, l in enumerate(L)], y=yd.data_ptr(),
                          y_b=ybd.data_ptr(), y_stride=y.shape[1], lam=lamd.data_ptr(), loss=loss.data_ptr(), dlogits=D.data_ptr(), ldd=width,
                          rows=rows, gscale=0.5, scale=None))
        outs.append((loss, D))
    ok(MC.call_ce_mix(lib, tasks, 0.1, MC.F32, S()))
    torch.cuda.synchronize()
    both = [(bits(l).clone(), bits(d).clone()) for l, d in outs]
    for i in range(2):
        outs[i][0].fill_(9.0)
        outs[i][1].fill_(9.0)
        ok(MC.call_ce_mix(lib, [tasks[i]], 0.1, MC.F32, S()))
        torch.cuda.synchronize()
        assert torch.equal(bits(outs[i][0]), both[i][0]) and torch.equal(bits(outs[i][1]), both[i][1]), f"task {i}"
        ref_loss, ref_grad = MC.ce_mix_model((A, B)[i][0], (A, B)[i][1], (A, B)[i][2], (A, B)[i][3], 0.1, 0.5)
        torch.testing.assert_close(outs[i][0].cpu().double(), ref_loss, rtol=1e-5, atol=1e-5)
        torch.testing.assert_close(outs[i][1].cpu().double(), torch.cat(ref_grad, 1), rtol=1e-4, atol=1e-6)
    t = tasks[1]
    for zero in (False, True):
        base = dict(t, rows=0) if zero else t
        call = lambda **kw: MC.call_ce_mix(lib, [dict(base, **kw)], 0.0, MC.F32, S())
        refused(call(y_b=None), "null pointer (y or y_b")
        refused(call(lam=None), "null pointer (lam")
        refused(call(loss=None), "null pointer (loss or dlogits")
        refused(call(rows=-1), "rows must be >= 0")
        refused(call(logits=[]), "1 .. 4 heads")
        refused(call(logits=[(t["logits"][0][0], 20, 0, 0, 0)]), "C must be >= 1")
        refused(call(logits=[(t["logits"][0][0], 20, 20, 19, 0)]), "pad must be >= C")
        refused(call(logits=[(None, 20, 20, 20, 0)]), "null pointer (logits")
        refused(call(lam=t["lam"] + 2), "not 4-byte aligned")
        refused(MC.call_ce_mix(lib, [base] * 5, 0.0, MC.F32, S()), "1 .. 4 tasks")
        refused(MC.call_ce_mix(lib, [base], 0.0, 9, S()), "unknown activation dtype")


@pytest.mark.parametrize("dt", [F32T, BF])
def test_ce_mix_scale_beside_null_scale_in_one_launch(lib, dt):
    """Two tasks in ONE two-target launch, the first with a scale word, the second with NULL in ``scales`` (the _s launches refuse
    such an entry; this one takes it as "no scale"): each task has the bits of its own single-task launch."""
    g = MC.gen(11)
    cases = (ce_case(67, (115, 478), g, "random"), ce_case(5, (20,), g, 0.3))
    sc = torch.tensor([0.7], device=DEV)
    keep, tasks, outs = [sc], [], []
    for i, (logits, y, yb, lam) in enumerate(cases):
        rows = y.shape[0]
        L = [l.to(DEV).contiguous() for l in logits]
        yd, ybd, lamd = y.to(DEV), yb.to(DEV), lam.to(DEV)
        loss = torch.empty(rows, device=DEV)
        width = sum(l.shape[1] for l in L)
        D = torch.empty(rows, width, dtype=dt, device=DEV)
        dcol = [sum(l.shape[1] for l in L[:h]) for h in range(len(L))]
        keep += [L, yd, ybd, lamd]
        tasks.append(dict(logits=[(l.data_ptr(), l.stride(0), l.shape[1], l.shape[1], dcol[h]) for h, l in enumerate(L)], y=yd.data_ptr(),
                          y_b=ybd.data_ptr(), y_stride=y.shape[1], lam=lamd.data_ptr(), loss=loss.data_ptr(), dlogits=D.data_ptr(), ldd=width,
                          rows=rows, gscale=0.37, scale=sc.data_ptr() if i == 0 else None))
        outs.append((loss, D))
    ok(MC.call_ce_mix(lib, tasks, 0.1, edt(dt), S()))
    torch.cuda.synchronize()
    both = [(bits(l).clone(), bits(d).clone()) for l, d in outs]
    for i in range(2):
        outs[i][0].fill_(9.0)
        outs[i][1].fill_(9.0)
        ok(MC.call_ce_mix(lib, [tasks[i]], 0.1, edt(dt), S()))
        torch.cuda.synchronize()
        assert torch.equal(bits(outs[i][0]), both[i][0]) and torch.equal(bits(outs[i][1]), both[i][1]), f"task {i}"
    # the scale reached the first task and only it: the second task's loss-independent gradient is the unscaled launch's
    geff = float(torch.tensor(0.37) * torch.tensor(0.7))
    for i, gs in enumerate((geff, 0.37)):
        _, ref_grad = MC.ce_mix_model(cases[i][0], cases[i][1], cases[i][2], cases[i][3], 0.1, gs)
        # f32: the bar of test_ce_mix_against_float64; bf16: that plus one rounding to 8 significant bits, 1e-4 + 2^-9 < 2^-8
        tol = dict(rtol=1e-4, atol=1e-6) if dt == F32T else dict(rtol=2.0 ** -8, atol=1e-6)
        torch.testing.assert_close(outs[i][1].cpu().double(), torch.cat(ref_grad, 1), **tol)
