"""The shaped cross entropy on the GPU (the tail of egk_ce_task, include/egopack_hip.h; ops.cross_entropy(margin=, gamma=);
DESIGN.md 3.17): parity with float64 autograd -- F.cross_entropy on z, times (1 - softmax(z)[t])^gamma (tests/ce_shape_common.py) --
the bits of the multi-task launch, of the stand-alone forward + backward pair, of the bf16 operand and of strided logits, "zero
tail is today's launch", and the terms off and on in the multi-task step (eager and captured).

Tolerances (tests/ce_shape_common.py, measured on the CPU by tests/test_ce_shape_cpu.py).  gamma = 0: the project's cross-entropy
tolerances, loss rtol 1e-5 / atol 1e-5, gradient rtol 1e-4 / atol 1e-6.  gamma > 0: the numpy f32 restatement of the arithmetic does
not stay inside them against float64 on these inputs (largest error: loss 1.84e-4, gradient 2.02e-5, both on the row whose q
rounds to 1 in f32: lse - z_t is 0 there, so 1 - q is 0 where float64 has ~1e-11, and (1 - q)^0.5 S with S ~ 30 is ~1e-4), so the
bound is 4 x that error, absolute: loss 7.36e-4, gradient 8.08e-5 for seeds |g| <= 1.  Entries where float64 itself has no finite
value are asserted as ``ce_shape_common.check`` says."""
import ctypes as C

import pytest
import torch

from tests import ce_shape_common as S

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF = torch.bfloat16


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


@pytest.fixture
def compute_restored():
    from egopack_amd import ops
    prev = ops.get_compute()
    yield
    ops.set_compute(prev)


def _dev(vs):
    return None if vs is None or all(v is None for v in vs) else tuple(None if v is None else v.to(DEV) for v in vs)


# ---- 1. parity against float64 autograd, through ops.cross_entropy outside a step (the stand-alone form) -------------------------------
@pytest.mark.parametrize("gamma", S.GAMMAS)
@pytest.mark.parametrize("eps", S.EPS)
@pytest.mark.parametrize("heads", S.HEADS, ids=S.HEAD_IDS)
def test_loss_and_gradient_match_float64_autograd(heads, eps, gamma):
    """Margin / weight / offset present in each combination.  (Fails without the feature: ``cross_entropy() got an unexpected
    keyword argument 'margin'``.)"""
    from egopack_amd import ops
    logits, y, gloss = S.problem(heads)
    worst = [0.0, 0.0]
    for presence in S.PRESENCE:
        ms, ws, offs = S.vectors(heads, presence)
        dl = [l.to(DEV).requires_grad_(True) for l in logits]
        with ops.compute_mode("f32"):
            loss = ops.cross_entropy(tuple(dl), y.to(DEV), eps, weight=_dev(ws), offset=_dev(offs), margin=_dev(ms), gamma=gamma)
            loss.backward(gloss.to(DEV))
        # the per-head losses: one head at a time (a single head also takes one tensor per argument)
        total = torch.zeros(S.ROWS, dtype=torch.float64)
        for h, l in enumerate(dl):
            with ops.compute_mode("f32"):
                one = ops.cross_entropy(l.detach(), y[:, h].contiguous().to(DEV), eps, weight=None if ws[h] is None else ws[h].to(DEV),
                                        offset=None if offs[h] is None else offs[h].to(DEV),
                                        margin=None if ms[h] is None else ms[h].to(DEV), gamma=gamma)
            el, eg = S.check(one, l.grad, logits[h], y[:, h], ws[h], offs[h], ms[h], eps, gamma, gloss, what=f"head {h} {presence}")
            worst = [max(worst[0], el), max(worst[1], eg)]
            total += one.detach().cpu().double()
        if len(heads) == 1:
            assert torch.equal(_bits(one), _bits(loss.detach()))   # (bits: the row with S = inf can be nan)
        else:  # the row's loss is the sum over the heads (f32: one rounding per addition)
            fin = torch.isfinite(total)
            torch.testing.assert_close(loss.detach().cpu().double()[fin], total[fin], rtol=1e-6, atol=1e-6)
    print(f"heads {heads} eps {eps} gamma {gamma}: max |loss error| {worst[0]:.3e}, max |gradient error| {worst[1]:.3e}")


def test_all_off_issues_the_launches_of_today():
    from egopack_amd import _lib, ops
    from tests.test_gpu_bounds import _counted
    logits, y, gloss = S.problem((115, 478))
    dl = [l.to(DEV).requires_grad_(True) for l in logits]
    with _counted(_lib.load()) as c:
        loss = ops.cross_entropy(tuple(dl), y.to(DEV), 0.1, margin=(None, None), gamma=0.0)
        loss.backward(gloss.to(DEV))
    assert c.names == {"ce_fwd": 2, "ce_bwd": 2}, c.names
    assert torch.equal(ops.cross_entropy(tuple(l.detach() for l in dl), y.to(DEV), 0.1), loss.detach())
    with _counted(_lib.load()) as c:  # on: ONE forward-only launch for both heads, one launch per head in backward; no torch arithmetic
        loss = ops.cross_entropy(tuple(dl), y.to(DEV), 0.1, gamma=2.0)
        loss.backward(gloss.to(DEV))
    assert c.names == {"ce_balanced": 3}, c.names


def test_bad_margins_and_gamma_raise_naming_the_head():
    from egopack_amd import ops
    logits, y, _ = S.problem((115, 478))
    dl, yd = tuple(l.to(DEV) for l in logits), y.to(DEV)
    m = [S.ldam(115).to(DEV), S.ldam(478).to(DEV)]
    with pytest.raises(ValueError, match="head 1"):
        ops.cross_entropy(dl, yd, margin=(m[0], m[1][:-1]))
    with pytest.raises(ValueError, match="head 0"):
        ops.cross_entropy(dl, yd, margin=(m[0].double(), None))
    with pytest.raises(ValueError, match="head 1"):
        ops.cross_entropy(dl, yd, margin=(None, m[1].cpu()))
    with pytest.raises(ValueError, match="2 heads"):
        ops.cross_entropy(dl, yd, margin=m[0])
    with pytest.raises(ValueError, match="gamma"):
        ops.cross_entropy(dl, yd, gamma=-1.0)


# ---- 2. the launch itself: bits ---------------------------------------------------------------------------------------------------------
def _launch(tasks, eps, dt, entry="egk_ce_w_fused_multi"):
    """``entry`` over ``tasks`` = [dict(logits, y, ws, offs, ms, gamma, pads, gscale, gloss=None, loss_only=0)] on plain device tensors;
    returns [(loss, operand)] per task.  The operand has two spare columns behind the last block (they must keep their fill)."""
    from egopack_amd import _lib
    lib = _lib.load()
    weighted = "_w_" in entry
    arr = ((_lib.CEWTask if weighted else _lib.CETask) * len(tasks))()
    keep, out = [], []
    for a, t in zip(arr, tasks):
        logits, y = t["logits"], t["y"]
        rows, width = logits[0].shape[0], sum(t["pads"]) + 2
        loss = torch.full((rows,), 7.0, device=DEV)
        D = torch.full((rows, width), 3.0, device=DEV, dtype=dt)
        b, col = (a.base if weighted else a), 0
        for h, l in enumerate(logits):
            b.logits[h], b.ld[h], b.C[h], b.pad[h], b.dcol[h] = l.data_ptr(), l.stride(0), l.shape[1], t["pads"][h], col
            if weighted:
                a.weight[h] = None if t["ws"][h] is None else t["ws"][h].data_ptr()
                a.offset[h] = None if t["offs"][h] is None else t["offs"][h].data_ptr()
            b.margin[h] = None if t["ms"][h] is None else t["ms"][h].data_ptr()
            col += t["pads"][h]
        b.n_heads, b.y, b.y_stride, b.loss, b.dlogits, b.ldd, b.rows, b.gscale = len(logits), y.data_ptr(), y.shape[1], \
            loss.data_ptr(), D.data_ptr(), D.stride(0), rows, t["gscale"]
        gl = t.get("gloss")
        b.focal_gamma, b.gloss, b.loss_only = t["gamma"], (None if gl is None else gl.data_ptr()), t.get("loss_only", 0)
        keep.append((logits, y, gl))
        out.append((loss, D))
    rc = getattr(lib, entry)(C.c_void_p(torch.cuda.current_stream().cuda_stream), arr, len(tasks), eps, 1 if dt == BF else 0)
    assert rc == 0, _lib.last_error()
    torch.cuda.synchronize()
    return out


def _bits(t):
    return t.view(torch.int16 if t.dtype == BF else torch.int32)


def _two_tasks():
    """Task 0: (115, 478) in pads (128, 512), every vector, gamma 0.5; task 1: one head of 65 (pad 128), margin only, gamma 2."""
    tasks = []
    for heads, pads, gs, presence, gamma in (((115, 478), (128, 512), 0.37, (True, True, True), 0.5), ((65,), (128,), 0.25, (True, False, False), 2.0)):
        logits, y, _ = S.problem(heads)
        ms, ws, offs = S.vectors(heads, presence)
        d = lambda vs: tuple(None if v is None else v.to(DEV) for v in vs)
        tasks.append(dict(logits=[l.to(DEV) for l in logits], y=y.to(DEV), ws=d(ws), offs=d(offs), ms=d(ms), gamma=gamma, pads=pads, gscale=gs,
                          host=(logits, y, ws, offs, ms)))
    return tasks


@pytest.mark.parametrize("eps", S.EPS)
def test_two_tasks_in_one_launch_have_the_bits_of_their_own_launch_and_bf16_is_the_rounded_f32(eps):
    tasks = _two_tasks()
    single = {dt: [_launch([t], eps, dt)[0] for t in tasks] for dt in (torch.float32, BF)}
    for dt in (torch.float32, BF):
        for i, ((loss, D), (loss1, D1)) in enumerate(zip(_launch(tasks, eps, dt), single[dt])):
            assert torch.equal(_bits(loss), _bits(loss1)), f"task {i}: loss bits"
            assert torch.equal(_bits(D), _bits(D1)), f"task {i}: operand bits"
    for i, ((loss32, D32), (loss16, D16)) in enumerate(zip(single[torch.float32], single[BF])):
        assert torch.equal(_bits(loss32), _bits(loss16))
        # (one rounding.  A nan -- the row with S = inf -- is a nan in both; its sign and payload are not a rounding's)
        nan = torch.isnan(D32)
        assert torch.equal(nan, torch.isnan(D16.float())), f"task {i}: the nan entries of the bf16 and the f32 operand differ"
        diff = (_bits(D32.to(BF)) != _bits(D16)) & ~nan
        assert not diff.any(), f"task {i}: bf16 operand != RNE(f32 operand) in {int(diff.sum())} non-nan element(s)"
        assert bool((D32[:, -2:] == 3.0).all()) and bool((D16[:, -2:].float() == 3.0).all()), "columns behind the blocks were written"
        t = tasks[i]
        logits, y, ws, offs, ms = t["host"]
        col, total = 0, torch.zeros(S.ROWS, dtype=torch.float64)
        for h, x in enumerate(logits):
            Cn = x.shape[1]
            ref, _, _ = S.reference(x, y[:, h], ws[h], offs[h], ms[h], eps, t["gamma"])
            total += ref
            # (the loss of one head is not in the launch's output: the gradient block is checked per head, the loss as the sum)
            S.check(ref.float(), D32[:, col:col + Cn], x, y[:, h], ws[h], offs[h], ms[h], eps, t["gamma"], torch.full((S.ROWS,), t["gscale"]),
                    what=f"task {i} head {h}")
            assert not D32[:, col + Cn:col + t["pads"][h]].ne(0).any(), "pad columns are not exactly 0"
            col += t["pads"][h]
        fin = torch.isfinite(total)
        ltol = S.tols(t["gamma"])[0]
        torch.testing.assert_close(loss32.cpu().double()[fin], total[fin], rtol=ltol["rtol"], atol=len(logits) * ltol["atol"])


@pytest.mark.parametrize("eps", S.EPS)
def test_stand_alone_forward_and_backward_have_the_bits_of_the_fused_launch(eps):
    """``ops.cross_entropy`` outside a step (a forward-only launch, then one launch per head with the incoming gradient as row
    seeds) against the fused launch with the same seed as ``gscale``: the same loss and gradient bits."""
    from egopack_amd import ops
    for t in _two_tasks():
        (loss_f, D), = _launch([t], eps, torch.float32)
        dl = [l.detach().clone().requires_grad_(True) for l in t["logits"]]
        nz = lambda vs: None if all(v is None for v in vs) else vs
        with ops.compute_mode("f32"):
            loss = ops.cross_entropy(tuple(dl), t["y"], eps, weight=nz(t["ws"]), offset=nz(t["offs"]), margin=nz(t["ms"]), gamma=t["gamma"])
            loss.backward(torch.full_like(loss, t["gscale"]))
        assert torch.equal(_bits(loss.detach()), _bits(loss_f)), "loss bits"
        col = 0
        for h, l in enumerate(dl):
            Cn = l.shape[1]
            assert torch.equal(_bits(l.grad), _bits(D[:, col:col + Cn].contiguous())), f"head {h}: gradient bits"
            col += t["pads"][h]
        # the row seeds multiply gscale: gscale * gloss[n] with gloss = 1 is the launch without them; loss_only writes the same loss
        (loss_g, D_g), = _launch([dict(t, gloss=torch.ones(S.ROWS, device=DEV))], eps, torch.float32)
        (loss_o, D_o), = _launch([dict(t, loss_only=1)], eps, torch.float32)
        assert torch.equal(_bits(loss_g), _bits(loss_f)) and torch.equal(_bits(D_g), _bits(D))
        assert torch.equal(_bits(loss_o), _bits(loss_f)) and bool((D_o == 3.0).all()), "loss_only wrote a gradient"


def test_strided_logits_give_the_bits_of_their_contiguous_copy():
    from egopack_amd import ops
    heads, eps, gamma = (115, 478), 0.1, 0.5
    logits, y, gloss = S.problem(heads)
    ms, ws, offs = S.vectors(heads, (True, True, True))
    out = []
    with ops.compute_mode("f32"):
        for strided in (False, True):
            dl = []
            for l in logits:
                if strided:
                    base = torch.full((l.shape[0], l.shape[1] + 5), float("nan"), device=DEV)
                    base[:, :l.shape[1]] = l.to(DEV)
                    v = base[:, :l.shape[1]]
                    assert not v.is_contiguous()
                    dl.append(v.detach().requires_grad_(True))
                else:
                    dl.append(l.to(DEV).requires_grad_(True))
            loss = ops.cross_entropy(tuple(dl), y.to(DEV), eps, weight=_dev(ws), offset=_dev(offs), margin=_dev(ms), gamma=gamma)
            loss.backward(gloss.to(DEV))
            out.append((loss.detach(), [l.grad for l in dl]))
    assert torch.equal(_bits(out[0][0]), _bits(out[1][0]))
    for a, b in zip(out[0][1], out[1][1]):
        assert torch.equal(_bits(a.contiguous()), _bits(b.contiguous()))


@pytest.mark.parametrize("dt", [torch.float32, BF], ids=["f32", "bf16"])
@pytest.mark.parametrize("eps", S.EPS)
def test_gamma_0_without_a_margin_is_the_balanced_launch_bit_for_bit(eps, dt):
    """A zero tail runs the balanced instantiation.  The shaped row function forms S and dS operation by operation as the balanced
    one does, so the shaped instantiation -- forced by row seeds of exactly 1, or by margins of exactly 0 -- has the same bits:
    switching a term on for one task of a launch changes nothing for the others."""
    t = dict(_two_tasks()[0], gamma=0.0)
    t["ms"] = (None, None)
    (loss0, D0), = _launch([t], eps, dt)
    (loss1, D1), = _launch([dict(t, gloss=torch.ones(S.ROWS, device=DEV))], eps, dt)
    (loss2, D2), = _launch([dict(t, ms=tuple(torch.zeros(c, device=DEV) for c in (115, 478)))], eps, dt)
    for loss, D in ((loss1, D1), (loss2, D2)):
        assert torch.equal(_bits(loss), _bits(loss0)) and torch.equal(_bits(D), _bits(D0))
    if dt == torch.float32:
        logits, y, ws, offs, ms = t["host"]
        col = 0
        for h, x in enumerate(logits):
            ref, _, _ = S.reference(x, y[:, h], ws[h], offs[h], None, eps, 0.0)
            S.check(ref.float(), D0[:, col:col + x.shape[1]], x, y[:, h], ws[h], offs[h], None, eps, 0.0, torch.full((S.ROWS,), t["gscale"]))
            col += t["pads"][h]


# ---- 3. the multi-task step --------------------------------------------------------------------------------------------------------------
SIZES = [("f32", 2), ("bf16", 8)]   # the smallest step of tests/test_gpu_class_balance.py (per-task launches) and the banked one (ONE launch)
SIZE_IDS = ["f32-B2", "bf16-B8-banked"]
GAMMA = {"ar": 0.5, "lta": 2.0}


def _build_step(compute, shape, batch=2, seed=11):
    """AR + LTA + PNR as tests/test_gpu_class_balance.py::_build_step builds it (T = 8, H = 64, dropout off, Adam).  ``shape``: None
    (the criteria bench.py builds), "none" (the new arguments, every margin None and gamma 0) or "on" (AR: margins on both heads,
    gamma 0.5, class weights; LTA: gamma 2 alone)."""
    import bench
    from egopack_amd import engine, ops
    from egopack_amd import train as T
    from egopack_amd.criterion import CrossEntropyNone, MetricSelectorWrapper
    from tests import class_balance_common as CB
    args = bench.parse_args(["--workload", "mtl", "--batch", str(batch), "--T", "8", "--hidden", "64", "--trn-hidden", "64", "--dropout", "0.0",
                             "--compute", compute])
    ops.set_compute(compute)
    ops.manual_seed(seed)
    model, tasks, crit, weights, dev, merged = bench.build_workload(args, 0, torch.device(DEV))
    model.to(DEV).train()
    for t in tasks.values():
        t.to(DEV).train()
    vec = {}
    if shape is not None:
        class DS:
            has_joint_label, num_labels = False, 2
        if shape == "on":
            vec = {"ar": dict(class_margins=[S.ldam(115), S.ldam(478)], focal_gamma=GAMMA["ar"],
                              class_weights=[CB.zipf_weights(115), CB.zipf_weights(478)]),
                   "lta": dict(focal_gamma=GAMMA["lta"])}
        else:
            vec = {"ar": dict(class_margins=[None, None], focal_gamma=0.0), "lta": dict(class_margins=None, focal_gamma=0.0)}
        crit = dict(crit)
        for t in ("ar", "lta"):
            crit[t] = MetricSelectorWrapper(CrossEntropyNone(), DS(), **vec[t]).to(DEV)
    cfg = T.load_config(["optimizer.lr=1e-2"])
    flat = [*model.configure_optimizers(0), *(p for t in ("ar", "oscc", "lta", "pnr") for p in tasks[t].configure_optimizers(0))]
    opt = T.build_optimizer(cfg, T.build_param_groups(cfg, model, tasks), layout_order=flat)
    step = engine.MTLStep(model, tasks, crit, weights, opt, fused_backbone=True)
    return step, opt, dev, merged, vec


def _run_eager(compute, shape, steps=3, batch=2):
    from egopack_amd import _lib
    from tests.test_gpu_bounds import _counted
    step, opt, dev, merged, _ = _build_step(compute, shape, batch)
    names, vectors = [], []
    for _ in range(steps):
        with _counted(_lib.load()) as c:
            total, vs = step.step(dev, merged)
        names.append(dict(c.names))
        vectors.append((total.clone().cpu(), {t: v.clone().cpu() for t, v in vs.items()}))
    torch.cuda.synchronize()
    return names, vectors, opt.flat_p.clone().cpu(), step.loss_sums()


@pytest.fixture(scope="module")
def off_runs():
    """The step built without the arguments, three eager steps, per size (computed once, shared, never changed)."""
    from egopack_amd import ops
    prev = ops.get_compute()
    out = {(c, b): _run_eager(c, None, batch=b) for c, b in SIZES}
    ops.set_compute(prev)
    return out


@pytest.mark.parametrize("compute,batch", SIZES, ids=SIZE_IDS)
def test_all_terms_off_is_the_step_of_today(compute, batch, off_runs, compute_restored):
    names0, vec0, p0, sums0 = off_runs[(compute, batch)]
    names1, vec1, p1, sums1 = _run_eager(compute, "none", batch=batch)
    assert names0 == names1, (names0, names1)                      # the same launch counts by egk_prof
    assert torch.equal(p0, p1) and sums0 == sums1                  # parameters bit-identical
    for (tot0, v0), (tot1, v1) in zip(vec0, vec1):
        assert torch.equal(tot0, tot1) and v0.keys() == v1.keys() and all(torch.equal(v0[t], v1[t]) for t in v0)
    assert bool(torch.isfinite(p0).all())


@pytest.mark.parametrize("compute,batch", SIZES, ids=SIZE_IDS)
def test_terms_on_in_the_step_match_float64_and_add_no_launch(compute, batch, off_runs, compute_restored):
    """The loss vectors, the objective and the head gradients (the classifier banks' gradient operands, which the fused launch
    writes with the seed w_t / N baked in) of an eager step against float64 on the step's OWN logits and labels -- the ones its
    criteria's ``select`` received in that step -- with that task's own terms.  f32: the tolerances of the module docstring; the bf16
    operand: one bf16 rounding (2^-8 relative) on top, as tests/test_gpu_class_balance.py states it.  No launch is added."""
    from egopack_amd import _lib
    from tests.test_gpu_bounds import _counted
    step, opt, dev, merged, vec = _build_step(compute, "on", batch)
    for _ in range(2):  # (the optimizer's flat buffers and with them the classifier banks exist after the first step)
        step.step(dev, merged)
    seen = {}
    for t in ("ar", "lta"):
        def spy(logits, gt, t=t, inner=step.criteria[t].select):
            seen[t] = (list(logits), [l.detach().clone() for l in logits], gt.detach().clone())
            return inner(logits, gt)
        step.criteria[t].select = spy
    with _counted(_lib.load()) as c:
        total, vs = step.step(dev, merged)
    names = dict(c.names)
    for t in ("ar", "lta"):
        del step.criteria[t].select
    torch.cuda.synchronize()
    off = off_runs[(compute, batch)][0][2]
    print("launches with the terms:", names, "\nlaunches without:", off)
    # AR carries class weights: its launch counts as ce_balanced; LTA (gamma alone) stays under ce_fwd; the banked step has ONE launch
    n_ce = names.get("ce_balanced", 0) + names.get("ce_fwd", 0)
    assert n_ce == off["ce_fwd"] == (1 if batch == 8 else 2) and "ce_bwd" not in names, (names, off)
    assert {k: v for k, v in names.items() if k not in ("ce_balanced", "ce_fwd")} == {k: v for k, v in off.items() if k != "ce_fwd"}
    objective = 0.0
    for t in ("ar", "lta"):
        live_logits, ls, gt = seen[t]
        ls, gt = [l.float().cpu() for l in ls], gt.cpu()
        y = dev[t].y.cpu()
        assert [l.shape[1] for l in ls] == [115, 478]
        ms = [v for v in vec[t].get("class_margins", [None, None])]
        ws = [v for v in vec[t].get("class_weights", [None, None])]
        n_full = y.shape[0]
        seed = torch.full((gt.shape[0],), step.weights[t] / n_full)
        want = torch.zeros(gt.shape[0], dtype=torch.float64)
        ltol, gtol = S.tols(GAMMA[t])
        dst = getattr(live_logits[0], "_egk_grad_dst", None)
        assert dst is not None, "the head's logits are not blocks of a classifier bank: the fused launch did not run"
        gbuf = dst[0].detach()
        for h, x in enumerate(ls):
            ref, dref, _ = S.reference(x, gt[:, h], ws[h], None, ms[h], 0.0, GAMMA[t], seed)
            want += ref
            c0 = live_logits[h]._egk_grad_dst[1]
            block = gbuf[:, c0:c0 + x.shape[1]].float().cpu().double()
            print(f"{compute} B={batch} {t} head {h}: max |operand - float64| = {float((block - dref).abs().max()):.3e}")
            torch.testing.assert_close(block, dref, rtol=gtol["rtol"] + (2.0 ** -8 if compute == "bf16" else 0.0), atol=gtol["atol"],
                                       msg=lambda s: f"{t} head {h} operand: {s}")
        if gt.shape != y.shape or not torch.equal(gt, y):  # a compacted head: node n is row live_inv[n], the other nodes have loss 0
            inv = dev[t].live_inv.cpu()
            want = torch.where(inv >= 0, want[inv.clamp(min=0)], torch.zeros((), dtype=want.dtype))
        torch.testing.assert_close(vs[t].cpu().double(), want, rtol=ltol["rtol"] + 1e-5, atol=2 * ltol["atol"], msg=lambda s: f"{t}: {s}")
        assert not torch.equal(vs[t].cpu(), off_runs[(compute, batch)][1][2][1][t]), "the terms changed nothing"
        objective = objective + step.weights[t] * vs[t].double().cpu().mean()
    objective = objective + step.weights["pnr"] * vs["pnr"].double().cpu().mean()
    torch.testing.assert_close(total.double().cpu(), objective, rtol=1e-5, atol=1e-6)


@pytest.mark.parametrize("compute,batch", SIZES, ids=SIZE_IDS)
def test_captured_step_replayed_twice_equals_two_eager_steps(compute, batch, compute_restored):
    def run(use_graph):
        step, opt, dev, merged, _ = _build_step(compute, "on", batch)
        if use_graph:
            step.capture(dev, merged, warmup=2)
            for _ in range(2):
                step.replay()
        else:
            for _ in range(4):
                step.step(dev, merged)
        torch.cuda.synchronize()
        return opt.flat_p.clone().cpu(), step.loss_sums(), int(opt._t_dev)
    p_e, sums_e, t_e = run(False)
    p_g, sums_g, t_g = run(True)
    assert t_e == t_g == 4
    assert torch.equal(p_e, p_g), "captured and eager parameters differ"
    assert sums_e == sums_g and all(n > 0 for _, n in sums_e.values()), (sums_e, sums_g)


def test_reweight_in_place_is_followed_by_a_captured_step(compute_restored):
    """Deferred re-weighting rewrites the wrapper's class-weight buffers in place: a captured step that was recorded with the
    all-ones side trains with the weights after the rewrite, no new capture -- its parameters equal an eager run's that did the
    same rewrite at the same step."""
    def run(use_graph):
        step, opt, dev, merged, _ = _build_step("f32", "on", 2)
        bufs = [step.criteria["ar"].class_weight_0, step.criteria["ar"].class_weight_1]
        full = [b.clone() for b in bufs]
        for b in bufs:
            b.fill_(1.0)
        if use_graph:
            step.capture(dev, merged, warmup=2)
            step.replay()
        else:
            for _ in range(3):
                step.step(dev, merged)
        before = opt.flat_p.clone()
        for b, f in zip(bufs, full):
            b.copy_(f)
        step.replay() if use_graph else step.step(dev, merged)
        torch.cuda.synchronize()
        return before.cpu(), opt.flat_p.clone().cpu()
    b_e, p_e = run(False)
    b_g, p_g = run(True)
    assert torch.equal(b_e, b_g) and torch.equal(p_e, p_g)
    assert not torch.equal(b_e, p_e)
