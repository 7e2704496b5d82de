"""Positive-class weighting and focal loss of the PNR head on the GPU (include/egopack_bce_balanced.h, ops.bce_with_logits /
ops.linear1_bce with pos / neg / gamma): parity with the float64 host model of tests/pnr_balance_common.py, the bit anchor at
(1, 1, 0), the one-pass form against the two-launch form, layouts of ``f``, "off is the old path" and "on" in the multi-task step
(eager and captured), the task / criterion plumbing and main_temporal.py with ``pnr_balance.mode=pos_weight`` (log line, checkpoint
entry, resume).  Tolerances: tests/pnr_balance_common.py."""
import subprocess
import sys
from pathlib import Path

import pytest
import torch

from tests import pnr_balance_common as PB

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF = torch.bfloat16
REPO = Path(__file__).resolve().parents[1]
N = 333  # two workgroups of the element-wise kernels, a ragged tail; the first 14 logits are 0, +-30, +-88, +-100 under both labels
ANCHOR = (1.0, 1.0, 0.0)


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


def _head(rows, cols, mode, seed=None):
    """The operands of tests/test_gpu_kernels.py::test_one_logit_head_with_bce_in_one_row_pass with labels of one positive in 8."""
    g = PB.gen(rows + cols if seed is None else seed)
    f = torch.randn(rows, cols, generator=g)
    W, b = torch.randn(1, cols, generator=g) * 0.05, torch.randn(1, generator=g)
    y = PB.labels(rows, g)
    if mode == "bf16":
        f = f.to(BF).float()
    return f, W, b, y


# ---- 1. parity against the host model ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["f32", "bf16"])
@pytest.mark.parametrize("sh", PB.TRIPLES, ids=str)
def test_two_launch_form_matches_the_host_model(sh, mode, compute_restored):
    """(Fails without the feature: ``bce_with_logits() takes 2 positional arguments``.)  ``mode`` is the element type of the logit
    gradient: the bf16 one is the rounding of the f32 one, bit for bit (no fused multiply-add that depends on the instantiation)."""
    from egopack_amd import ops
    x, y, gl = PB.problem(N, 11)
    ops.set_compute("f32")
    xd = x.to(DEV).requires_grad_(True)
    loss = ops.bce_with_logits(xd, y.to(DEV), *sh)
    loss.backward(gl.to(DEV))
    want, dwant = PB.model(x, y, *sh, gl)
    print(f"{sh}: max |loss - model| = {float((loss.detach().cpu().double() - want).abs().max()):.3e}, "
          f"max |dz - model| = {float((xd.grad.cpu().double() - dwant).abs().max()):.3e}")
    assert bool(torch.isfinite(loss).all()) and bool(torch.isfinite(xd.grad).all())
    torch.testing.assert_close(loss.detach().cpu(), want.float(), **PB.LOSS_TOL)
    torch.testing.assert_close(xd.grad.cpu(), dwant.float(), **PB.grad_tol(sh[0], sh[1]))
    if mode == "bf16":
        from egopack_amd import _lib
        from tests.test_gpu_bounds import P, S
        yd, gd, d16 = y.to(DEV), gl.to(DEV), torch.empty(N, dtype=BF, device=DEV)  # (held until the launch has run)
        rc = _lib.load().egk_bce_w_bwd(S(), P(xd.detach()), P(yd), P(gd), P(d16), N, *sh, 1)
        assert rc == 0, _lib.last_error()
        assert bool(torch.isfinite(d16.float()).all())
        torch.testing.assert_close(d16.float().cpu(), dwant.float(), **PB.OUT16)
        assert torch.equal(d16, xd.grad.to(BF)), "the bf16 gradient is not the rounding of the f32 gradient"


@pytest.mark.parametrize("rows,cols,mode", [(333, 256, "f32"), (77, 1000, "bf16"), (130, 1024, "bf16")])
@pytest.mark.parametrize("sh", PB.TRIPLES, ids=str)
def test_one_pass_form_matches_the_host_model_and_the_two_launch_form(sh, rows, cols, mode, compute_restored):
    """ops.linear1_bce with the scalars against the host model on the float64 logits of the same (rounded) operands, and against
    ops.linear + ops.bce_with_logits(..., pos, neg, gamma) -- the tolerances and scales of
    tests/test_gpu_kernels.py::test_one_logit_head_with_bce_in_one_row_pass for the plain pair."""
    from egopack_amd import ops
    f, W, b, y = _head(rows, cols, mode)
    seed = 0.7 / rows
    ops.set_compute(mode)
    Wr = W.to(BF).float() if mode == "bf16" else W
    z = (f.double() @ Wr.double().t()).squeeze(1) + b.double()
    want, dz = PB.model(z, y, *sh, seed)
    rf, rW, rb = dz[:, None] * Wr.double(), (dz @ f.double())[None, :], dz.sum()
    df = f.to(DEV).to(ops.act_dtype()).requires_grad_(True)
    dW, db = W.clone().to(DEV).requires_grad_(True), b.clone().to(DEV).requires_grad_(True)
    with ops.loss_seed(seed):
        assert ops.linear1_bce_ok(df, dW)
        loss, logits = ops.linear1_bce(df, dW, db, y.to(DEV), *sh)
    loss.backward(torch.full_like(loss, seed))
    f32m = mode == "f32"
    lt = dict(rtol=1e-4, atol=1e-4) if f32m else dict(rtol=1e-2, atol=2e-2)
    assert bool(torch.isfinite(loss).all()) and bool(torch.isfinite(df.grad.float()).all())
    torch.testing.assert_close(logits.cpu(), z.float(), **lt)
    torch.testing.assert_close(loss.detach().cpu(), want.float(), **lt)
    gscale, wscale = float(rf.abs().max()), float(rW.abs().max())
    assert (df.grad.float().cpu().double() - rf).abs().max() <= (1e-5 if f32m else 1.5e-2) * gscale
    assert (dW.grad.cpu().double() - rW).abs().max() <= (2e-5 if f32m else 1.5e-2) * wscale
    assert abs(float(db.grad.cpu()) - float(rb)) <= (2e-5 if f32m else 1e-2) * max(1.0, abs(float(rb)) * 100)
    # the two-launch form: classifier contraction + egk_bce_w_* -- same values up to summation order
    df2 = f.to(DEV).to(ops.act_dtype()).requires_grad_(True)
    dW2, db2 = W.clone().to(DEV).requires_grad_(True), b.clone().to(DEV).requires_grad_(True)
    z2 = ops.linear(df2, dW2, db2, out_f32=True).squeeze(1)
    l2 = ops.bce_with_logits(z2, y.to(DEV), *sh)
    l2.backward(torch.full_like(l2, seed))
    torch.testing.assert_close(loss.detach(), l2.detach(), **(dict(rtol=1e-4, atol=1e-5) if f32m else dict(rtol=5e-3, atol=5e-3)))
    assert (df.grad.float() - df2.grad.float()).abs().max().item() <= (1e-5 if f32m else 1e-2) * gscale
    assert (dW.grad - dW2.grad).abs().max().item() <= (2e-5 if f32m else 1e-2) * wscale


def test_extreme_logits_in_the_one_pass_form_are_finite_and_match_the_model(compute_restored):
    """A classifier of weight 0 and one bias per run: every row's logit is exactly 0, +-30, +-88 or +-100."""
    from egopack_amd import ops
    ops.set_compute("f32")
    rows, cols = 16, 64
    f = torch.randn(rows, cols, generator=PB.gen(3))
    y = torch.tensor([1, 0] * (rows // 2))
    for zval in PB.EXTREMES:
        for sh in PB.TRIPLES:
            df = f.to(DEV).requires_grad_(True)
            dW, db = torch.zeros(1, cols, device=DEV, requires_grad=True), torch.tensor([zval], device=DEV, requires_grad=True)
            with ops.loss_seed(0.25):
                loss, logits = ops.linear1_bce(df, dW, db, y.to(DEV), *sh)
            loss.backward(torch.full_like(loss, 0.25))
            assert bool((logits == zval).all())
            want, dz = PB.model(torch.full((rows,), zval), y, *sh, 0.25)
            assert bool(torch.isfinite(loss).all()) and bool(torch.isfinite(dW.grad).all()) and bool(torch.isfinite(db.grad).all())
            torch.testing.assert_close(loss.detach().cpu(), want.float(), **PB.LOSS_TOL)
            torch.testing.assert_close(db.grad.cpu(), dz.sum().float().reshape(1), rtol=1e-4, atol=rows * PB.grad_tol(*sh[:2])["atol"])
            assert not df.grad.ne(0).any()  # (df = g w with w = 0)


# ---- 2. the bit anchor -------------------------------------------------------------------------------------------------------------------
def test_anchor_scalars_give_the_bits_of_the_plain_two_launch_kernels():
    from egopack_amd import _lib, ops
    from tests.test_gpu_bounds import _counted
    x, y, gl = PB.problem(N, 13)
    out = {}
    with ops.compute_mode("f32"):
        for name, sh in (("plain", ()), ("shaped", ANCHOR), ("partly", (None, None, 0.0))):
            xd = x.to(DEV).requires_grad_(True)
            with _counted(_lib.load()) as c:
                loss = ops.bce_with_logits(xd, y.to(DEV), *sh)
                loss.backward(gl.to(DEV))
            out[name] = (loss.detach(), xd.grad, dict(c.names))
    assert out["plain"][2] == {"bce_fwd": 1, "bce_bwd": 1}, out["plain"][2]
    for name in ("shaped", "partly"):
        assert out[name][2] == {"bce_balanced": 2}, out[name][2]
        assert torch.equal(out[name][0], out["plain"][0]), "loss bits"
        assert torch.equal(out[name][1], out["plain"][1]), "gradient bits"
    # ... and the bf16 gradient, through the C ABI
    from tests.test_gpu_bounds import P, S
    lib = _lib.load()
    xd, yd, gd = x.to(DEV), y.to(DEV), gl.to(DEV)
    a, b = torch.empty(N, dtype=BF, device=DEV), torch.empty(N, dtype=BF, device=DEV)
    assert lib.egk_bce_bwd(S(), P(xd), P(yd), P(gd), P(a), N, 1) == 0 and lib.egk_bce_w_bwd(S(), P(xd), P(yd), P(gd), P(b), N, *ANCHOR, 1) == 0
    assert torch.equal(a, b)


@pytest.mark.parametrize("rows,cols,mode", [(333, 256, "f32"), (77, 1000, "bf16"), (2048, 1024, "bf16")])
def test_anchor_scalars_give_the_bits_of_the_plain_one_pass_launch(rows, cols, mode, compute_restored):
    from egopack_amd import _lib, ops
    from tests.test_gpu_bounds import _counted
    f, W, b, y = _head(rows, cols, mode)
    seed = 0.7 / rows
    ops.set_compute(mode)
    out = {}
    for name, sh in (("plain", ()), ("shaped", ANCHOR)):
        df = f.to(DEV).to(ops.act_dtype()).requires_grad_(True)
        dW, db = W.clone().to(DEV).requires_grad_(True), b.clone().to(DEV).requires_grad_(True)
        with _counted(_lib.load()) as c:
            with ops.loss_seed(seed):
                loss, logits = ops.linear1_bce(df, dW, db, y.to(DEV), *sh)
            loss.backward(torch.full_like(loss, seed))
        out[name] = (dict(c.names), logits, loss.detach(), df.grad, dW.grad, db.grad)
    plain, shaped = out["plain"][0], out["shaped"][0]
    assert plain.get("bce_fwd") == 1 and "bce_balanced" not in plain, plain
    assert shaped.get("bce_balanced") == 1 and "bce_fwd" not in shaped and "bce_bwd" not in shaped, shaped
    assert {k: v for k, v in shaped.items() if k != "bce_balanced"} == {k: v for k, v in plain.items() if k != "bce_fwd"}
    for what, a, b_ in zip(("logits", "loss", "df", "dw", "db"), out["shaped"][1:], out["plain"][1:]):
        assert torch.equal(a, b_), f"{what}: the shaped launch with (1, 1, 0) differs from the plain launch in bits"


# ---- 3. layouts ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", ["padded", "cat"])
@pytest.mark.parametrize("mode", ["f32", "bf16"])
def test_feature_layouts_give_the_bits_of_contiguous_copies(layout, mode, compute_restored):
    from egopack_amd import ops
    rows, cols, sh = 77, 264, (0.25, 0.75, 2.0)
    f, W, b, y = _head(rows, cols, mode)
    ops.set_compute(mode)
    t = f.to(DEV).to(ops.act_dtype())
    if layout == "padded":
        base = torch.full((rows, cols + 8), float("nan"), device=DEV, dtype=t.dtype)
        base[:, :cols] = t
        v = base[:, :cols]
    else:
        v = torch.cat([torch.full((rows, 8), float("nan"), device=DEV, dtype=t.dtype), t], dim=1)[:, 8:]
    assert not v.is_contiguous() and torch.equal(v, t)
    out = []
    for feat in (t.clone(), v):
        feat = feat.detach().requires_grad_(True)
        dW, db = W.clone().to(DEV).requires_grad_(True), b.clone().to(DEV).requires_grad_(True)
        with ops.loss_seed(0.01):
            loss, logits = ops.linear1_bce(feat, dW, db, y.to(DEV), *sh)
        loss.backward(torch.full_like(loss, 0.01))
        out.append((loss.detach(), logits, feat.grad, dW.grad, db.grad))
    for what, a, b_ in zip(("loss", "logits", "df", "dw", "db"), out[1], out[0]):
        assert torch.equal(a, b_), what
    # the two-launch form on a strided logit vector and a strided gradient
    x, yy, gl = PB.problem(N, 17)
    outs = []
    for strided in (False, True):
        xs = torch.stack([x, x], 1).to(DEV)[:, 0] if strided else x.to(DEV)
        gs = torch.stack([gl, gl], 1).to(DEV)[:, 1] if strided else gl.to(DEV)
        assert xs.is_contiguous() != strided
        xs = xs.detach().requires_grad_(True)
        loss = ops.bce_with_logits(xs, yy.to(DEV), *sh)
        loss.backward(gs)
        outs.append((loss.detach(), xs.grad))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])


# ---- 4. the multi-task step: off is the old path, on matches the model, captured == eager ---------------------------------------------------
SIZES = [("f32", 2), ("bf16", 2), ("bf16", 8)]
SIZE_IDS = ["f32-B2", "bf16-B2", "bf16-B8"]
STEP_SH = (31.0 * 32 / 62, 32.0 / 62, 0.0)
STEP_TRIPLES = [STEP_SH, (0.25, 0.75, 2.0)]


def _build_step(compute, balance, batch=2, seed=11):
    """tests/test_gpu_class_balance.py::_build_step with the PNR criterion in place of the AR / LTA wrappers: AR + LTA + PNR,
    B = ``batch`` per task, T = 8, H = 64, dropout off, Adam.  ``balance``: None (the criterion bench.py builds), "none" (the
    criterion constructed with three Nones) or a (pos, neg, gamma) triple."""
    import bench
    from egopack_amd import engine, ops
    from egopack_amd import train as T
    from egopack_amd.criterion import BCEWithLogitsNone
    args = bench.parse_args(["--workload", "mtl", "--batch", str(batch), "--T", "8", "--hidden", "64", "--trn-hidden", "64", "--dropout", "0.0",
                             "--compute", compute])
    ops.set_compute(compute)
    ops.manual_seed(seed)
    model, tasks, crit, weights, dev, merged = bench.build_workload(args, 0, torch.device(DEV))
    model.to(DEV).train()
    for t in tasks.values():
        t.to(DEV).train()
    if balance is not None:
        crit = dict(crit)
        crit["pnr"] = BCEWithLogitsNone(None, None, None) if balance == "none" else BCEWithLogitsNone(*balance)
    cfg = T.load_config(["optimizer.lr=1e-2"])
    flat = [*model.configure_optimizers(0), *(p for t in ("ar", "oscc", "lta", "pnr") for p in tasks[t].configure_optimizers(0))]
    opt = T.build_optimizer(cfg, T.build_param_groups(cfg, model, tasks), layout_order=flat)
    step = engine.MTLStep(model, tasks, crit, weights, opt, fused_backbone=True)
    return step, opt, dev, merged


def _run_eager(compute, balance, steps=3, batch=2):
    from egopack_amd import _lib
    from tests.test_gpu_bounds import _counted
    step, opt, dev, merged = _build_step(compute, balance, batch)
    names, vectors = [], []
    for _ in range(steps):
        with _counted(_lib.load()) as c:
            total, vs = step.step(dev, merged)
        names.append(dict(c.names))
        vectors.append((total.clone().cpu(), {t: v.clone().cpu() for t, v in vs.items()}))
    torch.cuda.synchronize()
    return names, vectors, opt.flat_p.clone().cpu(), step.loss_sums()


_OFF = {}


def _off_run(compute, batch):
    """Three eager steps without the feature: computed once per size, shared by the tests below, never changed."""
    if (compute, batch) not in _OFF:
        _OFF[compute, batch] = _run_eager(compute, None, batch=batch)
    return _OFF[compute, batch]


@pytest.mark.parametrize("compute,batch", SIZES, ids=SIZE_IDS)
def test_off_is_the_old_path_in_the_step(compute, batch, compute_restored):
    names0, vec0, p0, sums0 = _off_run(compute, batch)
    names1, vec1, p1, sums1 = _run_eager(compute, "none", batch=batch)
    assert all("bce_balanced" not in n for n in names0 + names1), names1
    assert all(n.get("bce_fwd") == 1 for n in names0), names0  # the plain one-pass launch
    assert names0 == names1
    assert torch.equal(p0, p1) and sums0 == sums1
    for (tot0, v0), (tot1, v1) in zip(vec0, vec1):
        assert torch.equal(tot0, tot1) and v0.keys() == v1.keys() and all(torch.equal(v0[t], v1[t]) for t in v0)
    assert bool(torch.isfinite(p0).all())


@pytest.mark.parametrize("sh", STEP_TRIPLES, ids=["pos_weight", "focal"])
@pytest.mark.parametrize("compute,batch", SIZES, ids=SIZE_IDS)
def test_on_in_the_step_matches_the_host_model_and_replaces_one_launch(compute, batch, sh, compute_restored):
    """The PNR loss vector of the eager step against the host model on the step's OWN logits (the ones the one-pass launch wrote in
    that very step), the objective sum_t w_t mean(loss_t), and the launches: one ``bce_balanced`` launch in place of the plain
    one-pass launch, every other kernel as often as in the step without the feature."""
    from egopack_amd import _lib
    from tests.test_gpu_bounds import _counted
    step, opt, dev, merged = _build_step(compute, sh, batch)
    for _ in range(2):
        step.step(dev, merged)
    seen = {}
    task = step.tasks["pnr"]

    def spy(features, targets, balance=None, inner=task.fused_head_loss):
        out = inner(features, targets, balance=balance)
        seen["balance"], seen["out"] = balance, None if out is None else (out[0].detach().clone(), out[1].detach().clone())
        return out
    task.fused_head_loss = spy
    with _counted(_lib.load()) as c:
        total, vs = step.step(dev, merged)
    names = dict(c.names)
    del task.fused_head_loss
    torch.cuda.synchronize()
    print("launches of the step with the scalars:", names)
    off_names, off_vec, _, _ = _off_run(compute, batch)
    print("launches of the step without:", off_names[2])
    assert names.get("bce_balanced") == 1 and "bce_fwd" not in names and "bce_bwd" not in names, names
    assert off_names[2].get("bce_fwd") == 1 and "bce_balanced" not in off_names[2], off_names[2]
    assert {k: v for k, v in names.items() if k != "bce_balanced"} == {k: v for k, v in off_names[2].items() if k != "bce_fwd"}
    f32sh = tuple(float(torch.tensor(v, dtype=torch.float64).float()) for v in sh)
    assert seen["balance"] == tuple(float(v) for v in sh) and seen["out"] is not None
    loss_seen, logits = seen["out"]
    y = dev["pnr"].y.cpu()
    assert logits.dtype == torch.float32 and logits.shape == y.shape and int(y.sum()) == batch  # one positive per sequence
    want, _ = PB.model(logits.cpu(), y, *f32sh)  # (the scalars travel as f32 kernel arguments)
    print(f"{compute} B={batch} {sh}: max |loss - model| = {float((vs['pnr'].cpu().double() - want).abs().max()):.3e}")
    torch.testing.assert_close(vs["pnr"].cpu(), want.float(), **PB.LOSS_TOL)
    assert torch.equal(vs["pnr"], loss_seen)
    assert not torch.equal(vs["pnr"].cpu(), off_vec[2][1]["pnr"]), "the scalars changed nothing"
    objective = sum(step.weights[t] * vs[t].double().cpu().mean() for t in ("ar", "lta", "pnr"))
    torch.testing.assert_close(total.double().cpu(), objective, rtol=1e-5, atol=1e-6)


@pytest.mark.parametrize("compute,batch", SIZES, ids=SIZE_IDS)
def test_captured_step_replayed_twice_equals_two_eager_steps(compute, batch, compute_restored):
    def run(use_graph):
        step, opt, dev, merged = _build_step(compute, STEP_SH, batch)
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


# ---- 5. training only -------------------------------------------------------------------------------------------------------------------------
def test_task_and_criterion_use_the_scalars_only_while_training():
    from egopack_amd import ops
    from egopack_amd.criterion import BCEWithLogitsNone
    from egopack_amd.models.tasks import PNRTask
    sh = (31.0, 1.0, 0.0)
    x, y, _ = PB.problem(N, 19)
    xd, yd = x.to(DEV), y.to(DEV)
    with ops.compute_mode("f32"):
        plain = ops.bce_with_logits(xd, yd)
        want, _ = PB.model(x, y, *sh)
        task = PNRTask(64, 64).to(DEV)
        assert torch.equal(task.train().compute_loss(xd, yd), plain)
        task.set_loss_balance(*sh)
        assert "balance" not in "".join(task.state_dict())
        torch.testing.assert_close(task.train().compute_loss(xd, yd).cpu(), want.float(), **PB.LOSS_TOL)
        assert torch.equal(task.eval().compute_loss(xd, yd), plain), "a validation loss is the plain BCE, bit for bit"
        crit = BCEWithLogitsNone(*sh).to(DEV)
        torch.testing.assert_close(crit.train()(xd, yd).cpu(), want.float(), **PB.LOSS_TOL)
        assert torch.equal(crit.train()(xd, yd), task.train().compute_loss(xd, yd))
        assert torch.equal(crit.eval()(xd, yd), plain)
        assert torch.equal(BCEWithLogitsNone().train()(xd, yd), plain)
        with pytest.raises(ValueError, match="finite and >= 0"):
            ops.bce_with_logits(xd, yd, pos=-1.0)
        # a PNR task with auxiliary classifiers goes through compute_loss as well
        aux = PNRTask(64, 64, aux_tasks=("ar", "lta")).to(DEV).train()
        aux.set_loss_balance(gamma=2.0)
        wf, _ = PB.model(x, y, 1.0, 1.0, 2.0)
        torch.testing.assert_close(aux.compute_loss(xd, yd).cpu(), wf.float(), **PB.LOSS_TOL)


# ---- 6. main_temporal.py: the log line, the checkpoint entry, resume ----------------------------------------------------------------------
CHILD = r"""
import sys
from pathlib import Path
sys.path.insert(0, sys.argv[1])
tmp = Path(sys.argv[2])
import main_temporal

BASE = ["k=1", "batch_size=4", "synthetic_samples=8", "model.hidden_size=64", "model.temporal_pooling.hidden_size=64",
        "oscc_feat_size=64", "save_model=True", "compute=f32", "optimizer.lr=1e-3", "enabled_tasks=[ar,lta,pnr]",
        "dataset_recognition.T=8", "dataset_lta.T=8", "dataset_pnr.T=8", "dataset_oscc.T=8",
        "pnr_balance.mode=pos_weight", "lr_scheduler.T_max=2", "use_graph=false", "save_every=1"]
main_temporal.main(BASE + ["num_epochs=2", f"checkpoint_dir={tmp / 'full'}"])
main_temporal.main(BASE + ["num_epochs=1", f"checkpoint_dir={tmp / 'part'}"])
part = tmp / "part" / "MTL_ar-lta-pnr" / "checkpoint.pth"
main_temporal.main(BASE + ["num_epochs=2", f"checkpoint_dir={tmp / 'resumed'}", f"resume_from={part}"])
print("RESUMED-WITH-OTHER-SCALARS", file=sys.stderr, flush=True)
main_temporal.main([a for a in BASE if not a.startswith("pnr_balance")] + ["pnr_balance.mode=focal", "num_epochs=1",
                   "save_model=False", f"checkpoint_dir={tmp / 'other'}", f"resume_from={part}"])
print("CHILD-OK")
"""


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("pnr_balance_runs")
    script = tmp / "child.py"
    script.write_text(CHILD)
    r = subprocess.run([sys.executable, str(script), str(REPO), str(tmp)], capture_output=True, text=True, cwd=str(tmp), timeout=600)
    assert r.returncode == 0 and "CHILD-OK" in r.stdout, (r.returncode, r.stdout[-3000:], r.stderr[-6000:])
    load = lambda *parts: torch.load(tmp.joinpath(*parts), weights_only=False)
    return dict(log=r.stderr + r.stdout, full=load("full", "MTL_ar-lta-pnr", "checkpoint.pth"),
                part=load("part", "MTL_ar-lta-pnr", "checkpoint.pth"), resumed=load("resumed", "MTL_ar-lta-pnr", "checkpoint.pth"))


@pytest.mark.timeout(600)
def test_main_temporal_logs_stores_and_resumes_bit_for_bit(runs):
    from egopack_amd import train as T
    log, full, part, res = runs["log"], runs["full"], runs["part"], runs["resumed"]
    # 8 sequences of 8 nodes, one positive each: pw = 7, k = 64 / 112
    pos, neg = float(torch.tensor(7 * 64 / 112, dtype=torch.float64).float()), float(torch.tensor(64 / 112, dtype=torch.float64).float())
    assert log.count(f"pnr balance: mode pos_weight, 8 positive / 56 negative nodes, pos {pos:.9g}, neg {neg:.9g}, gamma 0") == 3
    assert "pnr balance: mode focal, 8 positive / 56 negative nodes, pos 0.25, neg 0.75, gamma 2" in log
    pb = full["pnr_balance"]
    assert pb["config"]["mode"] == "pos_weight" and pb["config"]["pos_weight"] == "auto" and pb["counts"] == {"n_pos": 8, "n_neg": 56}
    cfg = T.load_config(["synthetic_samples=8", "dataset_pnr.T=8", "pnr_balance.mode=pos_weight"])
    want = T.build_pnr_balance(cfg, T.build_datasets(cfg, "train"))
    v = pb["scalars"]
    assert v.dtype == torch.float32 and v.shape == (3,) and v.device.type == "cpu"
    assert v.tolist() == [want["pos"], want["neg"], want["gamma"]] == [pos, neg, 0.0]
    assert "class_balance" not in full
    assert all("balance" not in key for ckpt in (full, part) for key in ckpt["task/pnr"])
    # the resumed run: no warning while the scalars agree, one line when they do not; the same bits as the uninterrupted run
    head, tail = log.split("RESUMED-WITH-OTHER-SCALARS")
    assert "differ from the checkpoint's" not in head and tail.count("differ from the checkpoint's") == 1
    assert part["epoch"] == 1 and res["epoch"] == full["epoch"] == 2
    moved = 0.0
    for key in ("temporal_graph", "task/recognition", "task/lta", "task/pnr"):
        for k, val in full[key].items():
            torch.testing.assert_close(res[key][k], val, rtol=0, atol=0, msg=lambda s: f"{key}.{k}: {s}")
            if val.is_floating_point():
                moved = max(moved, float((val - part[key][k]).abs().max()))
    assert moved > 0
    for i, st in full["optimizer"]["state"].items():
        for k in ("exp_avg", "exp_avg_sq"):
            assert torch.equal(st[k], res["optimizer"]["state"][i][k]), (i, k)
    assert torch.equal(res["pnr_balance"]["scalars"], v)
