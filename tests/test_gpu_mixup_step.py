"""Sequence mixup inside ``engine.MTLStep``: hidden 64, B = 4 sequences per task, T = 5 nodes, AR + LTA + PNR.

* hard swap: hand-written fields with lam in {0, 1} per sequence -- one step with them equals, bit for bit, one step without them on
  the batch whose swapped sequences were exchanged on the host (x and y), f32 and bf16, compact_heads off in both runs: lam in {0, 1}
  rows are bitwise copies and bitwise plain losses;
* general lambda, f32: the mixed input against the float64 mix of the staged input (the launch's bound), and the heads' loss vectors
  against the float64 two-target model on the step's own logits, at the tolerance tests/test_gpu_step_matrix.py uses for its f32 rows;
* captured == eager bit for bit over 3 steps with fresh fields each step, ONE capture -- also with grad_clip_norm, ema, uncertainty
  task weighting and bf16 optimizer state on;
* the launch ledger: without the fields no mix_rows and no ce_mix launch and the plain step's counts; with them exactly one of each
  and no plain fused cross entropy beside it;
* main_temporal.py mixup.alpha=0.4: two epochs train and log the mean lambda; interrupted and resumed equals uninterrupted."""
import logging

import pytest
import torch

from tests import mixup_common as MC
from tests import step_matrix_common as M

pytestmark = pytest.mark.gpu

DEV = "cuda"
B, T_NODES = 4, 5


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


@pytest.fixture
def compute_restored():
    from egopack_amd import ops
    before = ops.get_compute()
    yield
    ops.set_compute(before)


def build(compute, over=(), seed=11, batch=B, t_nodes=T_NODES):
    """The step the way tests/step_matrix_common.build_step builds it, at this file's size.  Returns (step, opt, batches, merged)."""
    import bench
    from egopack_amd import engine, ops
    from egopack_amd import train as T
    args = bench.parse_args(["--workload", "mtl", "--batch", str(batch), "--T", str(t_nodes), "--hidden", "64", "--trn-hidden", "64",
                             "--dropout", "0.0", "--compute", compute])
    ops.set_compute(compute)
    ops.manual_seed(seed)
    model, tasks, crit, weights, dev, merged = bench.build_workload(args, 0, torch.device(DEV))
    model.to(DEV).train()
    for t in tasks.values():
        t.to(DEV).train()
    cfg = T.load_config([f"optimizer.lr={M.LR}", f"optimizer.weight_decay={M.WD}", *over])
    crit = {t: c.to(DEV).train() for t, c in crit.items()}
    wd = cfg.optimizer.weight_decay
    flat = [*model.configure_optimizers(wd), *(p for t in M.ORDER for p in tasks[t].configure_optimizers(wd))]
    mode = T.task_weighting_config(cfg)["mode"]
    log_var = T.build_task_weighting(cfg, [t for t in engine.MTLStep.order if weights.get(t, 0) > 0 and t in tasks], DEV)
    opt = T.build_optimizer(cfg, T.build_param_groups(cfg, model, tasks), layout_order=flat, log_var=log_var)
    step = engine.MTLStep(model, tasks, crit, weights, opt, fused_backbone=True, task_weighting=mode, log_var=log_var)
    return step, opt, dev, merged


def set_fields(dev, ordinal, tasks=("ar", "lta"), alpha=0.4):
    """Fresh loader fields on the device batches, written IN PLACE when they exist (a captured step reads fixed buffers)."""
    from egopack_amd import data as D
    for t in tasks:
        d = dev[t]
        src, lam, my = D.mixup_fields(d.ptr.cpu(), d.y.cpu(), 3, 0, ordinal, t, alpha)
        if getattr(d, "mix_src", None) is None:
            d.mix_src, d.mix_lam, d.mix_y = src.to(DEV), lam.to(DEV), my.to(DEV)
        else:
            d.mix_src.copy_(src), d.mix_lam.copy_(lam), d.mix_y.copy_(my)


def snapshot(step, opt):
    torch.cuda.synchronize()
    out = dict(flat_p=opt.flat_p.detach().clone().cpu(), t=int(opt._t_dev.item()))
    for i, b in enumerate(opt.state_buffers()):
        out[f"state{i}"] = (b.detach().view(torch.int16) if b.dtype == torch.bfloat16 else b.detach()).clone().cpu()
    if opt.ema:
        out["flat_ema"] = opt.flat_ema.detach().clone().cpu()
    if step.task_log_var is not None:
        out["log_var"] = step.task_log_var.log_var.detach().clone().cpu()
    return out


def same(a, b):
    assert set(a) == set(b)
    for k in a:
        if torch.is_tensor(a[k]):
            assert torch.equal(a[k], b[k]), f"{k} differs in {int((a[k] != b[k]).sum())} of {a[k].numel()} elements"
        else:
            assert a[k] == b[k], k


# ---- hard swap ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("compute", ["f32", "bf16"])
def test_hard_swap_equals_the_step_on_the_exchanged_batch(compute, compute_restored):
    swaps = {"ar": [1, 0, 2, 3], "lta": [0, 3, 2, 1]}  # partner sequence of every sequence; lam 0 where it differs, 1 elsewhere

    def rows_of(partner):
        return torch.cat([torch.arange(p * T_NODES, (p + 1) * T_NODES) for p in partner])

    def run(mixed):
        step, opt, dev, merged = build(compute)
        step.compact_heads = False
        for t, partner in swaps.items():
            src = rows_of(partner).to(DEV)
            moved = torch.tensor([float(p == s) for s, p in enumerate(partner)]).repeat_interleave(T_NODES).to(DEV)
            d = dev[t]
            if mixed:
                d.mix_src, d.mix_lam, d.mix_y = src.to(torch.int32), moved, d.y[src].contiguous()
            else:  # the exchange on the host side of the step: x and y of the swapped sequences
                d.x.copy_(d.x[src].clone())
                d.y.copy_(d.y[src].clone())
        total, vs = step.step(dev, merged)
        snap = snapshot(step, opt)
        snap.update({f"loss.{t}": v.detach().clone().cpu() for t, v in vs.items()})
        snap["total"] = total.detach().clone().cpu()
        return snap
    same(run(True), run(False))


# ---- general lambda against float64 ------------------------------------------------------------------------------------------------------
def test_general_lambda_f32_against_the_float64_restatement(compute_restored):
    from egopack_amd import ops
    step, opt, dev, merged = build("f32")
    set_fields(dev, 0)
    seen, mixed_in = {}, []
    for t in ("ar", "lta"):
        def spy(logits, gt, t=t, inner=step.criteria[t].select):
            seen[t] = ([l.detach().clone() for l in logits], gt.detach().clone())
            return inner(logits, gt)
        step.criteria[t].select = spy
    inner_mix = ops.mix_rows

    def mix_spy(xs, outs, srcs, lams):
        r = inner_mix(xs, outs, srcs, lams)
        mixed_in.append(([x.detach().clone() for x in xs], [o.detach().clone() for o in outs]))
        return r
    ops.mix_rows = mix_spy
    try:
        total, vs = step.step(dev, merged)
    finally:
        ops.mix_rows = inner_mix
        for t in ("ar", "lta"):
            del step.criteria[t].select
    torch.cuda.synchronize()
    assert len(mixed_in) == 1, "ONE mix launch in front of the backbone"
    xs, outs = mixed_in[0]
    live = [t for t in ("ar", "lta", "oscc", "pnr") if dev.get(t) is not None]
    assert len(xs) == len(live)
    for t, x, o in zip(live, xs, outs):
        d = dev[t]
        src, lam = (d.mix_src.cpu(), d.mix_lam.cpu()) if t in ("ar", "lta") else (None, None)
        exact, bound = MC.mix_model(x.float().cpu(), src, lam), MC.mix_bound(x.float().cpu(), src, lam)
        assert bool(((o.double().cpu() - exact).abs() <= bound).all()), f"{t}: the mixed input"
        if src is None:
            assert torch.equal(o, x), "the unmixed task's rows are copied"
    row = M.rows()[1]  # (every factor off, f32: the row whose tolerances apply)
    for t in ("ar", "lta"):
        ltol, _ = M.ce_tols(row, t, "f32")
        logits, gt = seen[t]
        assert torch.equal(gt.cpu(), dev[t].y.cpu()), "a mixed task's head is not compacted"
        sm = float(getattr(step.criteria[t].criterion, "label_smoothing", 0.0))
        ref, _ = MC.ce_mix_model([l.float().cpu() for l in logits], dev[t].y.cpu(), dev[t].mix_y.cpu(), dev[t].mix_lam.cpu(), sm, 1.0)
        torch.testing.assert_close(vs[t].cpu().double(), ref, **ltol)
    assert bool(torch.isfinite(total))


# ---- captured == eager ---------------------------------------------------------------------------------------------------------------------
FEATURES = ["grad_clip_norm=0.05", f"ema.decay={M.EMA_DECAY}", "ema.warmup=true", "task_weighting.mode=uncertainty",
            "optimizer_state.dtype=bf16", "optimizer_state.rounding=stochastic", f"optimizer_state.seed={M.STATE_SEED}"]


@pytest.mark.parametrize("compute,over", [("f32", ()), ("bf16", ()), ("bf16", tuple(FEATURES))], ids=["f32", "bf16", "bf16-features"])
def test_captured_equals_eager_over_three_steps_with_fresh_fields(compute, over, compute_restored):
    def run(graph):
        step, opt, dev, merged = build(compute, over)
        for k in range(2):  # two eager steps first, in both runs (a capture needs the flat buffers and the learnt slots)
            set_fields(dev, k)
            step.step(dev, merged)
        if graph:
            step.capture(dev, merged, warmup=0)
        for k in range(2, 5):
            set_fields(dev, k)
            step.replay() if graph else step.step(dev, merged)
        snap = snapshot(step, opt)
        snap["loss_sums"] = step.loss_sums()
        if graph:
            assert step.captures == 1, "fresh pairings are values of a fixed shape: no new capture"
        assert bool(torch.isfinite(snap["flat_p"]).all())
        return snap
    eager, graph = run(False), run(True)
    assert eager["t"] == graph["t"] == 5
    same(graph, eager)


# ---- the launch ledger -------------------------------------------------------------------------------------------------------------------
def _ledger(mixed):
    from egopack_amd import ops
    step, opt, dev, merged = build("bf16", batch=8, t_nodes=8)  # (tests/step_matrix_common.py: the size of the banked ONE launch)
    if mixed:
        set_fields(dev, 0)
    for _ in range(2):
        step.step(dev, merged)
    torch.cuda.synchronize()
    ops.prof_enable(True)
    ops.prof_reset()
    try:
        step.step(dev, merged)
        torch.cuda.synchronize()
        return {name: line["launches"] for name, line in ops.prof_report().items() if line["launches"]}
    finally:
        ops.prof_enable(False)


def test_the_launch_ledger_with_and_without_the_fields(compute_restored):
    off, on = _ledger(False), _ledger(True)
    assert "mix_rows" not in off and "ce_mix" not in off, off
    assert off.get("ce_fwd") == 1, off
    assert on.get("mix_rows") == 1 and on.get("ce_mix") == 1 and "ce_fwd" not in on, (on, "the banked AR + LTA chain stays ONE launch")


# ---- the entry point -----------------------------------------------------------------------------------------------------------------------
BASE = ["k=1", "batch_size=4", "synthetic_samples=16", "model.hidden_size=64", "model.temporal_pooling.hidden_size=64", "oscc_feat_size=64",
        "save_model=True", "compute=f32", "optimizer.lr=1e-3", "enabled_tasks=[ar,lta,pnr]", "lr_scheduler.T_max=3", "use_graph=false",
        "mixup.alpha=0.4"]


@pytest.mark.timeout(600)
def test_main_temporal_trains_with_mixup_and_a_resumed_run_equals_the_uninterrupted_one(tmp_path, caplog):
    import main_temporal
    with caplog.at_level(logging.INFO):
        main_temporal.main(BASE + ["num_epochs=2", "save_every=1", f"checkpoint_dir={tmp_path / 'full'}"])
    lines = [r.getMessage() for r in caplog.records if "mixup mean lambda" in r.getMessage()]
    assert len(lines) == 2 and all("'ar'" in l and "'lta'" in l and "'pnr'" not in l for l in lines), lines
    main_temporal.main(BASE + ["num_epochs=1", "save_every=1", f"checkpoint_dir={tmp_path / 'part'}"])
    name = "MTL_ar-lta-pnr"
    part = tmp_path / "part" / name / "checkpoint.pth"
    assert torch.load(part, weights_only=False)["epoch"] == 1
    main_temporal.main(BASE + ["num_epochs=2", f"checkpoint_dir={tmp_path / 'resumed'}", f"resume_from={part}"])
    full = torch.load(tmp_path / "full" / name / "checkpoint.pth", weights_only=False)
    res = torch.load(tmp_path / "resumed" / name / "checkpoint.pth", weights_only=False)
    assert res["epoch"] == 2
    for key in ("temporal_graph", "task/recognition", "task/lta", "task/pnr"):
        for k, v in full[key].items():
            torch.testing.assert_close(res[key][k], v, rtol=0, atol=0, msg=lambda s: f"{key}.{k}: {s}")


@pytest.mark.timeout(600)
def test_main_temporal_mixup_over_the_resident_store_and_the_captured_loop(tmp_path, caplog):
    """dataset_*=synthetic_resident (the native builder's arenas, the feature store's gather) with the training loop's own capture:
    the mixed tasks' batches leave their arenas, the step is captured once and replayed on fresh fields."""
    import main_temporal
    groups = [f"{g}=synthetic_resident" for g in ("dataset_recognition", "dataset_lta", "dataset_oscc", "dataset_pnr")]
    args = [*groups, "k=1", "batch_size=4", "synthetic_samples=48", "model.hidden_size=64", "model.temporal_pooling.hidden_size=64",
            "oscc_feat_size=64", "num_epochs=2", "enabled_tasks=[ar,lta,pnr]", "save_model=True", f"checkpoint_dir={tmp_path}",
            "mixup.alpha=0.4", "mixup.tasks=[ar]"]
    with caplog.at_level(logging.INFO):
        out = main_temporal.main(args)
    ck = torch.load(tmp_path / "MTL_ar-lta-pnr" / "checkpoint.pth", weights_only=False)
    assert ck["epoch"] == 2 and all(torch.isfinite(v).all() for v in ck["temporal_graph"].values() if v.is_floating_point())
    lines = [r.getMessage() for r in caplog.records if "mixup mean lambda" in r.getMessage()]
    assert len(lines) == 2 and all("'ar'" in l and "'lta'" not in l for l in lines), lines
    replayed = [r.getMessage() for r in caplog.records if "steps replayed the captured step" in r.getMessage()]
    assert replayed and any(int(m.split(": ")[1].split()[0]) > 0 for m in replayed), replayed
    assert out["step"].captures <= 2, "fresh pairings are values: the loop's captures are the two input-buffer sets at most"
