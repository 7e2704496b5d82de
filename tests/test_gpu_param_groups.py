"""Parameter groups of the flat optimizers on the GPU (optim.FlatOptimizer over group dicts, egk_optim_step_groups): against the
torch classes on the CPU over the same groups, bit for bit against one egk_optim_step launch per segment, slices against one launch,
one group against the plain path, inside the captured training step, and across a checkpoint."""
import ctypes

import pytest
import torch

from tests import param_groups_common as PG

pytestmark = pytest.mark.gpu
DEV = "cuda"
TOL = dict(rtol=1e-5, atol=1e-6)  # tests/test_gpu_optim_rules.py, this comparison's own
SHAPES = [(33, 7), (5,), (64, 64), (3,), (130, 9)]
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


def gen(seed):
    return torch.Generator().manual_seed(seed)


def _flat(kind, params, **kw):
    from egopack_amd.optim import FlatAdam, FlatAdamW, FlatSGD
    return {"adam": FlatAdam, "adamw": FlatAdamW, "sgd": FlatSGD}[kind](params, **kw)


def _set_grads(params, grads):
    for p, gr in zip(params, grads):
        if p.grad is None:
            p.grad = gr.clone().to(p.device)
        else:
            p.grad.copy_(gr)


def _three_groups(p, extra=()):
    """{0, 2} at lr 1e-2 / wd 1e-2, {1, 3} at lr 1e-2 / wd 0, {4} at lr 1e-3 / wd 1e-2 (``extra``: parameters without a gradient).
    In constructor order the slots are [448 + 4096 | 8 + 8 | 1728]: the boundaries 4544 and 4560 fall inside one wave's 256
    elements (4352 .. 4607) of one 1024-element block (4096 .. 5119)."""
    return [{"params": [p[0], p[2]], "lr": 1e-2, "weight_decay": 1e-2}, {"params": [p[1], p[3]], "lr": 1e-2, "weight_decay": 0.0},
            {"params": [p[4], *extra], "lr": 1e-3, "weight_decay": 1e-2}]


# ---- 1. against the torch class on the CPU ------------------------------------------------------------------------------------------
VARIANTS = {
    "adam": ("adam", torch.optim.Adam, dict()),
    "adamw": ("adamw", torch.optim.AdamW, dict()),
    "sgd-nesterov": ("sgd", torch.optim.SGD, dict(momentum=0.9, nesterov=True)),
    "sgd-plain": ("sgd", torch.optim.SGD, dict()),
}


@pytest.mark.parametrize("scheduled", [False, True], ids=["fixed-lr", "chained-scheduler"])
@pytest.mark.parametrize("name", list(VARIANTS))
def test_three_groups_match_the_torch_class(name, scheduled):
    """Parameters and gradients N(0, 1), 20 steps, compared after steps 1, 2, 5 and 20: parameters and every state buffer.  One
    parameter never gets a gradient.  ``scheduled``: ChainedScheduler(LinearLR, CosineAnnealingLR) stepped every 5 steps on both
    sides -- every group's lr moves, the device table follows without anything being rebuilt."""
    kind, torch_cls, kw = VARIANTS[name]
    g = gen(61)
    ps = [torch.randn(s, generator=g) for s in SHAPES]
    grads = [[torch.randn(s, generator=g) for s in SHAPES] for _ in range(20)]
    cpu = [p.clone().requires_grad_(True) for p in ps]
    unused_cpu = torch.randn(4, generator=g).requires_grad_(True)
    ref = torch_cls(_three_groups(cpu, [unused_cpu]), **kw)
    dev = [p.clone().to(DEV).requires_grad_(True) for p in ps]
    unused = unused_cpu.detach().clone().to(DEV).requires_grad_(True)
    opt = _flat(kind, _three_groups(dev, [unused]), **kw)
    index = {0: 0, 2: 1, 1: 2, 3: 3, 4: 4}  # parameter -> its index in the state dict (groups one after the other)
    keys = opt._state_keys
    scheds = []
    if scheduled:
        L = torch.optim.lr_scheduler
        scheds = [L.ChainedScheduler([L.LinearLR(o, 0.1, 1, 3), L.CosineAnnealingLR(o, T_max=4)]) for o in (ref, opt)]
    for it in range(20):
        _set_grads(cpu, grads[it])
        _set_grads(dev, grads[it])
        ref.step()
        opt.step()
        stepped_on = tuple((g_["lr"], g_["weight_decay"]) for g_ in opt.param_groups)
        if (it + 1) % 5 == 0:
            for s in scheds:
                s.step()
            assert [g_["lr"] for g_ in opt.param_groups] == [g_["lr"] for g_ in ref.param_groups]
        if it + 1 not in (1, 2, 5, 20):
            continue
        sd = opt.state_dict()
        assert sorted(sd["state"]) == list(range(len(ps)))  # (nothing for the parameter without a gradient)
        assert [g_["params"] for g_ in sd["param_groups"]] == [[0, 1], [2, 3], [4, 5]]
        worst = 0.0
        for i, (c, d) in enumerate(zip(cpu, dev)):
            pairs = [(d.detach().cpu(), c.detach())] + [(sd["state"][index[i]][k].cpu(), ref.state[c][k]) for k in keys]
            for got, want in pairs:
                worst = max(worst, float(((got - want).abs() / (TOL["atol"] + TOL["rtol"] * want.abs())).max()))
        print(f"{name}: step {it + 1}, largest |got - want| / (atol + rtol |want|) over parameters and state = {worst:.3f}")
        for i, (c, d) in enumerate(zip(cpu, dev)):
            torch.testing.assert_close(d.detach().cpu(), c.detach(), **TOL, msg=lambda s, i=i: f"step {it + 1}, parameter {i}: {s}")
            for k in keys:
                torch.testing.assert_close(sd["state"][index[i]][k].cpu(), ref.state[c][k], **TOL,
                                           msg=lambda s, i=i, k=k: f"step {it + 1}, {k} of {i}: {s}")
    assert opt.group_segments() == [(0, 4544, 0), (4544, 4560, 1), (4560, 6288, 2)]
    assert torch.equal(unused.detach().cpu(), unused_cpu.detach())  # grad None -> skipped, as torch does
    if scheduled:
        assert stepped_on[0][0] != 1e-2 and opt._group_host == stepped_on  # (the table holds what the last step ran on)


# ---- 2. bit for bit, through the C ABI ----------------------------------------------------------------------------------------------
def _run_groups(prob, begins, seg_group, rows, gate=None, n_groups=None, group_hyper=None):
    """One egk_optim_step_groups launch on fresh device copies of ``prob``; the outputs in the layout of PG.reference."""
    from egopack_amd import _lib
    lib = _lib.load()
    n, ns = prob["n"], prob["n_state"]
    p, g, a, b = (prob[k].to(DEV).clone() for k in ("p", "g", "a", "b"))
    t, hyper = prob["t"].to(DEV), prob["hyper"].to(DEV)  # (hyper[0] = NaN: ignored)
    hi, lo = torch.zeros(n, dtype=BF, device=DEV), torch.zeros(n, dtype=BF, device=DEV)
    word = torch.tensor([100], dtype=torch.int64, device=DEV)
    gt = torch.tensor([gate], dtype=torch.int32, device=DEV) if gate is not None else None
    sb = torch.tensor(begins, dtype=torch.int64, device=DEV)
    sg = torch.tensor(seg_group, dtype=torch.int32, device=DEV)
    gh = PG.hyper_rows(rows).to(DEV) if group_hyper is None else group_hyper
    d = PG.descriptor(prob["kind"], prob["gdt"], n, p.data_ptr(), g.data_ptr(), a.data_ptr() if ns >= 1 else 0, b.data_ptr() if ns >= 2 else 0,
                      hyper.data_ptr(), t.data_ptr(), hi.data_ptr(), lo.data_ptr(), word.data_ptr(), gt.data_ptr() if gt is not None else None)
    tab = PG.group_table(0, sb, sg, gh, n_groups=n_groups if n_groups is not None else len(rows))
    assert lib.egk_optim_step_groups(PG.stream(), ctypes.byref(d), ctypes.byref(tab)) == 0, _lib.last_error()
    torch.cuda.synchronize()
    out = dict(p=p.cpu(), hi=hi.view(torch.int16).cpu(), lo=lo.view(torch.int16).cpu(), word=word.cpu())
    if ns >= 1:
        out["state0"] = a.cpu()
    if ns >= 2:
        out["state1"] = b.cpu()
    return out


def _same(got, want, what):
    assert sorted(got) == sorted(want), what
    for k in want:
        assert torch.equal(got[k], want[k]), (what, k, int((got[k] != want[k]).sum()))


@pytest.mark.parametrize("gate", [None, 1, 0], ids=["no-gate", "gate-open", "gate-closed"])
@pytest.mark.parametrize("gdt", [torch.float32, BF], ids=["f32", "bf16"])
@pytest.mark.parametrize("kind", list(PG.KINDS))
def test_groups_equal_one_plain_launch_per_segment_bit_for_bit(kind, gdt, gate):
    """n = 1003 (one block, a scalar tail) and n = 300007 (workgroup blocks wholly inside a segment beside blocks that straddle):
    a table of ONE group gives egk_optim_step's bits for that lr / weight_decay, five segments over three groups the bits of five
    egk_optim_step launches over the sub-ranges -- p, the state, both bf16 copies, the offset word.  A closed gate changes
    nothing but the word."""
    for n in (1003, 300007):
        prob = PG.problem(n, kind, gdt)
        begins = PG.SEG_BEGINS[n]
        one = _run_groups(prob, [0, begins[-1]], [0], [PG.ONE_GROUP], gate)
        five = _run_groups(prob, begins, PG.SEG_GROUPS, PG.GROUP_HYPER, gate)
        assert one["word"].tolist() == five["word"].tolist() == [107]
        if gate == 0:
            for out in (one, five):
                assert torch.equal(out["p"], prob["p"]) and not out["hi"].any() and not out["lo"].any()
                assert "state0" not in out or torch.equal(out["state0"], prob["a"])
                assert "state1" not in out or torch.equal(out["state1"], prob["b"])
            continue
        _same(one, PG.reference(prob, [0, begins[-1]], [0], [PG.ONE_GROUP], gate=gate), (n, "one group"))
        ref = PG.reference(prob, begins, PG.SEG_GROUPS, PG.GROUP_HYPER, gate=gate)
        _same(five, ref, (n, "five segments"))
        assert not torch.equal(one["p"], five["p"]) and not torch.equal(ref["p"], prob["p"]) and bool(torch.isfinite(ref["p"]).all())


@pytest.mark.parametrize("kind", ["adamw", "sgd_momentum"])
def test_an_out_of_range_group_id_is_clamped_into_the_table(kind):
    """``seg_group`` holds ids outside [0, n_groups): the kernel clamps them, so the rows around ``group_hyper`` -- NaN here, the
    guard of a sentinel-filled window -- are never read: the outputs are finite and equal those of the clamped table."""
    from tests.guarded import Guarded1D
    n = 4099
    prob = PG.problem(n, kind, torch.float32)
    window = Guarded1D(12, torch.float32, DEV, init=PG.hyper_rows(PG.GROUP_HYPER).reshape(-1))
    assert window.ptr % 16 == 0
    wild, clamped = [7, -3, 1, 64, -(1 << 31)], [2, 0, 1, 2, 0]
    got = _run_groups(prob, PG.SEG_BEGINS[n], wild, PG.GROUP_HYPER, n_groups=3, group_hyper=window.ptr)
    window.assert_untouched("group_hyper")
    assert all(bool(torch.isfinite(got[k]).all()) for k in ("p", "state0"))
    _same(got, PG.reference(prob, PG.SEG_BEGINS[n], clamped, PG.GROUP_HYPER), "clamped")


# ---- 3. slices equal one launch --------------------------------------------------------------------------------------------------------
RULES = [("adam", dict()), ("adamw", dict()), ("sgd", dict(momentum=0.9, dampening=0.1))]


def _pair(kind, seed=5, **kw):
    """Two three-group optimizers of one rule over equal parameters, flat buffers built, low halves allocated."""
    g = gen(seed)
    ps = [torch.randn(s, generator=g) for s in SHAPES]
    grads = [[torch.randn(s, generator=g) for s in SHAPES] for _ in range(3)]
    out = []
    for _ in range(2):
        dev = [p.clone().to(DEV).requires_grad_(True) for p in ps]
        opt = _flat(kind, _three_groups(dev), **kw)
        _set_grads(dev, grads[0])
        opt._materialise()
        opt.ensure_lo_shadows()
        opt.refresh_lo_shadows()
        out.append((opt, dev))
    return out, grads


def _bits(opt):
    torch.cuda.synchronize()
    bufs = [opt.flat_p, *opt.state_buffers(), opt.flat_w16.view(torch.int16), opt._t_dev]
    if opt.flat_w16lo is not None:
        bufs.append(opt.flat_w16lo.view(torch.int16))
    return [b.clone() for b in bufs]


@pytest.mark.parametrize("kind,kw", RULES, ids=[r[0] for r in RULES])
def test_three_slices_equal_one_launch(kind, kw):
    """``launch()`` once against ``launch(None, lo, hi)`` over three ranges cut at multiples of 8 that are no segment boundaries
    (what dist.GradSync's chunks and the engine's early and tail slices do): bit for bit over two steps."""
    (one, dev1), (three, dev3) = _pair(kind, **kw)[0]
    grads = _pair(kind, **kw)[1]
    n = one.flat_p.numel()
    cuts = [0, 4552, 5000, n]  # (4552: between the boundaries 4544 and 4560, inside group 1's segment)
    bounds = {b for b, _, _ in one.group_segments()} | {n}
    assert all(c % 8 == 0 for c in cuts) and not set(cuts[1:-1]) & bounds and len(one.group_segments()) == 3
    for it in range(2):
        _set_grads(dev1, grads[it])
        _set_grads(dev3, grads[it])
        one.prepare_hyper()
        one.launch()
        one.step_count += 1
        three.prepare_hyper()
        for lo, hi in zip(cuts[:-1], cuts[1:]):
            three.launch(None, lo, hi)
        three.step_count += 1
        for x, y in zip(_bits(one), _bits(three)):
            assert torch.equal(x, y), it
    assert int(one._t_dev.item()) == 2


# ---- 4. one group is the old path ------------------------------------------------------------------------------------------------------
def _counted_steps(opt, dev, grads, steps=3):
    from egopack_amd import _lib
    from tests.test_gpu_bounds import _counted
    _set_grads(dev, grads[0])
    opt._materialise()  # (its cast launch stays outside the count)
    with _counted(_lib.load()) as c:
        for it in range(steps):
            _set_grads(dev, grads[it])
            opt.step()
    return c.names, _bits(opt)


@pytest.mark.parametrize("kind,kw", RULES, ids=[r[0] for r in RULES])
def test_one_group_is_the_plain_path_and_equal_groups_change_no_bit(kind, kw):
    """A plain list, a single group dict, and two groups with the SAME lr / weight_decay over the same parameters and gradients,
    three steps each.  The single dict issues the plain entry points (``optim_groups`` records no launch) and gives the plain
    list's bits; the two equal groups go through egk_optim_step_groups and still give those bits: the lookup changes no arithmetic."""
    g = gen(7)
    ps = [torch.randn(s, generator=g) for s in SHAPES]
    grads = [[torch.randn(s, generator=g) for s in SHAPES] for _ in range(3)]
    fresh = lambda: [p.clone().to(DEV).requires_grad_(True) for p in ps]
    hp = dict(lr=1e-2, weight_decay=1e-2, **kw)
    plain_entry = "adam" if kind == "adam" else "optim"
    dev = fresh()
    names, plain = _counted_steps(_flat(kind, dev, **hp), dev, grads)
    assert names.get(plain_entry) == 3 and "optim_groups" not in names, names
    dev = fresh()
    names, single = _counted_steps(_flat(kind, [{"params": dev}], **hp), dev, grads)
    assert names.get(plain_entry) == 3 and "optim_groups" not in names, names
    dev = fresh()
    opt = _flat(kind, [{"params": [dev[0], dev[2], dev[4]]}, {"params": [dev[1], dev[3]]}], layout_order=dev, **hp)
    names, two = _counted_steps(opt, dev, grads)
    assert names.get("optim_groups") == 3 and "optim" not in names and "adam" not in names, names
    assert [s[2] for s in opt.group_segments()] == [0, 1, 0, 1, 0]
    for a, b, c in zip(plain, single, two):
        assert torch.equal(a, b), "a single group dict differs from the plain list"
        assert torch.equal(a, c), "two groups of equal lr / weight_decay differ from the plain list"
    assert float(plain[0].abs().max()) > 0


# ---- 5. in the step ---------------------------------------------------------------------------------------------------------------------
def _build_step(clip=0.0):
    """The small MTLStep workload of tests/test_gpu_optim_step.py under AdamW with ``no_decay_1d`` and the backbone at half the
    learning rate, built the way the entry points build it; f32 contractions, dropout off."""
    import bench
    from egopack_amd import engine, ops
    from egopack_amd import train as T
    args = bench.parse_args(["--workload", "mtl", "--batch", "8", "--T", "8", "--hidden", "128", "--trn-hidden", "256", "--dropout", "0.0"])
    args.compute = "f32"
    ops.set_compute("f32")
    ops.manual_seed(11)
    model, tasks, crit, weights, dev, merged = bench.build_workload(args, 0, torch.device(DEV))
    model.to(DEV).train()
    for t in tasks.values():
        t.to(DEV).train()
    cfg = T.load_config(["optimizer._target_=torch.optim.AdamW", "optimizer.lr=1e-2", "optimizer.weight_decay=1e-2",
                         "param_groups.no_decay_1d=true", "param_groups.lr_scale.temporal_graph=0.5", f"grad_clip_norm={clip}"])
    flat = [*model.configure_optimizers(0), *(p for t in ("ar", "oscc", "lta", "pnr") for p in tasks[t].configure_optimizers(0))]
    opt = T.build_optimizer(cfg, T.build_param_groups(cfg, model, tasks), layout_order=flat)
    step = engine.MTLStep(model, tasks, crit, weights, opt, fused_backbone=True)
    return step, opt, dev, merged


def _state(opt):
    torch.cuda.synchronize()
    return [t.clone().cpu() for t in (opt.flat_p, *opt.state_buffers(), opt.flat_w16.view(torch.int16), opt._t_dev)]


@pytest.mark.parametrize("clip", [0.0, 1.0], ids=["no-clip", "clip-1.0"])
def test_grouped_step_captured_and_replayed_equals_eager_bit_for_bit(clip, compute_restored):
    """Two eager steps, the capture and three replays against five eager steps; then a scheduler step and one more step on both
    sides: the replay reads the new per-group learning rates from the device table, nothing is captured again.  With clipping the
    epoch's gradient-norm statistics are identical too."""
    def run(use_graph):
        step, opt, dev, merged = _build_step(clip)
        assert [(g["name"], g["lr"], g["weight_decay"]) for g in opt.param_groups] == [
            ("temporal_graph", 5e-3, 1e-2), ("temporal_graph/no_decay", 5e-3, 0.0), ("tasks", 1e-2, 1e-2), ("tasks/no_decay", 1e-2, 0.0)]
        sched = torch.optim.lr_scheduler.StepLR(opt, 1, gamma=0.25)
        if use_graph:
            step.capture(dev, merged, warmup=2)
            graph = step._graph
            for _ in range(3):
                step.replay()
        else:
            for _ in range(5):
                step.step(dev, merged)
        five, table = _state(opt), opt._group_hyper.clone()
        sched.step()
        if use_graph:
            step.replay()
            assert step._graph is graph
        else:
            step.step(dev, merged)
        six = _state(opt)
        assert not torch.equal(table, opt._group_hyper) and float(opt._group_hyper[0, 0]) == pytest.approx(1.25e-3)
        assert len(opt.group_segments()) > 8 and opt.grouped
        return five, six, (opt.grad_norm_stats() if clip else None)
    eager, graph = run(False), run(True)
    assert int(eager[0][-1]) == int(graph[0][-1]) == 5 and int(eager[1][-1]) == int(graph[1][-1]) == 6
    for which, (e, g) in enumerate(zip(eager[:2], graph[:2])):
        for i, (a, b) in enumerate(zip(e, g)):
            assert torch.equal(a, b), f"after step {5 + which}: captured and eager differ in buffer {i}: max abs {float((a.float() - b.float()).abs().max()):.3e}"
    assert not torch.equal(eager[0][0], eager[1][0])
    if clip:
        assert eager[2] == graph[2] and eager[2]["steps"] == 6 and eager[2]["clipped"] > 0, (eager[2], graph[2])


# ---- 6. resume --------------------------------------------------------------------------------------------------------------------------
BASE = ["k=1", "batch_size=4", "synthetic_samples=16", "model.hidden_size=64", "model.temporal_pooling.hidden_size=64",
        "oscc_feat_size=64", "save_model=True", "compute=f32", "optimizer.lr=1e-3", "enabled_tasks=[ar,pnr]",
        "optimizer._target_=torch.optim.AdamW", "optimizer.weight_decay=1e-2", "param_groups.no_decay_1d=true",
        "param_groups.lr_scale.temporal_graph=0.5"]


@pytest.mark.timeout(900)
def test_main_temporal_resume_with_groups_equals_uninterrupted_run(tmp_path):
    """tests/test_gpu_optim_step.py::test_main_temporal_resume_equals_uninterrupted_run with parameter groups: 3 epochs in one go ==
    2 epochs, the save_every checkpoint, resume, 1 more epoch -- bit for bit; the checkpoint holds torch's multi-group layout."""
    import main_temporal
    base = BASE + ["lr_scheduler.T_max=3", "use_graph=false", "save_every=2"]
    main_temporal.main(base + ["num_epochs=3", f"checkpoint_dir={tmp_path / 'full'}"])
    main_temporal.main(base + ["num_epochs=2", f"checkpoint_dir={tmp_path / 'part'}"])
    part = tmp_path / "part" / "MTL_ar-pnr" / "checkpoint.pth"
    ck = torch.load(part, weights_only=False)
    groups = ck["optimizer"]["param_groups"]
    assert ck["epoch"] == 2 and [g["name"] for g in groups] == ["temporal_graph", "temporal_graph/no_decay", "tasks", "tasks/no_decay"]
    assert [g["weight_decay"] for g in groups] == [1e-2, 0.0, 1e-2, 0.0] and groups[0]["lr"] == pytest.approx(0.5 * groups[2]["lr"])
    assert groups[0]["lr"] < 0.5e-3 and [i for g in groups for i in g["params"]] == list(range(sum(len(g["params"]) for g in groups)))
    out = main_temporal.main(base + ["num_epochs=3", f"checkpoint_dir={tmp_path / 'resumed'}", f"resume_from={part}"])
    assert out["step"].optimizer.grouped
    full = torch.load(tmp_path / "full" / "MTL_ar-pnr" / "checkpoint.pth", weights_only=False)
    res = torch.load(tmp_path / "resumed" / "MTL_ar-pnr" / "checkpoint.pth", weights_only=False)
    assert res["epoch"] == 3
    moved = 0.0
    for key in ("temporal_graph", "task/recognition", "task/pnr"):
        for k, v in full[key].items():
            torch.testing.assert_close(res[key][k], v, rtol=0, atol=0, msg=lambda s: f"{key}.{k}: {s}")
            if v.is_floating_point():
                moved = max(moved, float((v - ck[key][k]).abs().max()))
    assert moved > 0  # (the third epoch trained)
    assert sorted(full["optimizer"]["state"]) == sorted(res["optimizer"]["state"])
    for i, st in full["optimizer"]["state"].items():
        for k in ("exp_avg", "exp_avg_sq"):
            assert torch.equal(st[k], res["optimizer"]["state"][i][k]), (i, k)
        assert float(st["step"]) == float(res["optimizer"]["state"][i]["step"]) > 0
    assert [(g["lr"], g["weight_decay"]) for g in full["optimizer"]["param_groups"]] == \
           [(g["lr"], g["weight_decay"]) for g in res["optimizer"]["param_groups"]]
