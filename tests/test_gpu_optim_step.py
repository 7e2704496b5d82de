"""AdamW and SGD inside the training step (engine.MTLStep): eager steps against the torch class, capture and replay against eager
(with and without the optimizer slice beside the step's last weight-gradient launch), clipping and skipped steps, and the
main_temporal.py entry point with ``optimizer._target_`` set (checkpoints the torch classes load; resume = uninterrupted)."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
TOL = dict(rtol=1e-5, atol=1e-6)  # tests/test_gpu_kernels.py::test_flat_adam_matches_torch_adam
SHAPES = [(33, 7), (5,), (64, 64), (3,)]

RULES = {
    "adamw": ("adamw", torch.optim.AdamW, dict(weight_decay=1e-2)),
    "sgd": ("sgd", torch.optim.SGD, dict(weight_decay=1e-3)),
    "sgd-momentum": ("sgd", torch.optim.SGD, dict(momentum=0.9, dampening=0.1)),
    "sgd-nesterov": ("sgd", torch.optim.SGD, dict(momentum=0.9, nesterov=True, weight_decay=1e-3)),
}


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
    from egopack_amd.optim import FlatAdamW, FlatSGD
    return {"adamw": FlatAdamW, "sgd": FlatSGD}[kind](params, **kw)


def _build(rule, compute="bf16", lr=1e-2, max_grad_norm=None, dropout="0.0"):
    """The small MTLStep workload of tests/test_gpu_grad_clip.py (AR + LTA + PNR, fused backbone) under the given rule."""
    import bench
    from egopack_amd import engine, ops
    kind, _, kw = RULES[rule]
    args = bench.parse_args(["--workload", "mtl", "--batch", "8", "--T", "8", "--hidden", "128", "--trn-hidden", "256", "--dropout", dropout])
    args.compute = compute
    ops.set_compute(compute)
    ops.manual_seed(11)
    model, tasks, crit, weights, dev, merged = bench.build_workload(args, 0, torch.device(DEV))
    model.to(DEV).train()
    for t in tasks.values():
        t.to(DEV).train()
    params = [*model.parameters(), *(p for t in tasks.values() for p in t.parameters())]
    opt = _flat(kind, params, lr=lr, max_grad_norm=max_grad_norm, **kw)
    step = engine.MTLStep(model, tasks, crit, weights, opt, fused_backbone=True)
    return step, opt, dev, merged


def _state(opt):
    torch.cuda.synchronize()
    return [t.clone().cpu() for t in (opt.flat_p, *opt.state_buffers(), opt.flat_w16.view(torch.int16), opt._t_dev)]


# ---- 1. eager steps against torch ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rule", list(RULES))
def test_eager_steps_match_the_torch_class(rule, compute_restored):
    """Three eager steps; after each, the parameters against the torch class on the CPU applied to the parameters before the step
    and the gradient the step left in ``flat_g`` (one flat CPU parameter; the torch optimizer keeps its own state over the steps)."""
    _, torch_cls, kw = RULES[rule]
    lr = 1e-2
    step, opt, dev, merged = _build(rule, lr=lr)
    q = torch.zeros(0, requires_grad=True)
    ref = None
    for it in range(3):
        if it == 0:  # (the first step builds the flat buffers: backward, then the layout, then the optimizer)
            step.forward_backward(dev, merged)
            opt._materialise()
            before = opt.flat_p.clone().cpu()
            opt.step()
        else:
            before = opt.flat_p.clone().cpu()
            step.step(dev, merged)
        torch.cuda.synchronize()
        if ref is None:
            q = before.clone().requires_grad_(True)
            ref = torch_cls([q], lr=lr, **kw)
        with torch.no_grad():
            q.copy_(before)
        q.grad = (opt.flat_g.cpu() * opt.grad_scale)
        assert float(q.grad.abs().max()) > 0
        ref.step()
        got = opt.flat_p.cpu()
        moved = float((got - before).abs().max())
        worst = float(((got - q.detach()).abs() / (TOL["atol"] + TOL["rtol"] * q.detach().abs())).max())
        print(f"{rule}: step {it + 1}, parameters moved by up to {moved:.3e}, largest error / tolerance {worst:.3f}")
        assert moved > 100 * TOL["atol"]
        torch.testing.assert_close(got, q.detach(), **TOL, msg=lambda s: f"step {it + 1}: {s}")
        for buf, key in zip(opt.state_buffers(), opt._state_keys):
            torch.testing.assert_close(buf.cpu(), ref.state[q][key], **TOL, msg=lambda s: f"step {it + 1}, {key}: {s}")
    assert int(opt._t_dev.item()) == 3 == opt.step_count


# ---- 2. capture and replay ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("early", [True, False], ids=["early-slice", "one-launch"])
@pytest.mark.parametrize("rule", list(RULES))
def test_captured_and_replayed_steps_equal_eager_bit_for_bit(rule, early, compute_restored):
    """Four steps: eager against capture (two warm-up steps) + two replays, f32 contractions (the arithmetic of an eager and of a
    captured step is then the same launch for launch); parameters, state, bf16 copies and the step counter.  ``early``: the
    optimizer slice beside the step's last weight-gradient launch (the default of MTLStep) or one launch at the end."""
    def run(use_graph):
        step, opt, dev, merged = _build(rule, compute="f32")
        step.early_adam = early
        if use_graph:
            step.capture(dev, merged, warmup=2)
            for _ in range(2):
                step.replay()
            assert (step._adam_stream is not None) == early  # (the slice beside the tail launch was planned, or was not)
        else:
            for _ in range(4):
                step.step(dev, merged)
        return _state(opt)
    eager, graph, graph2 = run(False), run(True), run(True)
    assert int(eager[-1]) == int(graph[-1]) == 4
    for i, (a, b, c) in enumerate(zip(eager, graph, graph2)):
        assert torch.equal(b, c), f"two captured runs differ in buffer {i}"
        assert torch.equal(a, b), f"captured and eager differ in buffer {i}: max abs {float((a.float() - b.float()).abs().max()):.3e}"


# ---- 3. clipping ----------------------------------------------------------------------------------------------------------------------
def _set_grads(params, grads):
    for p, gr in zip(params, grads):
        if p.grad is None:
            p.grad = gr.clone().to(p.device)
        else:
            p.grad.copy_(gr)


@pytest.mark.parametrize("rule", ["adamw", "sgd", "sgd-nesterov"])
def test_clipped_rule_matches_clip_grad_norm_and_the_torch_class(rule):
    """tests/test_gpu_grad_clip.py::test_clipped_flat_adam_matches_clip_grad_norm_and_torch_adam for AdamW and for SGD with weight
    decay: the coefficient multiplies the gradient BEFORE weight decay.  The second of five steps has a gradient that is not
    finite: it is skipped (nothing changes, the device counter stays at 1) and the torch class does not see it."""
    kind, torch_cls, kw = RULES[rule]
    g = gen(61)
    ps = [torch.randn(s, generator=g) for s in SHAPES]
    scales = [5.0, 1.0, 1e-3, 5.0, 1e-3]
    grads = [[torch.randn(s, generator=g) * sc for s in SHAPES] for sc in scales]
    cpu = [p.clone().requires_grad_(True) for p in ps]
    plain = [p.clone().requires_grad_(True) for p in ps]
    ref, ref_plain = torch_cls(cpu, lr=1e-2, **kw), torch_cls(plain, lr=1e-2, **kw)  # (plain: WITHOUT clipping -- does the case discriminate?)
    dev = [p.clone().to(DEV).requires_grad_(True) for p in ps]
    opt = _flat(kind, dev, lr=1e-2, max_grad_norm=1.0, **kw)
    coefs = []
    for it in range(5):
        _set_grads(dev, grads[it])
        if it == 1:
            dev[2].grad.view(-1)[77] = float("inf")
            before = _state(opt)
            opt.step()
            for a, b in zip(before, _state(opt)):
                assert torch.equal(a, b)
            assert int(opt._t_dev.item()) == 1
            continue
        _set_grads(cpu, grads[it])
        _set_grads(plain, grads[it])
        total_norm = torch.nn.utils.clip_grad_norm_(cpu, 1.0)
        coefs.append(min(1.0, float(1.0 / (total_norm + 1e-6))))
        ref.step()
        ref_plain.step()
        opt.step()
    assert any(c < 1 for c in coefs) and any(c == 1.0 for c in coefs), coefs
    sd = opt.state_dict()["state"]
    disc = lambda a, b: bool(((a - b).abs() > 100 * (TOL["atol"] + TOL["rtol"] * b.abs())).any())
    for i, (c, pl, d) in enumerate(zip(cpu, plain, dev)):
        assert disc(c.detach(), pl.detach()), i
        torch.testing.assert_close(d.detach().cpu(), c.detach(), **TOL)
        for k in opt._state_keys:
            assert disc(ref.state[c][k], ref_plain.state[pl][k]), (i, k)
            torch.testing.assert_close(sd[i][k].cpu(), ref.state[c][k], **TOL)
        assert float(sd[i]["step"]) == 4  # (the device counter: the skipped step is not in it)
    stats = opt.grad_norm_stats()
    assert stats["steps"] == 5 and stats["skipped"] == 1 and stats["clipped"] == sum(c < 1 for c in coefs)


def test_sgd_first_step_survives_a_skipped_first_step():
    """The FIRST step is the one that is skipped: the next one stores the (clipped) gradient as the buffer, as torch's first step."""
    g = gen(7)
    ps = [torch.randn(s, generator=g) for s in SHAPES]
    grads = [[torch.randn(s, generator=g) * 5 for s in SHAPES] for _ in range(3)]
    cpu = [p.clone().requires_grad_(True) for p in ps]
    ref = torch.optim.SGD(cpu, lr=1e-2, momentum=0.9, dampening=0.1)
    dev = [p.clone().to(DEV).requires_grad_(True) for p in ps]
    opt = _flat("sgd", dev, lr=1e-2, momentum=0.9, dampening=0.1, max_grad_norm=1.0)
    _set_grads(dev, grads[0])
    dev[0].grad.view(-1)[3] = float("nan")
    opt.step()
    assert int(opt._t_dev.item()) == 0 and not opt.state_buffers()[0].any()
    for it in (1, 2):
        _set_grads(dev, grads[it])
        _set_grads(cpu, grads[it])
        torch.nn.utils.clip_grad_norm_(cpu, 1.0)
        ref.step()
        opt.step()
        sd = opt.state_dict()["state"]
        for i, (c, d) in enumerate(zip(cpu, dev)):
            torch.testing.assert_close(d.detach().cpu(), c.detach(), **TOL)
            torch.testing.assert_close(sd[i]["momentum_buffer"].cpu(), ref.state[c]["momentum_buffer"], **TOL)
    # (with dampening 0.1 a first-step branch taken twice, or not at all, is off by 10 % of the gradient in the buffer)


# ---- 4. the entry point -----------------------------------------------------------------------------------------------------------
BASE = ["k=1", "batch_size=4", "synthetic_samples=16", "model.hidden_size=64", "model.temporal_pooling.hidden_size=64",
        "oscc_feat_size=64", "save_model=True", "compute=f32", "optimizer.lr=1e-3", "enabled_tasks=[ar,pnr]"]
TARGETS = {"adamw": (["optimizer._target_=torch.optim.AdamW", "optimizer.weight_decay=1e-2"], ("exp_avg", "exp_avg_sq")),
           "sgd": (["optimizer._target_=torch.optim.SGD", "+optimizer.momentum=0.9", "+optimizer.dampening=0.1"], ("momentum_buffer",))}


@pytest.mark.timeout(600)
def test_main_temporal_trains_with_adamw_and_writes_a_state_torch_adamw_loads(tmp_path):
    import main_temporal
    from egopack_amd.optim import FlatAdamW
    out = main_temporal.main(BASE + ["num_epochs=2", f"checkpoint_dir={tmp_path}", "optimizer._target_=torch.optim.AdamW"])
    opt = out["step"].optimizer
    assert type(opt) is FlatAdamW and opt.param_groups[0]["weight_decay"] == 1e-5 and opt.step_count > 0
    ck = torch.load(tmp_path / "MTL_ar-pnr" / "checkpoint.pth", weights_only=False)
    assert all(torch.isfinite(v).all() for v in ck["temporal_graph"].values() if v.is_floating_point())
    sd = ck["optimizer"]
    assert sd["state"] and all(set(st) == {"step", "exp_avg", "exp_avg_sq"} for st in sd["state"].values())
    assert sd["param_groups"][0]["decoupled_weight_decay"] is True
    params = [torch.zeros_like(p, device="cpu").requires_grad_(True) for p in opt.param_groups[0]["params"]]
    ref = torch.optim.AdamW(params, lr=1e-3)
    ref.load_state_dict(sd)
    assert ref.param_groups[0]["weight_decay"] == 1e-5 and ref.param_groups[0]["decoupled_weight_decay"] is True
    for i, st in sd["state"].items():
        assert torch.equal(ref.state[params[i]]["exp_avg_sq"], st["exp_avg_sq"]) and float(ref.state[params[i]]["step"]) == opt.step_count
        params[i].grad = torch.ones_like(params[i])
    ref.step()  # (torch steps on from the loaded state)
    assert all(torch.isfinite(p).all() for p in params)


@pytest.mark.timeout(900)
@pytest.mark.parametrize("rule", list(TARGETS))
def test_main_temporal_resume_equals_uninterrupted_run(rule, tmp_path):
    """tests/test_gpu_entrypoints.py::test_main_temporal_resume_equals_uninterrupted_run under AdamW and under SGD (momentum 0.9,
    dampening 0.1): 3 epochs in one go == 2 epochs, the save_every checkpoint, resume, 1 more epoch -- bit for bit."""
    import main_temporal
    over, keys = TARGETS[rule]
    base = BASE + over + ["lr_scheduler.T_max=3", "use_graph=false", "save_every=2"]
    main_temporal.main(base + ["num_epochs=3", f"checkpoint_dir={tmp_path / 'full'}"])
    main_temporal.main(base + ["num_epochs=2", f"checkpoint_dir={tmp_path / 'part'}"])
    part = tmp_path / "part" / "MTL_ar-pnr" / "checkpoint.pth"
    ck = torch.load(part, weights_only=False)
    assert ck["epoch"] == 2 and all(set(st) == {"step", *keys} for st in ck["optimizer"]["state"].values())
    out = main_temporal.main(base + ["num_epochs=3", f"checkpoint_dir={tmp_path / 'resumed'}", f"resume_from={part}"])
    assert out["step"].optimizer._state_keys == keys
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
    for i, st in full["optimizer"]["state"].items():
        for k in keys:
            assert torch.equal(st[k], res["optimizer"]["state"][i][k]), (i, k)
        assert float(st["step"]) == float(res["optimizer"]["state"][i]["step"]) > 0
