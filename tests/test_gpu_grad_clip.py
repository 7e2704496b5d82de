"""Global-norm gradient clipping inside the step (optim.FlatAdam ``max_grad_norm``, configuration key ``grad_clip_norm``):
the norm kernels, the optimizer against torch.nn.utils.clip_grad_norm_ + torch.optim.Adam, skipped steps, the eager and
the captured training steps, the entry point.

Adam's update is nearly invariant to a constant scale of the gradient, so a comparison of PARAMETERS alone can pass with
clipping broken: every parity test here compares ``exp_avg`` (scales with the coefficient) and ``exp_avg_sq`` (with its
square) too, and first checks on the reference's own numbers that the case discriminates."""
import ctypes
import logging
import math

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
TOL = dict(rtol=1e-5, atol=1e-6)  # tests/test_gpu_kernels.py::test_flat_adam_matches_torch_adam
CONFIG3_FLAT = 25003272  # elements of the flat buffers of BASELINE config 3 (AR + LTA + PNR, H = Hp = 1024: FlatAdam's slot rule)


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


def gen(seed):
    return torch.Generator().manual_seed(seed)


def _partials(x, lo, hi):
    """The kernel's partial sums of x[lo:hi] (a device tensor, f32 or bf16)."""
    from egopack_amd import _lib
    from egopack_amd.ops import _ck, _p, _stream
    lib = _lib.load()
    k = lib.egk_grad_sumsq_slots(hi - lo)
    out = torch.full((k + 2,), -1.0, dtype=torch.float64, device=DEV)  # (two guard words behind the slot range)
    _ck(lib.egk_grad_sumsq(_stream(), _p(x[lo:hi]), 1 if x.dtype == torch.bfloat16 else 0, hi - lo, _p(out), k), "egk_grad_sumsq")
    torch.cuda.synchronize()
    assert out[k:].tolist() == [-1.0, -1.0]
    return out[:k].cpu()


# ---- 2. the norm kernel -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("n", [1, 7, 8, 4097, 2 ** 20 + 3, CONFIG3_FLAT])
def test_sum_of_squares_kernel(n, dtype):
    """Against x.double().pow(2).sum() of the same stored values: relative error <= 2 n 2^-53 (the products of two f32 or bf16
    values are exact in f64, only the n additions round, in the kernel and in torch's f64 sum alike); whole buffers and inner
    slices at offsets the flat layout produces (multiples of 8 elements); two launches give bit-identical partial sums."""
    from egopack_amd import _lib
    g = torch.Generator(device=DEV).manual_seed(n % 1000 + 7)
    x = (torch.randn(n, device=DEV, generator=g) * 3).to(dtype)
    assert _lib.load().egk_grad_sumsq_slots(n) == min(1024, (n + 16383) // 16384)
    slices = [(0, n)]
    if n > 64:
        slices += [(8, n), (n // 3 // 8 * 8, n // 2 // 8 * 8), (n // 2 // 8 * 8, n // 8 * 8)]
    for lo, hi in slices:
        a, b = _partials(x, lo, hi), _partials(x, lo, hi)
        assert torch.equal(a, b), (n, lo, hi)
        got = math.fsum(a.tolist())
        want = float(x[lo:hi].double().pow(2).sum())
        rel = abs(got - want) / want
        print(f"sumsq n={n} {dtype} [{lo}, {hi}): {len(a)} partials, relative error {rel:.3e}, bound {2 * (hi - lo) * 2.0 ** -53:.3e}")
        assert rel <= 2 * (hi - lo) * 2.0 ** -53, (n, lo, hi, rel)


def test_sum_of_squares_kernel_refuses_what_the_flat_layout_never_produces():
    from egopack_amd import _lib
    lib = _lib.load()
    x = torch.zeros(64, device=DEV)
    out = torch.zeros(4, dtype=torch.float64, device=DEV)
    p = lambda t, off=0: ctypes.c_void_p(t.data_ptr() + off)
    assert lib.egk_grad_sumsq(None, p(x, 4), 0, 32, p(out), 1) == -1 and "16-byte aligned" in _lib.last_error()
    assert lib.egk_grad_sumsq(None, p(x), 0, 32, p(out), 2) == -1 and "partial sums" in _lib.last_error()
    assert lib.egk_grad_sumsq(None, p(x), 0, 0, p(out), 0) == -1 and "n >= 1" in _lib.last_error()
    assert lib.egk_grad_sumsq(None, None, 0, 32, p(out), 1) == -1 and "null pointer" in _lib.last_error()
    assert lib.egk_grad_sumsq_slots(0) == 0 and lib.egk_grad_sumsq_slots(1) == 1 and lib.egk_grad_sumsq_slots(1 << 40) == 1024
    torch.cuda.synchronize()
    assert float(out.abs().sum()) == 0.0  # (nothing was launched)


# ---- 3. the optimizer against torch ---------------------------------------------------------------------------------------------
SHAPES = [(33, 7), (5,), (64, 64), (3,)]


def _set_grads(params, grads):
    for p, gr in zip(params, grads):
        if p.grad is None:
            p.grad = gr.clone().to(p.device)
        else:
            p.grad.copy_(gr)


def _moments(opt, i):
    st = opt.state_dict()["state"][i]
    return st["exp_avg"].cpu(), st["exp_avg_sq"].cpu(), float(st["step"])


def _discriminates(a, b, factor=100):
    """|a - b| exceeds ``factor`` x the tolerance of TOL somewhere."""
    return bool(((a - b).abs() > factor * (TOL["atol"] + TOL["rtol"] * b.abs())).any())


def test_clipped_flat_adam_matches_clip_grad_norm_and_torch_adam():
    from egopack_amd.optim import FlatAdam
    g = gen(61)
    ps = [torch.randn(s, generator=g) for s in SHAPES]
    scales = [5.0, 1e-3, 5.0, 1e-3]
    grads = [[torch.randn(s, generator=g) * sc for s in SHAPES] for sc in scales]
    cpu = [p.clone().requires_grad_(True) for p in ps]
    plain = [p.clone().requires_grad_(True) for p in ps]
    ref = torch.optim.Adam(cpu, lr=1e-2, weight_decay=1e-3)
    ref_plain = torch.optim.Adam(plain, lr=1e-2, weight_decay=1e-3)  # (the reference WITHOUT clipping: does the case discriminate?)
    dev = [p.clone().to(DEV).requires_grad_(True) for p in ps]
    opt = FlatAdam(dev, lr=1e-2, weight_decay=1e-3, max_grad_norm=1.0)
    coefs = []
    for it in range(4):
        _set_grads(cpu, grads[it])
        _set_grads(plain, grads[it])
        _set_grads(dev, grads[it])
        total_norm = torch.nn.utils.clip_grad_norm_(cpu, 1.0)
        coefs.append(min(1.0, float(1.0 / (total_norm + 1e-6))))
        ref.step()
        ref_plain.step()
        opt.step()
        last = opt.grad_norm_stats(reset=False)["last_norm"]
        print(f"step {it}: reference norm {float(total_norm):.9g}, reported {last:.9g}, coefficient {coefs[-1]:.6g}")
        assert abs(last - float(total_norm)) <= 1e-6 * float(total_norm)
    assert any(c < 1 for c in coefs) and any(c == 1.0 for c in coefs), coefs
    for i, (c, pl, d) in enumerate(zip(cpu, plain, dev)):
        st, st_pl = ref.state[c], ref_plain.state[pl]
        assert _discriminates(c.detach(), pl.detach()) and _discriminates(st["exp_avg"], st_pl["exp_avg"])
        assert _discriminates(st["exp_avg_sq"], st_pl["exp_avg_sq"])
        m, v, t = _moments(opt, i)
        torch.testing.assert_close(d.detach().cpu(), c.detach(), **TOL)
        torch.testing.assert_close(m, st["exp_avg"], **TOL)
        torch.testing.assert_close(v, st["exp_avg_sq"], **TOL)
        assert t == 4
    stats = opt.grad_norm_stats()
    assert stats["steps"] == 4 and stats["clipped"] == sum(c < 1 for c in coefs) and stats["skipped"] == 0
    assert opt.grad_norm_stats()["steps"] == 0  # (read and cleared)


# ---- 4. a coefficient that clamps to 1 leaves the update bit for bit ---------------------------------------------------------------
def test_clamped_coefficient_is_exactly_the_unclipped_update():
    from egopack_amd.optim import FlatAdam
    g = gen(17)
    ps = [torch.randn(s, generator=g) for s in SHAPES]
    grads = [[torch.randn(s, generator=g) for s in SHAPES] for _ in range(3)]
    a = [p.clone().to(DEV).requires_grad_(True) for p in ps]
    b = [p.clone().to(DEV).requires_grad_(True) for p in ps]
    opt_a, opt_b = FlatAdam(a, lr=1e-2, weight_decay=1e-3, max_grad_norm=1e30), FlatAdam(b, lr=1e-2, weight_decay=1e-3)
    for it in range(3):
        _set_grads(a, grads[it])
        _set_grads(b, grads[it])
        opt_a.step()
        opt_b.step()
    for name in ("flat_p", "flat_m", "flat_v"):
        assert torch.equal(getattr(opt_a, name), getattr(opt_b, name)), name
    assert torch.equal(opt_a.flat_w16.view(torch.int16), opt_b.flat_w16.view(torch.int16))
    stats = opt_a.grad_norm_stats()
    assert stats["clipped"] == 0 and stats["skipped"] == 0 and stats["steps"] == 3 and stats["max_norm"] > 0


# ---- 5. a gradient norm that is not finite skips the step --------------------------------------------------------------------------
@pytest.mark.parametrize("bad", [float("inf"), float("nan")])
def test_non_finite_norm_skips_the_step(bad):
    from egopack_amd.optim import FlatAdam
    g = gen(23)
    ps = [torch.randn(s, generator=g) for s in SHAPES]
    grads = [[torch.randn(s, generator=g) * 5 for s in SHAPES] for _ in range(4)]
    cpu = [p.clone().requires_grad_(True) for p in ps]
    ref = torch.optim.Adam(cpu, lr=1e-2, weight_decay=1e-3)
    dev = [p.clone().to(DEV).requires_grad_(True) for p in ps]
    opt = FlatAdam(dev, lr=1e-2, weight_decay=1e-3, max_grad_norm=1.0)
    opt.ensure_lo_shadows()  # (no-op before the flat buffers exist; asked for again below, so that the low-half copies are covered too)
    for it in range(4):
        _set_grads(dev, grads[it])
        if it == 1:
            opt.ensure_lo_shadows()
            opt.refresh_lo_shadows()
            dev[2].grad.view(-1)[77] = bad  # (a value the test writes into the buffer)
            names = ("flat_p", "flat_m", "flat_v", "flat_w16", "flat_w16lo", "_t_dev")
            before = {k: getattr(opt, k).clone() for k in names}
            opt.step()
            torch.cuda.synchronize()
            for k in names:
                assert torch.equal(getattr(opt, k).view(torch.int16), before[k].view(torch.int16)), k
            assert int(opt._t_dev.item()) == 1
            stats = opt.grad_norm_stats(reset=False)
            assert stats["skipped"] == 1 and stats["steps"] == 2 and not math.isfinite(stats["last_norm"])
            continue
        _set_grads(cpu, grads[it])
        torch.nn.utils.clip_grad_norm_(cpu, 1.0)
        ref.step()  # (steps 1, 3, 4 only: bias corrections with t = 1, 2, 3)
        opt.step()
    stats = opt.grad_norm_stats()
    assert stats["skipped"] == 1 and stats["steps"] == 4 and stats["clipped"] == 3 and math.isfinite(stats["mean_norm"])
    for i, (c, d) in enumerate(zip(cpu, dev)):
        m, v, t = _moments(opt, i)
        assert t == 3  # (the device counter's value, not the number of calls)
        torch.testing.assert_close(d.detach().cpu(), c.detach(), **TOL)
        torch.testing.assert_close(m, ref.state[c]["exp_avg"], **TOL)
        torch.testing.assert_close(v, ref.state[c]["exp_avg_sq"], **TOL)
    # a state written after a skipped step resumes bit for bit
    sd = opt.state_dict()
    fresh = [p.detach().clone().requires_grad_(True) for p in dev]
    opt2 = FlatAdam(fresh, lr=1e-2, weight_decay=1e-3, max_grad_norm=1.0)
    opt2.load_state_dict(sd)
    assert opt2.step_count == 3
    extra = [torch.randn(s, generator=g) for s in SHAPES]
    for o, params in ((opt, dev), (opt2, fresh)):
        _set_grads(params, extra)
        o.step()
    assert torch.equal(opt.flat_p, opt2.flat_p) and torch.equal(opt.flat_m, opt2.flat_m) and torch.equal(opt.flat_v, opt2.flat_v)


# ---- 6. the training steps ------------------------------------------------------------------------------------------------------------
def _build(workload, compute, max_grad_norm, dropout="0.0"):
    """A small bench workload (MTLStep on AR + LTA + PNR, or EgoPackStep on OSCC with GraphONE) with its static batches."""
    import bench
    from egopack_amd import engine, ops
    from egopack_amd.optim import FlatAdam
    a = ["--workload", workload, "--batch", "8", "--T", "8", "--hidden", "128", "--trn-hidden", "256", "--dropout", dropout]
    args = bench.parse_args(a + (["--bank", "256"] if workload == "egopack_oscc" else []))
    args.compute = compute
    ops.set_compute(compute)
    ops.manual_seed(11)
    model, tasks, crit, weights, dev, merged = bench.build_workload(args, 0, torch.device(DEV))
    model.to(DEV).train()
    for t in tasks.values():
        t.to(DEV).train()
    params = [*model.parameters(), *(p for t in tasks.values() for p in t.parameters())]
    if workload == "egopack_oscc":
        from egopack_amd.models.graphONE.graphONE import GraphONE
        g = torch.Generator(device=DEV)
        g.manual_seed(7)
        banks = {t: torch.randn(args.bank, args.hidden, device=DEV, generator=g) for t in ("ar", "lta", "pnr")}
        graphone = GraphONE(banks, features_size=args.hidden, hidden_size=args.hidden, k=4, depth=2, residual=True).to(DEV)
        opt = FlatAdam(params + list(graphone.parameters()), lr=1e-3, weight_decay=1e-5, max_grad_norm=max_grad_norm)
        step = engine.EgoPackStep(model, tasks, graphone, weights, opt, backprop_temporal_graph=True, temporal_graph_train_mode=False)
    else:
        opt = FlatAdam(params, lr=1e-3, weight_decay=1e-5, max_grad_norm=max_grad_norm)
        step = engine.MTLStep(model, tasks, crit, weights, opt, fused_backbone=True)
    return step, opt, dev, merged


CASES = [("mtl", "f32"), ("mtl", "bf16"), ("egopack_oscc", "bf16")]


@pytest.fixture
def compute_restored():
    from egopack_amd import ops
    prev = ops.get_compute()
    yield
    ops.set_compute(prev)


def _first_norm(workload, compute, steps=1):
    """The gradient norm of step ``steps`` of an unclipped run (a bound that clamps: the unclipped update)."""
    step, opt, dev, merged = _build(workload, compute, 1e30)
    for _ in range(steps):
        step.step(dev, merged)
    return opt.grad_norm_stats()["last_norm"]


def _state(opt):
    torch.cuda.synchronize()
    return {k: getattr(opt, k).clone().cpu() for k in ("flat_p", "flat_m", "flat_v")}


@pytest.mark.parametrize("workload,compute", CASES)
def test_eager_step_norm_and_clipped_update(workload, compute, compute_restored):
    """The reported norm is grad_scale * ||flat_g|| of the step; the clipped step equals 'unclipped backward, flat_g *= coef by
    the test, unclipped Adam launch' from the same start state (the two differ by one extra f32 rounding of the gradient)."""
    limit = 0.5 * _first_norm(workload, compute, steps=2)  # (half the unclipped norm of the step it is applied to: clipping is active)
    assert limit > 0
    step, opt, dev, merged = _build(workload, compute, 1e30)
    step.step(dev, merged)  # (builds the flat buffers; unclipped)
    opt.max_grad_norm = limit
    step.step(dev, merged)
    stats = opt.grad_norm_stats()
    n = opt.flat_g.numel()
    want = opt.grad_scale * float(opt.flat_g.double().norm())
    rel = abs(stats["last_norm"] - want) / want
    print(f"{workload} {compute}: reported norm {stats['last_norm']:.9g}, flat_g norm {want:.9g}, relative difference {rel:.3e}")
    assert rel <= 2 * n * 2.0 ** -53 + 2.0 ** -24  # (test 2's bound on the sum -- halved by the square root -- plus one f32 rounding)
    assert stats["clipped"] == 1 and stats["steps"] == 2 and stats["last_norm"] > limit
    coef = torch.tensor(limit, dtype=torch.float32) / (torch.tensor(stats["last_norm"], dtype=torch.float32) + 1e-6)
    got = _state(opt)
    # the same two steps, the second one clipped by hand
    step2, opt2, dev2, merged2 = _build(workload, compute, None)
    step2.step(dev2, merged2)
    step2.forward_backward(dev2, merged2)
    unclipped_g = opt2.flat_g.clone()
    opt2.flat_g.mul_(coef.item())
    opt2.step()
    ref = _state(opt2)
    # (does the case discriminate?  the hand-clipped first moment against the one an unclipped step would leave)
    m_unclipped = ref["flat_m"] + (1 - 0.9) * (unclipped_g.cpu() - opt2.flat_g.cpu())
    assert _discriminates(ref["flat_m"], m_unclipped), float(coef)
    for k in got:
        torch.testing.assert_close(got[k], ref[k], **TOL, msg=lambda s, k=k: f"{k}: {s}")


@pytest.mark.parametrize("workload,compute", CASES)
def test_captured_clipped_step_equals_eager(workload, compute, compute_restored):
    """Four steps with clipping active, captured (two warm-up steps + two replays) against eager: parameters AND moments to the
    degree tests/test_gpu_models.py demands of the unclipped pair (MTL: atol 1e-6; EgoPack: bit for bit), the same norms;
    two captured runs are bit-identical."""
    limit = 0.5 * _first_norm(workload, compute)

    def run(use_graph):
        step, opt, dev, merged = _build(workload, compute, limit)
        if use_graph:
            step.capture(dev, merged, warmup=2)
            for _ in range(2):
                step.replay()
        else:
            for _ in range(4):
                step.step(dev, merged)
        st = _state(opt)
        return st, step.grad_norm_stats(), next(iter(opt.state_dict()["state"].values()))["step"]
    eager, stats_e, t_e = run(False)
    graph, stats_g, t_g = run(True)
    graph2, stats_g2, _ = run(True)
    print(f"{workload} {compute}: eager {stats_e}\n  captured {stats_g}")
    assert float(t_e) == float(t_g) == 4
    assert stats_e["steps"] == stats_g["steps"] == 4 and stats_e["clipped"] == stats_g["clipped"] >= 1 and stats_g["skipped"] == 0
    for k in eager:
        d = float((eager[k] - graph[k]).abs().max())
        print(f"  {k}: captured vs eager max abs {d:.3e}")
        assert torch.equal(graph[k], graph2[k]), k
    assert stats_g == stats_g2
    for k in eager:
        if workload == "egopack_oscc":
            assert torch.equal(graph[k], eager[k]), k
        else:
            torch.testing.assert_close(graph[k], eager[k], rtol=0, atol=1e-6, msg=lambda s, k=k: f"{k}: {s}")
    assert abs(stats_e["last_norm"] - stats_g["last_norm"]) <= 1e-5 * stats_e["last_norm"]


def test_skipped_step_inside_a_replayed_graph(compute_restored):
    """One element of the step's static INPUT features overwritten with inf between two replays: that replay changes neither the
    weights nor the moments nor the step counter, the next one (input restored) updates again."""
    limit = 0.5 * _first_norm("mtl", "bf16")
    step, opt, dev, merged = _build("mtl", "bf16", limit, dropout="0.5")
    step.capture(dev, merged, warmup=2)
    step.replay()
    names = ("flat_p", "flat_m", "flat_v", "flat_w16", "_t_dev")
    torch.cuda.synchronize()
    before = {k: getattr(opt, k).clone() for k in names}
    from egopack_amd import ops
    rng_word = lambda: int(ops.rng_device_offset(opt.flat_p.device).item())
    rng0 = rng_word()
    x = merged.x
    keep = x[5, 1, 9].clone()
    x[5, 1, 9] = float("inf")
    step.replay()
    torch.cuda.synchronize()
    for k in names:
        assert torch.equal(getattr(opt, k).view(torch.int16), before[k].view(torch.int16)), k
    assert rng_word() != rng0  # (the dropout offset word still moved on)
    x[5, 1, 9] = keep
    step.replay()
    torch.cuda.synchronize()
    assert not torch.equal(opt.flat_p, before["flat_p"]) and torch.isfinite(opt.flat_p).all() and torch.isfinite(opt.flat_m).all()
    stats = step.grad_norm_stats()
    assert stats["skipped"] == 1 and stats["steps"] == 5, stats
    assert float(next(iter(opt.state_dict()["state"].values()))["step"]) == 4 and opt.step_count == 4


def test_sharded_update_refuses_clipping():
    """dist.GradSync(shard_update=True) with a clipping optimizer: an error that says so."""
    from egopack_amd.dist import GradSync
    from egopack_amd.optim import FlatAdam
    p = [torch.randn(64, device=DEV).requires_grad_(True)]
    p[0].grad = torch.randn(64, device=DEV)
    opt = FlatAdam(p, max_grad_norm=1.0)
    opt._materialise()
    sync = GradSync(2, shard_update=True)
    with pytest.raises(RuntimeError, match="sharded update"):
        sync.reduce_and_step(opt)
    with pytest.raises(RuntimeError, match="sharded update"):
        sync.start(opt, 0, 64)


# ---- 8. the entry point -------------------------------------------------------------------------------------------------------------
RESIDENT = [f"{g}=synthetic_resident" for g in ("dataset_recognition", "dataset_lta", "dataset_oscc", "dataset_pnr")]


@pytest.mark.timeout(600)
def test_main_temporal_with_grad_clip_norm_logs_the_norms(tmp_path, caplog):
    import main_temporal
    args = [*RESIDENT, "k=1", "batch_size=4", "synthetic_samples=24", "model.hidden_size=64", "model.temporal_pooling.hidden_size=64",
            "oscc_feat_size=64", "num_epochs=2", "enabled_tasks=[ar,lta,pnr]", "save_model=True"]
    with caplog.at_level(logging.INFO):
        out = main_temporal.main(args + ["grad_clip_norm=1.0", f"checkpoint_dir={tmp_path}"])
    assert out["step"].optimizer.max_grad_norm == 1.0
    lines = [r.getMessage() for r in caplog.records if "gradient norm mean" in r.getMessage()]
    assert len(lines) == 2, lines
    for line in lines:
        assert "largest" in line and "clipped" in line and "skipped 0" in line, line
    replayed = [r.getMessage() for r in caplog.records if "replayed the captured step" in r.getMessage()]
    assert replayed and not replayed[-1].startswith("epoch 2: 0 steps"), replayed  # (the captured step ran)
    ck = torch.load(tmp_path / "MTL_ar-lta-pnr" / "checkpoint.pth", weights_only=False)
    assert all(torch.isfinite(v).all() for v in ck["temporal_graph"].values() if v.is_floating_point())
    its = [int(r.getMessage().split(":")[1].split()[0]) for r in caplog.records if " iterations, train loss" in r.getMessage()]
    steps = {float(s["step"]) for s in ck["optimizer"]["state"].values()}
    assert len(its) == 2 and steps == {float(sum(its))}, (its, steps)  # (every iteration of both epochs, read from the device counter)
    caplog.clear()
    with caplog.at_level(logging.INFO):
        main_temporal.main(args + [f"checkpoint_dir={tmp_path / 'off'}"])
    assert not [r for r in caplog.records if "gradient norm" in r.getMessage()]  # (off: nothing is logged)


@pytest.mark.timeout(600)
def test_main_temporal_resume_with_clipping_equals_uninterrupted_run(tmp_path):
    """tests/test_gpu_entrypoints.py::test_main_temporal_resume_equals_uninterrupted_run with clipping on: 3 epochs in one go ==
    2 epochs, the save_every checkpoint, resume, 1 more epoch -- bit for bit."""
    import main_temporal
    base = ["k=1", "batch_size=4", "synthetic_samples=16", "model.hidden_size=64", "model.temporal_pooling.hidden_size=64",
            "oscc_feat_size=64", "save_model=True", "compute=f32", "optimizer.lr=1e-3", "enabled_tasks=[ar,pnr]",
            "lr_scheduler.T_max=3", "use_graph=false", "grad_clip_norm=1.0", "save_every=2"]
    main_temporal.main(base + ["num_epochs=3", f"checkpoint_dir={tmp_path / 'full'}"])
    main_temporal.main(base + ["num_epochs=2", f"checkpoint_dir={tmp_path / 'part'}"])
    part = tmp_path / "part" / "MTL_ar-pnr" / "checkpoint.pth"
    ck = torch.load(part, weights_only=False)
    assert ck["epoch"] == 2 and "optimizer" in ck
    out = main_temporal.main(base + ["num_epochs=3", f"checkpoint_dir={tmp_path / 'resumed'}", f"resume_from={part}"])
    assert out["step"].optimizer.clipping
    full = torch.load(tmp_path / "full" / "MTL_ar-pnr" / "checkpoint.pth", weights_only=False)
    res = torch.load(tmp_path / "resumed" / "MTL_ar-pnr" / "checkpoint.pth", weights_only=False)
    assert res["epoch"] == 3
    for key in ("temporal_graph", "task/recognition", "task/pnr"):
        for k, v in full[key].items():
            torch.testing.assert_close(res[key][k], v, rtol=0, atol=0, msg=lambda s: f"{key}.{k}: {s}")
    for i, st in full["optimizer"]["state"].items():
        assert torch.equal(st["exp_avg"], res["optimizer"]["state"][i]["exp_avg"]) and float(st["step"]) == float(res["optimizer"]["state"][i]["step"])
