"""LAMB on the GPU (include/egopack_lamb.h, optim.FlatLAMB): the three launches against the float64 model of
tests/lamb_common.py on raw buffers, any cut of the buffers, the degenerate slots, the closed gate, the copies and the average, the
captured step against the eager one, and the entry point once in a child process.

Tolerances: p, m, v at TOL of tests/test_gpu_optim_rules.py; trust within 1e-6 relative (lamb_common.TRUST_RTOL); everything that
compares two runs of the kernels is bit for bit, except a piece cut in two, whose f64 sums differ in their last bits: trust within
one f32 ulp there.  Every figure is printed before it is asserted ("LAMB ..." lines)."""
import math
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

from tests import ema_common as E
from tests import lamb_common as L
from tests import step_matrix_common as M

pytestmark = pytest.mark.gpu
DEV = "cuda"
REPO = Path(__file__).resolve().parents[1]
ULP = 2.0 ** -23


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


def _stream():
    import ctypes
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _ok(rc, what):
    from egopack_amd import _lib
    assert rc == 0, f"{what} returned {rc}: {_lib.last_error()}"


class Raw:
    """The raw-buffer problem of lamb_common on the device and the three launches over it."""

    def __init__(self, p, m, v, sizes=L.SIZES, slot_group=L.SLOT_GROUP, groups=L.GROUPS, gdt=torch.float32, ema=None):
        from egopack_amd import _lib
        self.lib, self.gdt = _lib.load(), gdt
        self.T = L.tables(DEV, sizes, slot_group, groups)
        dev = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(DEV)
        self.p, self.m, self.v = dev(p), dev(m), dev(v)
        n = self.p.numel()
        self.g = torch.zeros(n, dtype=gdt, device=DEV)
        self.hyper = torch.zeros(4, dtype=torch.float32, device=DEV)
        self.w16, self.w16lo = (torch.full((n,), float("nan"), dtype=torch.bfloat16, device=DEV) for _ in range(2))
        self.ema = ema.to(DEV) if ema is not None else None
        self.t_dev = torch.zeros(1, dtype=torch.int64, device=DEV)
        self.ptr = dict(p=self.p.data_ptr(), g=self.g.data_ptr(), m=self.m.data_ptr(), v=self.v.data_ptr(), hyper=self.hyper.data_ptr(),
                        w16=self.w16.data_ptr(), w16lo=self.w16lo.data_ptr(),
                        **{k: self.T[k].data_ptr() for k in ("slot_begin", "slot_piece0", "slot_group", "group_hyper", "part", "trust", "norms")})

    def step(self, g, t, cuts=None, gate=None, trust_clip=False, always_adapt=False, ema_decay=0.0, ema_warmup=0):
        """One LAMB step at counted step ``t``; ``cuts``: the [lo, hi) ranges of the moments launches, in order (None: one)."""
        self.g.copy_(torch.from_numpy(g).to(self.gdt))
        self.hyper.copy_(torch.from_numpy(L.hyper(t)))
        self.t_dev.fill_(t)
        n, gp = self.p.numel(), (gate.data_ptr() if gate is not None else None)
        for lo, hi in (cuts or [(0, n)]):
            _ok(L.moments(self.lib, _stream(), self.ptr, self.T, lo, hi, g_dtype=1 if self.gdt == torch.bfloat16 else 0, gate=gp), "egk_lamb_moments")
        _ok(L.trust(self.lib, _stream(), self.ptr, self.T, trust_clip, always_adapt, gate=gp), "egk_lamb_trust")
        _ok(L.apply(self.lib, _stream(), self.ptr, self.T, gate=gp, ema=self.ema.data_ptr() if self.ema is not None else None,
                    ema_decay=ema_decay, ema_warmup=ema_warmup, t_dev=self.t_dev.data_ptr()), "egk_lamb_apply")
        torch.cuda.synchronize()

    def host(self):
        return dict(p=self.p.cpu().numpy(), m=self.m.cpu().numpy(), v=self.v.cpu().numpy(), trust=self.T["trust"].cpu().numpy(),
                    norms=self.T["norms"].cpu().numpy().reshape(-1, 2))


# ---- the kernels against the model -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("gdt", [torch.float32, torch.bfloat16], ids=["g=f32", "g=bf16"])
def test_three_steps_match_the_float64_model(gdt):
    """Slots of 8, 24, 4096, 4104, 8200 and 4608 (a padded [2, 72] classifier) elements, two groups of which one decays nothing,
    s = 0.5.  Every step is held to the model of the state the kernels stored before it."""
    pr = L.problem()
    R = Raw(pr["p"], pr["m"], pr["v"], gdt=gdt)
    worst = dict(p=0.0, m=0.0, v=0.0, trust=0.0)
    for t in (1, 2, 3):
        g = pr["g"][t - 1]
        g = torch.from_numpy(g).to(gdt).float().numpy()
        before = R.host()
        R.step(g, t)
        got = R.host()
        p, m, v, trust, norms = L.lamb_model(before["p"], g, before["m"], before["v"], pr["begin"], L.SLOT_GROUP, L.GROUPS, L.hyper(t))
        for k, ref in (("p", p), ("m", m), ("v", v)):
            worst[k] = max(worst[k], L.excess(got[k], ref, **L.TOL))
        worst["trust"] = max(worst["trust"], float(np.max(np.abs(got["trust"] - trust) / trust)))
        assert np.allclose(got["norms"], norms, rtol=1e-6, atol=0.0), (got["norms"], norms)
        assert not np.array_equal(got["p"], before["p"]) and trust[1] == 1.0 and trust[4] == 1.0 and got["trust"][1] == 1.0
        for k in ("p", "m", "v"):  # the padding keeps its zero BITS
            assert not got[k][~pr["mask"]].view(np.int32).any(), k
    print(f"LAMB model {gdt} |error|/tolerance p {worst['p']:.3e} m {worst['m']:.3e} v {worst['v']:.3e}; trust worst relative error "
          f"{worst['trust']:.3e} (bound {L.TRUST_RTOL:.0e})")
    assert worst["p"] <= 1 and worst["m"] <= 1 and worst["v"] <= 1, worst
    assert worst["trust"] <= L.TRUST_RTOL, worst


# ---- any cut ---------------------------------------------------------------------------------------------------------------------------
def _run_cut(cuts):
    pr = L.problem()
    R = Raw(pr["p"], pr["m"], pr["v"])
    for t in (1, 2):
        R.step(pr["g"][t - 1], t, cuts=cuts)
    return R.host()


def test_slices_on_slot_and_piece_boundaries_in_any_order_give_the_same_bits():
    one = _run_cut(None)
    _, _, pieces = L.piece_table(L.SIZES)
    cuts = list(zip(pieces[:-1], pieces[1:]))
    order = np.random.default_rng(3).permutation(len(cuts))
    shuffled = _run_cut([cuts[i] for i in order])
    slots = _run_cut([(0, 32), (8232, 21040), (32, 8232)])
    for other in (shuffled, slots):
        for k in ("p", "m", "v", "trust", "norms"):
            assert np.array_equal(one[k].view(np.int64 if one[k].dtype == np.float64 else np.int32),
                                  other[k].view(np.int64 if one[k].dtype == np.float64 else np.int32)), k


def test_chunks_that_cut_every_piece_once_move_trust_by_at_most_one_ulp():
    """dist.chunk_bounds(n, 4104), which lists the chunks in reverse order: m and v bit for bit, trust within one f32 ulp (the f64 sums of a piece cut in two
    differ by ~1e-16 relative, which moves the f32 rounding by at most one step), p at TOL."""
    from egopack_amd import dist
    one = _run_cut(None)
    n = sum(L.SIZES)
    chunks = list(dist.chunk_bounds(n, 4104))  # (last chunk first)
    assert all(b % 8 == 0 and e % 8 == 0 for b, e in chunks) and sum(e - b for b, e in chunks) == n and len(chunks) == 6
    cut = _run_cut(chunks)
    assert np.array_equal(one["m"].view(np.int32), cut["m"].view(np.int32)) and np.array_equal(one["v"].view(np.int32), cut["v"].view(np.int32))
    rel = float(np.max(np.abs(cut["trust"] - one["trust"]) / one["trust"]))
    print(f"LAMB cut trust worst relative difference {rel:.3e} (one ulp {ULP:.3e}); p |difference|/tolerance {L.excess(cut['p'], one['p'], **L.TOL):.3e}")
    assert rel <= ULP and L.within(cut["p"], one["p"], **L.TOL)


# ---- degenerate slots ------------------------------------------------------------------------------------------------------------------
def test_degenerate_slots_trust_clip_and_always_adapt():
    """Slot 0: p = 0 (P = 0).  Slot 1 (wd 0): g = m = v = 0 (U = 0).  Slot 2: a small p, so the ratio is below 1; slot 3: a large one."""
    pr = L.problem()
    p = pr["p"].copy()
    b = pr["begin"]
    p[b[0]:b[1]] = 0.0
    p[b[3]:b[4]] *= 1000.0
    g = pr["g"][0].copy()
    g[b[1]:b[2]] = 0.0
    runs = {}
    for name, kw in (("plain", {}), ("clip", dict(trust_clip=True)), ("adapt", dict(always_adapt=True))):
        R = Raw(p, pr["m"], pr["v"])
        R.step(g, 1, **kw)
        got = runs[name] = R.host()
        ref = L.lamb_model(p, g, pr["m"], pr["v"], b, L.SLOT_GROUP, L.GROUPS, L.hyper(1), **kw)
        assert L.within(got["p"], ref[0], **L.TOL) and float(np.max(np.abs(got["trust"] - ref[3]) / ref[3])) <= L.TRUST_RTOL, name
        assert got["trust"][0] == 1.0 and got["norms"][0, 0] == 0.0 and got["norms"][0, 1] > 0.0        # P = 0
        assert got["trust"][1] == 1.0 and got["norms"][1, 1] == 0.0 and got["norms"][1, 0] > 0.0        # U = 0 (wd 0: u is Adam's alone)
        assert np.array_equal(got["p"][b[1]:b[2]], p[b[1]:b[2]])                                        # ... and nothing moves there
        for k in ("p", "m", "v"):
            assert not got[k][~pr["mask"]].view(np.int32).any(), (name, k)
    assert runs["plain"]["trust"][3] > 1.0 and runs["clip"]["trust"][3] == 1.0 and runs["plain"]["trust"][2] < 1.0
    assert runs["clip"]["trust"][2] == runs["plain"]["trust"][2]
    assert runs["plain"]["trust"][4] == 1.0 and runs["adapt"]["trust"][4] != 1.0  # (wd 0: the ratio only with always_adapt)


# ---- the optimizer: closed gate, copies, average, lr between replays ---------------------------------------------------------------------
def _params(seed=0):
    """Parameters whose slots are lamb_common's: [8], [24], [64, 64], [4104], [8200] and a [2, 72] classifier (padded to 64 rows)."""
    gen = torch.Generator().manual_seed(seed)
    shapes = [(8,), (24,), (64, 64), (4104,), (8200,), (2, 72)]
    return [torch.nn.Parameter((torch.randn(*s, generator=gen) * 0.1).to(DEV)) for s in shapes]


def _opt(params, **kw):
    from egopack_amd import optim
    groups = [{"params": [params[i] for i in (0, 2, 3, 5)], "lr": L.GROUPS[0][0], "weight_decay": L.GROUPS[0][1]},
              {"params": [params[i] for i in (1, 4)], "lr": L.GROUPS[1][0], "weight_decay": L.GROUPS[1][1]}]
    return optim.FlatLAMB(groups, eps=L.EPS, layout_order=params, **kw)


def _set_grads(params, seed):
    gen = torch.Generator().manual_seed(seed)
    for p in params:
        g = torch.randn(*p.shape, generator=gen).to(DEV)
        if p.grad is None:
            p.grad = g
        else:
            p.grad.copy_(g)


def _state(opt):
    torch.cuda.synchronize()
    out = dict(p=opt.flat_p.clone(), m=opt.flat_m.clone(), v=opt.flat_v.clone(), w16=opt.flat_w16.view(torch.int16).clone(),
               trust=opt._lamb_trust.clone(), t=int(opt._t_dev.item()))
    if opt.flat_w16lo is not None:
        out["w16lo"] = opt.flat_w16lo.view(torch.int16).clone()
    if opt.ema:
        out["ema"] = opt.flat_ema.clone()
    return out


def test_the_optimizer_builds_the_tables_of_its_layout_and_reports_trust():
    params = _params()
    opt = _opt(params)
    _set_grads(params, 1)
    opt.step()
    begin, piece0, pieces = L.piece_table(L.SIZES)
    assert opt._slot_begin.tolist() == begin and opt._slot_piece0.tolist() == piece0 and opt._piece_begin == pieces
    assert opt._slot_group.tolist() == L.SLOT_GROUP and tuple(opt._lamb_part.shape) == (piece0[-1], 2, 2)
    assert opt._group_hyper.cpu()[:, :2].tolist() == [[L.f32(a), L.f32(b)] for a, b in L.GROUPS]
    tr = opt.trust_ratios()
    order = opt._all_params()  # (the state dict's indices: group 0's parameters, then group 1's)
    assert sorted(tr) == [0, 1, 2, 3, 4, 5] and [tuple(q.shape) for q in order[4:]] == [(24,), (8200,)]
    assert tr[4][0] == 1.0 and tr[5][0] == 1.0 and all(tr[i][0] != 1.0 for i in (0, 1, 2, 3))  # (group 1 decays nothing)
    for i, (t_, np_, nu_) in tr.items():
        assert abs(np_ - float(order[i].detach().double().norm())) <= 2e-2 * np_ and nu_ > 0  # (||p|| before the step moved it a little)
    assert sorted(opt.trust_ratios({p: f"w{i}" for i, p in enumerate(params)})) == [f"w{i}" for i in range(6)]
    with pytest.raises(ValueError, match="strictly inside the piece.*chunk_mb"):
        opt.prepare_hyper()
        opt.launch(None, 4136, 4200)
    assert opt._lamb_covered == 0  # (the refused launch counted nothing)


def test_closed_gate_changes_nothing_but_the_offset_word():
    """A gradient with an inf under max_grad_norm: egk_grad_norm_finalize closes the gate and takes the step back out of t_dev; the
    three launches leave p, m, v, trust, the copies and the average alone, and the offset word still moves on."""
    params = _params()
    opt = _opt(params, max_grad_norm=1.0, ema_decay=0.9)
    _set_grads(params, 1)
    opt.step()
    opt.ensure_lo_shadows()
    _set_grads(params, 2)
    opt.step()
    before = _state(opt)
    assert before["t"] == 2
    _set_grads(params, 3)
    params[2].grad[3, 5] = float("inf")
    word = torch.tensor([100], dtype=torch.int64, device=DEV)
    opt.prepare_hyper()
    opt.norm_partials()
    opt.norm_finalize()
    opt.launch(bump=(word, 7))
    after = _state(opt)
    assert word.item() == 107 and after["t"] == 2 and int(opt._gate.item()) == 0
    for k in before:
        assert torch.equal(before[k], after[k]) if torch.is_tensor(before[k]) else before[k] == after[k], k
    opt._t_mirror = opt.step_count = 2
    _set_grads(params, 3)
    opt.step()
    end = _state(opt)
    assert end["t"] == 3 and not torch.equal(end["p"], before["p"]) and int(opt._gate.item()) == 1 and bool(torch.isfinite(end["p"]).all())


def test_copies_are_cast_and_split_of_the_stored_parameters_and_the_average_follows_the_model():
    params = _params()
    opt = _opt(params, ema_decay=0.9, ema_warmup=True)
    _set_grads(params, 1)
    opt.step()
    opt.ensure_lo_shadows()
    for t in (2, 3):
        e0 = opt.flat_ema.cpu().clone()
        _set_grads(params, t)
        opt.step()
        st = _state(opt)
        p = st["p"].cpu()
        hi = p.to(torch.bfloat16)
        assert torch.equal(st["w16"].cpu(), hi.view(torch.int16)), "bf16 copy"
        assert torch.equal(st["w16lo"].cpu(), (p - hi.float()).to(torch.bfloat16).view(torch.int16)), "low half"
        assert torch.equal(st["ema"].cpu(), E.ema_model(e0, p, E.ema_weight(0.9, True, t))), "ema"
        assert opt._lo_is_fresh(0, p.numel())


def _replayed(lrs):
    """prepare + launch captured once; one replay per entry of ``lrs`` (None: leave the groups alone), the lr written into group 0
    between the replays."""
    params = _params()
    opt = _opt(params)
    _set_grads(params, 1)
    opt.step()
    opt.sync_hyper_source()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        opt.prepare_hyper(in_capture=True)
        opt.launch()
    out = []
    for lr in lrs:
        if lr is not None:
            opt.param_groups[0]["lr"] = lr
        opt.sync_hyper_source()
        g.replay()
        opt.note_captured_step()
        opt.step_count += 1
        out.append(_state(opt))
    return out


def test_an_lr_written_between_two_replays_shows_in_the_next_replay():
    plain = _replayed([None, None])
    sched = _replayed([None, 5e-2])
    assert plain[0]["t"] == 2 and plain[1]["t"] == 3
    for k in ("p", "m", "v", "trust"):
        assert torch.equal(plain[0][k], sched[0][k]), k
    assert torch.equal(plain[1]["m"], sched[1]["m"]) and torch.equal(plain[1]["trust"], sched[1]["trust"])  # (lr enters the apply alone)
    b = L.piece_table(L.SIZES)[0]
    moved = lambda run: (run[1]["p"] - run[0]["p"]).cpu()
    own, other = slice(b[2], b[3]), slice(b[4], b[5])
    assert torch.equal(moved(plain)[other], moved(sched)[other])                       # group 1 keeps its lr
    big = moved(plain)[own].abs() > 1e-2 * moved(plain)[own].abs().max()               # (moves well above the rounding of p)
    ratio = moved(sched)[own][big] / moved(plain)[own][big]
    assert int(big.sum()) > 1000 and float((ratio - 5.0).abs().max()) < 1e-2, ratio    # 5e-2 / 1e-2


# ---- step level ------------------------------------------------------------------------------------------------------------------------
LAMB = ["optimizer._target_=egopack_amd.optim.FlatLAMB", f"optimizer.lr={M.LR}", f"optimizer.weight_decay={M.WD}", "+optimizer.eps=1e-6"]
FEATURES = ["param_groups.no_decay_1d=true", "ema.decay=0.99", "task_weighting.mode=uncertainty"]
SIZES = [("f32", 2), ("bf16", 8)]


def _build(size, features=False, clip=None):
    """step_matrix_common.build_step with the LAMB target (that builder takes its target from its own table)."""
    import bench
    from egopack_amd import engine, ops
    from egopack_amd import train as T
    compute, batch = size
    args = bench.parse_args(["--workload", "mtl", "--batch", str(batch), "--T", str(M.T_NODES), "--hidden", "64", "--trn-hidden", "64",
                             "--dropout", "0.0", "--compute", compute])
    ops.set_compute(compute)
    ops.manual_seed(11)
    model, tasks, crit, weights, dev, merged = bench.build_workload(args, 0, torch.device(DEV))
    model.to(DEV).train()
    for t in tasks.values():
        t.to(DEV).train()
    cfg = T.load_config(LAMB + (FEATURES + [f"grad_clip_norm={clip!r}"] if features else []))
    crit = {t: c.to(DEV).train() for t, c in crit.items()}
    wd = cfg.optimizer.weight_decay
    flat = [*model.configure_optimizers(wd), *(p for t in M.ORDER for p in tasks[t].configure_optimizers(wd))]
    mode = T.task_weighting_config(cfg)["mode"]
    log_var = T.build_task_weighting(cfg, [t for t in engine.MTLStep.order if weights.get(t, 0) > 0 and t in tasks], DEV)
    opt = T.build_optimizer(cfg, T.build_param_groups(cfg, model, tasks), layout_order=flat, log_var=log_var)
    step = engine.MTLStep(model, tasks, crit, weights, opt, fused_backbone=True, task_weighting=mode, log_var=log_var)
    return step, opt, dev, merged


_CLIP = {}


def _clip_of(size):
    """Half the smallest unclipped norm of the four steps: the clip must bite."""
    if size not in _CLIP:
        step, opt, dev, merged = _build(size, True, clip=1e30)
        norms = []
        for _ in range(4):
            step.step(dev, merged)
            norms.append(opt.grad_norm_stats(reset=False)["last_norm"])
        assert all(n > 0 and n == n for n in norms), norms
        _CLIP[size] = 0.5 * min(norms)
    return _CLIP[size]


def _four(size, how, features):
    step, opt, dev, merged = _build(size, features, _clip_of(size) if features else None)
    launches = []
    inner = opt._launch_rule
    opt._launch_rule = lambda sl, *a: (launches.append((sl.start, sl.stop)), inner(sl, *a))[1]
    if how == "graph":
        step.capture(dev, merged, warmup=2)
        for _ in range(2):
            step.replay()
    else:
        for _ in range(4):
            step.step(dev, merged)
    out = _state(opt)
    out["loss_sums"] = step.loss_sums()
    if step.task_log_var is not None:
        out["log_var"] = step.task_log_var.log_var.detach().clone()
    out["form"] = launches
    assert bool(torch.isfinite(out["p"]).all()) and out["t"] == 4
    return out, step, opt


@pytest.mark.parametrize("features", [False, True], ids=["plain", "clip-groups-ema-uncertainty"])
@pytest.mark.parametrize("size", SIZES, ids=["f32B2", "bf16B8"])
def test_captured_step_replayed_twice_equals_four_eager_steps(size, features, compute_restored):
    """flat_p, the moments, trust, the copies, the average, log_var and the loss sums: bit for bit.  The launch form the capture took
    is printed: the (lo, hi) of every moments launch, eager steps first."""
    eager, _, _ = _four(size, "eager", features)
    graph, _, opt = _four(size, "graph", features)
    n = opt.flat_p.numel()
    cap = [c for c in graph["form"] if c != (0, n)]
    print(f"LAMB captured {size} features={features}: {n} elements, moments launches {graph['form']} -> "
          f"{'early + late slice' if cap else 'one launch'}")
    for k in eager:
        if torch.is_tensor(eager[k]):
            assert torch.equal(eager[k], graph[k]), f"{k}: {int((eager[k] != graph[k]).sum())} of {eager[k].numel()} elements differ"
    assert eager["loss_sums"] == graph["loss_sums"] and all(n_ > 0 for _, n_ in eager["loss_sums"].values())
    if features:  # the 1-d slots (weight decay 0) and log_var: trust exactly 1; the decayed matrices: not
        tr = opt.trust_ratios()
        flat = [(p, tr[i]) for i, p in enumerate(opt._all_params()) if i in tr]
        assert all(t_[0] == 1.0 for p, t_ in flat if p.dim() <= 1), [(tuple(p.shape), t_) for p, t_ in flat if p.dim() <= 1]
        assert sum(t_[0] != 1.0 for p, t_ in flat if p.dim() == 2) >= 10
        assert not torch.equal(graph["log_var"], torch.zeros_like(graph["log_var"]))


@pytest.mark.parametrize("size", SIZES, ids=["f32B2", "bf16B8"])
def test_update_half_with_the_features_on_matches_the_model(size, compute_restored):
    """Two steps, ``forward_backward``, a snapshot, ``opt.step()``: p, m, v, trust and the average against the float64 model of the
    snapshot with the clip coefficient of tests/small_constants_common.py in s."""
    from tests import small_constants_common as SC
    clip = _clip_of(size)
    step, opt, dev, merged = _build(size, True, clip)
    for _ in range(2):
        step.step(dev, merged)
    opt.grad_norm_stats()
    step.forward_backward(dev, merged)
    torch.cuda.synchronize()
    snap = {k: x.detach().float().cpu().numpy().copy() for k, x in dict(p=opt.flat_p, g=opt.flat_g, m=opt.flat_m, v=opt.flat_v).items()}
    e0, t = opt.flat_ema.cpu().clone(), int(opt._t_dev.item()) + 1
    opt.step()
    torch.cuda.synchronize()
    norm = float(opt.grad_scale) * math.sqrt(float(np.sum(snap["g"].astype(np.float64) ** 2)))
    coef = SC.clip_ref(norm, clip)
    stats = opt.grad_norm_stats()
    assert coef < 1 and stats["clipped"] == 1 and stats["skipped"] == 0
    hy = L.hyper(t, s=L.f32(float(opt.grad_scale) * coef))
    begin = opt._slot_begin.tolist()
    groups = [(g["lr"], g["weight_decay"]) for g in opt.param_groups]
    ref = L.lamb_model(snap["p"], snap["g"], snap["m"], snap["v"], begin, opt._slot_group.tolist(), groups, hy, eps=1e-6)
    got = dict(p=opt.flat_p.cpu().numpy(), m=opt.flat_m.cpu().numpy(), v=opt.flat_v.cpu().numpy(), trust=opt._lamb_trust.cpu().numpy())
    figs = {k: L.excess(got[k], r, **L.TOL) for k, r in (("p", ref[0]), ("m", ref[1]), ("v", ref[2]))}
    figs["trust"] = float(np.max(np.abs(got["trust"] - ref[3]) / ref[3]))
    print(f"LAMB update {size} |error|/tolerance {figs}")
    assert figs["p"] <= 1 and figs["m"] <= 1 and figs["v"] <= 1 and figs["trust"] <= L.TRUST_RTOL, figs
    assert not np.array_equal(got["p"], snap["p"])
    want = E.ema_model(e0, opt.flat_p.cpu(), E.ema_weight(0.99, opt.ema_warmup, t))
    assert torch.equal(opt.flat_ema.cpu(), want), "flat_ema"
    lo, ln = opt._slot_of[id(step.task_log_var.log_var)]
    assert float(got["trust"][-1]) == 1.0 and lo + ln == opt.flat_p.numel() and np.all(got["p"][lo:lo + 3] != snap["p"][lo:lo + 3])


def test_a_planted_inf_skips_the_step_inside_the_replayed_graph(compute_restored):
    size = SIZES[0]
    step, opt, dev, merged = _build(size, True, _clip_of(size))
    step.capture(dev, merged, warmup=2)
    step.replay()
    before = _state(opt)
    keep = merged.x[5, 1, 9].clone()
    merged.x[5, 1, 9] = float("inf")
    step.replay()
    after = _state(opt)
    merged.x[5, 1, 9] = keep
    step.replay()
    end = _state(opt)
    assert before["t"] == 3 and after["t"] == 3 and end["t"] == 4 and step.grad_norm_stats()["skipped"] == 1
    for k in before:
        assert torch.equal(before[k], after[k]) if torch.is_tensor(before[k]) else before[k] == after[k], k
    assert not torch.equal(end["p"], before["p"]) and bool(torch.isfinite(end["p"]).all())


# ---- the entry point, once, in a child process -------------------------------------------------------------------------------------------
CHILD = r"""
import sys
from pathlib import Path
sys.path.insert(0, sys.argv[1])
tmp = Path(sys.argv[2])
import main_temporal

BASE = ["k=1", "batch_size=4", "synthetic_samples=8", "model.hidden_size=64", "model.temporal_pooling.hidden_size=64",
        "oscc_feat_size=64", "save_model=True", "compute=f32", "lr_scheduler.T_max=3", "save_every=2", "use_graph=false",
        "optimizer._target_=egopack_amd.optim.FlatLAMB", "optimizer.lr=1e-3", "optimizer.weight_decay=1e-2", "+optimizer.eps=1e-6",
        "+optimizer.trust_clip=true"]


def mark(what):
    print(f"LAMB-RUN {what}", file=sys.stderr, flush=True)


mark("full")
main_temporal.main(BASE + ["num_epochs=3", f"checkpoint_dir={tmp / 'full'}"])
mark("part")
main_temporal.main(BASE + ["num_epochs=2", f"checkpoint_dir={tmp / 'part'}"])
mark("resumed")
part = tmp / "part" / "MTL_ar-lta-oscc-pnr" / "checkpoint.pth"
main_temporal.main(BASE + ["num_epochs=3", f"checkpoint_dir={tmp / 'resumed'}", f"resume_from={part}"])
mark("dry")
main_temporal.main([a for a in BASE if a != "use_graph=false"] + ["num_epochs=1", "exchange_dry_run=2", "model.temporal_pooling.dropout=0",
                                                                    f"checkpoint_dir={tmp / 'dry'}"])
mark("end")
print("CHILD-OK")
"""
NAME = "MTL_ar-lta-oscc-pnr"
MODULE_KEYS = ("temporal_graph", "task/recognition", "task/oscc", "task/lta", "task/pnr")


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("lamb_runs")
    script = tmp / "child.py"
    script.write_text(CHILD)
    r = subprocess.run([sys.executable, str(script), str(REPO), str(tmp)], capture_output=True, text=True, cwd=str(tmp), timeout=600)
    assert r.returncode == 0 and "CHILD-OK" in r.stdout, (r.returncode, r.stdout[-3000:], r.stderr[-6000:])
    load = lambda d: torch.load(tmp / d / NAME / "checkpoint.pth", weights_only=False)
    parts = {}
    for chunk in r.stderr.split("LAMB-RUN ")[1:]:
        head, _, body = chunk.partition("\n")
        parts[head.strip()] = body
    return dict(logs=parts, **{d: load(d) for d in ("full", "part", "resumed", "dry")})


def test_main_temporal_with_lamb_resumes_bit_for_bit(runs):
    full, part, res = runs["full"], runs["part"], runs["resumed"]
    assert part["epoch"] == 2 and res["epoch"] == full["epoch"] == 3
    for key in MODULE_KEYS:
        for k, v in full[key].items():
            assert torch.equal(v, res[key][k]), f"{key}.{k}"
    oa, ob = full["optimizer"], res["optimizer"]
    assert sorted(oa["state"]) == sorted(ob["state"]) and oa["state"]
    assert all(g["trust_clip"] is True and g["always_adapt"] is False for g in oa["param_groups"])
    for i, st in oa["state"].items():
        for k, v in st.items():
            assert torch.equal(torch.as_tensor(v), torch.as_tensor(ob["state"][i][k])), f"optimizer state {i}.{k}"
    moved = max(float((v - part["temporal_graph"][k]).abs().max()) for k, v in full["temporal_graph"].items() if v.is_floating_point())
    assert moved > 0
    assert runs["logs"]["full"].count("trust ratio min") == 3, "one trust line per epoch"


def test_main_temporal_with_lamb_and_the_exchange_dry_run(runs):
    """``exchange_dry_run=2`` completes with finite losses.  dist.py: the dry run scales the gradient by 1 / world and all-reduces
    it over the one rank there is, so it steps on HALF the one-rank gradient -- another arithmetic than the one-rank step's, and the
    two checkpoints are not compared at TOL."""
    log = runs["logs"]["dry"]
    assert "train loss" in log and "nan" not in log.lower().split("train loss", 1)[1].split("\n", 1)[0]
    for key in MODULE_KEYS:
        for k, v in runs["dry"][key].items():
            assert not v.is_floating_point() or bool(torch.isfinite(v).all()), f"{key}.{k}"
    assert "trust ratio min" in log
