"""The weight average kept inside the optimizer launch (include/egopack_ema.h, optim.FlatOptimizer ``ema_decay``) on the GPU: the
kernel bit for bit against a host model, a closed gate, ``ema_weights()``, the captured step against the eager one, the off path,
and -- in ONE child process that the last tests share -- an interrupted and resumed main_temporal.py run, checkpoint_ema.pth, and
validation under the average.

The host model (tests/ema_common.py) is ``ema + w * (p_new - ema)`` as three separately rounded f32 torch operations on the CPU
with w = numpy.float32(1.0 - d_t) from Python doubles; every comparison here is torch.equal."""
import ctypes
import json
import subprocess
import sys
from pathlib import Path

import pytest
import torch

from tests import ema_common as E
from tests import param_groups_common as PG

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF = torch.bfloat16
REPO = Path(__file__).resolve().parents[1]
SHAPES = [(33, 7), (5,), (64, 64), (3,), (130, 9)]
DECAY = 0.99
ROWS = [(1e-2, 1e-2), (1e-2, 0.0), (1e-3, 1e-2)]  # (lr, weight_decay) of the three groups
ONE = (3e-3, 2e-2)                                # ... and of the one


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


# ---- 1. the kernel against the host model, bit for bit ----------------------------------------------------------------------------------
class _Side:
    """Device copies of one problem over a buffer of ``total`` elements; launches run over [lo, hi) of it."""

    def __init__(self, prob, ema0):
        self.prob, n = prob, prob["n"]
        self.p, self.g, self.a, self.b = (prob[k].to(DEV).clone() for k in ("p", "g", "a", "b"))
        self.t = torch.zeros(1, dtype=torch.int64, device=DEV)
        self.hi, self.lo = torch.zeros(n, dtype=BF, device=DEV), torch.zeros(n, dtype=BF, device=DEV)
        self.word = torch.tensor([100], dtype=torch.int64, device=DEV)
        self.ema = ema0.to(DEV).clone()

    def desc(self, lo, hi, hyper, weight_decay):
        ns = self.prob["n_state"]
        return PG.descriptor(self.prob["kind"], self.prob["gdt"], hi - lo, self.p.data_ptr(), self.g.data_ptr(),
                             self.a.data_ptr() if ns >= 1 else 0, self.b.data_ptr() if ns >= 2 else 0, hyper.data_ptr(), self.t.data_ptr(),
                             self.hi.data_ptr(), self.lo.data_ptr(), self.word.data_ptr(), None, off=lo, weight_decay=weight_decay)

    def bits(self):
        ns = self.prob["n_state"]
        out = dict(p=self.p, hi=self.hi.view(torch.int16), lo=self.lo.view(torch.int16), word=self.word)
        if ns >= 1:
            out["state0"] = self.a
        if ns >= 2:
            out["state1"] = self.b
        return {k: v.cpu() for k, v in out.items()}


def _three_steps(kind, gdt, groups, warmup, total, lo, hi):
    """Three successive steps (t = 1, 2, 3) over [lo, hi) of a ``total``-element buffer: once through egk_optim_step_ema, once
    through egk_optim_step / egk_optim_step_groups.  p, the state, both copies and the word must agree bit for bit after every step;
    ``ema`` must equal the host model applied to the downloaded new p, and stay untouched outside the slice."""
    from egopack_amd import _lib
    lib = _lib.load()
    prob = PG.problem(total, kind, gdt)
    ema0 = torch.randn(total, generator=gen(total + 17))
    with_ema, without = _Side(prob, ema0), _Side(prob, ema0)
    table = None
    if groups == 3:
        begins, seg_group = E.segments(total)
        sb = torch.tensor(begins, dtype=torch.int64, device=DEV)
        sg = torch.tensor(seg_group, dtype=torch.int32, device=DEV)
        gh = PG.hyper_rows(ROWS).to(DEV)
        table = PG.group_table(lo, sb, sg, gh)
    e = _lib.EmaDesc()
    e.ema, e.decay, e.warmup = with_ema.ema.data_ptr() + 4 * lo, DECAY, int(warmup)
    ema_host = ema0.clone()
    weights = []
    for t in (1, 2, 3):
        hyper = prob["hyper"].clone()
        hyper[0] = float("nan") if table is not None else ONE[0]
        hyper[1], hyper[2] = 1 - 0.9 ** t, (1 - 0.999 ** t) ** 0.5
        hyper = hyper.to(DEV)
        wd = float("nan") if table is not None else ONE[1]
        for side in (with_ema, without):
            side.t.fill_(t)
        tp = ctypes.byref(table) if table is not None else None
        d = with_ema.desc(lo, hi, hyper, wd)
        assert lib.egk_optim_step_ema(PG.stream(), ctypes.byref(d), tp, ctypes.byref(e)) == 0, _lib.last_error()
        d = without.desc(lo, hi, hyper, wd)
        if table is not None:
            assert lib.egk_optim_step_groups(PG.stream(), ctypes.byref(d), tp) == 0, _lib.last_error()
        else:
            assert lib.egk_optim_step(PG.stream(), ctypes.byref(d)) == 0, _lib.last_error()
        torch.cuda.synchronize()
        got, want = with_ema.bits(), without.bits()
        for k in want:
            assert torch.equal(got[k], want[k]), (t, k, int((got[k] != want[k]).sum()))
        assert got["word"].tolist() == [100 + 7 * t]
        w = E.ema_weight(DECAY, warmup, t)
        weights.append(float(w))
        ema_host[lo:hi] = E.ema_model(ema_host[lo:hi], got["p"][lo:hi], w)
        ema_dev = with_ema.ema.cpu()
        assert torch.equal(ema_dev[lo:hi], ema_host[lo:hi]), (t, int((ema_dev[lo:hi] != ema_host[lo:hi]).sum()))
        assert torch.equal(ema_dev[:lo], ema0[:lo]) and torch.equal(ema_dev[hi:], ema0[hi:]), "ema outside the slice was touched"
    assert torch.equal(without.ema.cpu(), ema0)
    assert not torch.equal(ema_host[lo:hi], ema0[lo:hi]) and bool(torch.isfinite(ema_host).all())
    assert len(set(weights)) == (3 if warmup else 1)
    p_end = with_ema.p.cpu()
    assert torch.equal(p_end[:lo], prob["p"][:lo]) and torch.equal(p_end[hi:], prob["p"][hi:]) and not torch.equal(p_end, prob["p"])


@pytest.mark.parametrize("warmup", [False, True], ids=["fixed-decay", "warmup"])
@pytest.mark.parametrize("groups", [1, 3], ids=["one-group", "three-groups"])
@pytest.mark.parametrize("gdt", [torch.float32, BF], ids=["f32", "bf16"])
@pytest.mark.parametrize("kind", list(PG.KINDS))
def test_the_launch_equals_the_host_model_bit_for_bit(kind, gdt, groups, warmup):
    """n = 8 (below one 16-byte-access block), 1016 (one quad short of a 1024 block), 1024 (exactly one), 3080 (three blocks and a
    rest), and the slice [1032, 3600) of a 4104-element buffer."""
    for n in (8, 1016, 1024, 3080):
        _three_steps(kind, gdt, groups, warmup, n, 0, n)
    _three_steps(kind, gdt, groups, warmup, 4104, 1032, 3600)


@pytest.mark.parametrize("kind", ["adamw", "sgd"])
def test_a_scalar_tail_follows_the_same_model(kind):
    """n % 4 != 0: the last one to three elements take the scalar path of the launch."""
    for n in (3, 1003, 3079):
        _three_steps(kind, torch.float32, 1, True, n, 0, n)


# ---- 2. a closed gate -------------------------------------------------------------------------------------------------------------------
def _set_grads(params, grads):
    for p, gr in zip(params, grads):
        if p.grad is None:
            p.grad = gr.clone().to(p.device)
        else:
            p.grad.copy_(gr)


def _clipped_step(opt, word):
    """``FlatOptimizer.step`` with the dropout offset word handed to the launch, as the engine's step does."""
    opt.prepare_hyper()
    opt.norm_partials()
    opt.norm_finalize()
    opt.launch(bump=(word, 7))
    opt.step_count += 1


@pytest.mark.parametrize("bad", [float("inf"), float("nan")])
def test_a_closed_gate_leaves_the_average_alone(bad):
    """The first step's gradient is not finite under max_grad_norm=1.0: ema, p and the state keep their bits, the offset word moves,
    the step is taken back out of the device counter -- so the NEXT step's warm-up weight is that of t = 1."""
    from egopack_amd.optim import FlatAdam
    g = gen(23)
    ps = [torch.randn(s, generator=g) for s in SHAPES]
    grads = [[torch.randn(s, generator=g) * 5 for s in SHAPES] for _ in range(2)]
    dev = [p.clone().to(DEV).requires_grad_(True) for p in ps]
    opt = FlatAdam(dev, lr=1e-2, weight_decay=1e-3, max_grad_norm=1.0, ema_decay=DECAY, ema_warmup=True)
    _set_grads(dev, grads[0])
    opt._materialise()
    opt.ensure_lo_shadows()
    opt.refresh_lo_shadows()
    with torch.no_grad():
        opt.flat_ema.add_(0.25)  # (an average that is not the parameters: a write of p into it would be seen)
    word = torch.tensor([100], dtype=torch.int64, device=DEV)
    dev[2].grad.view(-1)[77] = bad
    names = ("flat_p", "flat_m", "flat_v", "flat_w16", "flat_w16lo", "flat_ema", "_t_dev")
    before = {k: getattr(opt, k).clone() for k in names}
    _clipped_step(opt, word)
    torch.cuda.synchronize()
    for k in names:
        assert torch.equal(getattr(opt, k).view(torch.int16), before[k].view(torch.int16)), k
    assert word.tolist() == [107] and int(opt._t_dev.item()) == 0
    assert opt.grad_norm_stats(reset=False)["skipped"] == 1
    _set_grads(dev, grads[1])
    _clipped_step(opt, word)
    torch.cuda.synchronize()
    assert word.tolist() == [114] and int(opt._t_dev.item()) == 1
    assert not torch.equal(opt.flat_p, before["flat_p"])
    want = E.ema_model(before["flat_ema"].cpu(), opt.flat_p.cpu(), E.ema_weight(DECAY, True, 1))
    assert torch.equal(opt.flat_ema.cpu(), want)
    assert not torch.equal(want, E.ema_model(before["flat_ema"].cpu(), opt.flat_p.cpu(), E.ema_weight(DECAY, True, 2)))


# ---- 3. ema_weights() -------------------------------------------------------------------------------------------------------------------
def _flat(kind, params, **kw):
    from egopack_amd.optim import FlatAdam, FlatAdamW, FlatSGD
    return {"adam": FlatAdam, "adamw": FlatAdamW, "sgd": FlatSGD}[kind](params, **kw)


RULES = [("adam", dict()), ("adamw", dict()), ("sgd", dict(momentum=0.9, dampening=0.1)), ("sgd", dict())]
RULE_IDS = ["adam", "adamw", "sgd-momentum", "sgd-plain"]


@pytest.mark.parametrize("kind,kw", RULES, ids=RULE_IDS)
def test_ema_weights_swaps_the_average_in_and_restores_every_bit(kind, kw):
    from egopack_amd import _lib
    lib = _lib.load()
    g = gen(5)
    ps = [torch.randn(s, generator=g) for s in SHAPES]
    grads = [[torch.randn(s, generator=g) for s in SHAPES] for _ in range(2)]
    dev = [p.clone().to(DEV).requires_grad_(True) for p in ps]
    opt = _flat(kind, dev, lr=1e-2, weight_decay=1e-2, ema_decay=0.9, **kw)
    _set_grads(dev, grads[0])
    opt._materialise()
    assert torch.equal(opt.flat_ema, opt.flat_p) and opt.flat_ema.data_ptr() != opt.flat_p.data_ptr()
    opt.ensure_lo_shadows()
    opt.refresh_lo_shadows()
    for it in range(2):
        _set_grads(dev, grads[it])
        opt.step()
    names = ("flat_p", "flat_ema", "flat_w16", "flat_w16lo")
    before = {k: getattr(opt, k).clone() for k in names}
    n = opt.flat_p.numel()
    assert not torch.equal(before["flat_p"], before["flat_ema"]) and opt._lo_is_fresh(0, n)
    # what egk_cast / egk_split_bf16 make of the average
    w16 = torch.zeros(n, dtype=BF, device=DEV)
    w16lo = torch.zeros(n, dtype=BF, device=DEV)
    assert lib.egk_cast(PG.stream(), before["flat_ema"].data_ptr(), 0, w16.data_ptr(), 1, n) == 0
    assert lib.egk_split_bf16(PG.stream(), before["flat_ema"].data_ptr(), n, None, w16lo.data_ptr(), n, 1, n) == 0
    with opt.ema_weights() as inside:
        assert inside is opt
        torch.cuda.synchronize()
        assert torch.equal(opt.flat_p, before["flat_ema"]) and torch.equal(opt.flat_ema, before["flat_p"])
        assert torch.equal(opt.flat_w16.view(torch.int16), w16.view(torch.int16))
        assert opt._lo_is_fresh(0, n) and torch.equal(opt.flat_w16lo.view(torch.int16), w16lo.view(torch.int16))
        off, _ = opt._slot_of[id(dev[4])]
        assert torch.equal(dev[4].detach().reshape(-1), before["flat_ema"][off:off + dev[4].numel()])  # (the model's own views)
        with pytest.raises(RuntimeError, match="nesting"):
            with opt.ema_weights():
                pass
        with pytest.raises(RuntimeError, match="ema_weights"):
            opt.step()
        with pytest.raises(RuntimeError, match="ema_weights"):
            opt.launch()
        assert opt._ema_swapped
    torch.cuda.synchronize()
    for k in names:
        assert torch.equal(getattr(opt, k).view(torch.int16), before[k].view(torch.int16)), k
    assert opt._lo_is_fresh(0, n) and not opt._ema_swapped
    # the state dict holds the average per parameter, and a fresh optimizer that loads it continues bit for bit
    sd = opt.state_dict()
    assert sorted(sd["ema"]["values"]) == list(range(len(SHAPES))) and sd["ema"]["decay"] == 0.9 and sd["ema"]["warmup"] is False
    off, _ = opt._slot_of[id(dev[2])]
    assert torch.equal(sd["ema"]["values"][2].reshape(-1), before["flat_ema"][off:off + dev[2].numel()])
    fresh = [p.detach().clone().requires_grad_(True) for p in dev]
    opt2 = _flat(kind, fresh, lr=1e-2, weight_decay=1e-2, ema_decay=0.9, **kw)
    opt2.load_state_dict(sd)
    assert opt2.materialised and torch.equal(opt2.flat_ema, opt.flat_ema)
    extra = [torch.randn(s, generator=g) for s in SHAPES]
    for o, params in ((opt, dev), (opt2, fresh)):
        _set_grads(params, extra)
        o.step()
    assert torch.equal(opt.flat_p, opt2.flat_p) and torch.equal(opt.flat_ema, opt2.flat_ema)
    assert not torch.equal(opt.flat_ema, before["flat_ema"])
    # a state without an average: it starts from the parameters; an average of the wrong shape is refused by index
    opt3 = _flat(kind, [p.detach().clone().requires_grad_(True) for p in dev], lr=1e-2, weight_decay=1e-2, ema_decay=0.9, **kw)
    opt3.load_state_dict({k: v for k, v in sd.items() if k != "ema"})
    assert torch.equal(opt3.flat_ema, opt3.flat_p)
    bad = {**sd, "ema": {**sd["ema"], "values": {**sd["ema"]["values"], 3: torch.zeros(4)}}}
    with pytest.raises(ValueError, match="parameter 3"):
        opt3.load_state_dict(bad)


# ---- 4. the off path, and every rule through the descriptor with the average on ---------------------------------------------------------
@pytest.mark.parametrize("kind,kw", RULES, ids=RULE_IDS)
def test_off_is_the_old_path_and_on_changes_no_bit_of_the_update(kind, kw):
    """Three steps each: without ``ema_decay`` (and with 0) no ``flat_ema`` exists and ``optim_ema`` records no launch; with it every
    launch is one ``optim_ema`` launch -- plain Adam included -- and p, the state and the bf16 copies have the bits of the run
    without.  One group and three."""
    from egopack_amd import _lib
    from tests.test_gpu_bounds import _counted
    g = gen(7)
    ps = [torch.randn(s, generator=g) for s in SHAPES]
    grads = [[torch.randn(s, generator=g) for s in SHAPES] for _ in range(3)]
    hp = dict(lr=1e-2, weight_decay=1e-2, **kw)

    def run(grouped, **ema):
        dev = [p.clone().to(DEV).requires_grad_(True) for p in ps]
        params = [{"params": [dev[0], dev[2]]}, {"params": [dev[1], dev[3]], "weight_decay": 0.0}, {"params": [dev[4]], "lr": 1e-3}] \
            if grouped else dev
        opt = _flat(kind, params, **hp, **ema, **({"layout_order": dev} if grouped else {}))
        _set_grads(dev, grads[0])
        opt._materialise()
        with _counted(_lib.load()) as c:
            for it in range(3):
                _set_grads(dev, grads[it])
                opt.step()
        torch.cuda.synchronize()
        bits = [b.clone() for b in (opt.flat_p, *opt.state_buffers(), opt.flat_w16.view(torch.int16), opt._t_dev)]
        return opt, c.names, bits

    for grouped in (False, True):
        old_entry = "optim_groups" if grouped else ("adam" if kind == "adam" else "optim")
        off, names, plain = run(grouped)
        assert off.flat_ema is None and not off.ema and names.get(old_entry) == 3 and "optim_ema" not in names, names
        zero, names, bits = run(grouped, ema_decay=0, ema_warmup=True)
        assert zero.flat_ema is None and names.get(old_entry) == 3 and "optim_ema" not in names, names
        assert all(torch.equal(a, b) for a, b in zip(plain, bits))
        on, names, bits = run(grouped, ema_decay=DECAY, ema_warmup=True)
        assert names.get("optim_ema") == 3 and not {"adam", "optim", "optim_groups"} & set(names), names
        for i, (a, b) in enumerate(zip(plain, bits)):
            assert torch.equal(a, b), f"the average changed the update: buffer {i}"
        assert on.flat_ema is not None and not torch.equal(on.flat_ema, on.flat_p) and bool(torch.isfinite(on.flat_ema).all())


# ---- 5. captured == eager ---------------------------------------------------------------------------------------------------------------
def _build_step(decay):
    """The small MTLStep workload of tests/test_gpu_param_groups.py (AdamW, ``no_decay_1d``, the backbone at half the learning
    rate), built the way the entry points build it; f32 contractions, dropout off."""
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
                         "param_groups.no_decay_1d=true", "param_groups.lr_scale.temporal_graph=0.5", f"ema.decay={decay}",
                         "ema.warmup=true"])
    flat = [*model.configure_optimizers(0), *(p for t in ("ar", "oscc", "lta", "pnr") for p in tasks[t].configure_optimizers(0))]
    opt = T.build_optimizer(cfg, T.build_param_groups(cfg, model, tasks), layout_order=flat)
    step = engine.MTLStep(model, tasks, crit, weights, opt, fused_backbone=True)
    return step, opt, dev, merged


def test_captured_step_equals_eager_and_the_average_does_not_change_the_trajectory(compute_restored):
    """Four eager steps against two eager steps, the capture and two replays: ``flat_ema`` bit-identical (the warm-up weight comes
    from the device counter, nothing is captured as a host value); and the parameters, the moments and the bf16 copies are those of
    the same run with ``ema.decay=0``."""
    def run(use_graph, decay):
        step, opt, dev, merged = _build_step(decay)
        if use_graph:
            step.capture(dev, merged, warmup=2)
            for _ in range(2):
                step.replay()
        else:
            for _ in range(4):
                step.step(dev, merged)
        torch.cuda.synchronize()
        state = [t.clone().cpu() for t in (opt.flat_p, *opt.state_buffers(), opt.flat_w16.view(torch.int16), opt._t_dev)]
        return state, (opt.flat_ema.clone().cpu() if opt.ema else None), opt
    eager, ema_eager, opt = run(False, DECAY)
    graph, ema_graph, _ = run(True, DECAY)
    off, none, opt_off = run(False, 0)
    assert int(eager[-1]) == int(graph[-1]) == int(off[-1]) == 4 and none is None and opt_off.flat_ema is None
    assert opt.grouped and opt.ema and opt.ema_warmup
    for i, (a, b, c) in enumerate(zip(eager, graph, off)):
        assert torch.equal(a, b), f"captured and eager differ in buffer {i}"
        assert torch.equal(a, c), f"the average changed buffer {i} of the trajectory"
    assert torch.equal(ema_eager, ema_graph)
    assert not torch.equal(ema_eager, eager[0]) and bool(torch.isfinite(ema_eager).all())


# ---- 6. main_temporal.py: resume, checkpoint_ema.pth, validation under the average (one child process) ----------------------------------
CHILD = r"""
import json, sys
from pathlib import Path
import torch
sys.path.insert(0, sys.argv[1])
tmp = Path(sys.argv[2])
import main_temporal
from egopack_amd import train as T

BASE = ["k=1", "batch_size=4", "synthetic_samples=8", "model.hidden_size=64", "model.temporal_pooling.hidden_size=64",
        "oscc_feat_size=64", "save_model=True", "compute=f32", "optimizer.lr=1e-3", "enabled_tasks=[ar,pnr]",
        "ema.decay=0.99", "ema.warmup=true", "lr_scheduler.T_max=3", "use_graph=false", "save_every=2"]
main_temporal.main(BASE + ["num_epochs=3", f"checkpoint_dir={tmp / 'full'}"])
main_temporal.main(BASE + ["num_epochs=2", f"checkpoint_dir={tmp / 'part'}"])
part = tmp / "part" / "MTL_ar-pnr" / "checkpoint.pth"
out = main_temporal.main(BASE + ["num_epochs=3", f"checkpoint_dir={tmp / 'resumed'}", f"resume_from={part}"])

# validation under the average: the logits of one validation batch inside ema_weights() ...
opt, step, device = out["optimizer"], out["step"], torch.device("cuda")


def logits_of(step, loaders):
    step.model.eval()
    for t in step.tasks.values():
        t.eval()
    got = {}
    with torch.no_grad():
        for t in step.enabled:
            b = next(iter(loaders[t]))
            _, vectors, logits = step.losses({t: b.to(device)})
            flat = []
            def walk(x):
                if torch.is_tensor(x):
                    flat.append(x.detach().float().cpu().clone())
                elif isinstance(x, dict):
                    for k in sorted(x):
                        walk(x[k])
                elif isinstance(x, (list, tuple)):
                    for y in x:
                        walk(y)
            walk(logits)
            walk(vectors)
            got[t] = flat
    return got


with opt.ema_weights():
    averaged = logits_of(step, out["val_loaders"])
raw = logits_of(step, out["val_loaders"])
# ... against a fresh model that loaded checkpoint_ema.pth through resume_from= (no epoch left to train)
ema_file = tmp / "resumed" / "MTL_ar-pnr" / "checkpoint_ema.pth"
fresh = main_temporal.main(BASE + ["num_epochs=3", "save_model=False", f"checkpoint_dir={tmp / 'fresh'}", f"resume_from={ema_file}"])
loaded = logits_of(fresh["step"], fresh["val_loaders"])
# ... and the file through load_checkpoint with strict_tasks=True into the resumed run's own modules (afterwards: nothing else runs)
T.load_checkpoint(ema_file, out["model"], out["tasks"], strict_tasks=True, device=device)
strict = {"temporal_graph": {k: v.detach().cpu() for k, v in out["model"].state_dict().items()}}
torch.save({"averaged": averaged, "raw": raw, "loaded": loaded, "strict": strict}, tmp / "logits.pt")
print("CHILD-OK")
"""


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    """3 epochs in one go, 2 epochs + the save_every checkpoint, the resumed third epoch -- with the average on -- in a child process."""
    tmp = tmp_path_factory.mktemp("ema_runs")
    script = tmp / "child.py"
    script.write_text(CHILD)
    r = subprocess.run([sys.executable, str(script), str(REPO), str(tmp)], capture_output=True, text=True, cwd=str(tmp), timeout=900)
    assert r.returncode == 0 and "CHILD-OK" in r.stdout, (r.returncode, r.stdout[-3000:], r.stderr[-6000:])
    load = lambda *parts: torch.load(tmp.joinpath(*parts), weights_only=False)
    return dict(tmp=tmp, log=r.stderr + r.stdout, full=load("full", "MTL_ar-pnr", "checkpoint.pth"), part=load("part", "MTL_ar-pnr", "checkpoint.pth"),
                resumed=load("resumed", "MTL_ar-pnr", "checkpoint.pth"), full_ema=load("full", "MTL_ar-pnr", "checkpoint_ema.pth"),
                resumed_ema=load("resumed", "MTL_ar-pnr", "checkpoint_ema.pth"), logits=load("logits.pt"))


MODULE_KEYS = ("temporal_graph", "task/recognition", "task/pnr")


@pytest.mark.timeout(900)
def test_main_temporal_resume_with_the_average_equals_the_uninterrupted_run(runs):
    full, part, res = runs["full"], runs["part"], runs["resumed"]
    assert part["epoch"] == 2 and res["epoch"] == full["epoch"] == 3
    assert part["optimizer"]["ema"]["decay"] == 0.99 and part["optimizer"]["ema"]["warmup"] is True
    moved = 0.0
    for key in MODULE_KEYS:
        for k, v in full[key].items():
            torch.testing.assert_close(res[key][k], v, rtol=0, atol=0, msg=lambda s: f"{key}.{k}: {s}")
            if v.is_floating_point():
                moved = max(moved, float((v - part[key][k]).abs().max()))
    assert moved > 0  # (the third epoch trained)
    a, b = full["optimizer"], res["optimizer"]
    assert sorted(a["state"]) == sorted(b["state"]) == sorted(a["ema"]["values"]) == sorted(b["ema"]["values"]) and a["state"]
    for i, st in a["state"].items():
        for k in ("exp_avg", "exp_avg_sq"):
            assert torch.equal(st[k], b["state"][i][k]), (i, k)
        assert float(st["step"]) == float(b["state"][i]["step"]) > 0
        assert torch.equal(a["ema"]["values"][i], b["ema"]["values"][i]), f"the average of parameter {i} differs after the resume"
    assert any(not torch.equal(a["ema"]["values"][i], part["optimizer"]["ema"]["values"][i]) for i in a["ema"]["values"])
    # one line per validation says which weights were scored
    assert runs["log"].count("validating the averaged weights (ema.decay 0.99, warm-up)") >= 3 + 2 + 1


@pytest.mark.timeout(900)
def test_checkpoint_ema_holds_the_reference_layout_and_the_averaged_weights(runs):
    """checkpoint_ema.pth: the reference's keys alone; its weights are the ``"ema"`` values of the ordinary checkpoint, parameter by
    parameter in the order the entry point hands them to the optimizer; it went through ``load_checkpoint(strict_tasks=True)``."""
    ck, ema_ck = runs["resumed"], runs["resumed_ema"]
    assert sorted(ema_ck) == sorted(["temporal_graph", "epoch", "task/recognition", "task/oscc", "task/lta", "task/pnr"])
    assert ema_ck["epoch"] == 3 and "optimizer" not in ema_ck
    for key in MODULE_KEYS:
        assert list(ema_ck[key]) == list(ck[key])
    for k, v in runs["full_ema"]["temporal_graph"].items():
        assert torch.equal(v, ema_ck["temporal_graph"][k]), k
    # every averaged tensor of the file is one of the optimizer's "ema" values, and it differs from the raw weight beside it
    values = list(ck["optimizer"]["ema"]["values"].values())
    matched, differ = 0, 0
    for key in MODULE_KEYS:
        for k, v in ema_ck[key].items():
            raw = ck[key][k]
            if torch.equal(v, raw):
                continue  # (buffers, and parameters without a gradient: never averaged, never moved)
            differ += 1
            matched += any(v.shape == e.shape and torch.equal(v, e) for e in values)
    assert differ > 0 and matched == differ
    # the strict load put the averaged weights into the modules
    for k, v in runs["logits"]["strict"]["temporal_graph"].items():
        assert torch.equal(v, ema_ck["temporal_graph"][k]), k


@pytest.mark.timeout(900)
def test_validation_inside_ema_weights_equals_a_fresh_model_that_loaded_checkpoint_ema(runs):
    lg = runs["logits"]
    assert sorted(lg["averaged"]) == sorted(lg["loaded"]) == ["ar", "pnr"]
    for t in lg["averaged"]:
        assert len(lg["averaged"][t]) == len(lg["loaded"][t]) > 0
        for i, (a, b) in enumerate(zip(lg["averaged"][t], lg["loaded"][t])):
            assert torch.equal(a, b), (t, i, float((a - b).abs().max()))
        assert any(not torch.equal(a, b) for a, b in zip(lg["averaged"][t], lg["raw"][t])), "the average scored like the raw weights"
