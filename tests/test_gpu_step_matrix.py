"""The opt-in features of the training step together, on the GPU: every row of the pairwise cover of
tests/step_matrix_common.py builds its step through the production builders and is held to the composed float64 host model --
(a) the loss half, (b) the update half, (c) captured equals eager, (d) the split form equals ``step.step``; row 0 ("all on") also
(e) inert factors stay inert and (f) a skipped step inside a replayed graph; (g) main_temporal.py with everything on, once, in a
child process: an interrupted and resumed run equals the uninterrupted one, and -- with the pooling's dropout off, whose masks a
replayed step draws from other offsets than an eager one -- the captured run ends where the eager one does.

Tolerances: tests/step_matrix_common.py names the owner of each.  Every comparison prints its worst error relative to its
tolerance on a line that starts with ``STEP-MATRIX`` (profiles/step_matrix.txt is that printout; nothing in it is a threshold).

Captured against eager, and the split form against ``step.step``: bit for bit, in every row -- what row 1 (all defaults) shows at
these sizes holds with every feature on."""
import subprocess
import sys
from pathlib import Path

import pytest
import torch

from tests import step_matrix_common as M

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF = torch.bfloat16
REPO = Path(__file__).resolve().parents[1]
ROWS = M.rows()
ROW_IDS = [r["id"] for r in ROWS]


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


def _note(row, test, what, value):
    print(f"STEP-MATRIX {row['id']} {test} {what} {value:.3e}" if isinstance(value, float) else f"STEP-MATRIX {row['id']} {test} {what} {value}")


def _inside(row, test, what, got, want, rtol, atol):
    r = M.ratio(got, want, rtol, atol)
    _note(row, test, f"{what} |error|/tolerance", r)
    assert r <= 1, f"{row['id']} {what}: {r:.3g} x the tolerance (rtol {rtol}, atol {atol})"


# ---- the clip must bite: half the smallest norm of the row's own unclipped run, measured once per row ---------------------------------
_CLIP = {}


def _clip_of(row):
    if not M.on(row, "grad_clip_norm"):
        return None
    key = row["levels"]
    if key not in _CLIP:
        step, opt, dev, merged, _ = M.build_step(row, clip=1e30)  # (a bound that clamps: the unclipped update)
        norms = []
        for _ in range(4):
            step.step(dev, merged)
            norms.append(opt.grad_norm_stats(reset=False)["last_norm"])
        assert all(n > 0 and n == n for n in norms), norms
        _CLIP[key] = 0.5 * min(norms)
        _note(row, "clip", "unclipped norms of steps 1-4", [round(n, 6) for n in norms])
    return _CLIP[key]


def _bits(t):
    return t.view(torch.int16) if t.dtype == BF else t


def _snapshot(step, opt):
    """Every buffer the comparisons read, on the host: parameters, the state buffers (as stored), the average, log_var, the counted
    step."""
    torch.cuda.synchronize()
    out = dict(flat_p=opt.flat_p.detach().clone().cpu(), t=int(opt._t_dev.item()))
    for i, b in enumerate(opt.state_buffers()):
        out[f"state{i}"] = _bits(b.detach().clone()).cpu()
    if opt.ema:
        out["flat_ema"] = opt.flat_ema.detach().clone().cpu()
    if step.task_log_var is not None:
        out["log_var"] = step.task_log_var.log_var.detach().clone().cpu()
    return out


def _same(row, test, a, b, keys=None):
    for k in (keys or a):
        x, y = a[k], b[k]
        if torch.is_tensor(x):
            diff = int((x != y).sum()) if x.shape == y.shape else -1
            _note(row, test, f"{k} elements that differ", diff)
            assert x.shape == y.shape and torch.equal(x, y), f"{row['id']} {test}: {k} differs in {diff} of {x.numel()} elements"
        else:
            assert x == y, f"{row['id']} {test}: {k}: {x} != {y}"


# ---- (a) the loss half ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("row", ROWS, ids=ROW_IDS)
def test_loss_half_matches_the_composed_float64_model(row, compute_restored):
    """Two eager steps, then a third with the criteria's ``select`` and the PNR head's one-pass launch spied: on the step's OWN
    logits and labels the loss vectors, the objective, d J / d log_var and the head gradient operands (the classifier banks'
    ``_egk_grad_dst`` blocks, the seed w_t scale_t / N baked in) against ``loss_model``."""
    compute, batch = row["size"]
    step, opt, dev, merged, _ = M.build_step(row, _clip_of(row))
    for _ in range(2):
        step.step(dev, merged)
    torch.cuda.synchronize()
    log_var = step.task_log_var.log_var.detach().float().cpu().clone() if step.task_log_var is not None else None
    seen = {}
    for t in ("ar", "lta"):
        def spy(logits, gt, t=t, inner=step.criteria[t].select):
            seen[t] = (list(logits), [l.detach().clone() for l in logits], gt.detach().clone())
            return inner(logits, gt)
        step.criteria[t].select = spy
    task = step.tasks["pnr"]

    def pnr_spy(features, targets, balance=None, inner=task.fused_head_loss):
        out = inner(features, targets, balance=balance)
        seen["pnr"] = (balance, None if out is None else (out[0].detach().clone(), out[1].detach().clone()))
        return out
    task.fused_head_loss = pnr_spy
    total, vs = step.step(dev, merged)
    for t in ("ar", "lta"):
        del step.criteria[t].select
    del task.fused_head_loss
    torch.cuda.synchronize()
    assert seen["pnr"][1] is not None, "the PNR head left the one-pass launch"
    sh = M.pnr_triple(row, batch)
    assert seen["pnr"][0] == (None if sh is None else tuple(float(v) for v in sh)), seen["pnr"][0]
    logits = {t: [l.float().cpu() for l in seen[t][1]] for t in ("ar", "lta")}
    labels = {t: seen[t][2].cpu() for t in ("ar", "lta")}
    logits["pnr"], labels["pnr"] = seen["pnr"][1][1].float().cpu(), dev["pnr"].y.cpu()
    n_full = {t: int(dev[t].y.shape[0]) for t in ("ar", "lta", "pnr")}
    ref = M.loss_model(row, logits, labels, step.weights, n_full, log_var, batch)
    if row["task_weighting"] != "none":
        got_scales = step.task_scales()
        for t, sc in ref["scales"].items():
            assert abs(got_scales[t] - sc) <= M.TW.ulp32(sc), (t, got_scales[t], sc)
    for t in ("ar", "lta"):
        ltol, gtol = M.ce_tols(row, t, compute)
        live_logits, _, gt = seen[t]
        dst = getattr(live_logits[0], "_egk_grad_dst", None)
        assert dst is not None, f"{t}: the logits are not blocks of a classifier bank: the fused launch did not run"
        gbuf = dst[0].detach()
        for h, x in enumerate(logits[t]):
            c0 = live_logits[h]._egk_grad_dst[1]
            block = gbuf[:, c0:c0 + x.shape[1]].float().cpu().double()
            # (class balance / ce_shape shaped it, task_weighting scaled its seed: the looser of ce_shape_common.tols and the
            #  bit-exact scaled seed of tests/test_gpu_task_weighting.py is the former)
            _inside(row, "loss", f"{t} head {h} operand", block, ref["operands"][t][h], **gtol)
        want = ref["vectors"][t]
        y = dev[t].y.cpu()
        if gt.shape != y.shape or not torch.equal(gt.cpu(), y):  # a compacted head: node n is row live_inv[n], the other nodes have loss 0
            inv = dev[t].live_inv.cpu()
            want = torch.where(inv >= 0, want[inv.clamp(min=0)], torch.zeros((), dtype=want.dtype))
        _inside(row, "loss", f"{t} loss vector", vs[t].cpu(), want, **ltol)
    # PNR: the loss vector against its model on the logits the one-pass launch wrote (tests/test_gpu_pnr_balance.py, in the step)
    _inside(row, "loss", "pnr loss vector", vs["pnr"].cpu(), ref["vectors"]["pnr"], **M.PB.LOSS_TOL)
    assert torch.equal(vs["pnr"], seen["pnr"][1][0])
    # the objective of the step's own loss vectors: egk_task_scale_grad's tolerance with task scales (tests/test_gpu_task_weighting.py),
    # the weighted mean's without (tests/test_gpu_ce_shape.py)
    own = {t: vs[t].detach().cpu() for t in ("ar", "lta", "pnr")}
    J, ds = M.objective_model(row, own, step.weights, n_full, log_var)
    otol = M.OBJECTIVE_TOL if row["task_weighting"] != "none" else dict(rtol=1e-5, atol=1e-6)
    _inside(row, "loss", "objective of the step's own vectors", total.double().cpu(), J, **otol)
    # ... and against the model's own vectors, at the loss vectors' tolerance (the looser of the two)
    slack = sum(step.weights[t] * ref["scales"][t] * (M.ce_tols(row, t, compute)[0]["atol"] + 2e-5 * abs(float(ref["vectors"][t].sum())) / n_full[t])
                for t in ("ar", "lta")) + step.weights["pnr"] * ref["scales"]["pnr"] * 2e-5 + 1e-5 * abs(ref["objective"])
    _note(row, "loss", "objective |error|/tolerance", abs(float(total) - ref["objective"]) / slack)
    assert abs(float(total) - ref["objective"]) <= slack
    if row["task_weighting"] == "uncertainty":
        _inside(row, "loss", "d J / d log_var", step.task_log_var.log_var.grad.detach().double().cpu(), ds, **M.DS_TOL)


# ---- (b) the update half ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("row", ROWS, ids=ROW_IDS)
def test_update_half_matches_the_composed_float64_model(row, compute_restored):
    """The state after two steps, ``forward_backward``, a snapshot, ``opt.step()``: every buffer against ``update_model`` of the
    snapshot.  A bf16 state: every stored element is a bf16 neighbour of the model's unrounded moment, and the parameters and the
    average meet the f32-state tolerance -- the update reads the unrounded moments."""
    clip = _clip_of(row)
    step, opt, dev, merged, _ = M.build_step(row, clip)
    for _ in range(2):
        step.step(dev, merged)
    if opt.clipping:
        opt.grad_norm_stats()  # (read and cleared: the figures below are the third step's alone)
    step.forward_backward(dev, merged)
    torch.cuda.synchronize()
    widen = lambda b: b.detach().float().cpu().clone()
    snap = dict(p=widen(opt.flat_p), g=widen(opt.flat_g), state=[widen(b) for b in opt.state_buffers()],
                ema=widen(opt.flat_ema) if opt.ema else None, t=int(opt._t_dev.item()), grad_scale=float(opt.grad_scale))
    assert snap["t"] == 2 and (opt.flat_ema is not None) == M.on(row, "ema") and opt.bf16_state == M.on(row, "optimizer_state")
    assert len(snap["state"]) == (1 if row["rule"] == "sgd" else 2) and opt.grouped == (M.on(row, "param_groups") or step.task_log_var is not None)
    lv = step.task_log_var.log_var if step.task_log_var is not None else None
    opt.step()
    torch.cuda.synchronize()
    groups = M.groups_of(opt, lv)
    if lv is not None:  # the learned log-variances: the LAST slot, a group of its own, clipped, averaged and rounded like any other
        lo, hi = groups["log_var"]
        assert hi == opt.flat_p.numel() and opt.param_groups[-1]["name"] == "task_weighting" and float(groups["wd"][lo]) == 0.0
        assert bool((snap["g"][lo:lo + 3] != 0).all()), "log_var has no gradient"
    ref = M.update_model(row, snap["p"], snap["g"], snap["state"], snap["ema"], snap["t"] + 1, groups, clip=clip or 0.0,
                         grad_scale=snap["grad_scale"])
    assert not ref["skipped"] and int(opt._t_dev.item()) == snap["t"] + 1
    # (the rule wrote p; groups, the clip coefficient and the state's element type act on it too: tests/test_gpu_optim_rules.py TOL is
    #  the loosest of theirs -- tests/test_gpu_param_groups.py and tests/test_gpu_optim_state.py are bit for bit)
    _inside(row, "update", "flat_p", opt.flat_p.cpu(), ref["p"], **M.RULE_TOL)
    moved = float((opt.flat_p.cpu() - snap["p"]).abs().max())
    assert moved > 0
    for i, (b, want, sc) in enumerate(zip(opt.state_buffers(), ref["state"], ref["state_scale"])):
        if opt.bf16_state:
            assert b.dtype == BF
            ok = M.bf16_state_ok(b.float().cpu(), want, sc)
            _note(row, "update", f"state{i} bf16 elements outside the model's bracket", int((~ok).sum()))
            assert bool(ok.all()), f"{row['id']} state{i}: {int((~ok).sum())} stored elements are no bf16 neighbour of the model's moment"
            assert int((b.float().cpu() != snap["state"][i]).sum()) > 0
        else:
            _inside(row, "update", f"state{i}", b.cpu(), want, **M.RULE_TOL)
            # (that tolerance's atol of 1e-6 is above the whole second moment of these gradients: the moments are also held to the
            #  slack the bf16 bracket uses -- 16 f32 ulps of the magnitude of the terms that were added)
            r = float(((b.cpu().double() - want).abs() / (M.STATE_ULPS * sc + 1e-45)).max())
            _note(row, "update", f"state{i} |error|/(16 f32 ulps of the terms)", r)
            assert r <= 1, f"{row['id']} state{i}: {r:.3g} x 16 f32 ulps of its terms"
    if opt.ema:  # (tests/test_gpu_ema.py is bit for bit GIVEN p; p carries the rule's tolerance: the looser)
        _inside(row, "update", "flat_ema", opt.flat_ema.cpu(), ref["ema"], **M.RULE_TOL)
        assert not torch.equal(opt.flat_ema.cpu(), snap["ema"])
    if opt.clipping:
        stats = opt.grad_norm_stats()
        rel = abs(stats["last_norm"] - ref["norm"]) / ref["norm"]
        _note(row, "update", "norm |error|/bound", rel / M.norm_bound(opt.flat_g.numel()))
        assert rel <= M.norm_bound(opt.flat_g.numel()), (stats["last_norm"], ref["norm"])
        assert stats["clipped"] == 1 and stats["steps"] == 1 and stats["skipped"] == 0 and ref["coef"] < 1, (stats, ref["coef"])
    if lv is not None:
        lo, _ = groups["log_var"]
        got, want = lv.detach().double().cpu(), ref["p"][lo:lo + lv.numel()].double()
        assert bool((got != snap["p"][lo:lo + lv.numel()].double()).all()), "log_var did not move"
        _inside(row, "update", "log_var", got, want, **M.RULE_TOL)


# ---- (c) captured equals eager, (d) the split form equals step.step ---------------------------------------------------------------------
_EAGER = {}


def _four_steps(row, how, clip, manual=None):
    """Four steps from the row's start state: "eager" (four ``step.step``), "graph" (``capture(warmup=2)`` and two replays) or
    "split" (three ``step.step``, then ``forward_backward`` + ``opt.step()``)."""
    step, opt, dev, merged, _ = M.build_step(row, clip, manual=manual)
    if how == "graph":
        step.capture(dev, merged, warmup=2)
        for _ in range(2):
            step.replay()
    else:
        for _ in range(4 if how == "eager" else 3):
            step.step(dev, merged)
        if how == "split":
            step.forward_backward(dev, merged)
            opt.step()
    out = _snapshot(step, opt)
    if how != "split":
        out["loss_sums"] = step.loss_sums()
        if opt.clipping:
            out["grad_norm_stats"] = step.grad_norm_stats()
    assert bool(torch.isfinite(out["flat_p"]).all())
    return out


def _eager(row):
    if row["levels"] not in _EAGER:
        _EAGER[row["levels"]] = _four_steps(row, "eager", _clip_of(row))
    return _EAGER[row["levels"]]


@pytest.mark.parametrize("row", ROWS, ids=ROW_IDS)
def test_captured_step_replayed_twice_equals_four_eager_steps(row, compute_restored):
    """flat_p, every state buffer, flat_ema, log_var, loss_sums(), the counted step and the gradient-norm statistics: bit for bit."""
    eager = _eager(row)
    graph = _four_steps(row, "graph", _clip_of(row))
    assert eager["t"] == graph["t"] == 4
    _same(row, "captured", graph, eager)
    assert all(n > 0 for _, n in eager["loss_sums"].values())
    if M.on(row, "grad_clip_norm"):
        assert eager["grad_norm_stats"]["clipped"] >= 1 and eager["grad_norm_stats"]["skipped"] == 0, eager["grad_norm_stats"]


@pytest.mark.parametrize("row", ROWS, ids=ROW_IDS)
def test_split_form_equals_step_step(row, compute_restored):
    """After three steps ``forward_backward`` + ``opt.step()`` leaves what ``step.step`` leaves, bit for bit."""
    eager = _eager(row)
    split = _four_steps(row, "split", _clip_of(row))
    _same(row, "split", split, eager, keys=list(split))


# ---- (e) inert factors stay inert, (f) a skipped step: row 0 ----------------------------------------------------------------------------
def test_inert_factors_stay_inert_with_everything_else_on(compute_restored):
    """Row 0 without the average: the same flat_p bits (the average reads the update, it never feeds it).  Row 0 with a manual scale
    of exactly 1.0 on every task: the bits of ``task_weighting.mode=none`` with the other factors unchanged."""
    row = ROWS[0]
    clip = _clip_of(row)
    on_ = _eager(row)
    off = _four_steps(M.variant(row, ema="off"), "eager", clip)
    assert "flat_ema" in on_ and "flat_ema" not in off
    _same(row, "inert-ema", off, on_, keys=[k for k in off if k not in ("loss_sums", "grad_norm_stats")])
    assert off["loss_sums"] == on_["loss_sums"] and off["grad_norm_stats"] == on_["grad_norm_stats"]
    manual = _four_steps(M.variant(row, task_weighting="manual"), "eager", clip, manual={t: 1.0 for t in ("ar", "lta", "pnr")})
    none = _four_steps(M.variant(row, task_weighting="none"), "eager", clip)
    _same(row, "inert-scale-1", manual, none, keys=[k for k in none if k != "loss_sums"])
    # (the REPORTED per-task loss sums come from another launch with task scales -- egk_task_scale_grad sums the elements in f64, the
    #  weighted-mean launch sums each step's vector in f32 first: equal to the bound tests/test_gpu_task_weighting.py holds those sums to)
    for t, (s_, n_) in none["loss_sums"].items():
        assert manual["loss_sums"][t][1] == n_ and abs(manual["loss_sums"][t][0] - s_) <= 1e-6 * abs(s_), (t, manual["loss_sums"][t], s_)
    assert not torch.equal(none["flat_p"], on_["flat_p"][:none["flat_p"].numel()]), "the learned weights changed nothing"


def test_skipped_step_inside_a_replayed_graph_with_everything_on(compute_restored):
    """Row 0.  An inf planted in the static input between two replays: that replay changes none of flat_p, the states, flat_ema,
    log_var or the counted step; the next clean replay equals an eager run that skipped the same step, bit for bit -- the warm-up
    weight of the average and the rounding stream of the bf16 state both key on the COUNTED step, which a skipped step leaves."""
    row = ROWS[0]
    clip = _clip_of(row)

    def run(use_graph):
        step, opt, dev, merged, _ = M.build_step(row, clip)
        one = step.replay if use_graph else (lambda: step.step(dev, merged))
        if use_graph:
            step.capture(dev, merged, warmup=2)
        else:
            for _ in range(2):
                one()
        one()
        before = _snapshot(step, opt)
        keep = merged.x[5, 1, 9].clone()
        merged.x[5, 1, 9] = float("inf")
        one()
        after = _snapshot(step, opt)
        merged.x[5, 1, 9] = keep
        one()
        end = _snapshot(step, opt)
        return before, after, end, step.grad_norm_stats()
    g_before, g_after, g_end, g_stats = run(True)
    assert g_before["t"] == 3
    _same(row, "skipped", g_after, g_before)
    assert g_end["t"] == 4 and g_stats["skipped"] == 1 and g_stats["steps"] == 5, g_stats
    assert not torch.equal(g_end["flat_p"], g_before["flat_p"]) and bool(torch.isfinite(g_end["flat_p"]).all())
    assert not torch.equal(g_end["log_var"], g_before["log_var"]) and not torch.equal(g_end["flat_ema"], g_before["flat_ema"])
    e_before, e_after, e_end, e_stats = run(False)
    _same(row, "skipped-eager", e_after, e_before)
    _same(row, "skipped-vs-eager", g_end, e_end)
    assert e_stats["skipped"] == 1
    # every step reads the same static batch, so the step that followed the skipped one must BE step 4 of the undisturbed run: had the
    # skipped step moved the counted step on, the average's warm-up weight and the state's rounding bits would be those of step 5
    _same(row, "skipped-vs-undisturbed", g_end, _eager(row), keys=list(g_end))


# ---- (g) the entry point, once, in a child process ----------------------------------------------------------------------------------------
CHILD = r"""
import sys
from pathlib import Path
sys.path.insert(0, sys.argv[1])
tmp = Path(sys.argv[2])
import main_temporal

BASE = ["k=1", "batch_size=4", "synthetic_samples=8", "model.hidden_size=64", "model.temporal_pooling.hidden_size=64",
        "oscc_feat_size=64", "save_model=True", "compute=f32", "optimizer.lr=1e-3", "lr_scheduler.T_max=3", "save_every=2",
        "class_balance.mode=weight", "ce_shape.margin=ldam", "ce_shape.gamma=1", "ce_shape.reweight_after=2",
        "pnr_balance.mode=focal", "task_weighting.mode=uncertainty", "grad_clip_norm=0.25", "ema.decay=0.99", "ema.warmup=true",
        "optimizer_state.dtype=bf16", "param_groups.no_decay_1d=true", "lta_sampling.mode=philox"]
EAGER, GRAPH = ["use_graph=false"], ["use_graph=true"]
name = "MTL_ar-lta-oscc-pnr"


def mark(what):
    print(f"STEP-MATRIX-RUN {what}", file=sys.stderr, flush=True)


mark("full")
main_temporal.main(BASE + EAGER + ["num_epochs=3", f"checkpoint_dir={tmp / 'full'}"])
mark("part")
main_temporal.main(BASE + EAGER + ["num_epochs=2", f"checkpoint_dir={tmp / 'part'}"])
mark("resumed")
part = tmp / "part" / name / "checkpoint.pth"
main_temporal.main(BASE + EAGER + ["num_epochs=3", f"checkpoint_dir={tmp / 'resumed'}", f"resume_from={part}"])
# the other value of use_graph.  A replayed step draws its dropout masks from other Philox offsets than an eager one (the reason the
# resume tests step eagerly), so this pair runs with the pooling's dropout off: everything else as above
NO_DROPOUT = ["model.temporal_pooling.dropout=0"]
mark("graph")
main_temporal.main(BASE + GRAPH + NO_DROPOUT + ["num_epochs=3", f"checkpoint_dir={tmp / 'graph'}"])
mark("eager")
main_temporal.main(BASE + EAGER + NO_DROPOUT + ["num_epochs=3", f"checkpoint_dir={tmp / 'eager'}"])
mark("end")
print("CHILD-OK")
"""
NAME = "MTL_ar-lta-oscc-pnr"
MODULE_KEYS = ("temporal_graph", "task/recognition", "task/oscc", "task/lta", "task/pnr")


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    """Everything on, all four tasks: 3 epochs in one go; 2 epochs and the save_every checkpoint; the resumed third epoch; and the 3
    epochs without dropout, once with the captured step and once eagerly -- one fresh child process, started with a time limit."""
    tmp = tmp_path_factory.mktemp("step_matrix_runs")
    script = tmp / "child.py"
    script.write_text(CHILD)
    r = subprocess.run([sys.executable, str(script), str(REPO), str(tmp)], capture_output=True, text=True, cwd=str(tmp), timeout=900)
    assert r.returncode == 0 and "CHILD-OK" in r.stdout, (r.returncode, r.stdout[-3000:], r.stderr[-6000:])
    load = lambda d: torch.load(tmp / d / NAME / "checkpoint.pth", weights_only=False)
    log, parts = r.stderr, {}
    for chunk in log.split("STEP-MATRIX-RUN ")[1:]:
        head, _, body = chunk.partition("\n")
        parts[head.strip()] = body
    return dict(logs=parts, full=load("full"), part=load("part"), resumed=load("resumed"), graph=load("graph"), eager=load("eager"))


def _checkpoints_equal(a, b, what):
    for key in MODULE_KEYS:
        assert list(a[key]) == list(b[key]), key
        for k, v in a[key].items():
            assert torch.equal(v, b[key][k]), f"{what}: {key}.{k}"
    oa, ob = a["optimizer"], b["optimizer"]
    assert sorted(oa["state"]) == sorted(ob["state"]) and oa["state"]
    for i, st in oa["state"].items():
        assert sorted(st) == sorted(ob["state"][i])
        for k, v in st.items():
            if torch.is_tensor(v) and v.numel() > 1:
                assert torch.equal(v, ob["state"][i][k]), f"{what}: optimizer state {i}.{k}"
            else:
                assert float(v) == float(ob["state"][i][k]) and (k != "step" or float(v) > 0), f"{what}: optimizer state {i}.{k}"
    for k in ("state_dtype", "state_rounding", "state_seed"):
        assert oa[k] == ob[k]
    assert sorted(oa["ema"]["values"]) == sorted(ob["ema"]["values"]) == sorted(oa["state"])
    for i, v in oa["ema"]["values"].items():
        assert torch.equal(v, ob["ema"]["values"][i]), f"{what}: the average of parameter {i}"
    ta, tb = a["task_weighting"], b["task_weighting"]
    assert ta["tasks"] == tb["tasks"] == ["ar", "lta", "oscc", "pnr"] and ta["config"] == tb["config"]
    assert torch.equal(ta["log_var"], tb["log_var"]) and bool((ta["log_var"] != 0).all()), f"{what}: log_var"
    ca, cb = a["class_balance"], b["class_balance"]
    assert ca["config"] == cb["config"] and ca["vectors"].keys() == cb["vectors"].keys() == {"ar", "lta"}
    for t in ca["vectors"]:
        for x, y in zip(ca["vectors"][t]["weights"], cb["vectors"][t]["weights"]):
            assert torch.equal(x, y)
    assert torch.equal(a["pnr_balance"]["scalars"], b["pnr_balance"]["scalars"]) and a["pnr_balance"]["counts"] == b["pnr_balance"]["counts"]


def _validation(log):
    """The validation lines of a run's log without their time stamps: the meters' lines and the loss line of every validated epoch."""
    meters = [line.split("[val ", 1)[1] for line in log.splitlines() if "[val " in line]
    losses = [line.split("validation losses:", 1)[1] for line in log.splitlines() if "validation losses:" in line]
    return meters, losses


@pytest.mark.timeout(900)
def test_main_temporal_with_everything_on_resumes_bit_for_bit(runs):
    full, part, res, logs = runs["full"], runs["part"], runs["resumed"], runs["logs"]
    assert part["epoch"] == 2 and res["epoch"] == full["epoch"] == 3
    assert part["optimizer"]["state_dtype"] == "bf16" and part["optimizer"]["ema"]["decay"] == 0.99
    assert part["task_weighting"]["config"]["mode"] == "uncertainty" and part["pnr_balance"]["config"]["mode"] == "focal"
    _checkpoints_equal(full, res, "resumed against uninterrupted")
    moved = max(float((v - part["temporal_graph"][k]).abs().max()) for k, v in full["temporal_graph"].items() if v.is_floating_point())
    assert moved > 0 and not torch.equal(full["task_weighting"]["log_var"], part["task_weighting"]["log_var"])  # (the third epoch trained)
    # the features were on: the clip bit, the class weights came in at epoch 2 -- in the uninterrupted run, and, from the checkpoint's
    # epoch, in the resumed one (its only epoch trains with them)
    clipped = [int(line.split("clipped ", 1)[1].split()[0]) for line in logs["full"].splitlines() if "gradient norm mean" in line]
    assert len(clipped) == 3 and all(c > 0 for c in clipped), clipped
    assert logs["full"].count("from epoch 2 on the class weights apply") == 1 and "skipped 0" in logs["full"]
    assert "differ from the checkpoint's" not in logs["resumed"]
    # the logged validation of the last epoch is identical
    (m_full, l_full), (m_res, l_res) = _validation(logs["full"]), _validation(logs["resumed"])
    assert m_res and len(m_full) == 3 * len(m_res) and len(l_full) == 3 and len(l_res) == 1
    assert m_full[-len(m_res):] == m_res and l_full[-1] == l_res[0], (m_full[-len(m_res):], m_res, l_full[-1], l_res)


@pytest.mark.timeout(900)
def test_main_temporal_with_the_captured_step_ends_on_the_eager_checkpoint(runs):
    """``use_graph=true`` against ``use_graph=false`` (both without dropout, whose masks a replayed step draws from other offsets):
    the same checkpoint, bit for bit (the degree (c) found), the same logged validation, and the captured step did run."""
    replayed = [line for line in runs["logs"]["graph"].splitlines() if "replayed the captured step" in line]
    assert len(replayed) == 3 and not any(": 0 steps replayed" in line for line in replayed[1:]), replayed
    assert all(": 0 steps replayed" in line for line in runs["logs"]["eager"].splitlines() if "replayed the captured step" in line)
    _checkpoints_equal(runs["eager"], runs["graph"], "captured against eager")
    assert _validation(runs["logs"]["graph"]) == _validation(runs["logs"]["eager"])
    # (and dropout was on in the three runs of the resume test: they end elsewhere)
    assert not torch.equal(runs["full"]["temporal_graph"]["temporal_pooling.proj.0.weight"],
                           runs["eager"]["temporal_graph"]["temporal_pooling.proj.0.weight"])
