"""The opt-in features of the training step TOGETHER: the factor table, a fixed pairwise cover of it, the builder
that goes through the production builders of egopack_amd/train.py, the composed float64 host model -- put together from the
per-feature models of tests/*_common.py, never from a launch -- and its mutants, one composition slip each.  Shared by
tests/test_step_matrix_cpu.py (cover, reachability in f32, teeth) and tests/test_gpu_step_matrix.py.  Imports without a GPU.

    loss half    AR / LTA  ce_shape_common.reference(x, y, w, a, m, eps, gamma, seed)       PNR  pnr_balance_common.model
                 OSCC      class_balance_common.model (plain)                               J    task_weighting_common.objective
                 seed_t = w_t * scale_t / N_t        (N_t: the NODES of the task's batch, also for a compacted head)
    update half  norm = grad_scale * ||g||  over ALL slots, log_var's included
                 coef = min(1, c / (norm + 1e-6))                                           (small_constants_common.clip_ref)
                 the rule per element with its group's lr and weight decay on  g * grad_scale * coef
                 ema  = ema_common.ema_model(ema, p_new, ema_weight(decay, warmup, t))

Tolerances: none is invented here; the constants under "tolerances" name the test that owns each one."""
import math

import numpy as np
import torch

from tests import ce_shape_common as S
from tests import class_balance_common as CB
from tests import ema_common as E
from tests import pnr_balance_common as PB
from tests import small_constants_common as SC
from tests import task_weighting_common as TW

DEV = "cuda"
F64 = torch.float64
BF = torch.bfloat16

# ---- the factor table: level 0 is the default, the last level is "on" ---------------------------------------------------------------
FACTORS = ("rule", "param_groups", "grad_clip_norm", "ema", "optimizer_state", "class_balance", "ce_shape", "pnr_balance",
           "task_weighting", "size")
LEVELS = {
    "rule": ("adam", "adamw", "sgd"),                       # optimizer._target_: torch.optim.Adam | AdamW | SGD with momentum 0.9
    "param_groups": ("off", "on"),                          # no_decay_1d=true, lr_scale {temporal_graph: 0.5, tasks: 2.0}
    "grad_clip_norm": ("off", "on"),                        # half the row's unclipped norm (``the clip must bite``)
    "ema": ("off", "on"),                                   # decay 0.99, warmup
    "optimizer_state": ("f32", "bf16"),                     # bf16: stochastic rounding, seed 5
    "class_balance": ("none", "weight", "logit_adjust"),
    "ce_shape": ("off", "on"),                              # margin ldam, gamma 0.5 (AR) / 2.0 (LTA)
    "pnr_balance": ("none", "pos_weight", "focal"),
    "task_weighting": ("none", "manual", "uncertainty"),
    "size": (("f32", 2), ("bf16", 8)),                      # tests/test_gpu_ce_shape.py SIZES: per-task launches | the banked ONE launch
}
TARGETS = {"adam": "torch.optim.Adam", "adamw": "torch.optim.AdamW", "sgd": "torch.optim.SGD"}
LR, WD = 1e-2, 1e-2            # optimizer.lr / optimizer.weight_decay of every row (a decay large enough that its slips show)
MOMENTUM = 0.9
LR_SCALE = {"temporal_graph": 0.5, "tasks": 2.0}
EMA_DECAY, EMA_WARMUP = 0.99, True
STATE_SEED = 5
GAMMA = {"ar": 0.5, "lta": 2.0}
MANUAL = {"ar": 0.75, "lta": 1.5, "pnr": 0.6}               # unequal, away from 1, none a power of two
HEADS = (115, 478)
T_NODES = 8
ORDER = ("ar", "lta", "oscc", "pnr")
MAX_ROWS = 16

# Level indices in the order of FACTORS.  Row 0: every factor at its last level; row 1: every factor at level 0; together the rows
# hold every pair of levels of two different factors (``uncovered``).  Written out, not generated: the ids of the GPU tests are stable.
ROWS = [
    (2, 1, 1, 1, 1, 2, 1, 2, 2, 1),
    (0, 0, 0, 0, 0, 0, 0, 0, 0, 0),
    (1, 1, 0, 0, 1, 1, 0, 1, 1, 1),
    (0, 0, 1, 1, 0, 1, 1, 1, 1, 0),
    (1, 0, 0, 1, 0, 0, 1, 0, 2, 1),
    (1, 0, 1, 0, 1, 2, 0, 2, 0, 0),
    (2, 1, 0, 0, 0, 1, 1, 0, 0, 0),
    (0, 1, 1, 0, 1, 0, 0, 0, 2, 0),
    (2, 0, 0, 1, 0, 0, 0, 2, 1, 0),
    (0, 0, 0, 1, 0, 2, 0, 1, 0, 1),
    (0, 1, 1, 0, 1, 2, 1, 0, 1, 1),
    (0, 1, 1, 1, 0, 1, 0, 2, 2, 1),
    (2, 0, 1, 0, 1, 0, 1, 1, 2, 1),
]
# Pairs of levels that are refused by name before any launch, ((factor, level), (factor, level), reason): none was found.
REFUSED = []


def row_id(levels) -> str:
    short = {"none": "0", "off": "0", "on": "1", "f32": "f32", "bf16": "bf16"}
    parts = []
    for f, i in zip(FACTORS, levels):
        v = LEVELS[f][i]
        parts.append(f"{v[0]}B{v[1]}" if f == "size" else short.get(v, v))
    return "-".join(parts)


def rows():
    """The fixed rows as dicts: factor -> level value, plus ``levels`` (the indices) and ``id``."""
    out = []
    for k, levels in enumerate(ROWS):
        r = {f: LEVELS[f][i] for f, i in zip(FACTORS, levels)}
        r["levels"], r["id"] = tuple(levels), f"r{k:02d}-{row_id(levels)}"
        out.append(r)
    return out


def variant(row, **levels):
    """``row`` with the named factors at other level VALUES (a row outside the fixed list, for the 'inert factor' comparisons)."""
    idx = list(row["levels"])
    for f, v in levels.items():
        idx[FACTORS.index(f)] = LEVELS[f].index(v)
    r = {f: LEVELS[f][i] for f, i in zip(FACTORS, idx)}
    r["levels"], r["id"] = tuple(idx), "variant-" + row_id(idx)
    return r


def all_pairs():
    return {((f, a), (g, b)) for i, f in enumerate(FACTORS) for g in FACTORS[i + 1:]
            for a in range(len(LEVELS[f])) for b in range(len(LEVELS[g]))}


def uncovered(level_rows=None):
    """The pairs of levels of two different factors that no row holds, the refused ones left out."""
    level_rows = ROWS if level_rows is None else level_rows
    seen = {((f, r[i]), (g, r[j])) for r in level_rows for i, f in enumerate(FACTORS) for j, g in enumerate(FACTORS) if i < j}
    refused = {(a, b) for a, b, _ in REFUSED} | {(b, a) for a, b, _ in REFUSED}
    return all_pairs() - seen - refused


def on(row, factor) -> bool:
    return row["levels"][FACTORS.index(factor)] != 0


# ---- the configuration of a row -----------------------------------------------------------------------------------------------------
def overrides(row, clip=None):
    """The command-line overrides of the row.  ``clip``: the bound of a row that clips (None: 1.0, for the configuration checks)."""
    over = [f"optimizer._target_={TARGETS[row['rule']]}", f"optimizer.lr={LR}", f"optimizer.weight_decay={WD}"]
    if row["rule"] == "sgd":
        over.append(f"+optimizer.momentum={MOMENTUM}")
    if on(row, "param_groups"):
        over += ["param_groups.no_decay_1d=true"] + [f"param_groups.lr_scale.{k}={v}" for k, v in LR_SCALE.items()]
    if on(row, "grad_clip_norm"):
        over.append(f"grad_clip_norm={1.0 if clip is None else repr(float(clip))}")
    if on(row, "ema"):
        over += [f"ema.decay={EMA_DECAY}", f"ema.warmup={'true' if EMA_WARMUP else 'false'}"]
    if on(row, "optimizer_state"):
        over += ["optimizer_state.dtype=bf16", "optimizer_state.rounding=stochastic", f"optimizer_state.seed={STATE_SEED}"]
    over.append(f"class_balance.mode={row['class_balance']}")
    if on(row, "ce_shape"):
        over += ["ce_shape.margin=ldam", f"ce_shape.gamma={GAMMA['ar']}"]  # (one exponent per run in the config; the criteria below: per task)
    over.append(f"pnr_balance.mode={row['pnr_balance']}")
    over.append(f"task_weighting.mode={row['task_weighting']}")
    return over


def terms(row, task):
    """The vectors and the exponent the AR / LTA criterion of the row carries: dict(w, a, m: [per head] of host f32 vectors or
    None, gamma)."""
    none = [None] * len(HEADS)
    return dict(w=[CB.zipf_weights(c) for c in HEADS] if row["class_balance"] == "weight" else none,
                a=[CB.zipf_offsets(c) for c in HEADS] if row["class_balance"] == "logit_adjust" else none,
                m=[S.ldam(c) for c in HEADS] if on(row, "ce_shape") else none,
                gamma=GAMMA[task] if on(row, "ce_shape") else 0.0)


def pnr_triple(row, batch):
    """(pos, neg, gamma) of the row through train.pnr_scalars on the counts of the step's batch -- one positive node per sequence
    of T_NODES -- or None with the feature off."""
    if row["pnr_balance"] == "none":
        return None
    from egopack_amd import train as T
    pb = T.pnr_balance_config({"pnr_balance": {"mode": row["pnr_balance"]}})
    return T.pnr_scalars(pb, batch, batch * (T_NODES - 1))


def criteria(row, base, batch):
    """The criteria of the row, built as train.build_criteria builds them: a task's wrapper gets the keywords of the features that
    are on and no others; with every loss feature off these are the criteria bench.py builds."""
    from egopack_amd.criterion import BCEWithLogitsNone, CrossEntropyNone, MetricSelectorWrapper

    class DS:
        has_joint_label, num_labels = False, 2
    crit = dict(base)
    for t in ("ar", "lta"):
        tm, kw = terms(row, t), {}
        if row["class_balance"] != "none":
            kw.update(class_weights=tm["w"] if row["class_balance"] == "weight" else None,
                      class_offsets=tm["a"] if row["class_balance"] == "logit_adjust" else None)
        if on(row, "ce_shape"):
            kw.update(class_margins=tm["m"], focal_gamma=tm["gamma"])
        if kw:
            crit[t] = MetricSelectorWrapper(CrossEntropyNone(), DS(), **kw)
    sh = pnr_triple(row, batch)
    if sh is not None:
        crit["pnr"] = BCEWithLogitsNone(*sh)
    return crit


def build_step(row, clip=None, manual=None, seed=11):
    """The step of the row the way main_temporal.main builds it: load_config with the row's overrides, build_task_weighting,
    build_param_groups, build_optimizer(layout_order=, log_var=), the criteria with the row's vectors and scalars, engine.MTLStep
    with the mode and log_var.  The workload is bench.py's (AR + LTA + PNR, T = 8, H = 64, dropout off) at the row's size.
    Returns (step, opt, dev, merged, cfg).  ``manual``: the scales of a manual row (default MANUAL)."""
    import bench
    from egopack_amd import engine, ops
    from egopack_amd import train as T
    compute, batch = row["size"]
    args = bench.parse_args(["--workload", "mtl", "--batch", str(batch), "--T", str(T_NODES), "--hidden", "64", "--trn-hidden", "64",
                             "--dropout", "0.0", "--compute", compute])
    ops.set_compute(compute)
    ops.manual_seed(seed)
    model, tasks, crit, weights, dev, merged = bench.build_workload(args, 0, torch.device(DEV))
    model.to(DEV).train()
    for t in tasks.values():
        t.to(DEV).train()
    cfg = T.load_config(overrides(row, clip))
    crit = {t: c.to(DEV).train() for t, c in criteria(row, crit, batch).items()}
    wd = cfg.optimizer.weight_decay
    flat = [*model.configure_optimizers(wd), *(p for t in ORDER for p in tasks[t].configure_optimizers(wd))]
    mode = T.task_weighting_config(cfg)["mode"]
    log_var = T.build_task_weighting(cfg, [t for t in engine.MTLStep.order if weights.get(t, 0) > 0 and t in tasks], DEV)
    opt = T.build_optimizer(cfg, T.build_param_groups(cfg, model, tasks), layout_order=flat, log_var=log_var)
    step = engine.MTLStep(model, tasks, crit, weights, opt, fused_backbone=True, task_weighting=mode, log_var=log_var)
    if mode == "manual":
        step.set_task_scale(MANUAL if manual is None else manual)
    return step, opt, dev, merged, cfg


# ---- tolerances: each belongs to the test that owns the tensor's last operation ---------------------------------------------------
RULE_TOL = dict(rtol=1e-5, atol=1e-6)       # tests/test_gpu_optim_rules.py TOL (= tests/test_gpu_grad_clip.py TOL): p, the state, ema
OBJECTIVE_TOL = dict(rtol=1e-6, atol=0.0)   # tests/test_gpu_task_weighting.py: J from the step's own loss vectors
DS_TOL = dict(rtol=1e-6, atol=1e-9)         # ... and d J / d log_var
CAPTURED_ATOL = 1e-6                        # tests/test_gpu_grad_clip.py::test_captured_clipped_step_equals_eager (MTL)


def ce_tols(row, task, compute):
    """(loss, operand) tolerances of an AR / LTA head: ce_shape_common.tols(gamma) with the allowances of
    tests/test_gpu_ce_shape.py::test_terms_on_in_the_step_match_float64_and_add_no_launch -- the loss vector rtol + 1e-5 and twice
    the atol (two heads summed), the operand one bf16 rounding (2^-8 relative) in bf16 mode."""
    ltol, gtol = S.tols(terms(row, task)["gamma"])
    return (dict(rtol=ltol["rtol"] + 1e-5, atol=2 * ltol["atol"]),
            dict(rtol=gtol["rtol"] + (2.0 ** -8 if compute == "bf16" else 0.0), atol=gtol["atol"]))


def norm_bound(n) -> float:
    """tests/test_gpu_grad_clip.py::test_eager_step_norm_and_clipped_update: relative, the f64 sum's bound plus one f32 rounding."""
    return 2 * n * 2.0 ** -53 + 2.0 ** -24


def ratio(got, want, rtol, atol):
    """max |got - want| / (atol + rtol |want|): <= 1 is inside the tolerance."""
    got, want = torch.as_tensor(got, dtype=F64).reshape(-1), torch.as_tensor(want, dtype=F64).reshape(-1)
    if not got.numel():
        return 0.0
    den = atol + rtol * want.abs()
    d = (got - want).abs()
    return float(torch.where(den > 0, d / den.clamp(min=1e-300), torch.where(d > 0, torch.full_like(d, float("inf")), torch.zeros_like(d))).max())


# ---- the loss half ---------------------------------------------------------------------------------------------------------------
LOSS_MUTANTS = {
    # name: (the factors that must be on, the tensor it moves)
    "scale_not_on_seed": ({"task_weighting"}, "operands"),    # the task scale applied to the loss but not to the seed
    "uncertainty_no_s": ({"task_weighting"}, "objective"),    # the + s_t term dropped from the uncertainty objective
    "focal_unmargined": ({"ce_shape"}, "vectors"),            # the focal factor from the probability BEFORE the margin
    "focal_weighted_pt": ({"ce_shape", "class_balance"}, "vectors"),  # class weights inside the focal factor's p_t: p_t = exp(-w_t nll)
    "pnr_swapped": ({"pnr_balance"}, "vectors"),              # PNR's pos / neg swapped
}


def mutant_applies(name, row) -> bool:
    need = (LOSS_MUTANTS.get(name) or UPDATE_MUTANTS[name])[0]
    if not all(on(row, f) for f in need):
        return False
    if name == "uncertainty_no_s":
        return row["task_weighting"] == "uncertainty"
    if name == "focal_weighted_pt":
        return row["class_balance"] == "weight"
    if name == "norm_without_log_var":
        return row["task_weighting"] == "uncertainty"
    return True


def task_scales(row, enabled, log_var=None):
    """The f32 scales the kernels read: 1 (none), the manual scales, or exp(-s) as egk_task_scale_prepare stores it."""
    if row["task_weighting"] == "none":
        return [1.0] * len(enabled)
    if row["task_weighting"] == "manual":
        return [TW.fl32(MANUAL[t]) for t in enabled]
    return [TW.prepared_scale(float(v)) for v in log_var]


def _shaped_mutant(x, y, w, a, m, gamma, gloss, mutant):
    """ce_shape_common.reference with ONE slip in where the focal factor's p_t comes from; float64 autograd."""
    import torch.nn.functional as F
    x = x.detach().double().cpu().clone().requires_grad_(True)
    N, C = x.shape
    y = y.detach().cpu().to(torch.int64)
    live = (y >= 0) & (y < C)
    yy = torch.where(live, y, torch.full_like(y, -1))
    t = yy.clamp(min=0)
    z0 = x if a is None else x + a.double()
    z = z0 if m is None else z0 - F.one_hot(t, C).double() * m.double()[t][:, None]
    Sv = F.cross_entropy(z, yy, weight=None if w is None else w.double(), ignore_index=-1, reduction="none")
    if mutant == "focal_unmargined":
        q = torch.softmax(z0, 1).gather(1, t[:, None])[:, 0]
    else:  # focal_weighted_pt
        q = torch.exp(-Sv)
    loss = Sv if gamma == 0 else (1 - q).clamp(min=0) ** gamma * Sv
    loss = torch.where(live, loss, torch.zeros_like(loss))
    (loss * gloss.double()).sum().backward()
    return loss.detach(), x.grad


def loss_model(row, logits, labels, weights, n_full, log_var=None, batch=None, mutant=None):
    """The loss half in float64.  ``logits``: {task: [one tensor per head] (AR, LTA) | one tensor}, on the rows the head ran on;
    ``labels``: {task: y} on the same rows; ``n_full``: {task: the nodes of the task's batch}; ``weights``: {task: w_t};
    ``log_var``: the f32 log-variances at the START of the step (uncertainty).  Returns dict(vectors, operands, seeds, scales,
    objective, ds): per task the loss vector and d J / d logits with the seed w_t * scale_t / N_t baked in."""
    enabled = [t for t in ORDER if t in logits]
    scales = task_scales(row, enabled, log_var)
    out = dict(vectors={}, operands={}, seeds={}, scales=dict(zip(enabled, scales)))
    for i, t in enumerate(enabled):
        seed = weights[t] * (1.0 if mutant == "scale_not_on_seed" else scales[i]) / n_full[t]
        out["seeds"][t] = seed
        y = labels[t].detach().cpu()
        if t in ("ar", "lta"):
            tm = terms(row, t)
            xs = [x.detach().float().cpu() for x in logits[t]]
            total, grads = torch.zeros(xs[0].shape[0], dtype=F64), []
            g = torch.full((xs[0].shape[0],), seed, dtype=F64)
            for h, x in enumerate(xs):
                if mutant in ("focal_unmargined", "focal_weighted_pt"):
                    loss, dz = _shaped_mutant(x, y[:, h], tm["w"][h], tm["a"][h], tm["m"][h], tm["gamma"], g, mutant)
                else:
                    loss, dz, _ = S.reference(x, y[:, h], tm["w"][h], tm["a"][h], tm["m"][h], 0.0, tm["gamma"], g)
                total += loss
                grads.append(dz)
            out["vectors"][t], out["operands"][t] = total, grads
        elif t == "pnr":
            pos, neg, gamma = pnr_triple(row, batch) or (1.0, 1.0, 0.0)
            if mutant == "pnr_swapped":
                pos, neg = neg, pos
            out["vectors"][t], out["operands"][t] = PB.model(logits[t].detach().float().cpu(), y, pos, neg, gamma, seed)
        else:  # OSCC: the plain cross entropy
            x = logits[t].detach().float().cpu()
            loss, _, dz = CB.model(x, y, gloss=torch.full((x.shape[0],), seed, dtype=F64))
            out["vectors"][t], out["operands"][t] = loss, dz
    out["objective"], out["ds"] = objective_model(row, out["vectors"], weights, n_full, log_var, mutant)
    return out


def objective_model(row, vectors, weights, n_full, log_var=None, mutant=None):
    """(J, d J / d log_var or None) through task_weighting_common.objective from the given loss vectors (the model's, or the
    step's own): J = sum_t w_t (scale_t L_t [+ s_t]), L_t = sum(loss_t) / N_t."""
    enabled = [t for t in ORDER if t in vectors]
    scales = task_scales(row, enabled, log_var)
    s = [float(v) for v in log_var] if row["task_weighting"] == "uncertainty" else None
    J, ds, _ = TW.objective([vectors[t].detach().double().cpu() for t in enabled], [weights[t] for t in enabled], scales, s,
                            [n_full[t] for t in enabled])
    if mutant == "uncertainty_no_s" and s is not None:
        J -= sum(weights[t] * s_ for t, s_ in zip(enabled, s))
    return J, ds


def loss_restate_f32(row, logits, labels, weights, n_full, log_var=None, batch=None):
    """The loss half restated in f32: ce_shape_common.restate_f32 per head (the kernel's arithmetic in numpy f32), the BCE formulas
    of pnr_balance_common in torch f32, the seeds as ONE f32 product fl32(fl32(w / N) * scale), the objective summed in f64 from
    the f32 vectors and rounded once."""
    enabled = [t for t in ORDER if t in logits]
    scales = task_scales(row, enabled, log_var)
    out = dict(vectors={}, operands={})
    for i, t in enumerate(enabled):
        seed = TW.scaled_seed(weights[t] / n_full[t], scales[i])
        y = labels[t]
        if t in ("ar", "lta"):
            tm = terms(row, t)
            g = torch.full((logits[t][0].shape[0],), seed, dtype=torch.float32)
            total, grads = None, []
            for h, x in enumerate(logits[t]):
                loss, dz = S.restate_f32(x, y[:, h], tm["w"][h], tm["a"][h], tm["m"][h], 0.0, tm["gamma"], g)
                total = loss if total is None else (total + loss).astype(np.float32)
                grads.append(torch.from_numpy(dz))
            out["vectors"][t], out["operands"][t] = torch.from_numpy(total), grads
        else:
            pos, neg, gamma = pnr_triple(row, batch) or (1.0, 1.0, 0.0)
            f = torch.float32
            z, tt = logits[t].to(f), (y != 0).to(f)
            c = torch.where(y != 0, torch.tensor(pos, dtype=f), torch.tensor(neg, dtype=f))
            sp = lambda v: v.clamp(min=0) + torch.log1p(torch.exp(-v.abs()))
            if gamma == 0:
                loss, dz = c * ((1 - tt) * z + sp(-z)), c * (torch.sigmoid(z) - tt) * f32(seed)
            else:
                sg = 2 * tt - 1
                u = sg * z
                ce, mod, pt = sp(-u), torch.exp(-f32(gamma) * sp(u)), torch.sigmoid(u)
                loss, dz = c * mod * ce, sg * c * mod * (f32(gamma) * pt * (-ce) - (1 - pt)) * f32(seed)
            out["vectors"][t], out["operands"][t] = loss, dz
    J, ds = objective_model(row, out["vectors"], weights, n_full, log_var)
    out["objective"], out["ds"] = TW.fl32(J), None if ds is None else [TW.fl32(v) for v in ds]
    return out


def f32(x):
    return torch.tensor(float(x), dtype=torch.float32)


# ---- the update half -------------------------------------------------------------------------------------------------------------
UPDATE_MUTANTS = {
    "norm_without_log_var": ({"grad_clip_norm", "task_weighting"}, "norm"),      # the norm taken without the log_var slot
    "clip_after_decay": ({"grad_clip_norm"}, "update"),                          # the coefficient on g + wd p instead of on g
    "lr_scale_on_decay": ({"param_groups"}, "update"),                           # lr_scale also scaling the weight decay
    "no_decay_ignored": ({"param_groups"}, "update"),                            # no_decay_1d ignored for the 1-D parameters
    "ema_before_update": ({"ema"}, "ema"),                                       # the average taken of the parameters before the update
    "ema_weight_prev": ({"ema"}, "ema"),                                         # the warm-up weight of step t - 1
}
MUTANTS = {**LOSS_MUTANTS, **UPDATE_MUTANTS}


def hyper_of(row):
    """The rule's scalars at the precision the launch receives them (f32 numbers; they are the rule's inputs, not its error:
    task_weighting_common.adam_first_step).  Adam forms 1 - beta in f32 from the f32 beta, AdamW takes it in double and rounds once
    (csrc/optim_rules.hip)."""
    fl = TW.fl32
    b1, b2 = 0.9, 0.999
    if row["rule"] == "adam":
        omb1, omb2 = float(np.float32(1) - np.float32(b1)), float(np.float32(1) - np.float32(b2))
    else:
        omb1, omb2 = fl(1.0 - b1), fl(1.0 - b2)
    return dict(b1=b1, b2=fl(b2), omb1=omb1, omb2=omb2, eps=fl(1e-8), mu=fl(MOMENTUM))


def uniform_groups(n, log_var=None):
    """The group table of a row without parameter groups over n elements (``log_var``: its (lo, hi) slot, a group of its own with
    weight decay 0 -- train.build_optimizer)."""
    g = dict(lr=torch.full((n,), TW.fl32(LR), dtype=F64), wd=torch.full((n,), TW.fl32(WD), dtype=F64), scale=torch.ones(n, dtype=F64),
             bare=torch.zeros(n, dtype=torch.bool), base_wd=TW.fl32(WD), log_var=log_var)
    if log_var is not None:
        g["wd"][log_var[0]:log_var[1]] = 0.0
    return g


def groups_of(opt, log_var_param=None):
    """Per element of the optimizer's flat buffers: lr and weight decay (the f32 rows the grouped launch reads), the group's lr
    scale, whether the group is a ``/no_decay`` one, and the slot of log_var."""
    n = opt.flat_p.numel()
    slot = None
    if log_var_param is not None:
        lo, ln = opt._slot_of[id(log_var_param)]
        slot = (lo, lo + ln)
    g = uniform_groups(n, None)
    g["log_var"] = slot
    segs = opt.group_segments() if opt.grouped else [(0, n, 0)]
    for b, e, gi in segs:
        G = opt.param_groups[gi]
        g["lr"][b:e], g["wd"][b:e] = TW.fl32(G["lr"]), TW.fl32(G["weight_decay"])
        g["scale"][b:e] = float(G["lr"]) / LR
        g["bare"][b:e] = str(G.get("name", "")).endswith("/no_decay")
    return g


def update_model(row, p, g, state, ema, t, groups, clip=0.0, grad_scale=1.0, mutant=None, dtype=F64):
    """One optimizer step in ``dtype`` (float64: the model; float32: its restatement) from a snapshot.  p, g: the f32 flat
    parameters and gradient; state: the rule's buffers as f32 (a bf16 state widened: the model computes on what is stored); ema:
    the f32 average or None; t: the counted step THIS update is (the device counter before it, plus one); groups: ``groups_of``.
    Order: norm over all slots -> coefficient -> the rule per group -> ema on the new parameters.  Returns dict(norm, coef, skipped,
    p, state (UNROUNDED), state_scale (the magnitude the state's rounding errors are relative to), ema, t)."""
    hy = hyper_of(row)
    c_ = lambda v: torch.as_tensor(v, dtype=dtype)
    p0, g0 = p.detach().cpu().to(dtype), g.detach().cpu().to(dtype)
    sq = g.detach().cpu().double() ** 2  # (the norm's partial sums are f64 in the kernel too)
    if mutant == "norm_without_log_var" and groups["log_var"] is not None:
        sq[groups["log_var"][0]:groups["log_var"][1]] = 0.0
    norm = grad_scale * math.sqrt(float(sq.sum()))
    clipping = on(row, "grad_clip_norm")
    if clipping and not math.isfinite(norm):
        return dict(norm=norm, coef=float("nan"), skipped=True, p=p0, state=[s.detach().cpu().to(dtype) for s in state], state_scale=None,
                    ema=ema, t=t - 1)
    coef = SC.clip_ref(norm, clip) if clipping else 1.0
    gs = TW.fl32(grad_scale * coef)  # (the grad_scale word of the step constants: one f32 number)
    lr, wd = groups["lr"].to(dtype), groups["wd"].clone().to(dtype)
    if mutant == "lr_scale_on_decay":
        wd = wd * groups["scale"].to(dtype)
    if mutant == "no_decay_ignored":
        bare = groups["bare"].clone()
        if groups["log_var"] is not None:
            bare[groups["log_var"][0]:groups["log_var"][1]] = False
        wd = torch.where(bare, c_(groups["base_wd"]), wd)
    late = mutant == "clip_after_decay"
    rule = row["rule"]
    st = [s.detach().cpu().to(dtype) for s in state]
    if rule == "adamw":
        pn = p0 * (1.0 - lr * wd * (TW.fl32(coef) if late else 1.0))
        gg = g0 * c_(gs)
        mag = gg.abs()
    else:
        gg = (g0 * c_(grad_scale) + wd * p0) * c_(TW.fl32(coef)) if late else g0 * c_(gs) + wd * p0
        pn = p0
        mag = (g0 * c_(gs)).abs() + (wd * p0).abs()  # (the terms of the sum, not the sum: it may cancel)
    if rule in ("adam", "adamw"):
        m = st[0] + (gg - st[0]) * c_(hy["omb1"])
        v = st[1] * c_(hy["b2"]) + c_(hy["omb2"]) * gg * gg
        bc1, bc2s = TW.fl32(1.0 - hy["b1"] ** t), TW.fl32(math.sqrt(1.0 - 0.999 ** t))
        pn = pn - (lr / c_(bc1)) * (m / (v.sqrt() / c_(bc2s) + c_(hy["eps"])))
        new, scale = [m, v], [st[0].abs() + mag, st[1].abs() + mag * mag]
    else:
        buf = gg if t == 1 else c_(hy["mu"]) * st[0] + gg
        pn = pn - lr * buf
        new, scale = [buf], [st[0].abs() + mag]
    ema_new = None
    if ema is not None:
        src = p0 if mutant == "ema_before_update" else pn
        w = E.ema_weight(EMA_DECAY, EMA_WARMUP, t - 1 if mutant == "ema_weight_prev" else t)
        ema_new = E.ema_model(ema.detach().cpu().float(), src.float(), w)
    return dict(norm=norm, coef=coef, skipped=False, p=pn, state=new, state_scale=scale, ema=ema_new, t=t)


# ---- a bf16 state: which stored values the model admits -----------------------------------------------------------------------------
STATE_ULPS = 2.0 ** -20  # 16 f32 ulps of the terms' magnitude: at most 6 separately rounded f32 operations lead to a stored
#                          moment (csrc/optim_rules.hip), each within 2^-24 of the largest term, the coefficient word one more


def bf16_bracket(x, slack):
    """(lo, hi) magnitudes, f32 tensors: the bf16 value at or below |x| - slack and the one at or above |x| + slack.  A launch stores
    one of the two bf16 neighbours of ITS f32 moment (tests/optim_state_common.py: (bits + r) >> 16 never moves further), and that
    moment is within ``slack`` of the model's."""
    x, slack = x.detach().double().abs(), slack.detach().double()
    a = (x - slack).clamp(min=0).to(torch.float32)
    b = (x + slack).to(torch.float32)
    a = torch.where(a.double() > (x - slack).clamp(min=0), torch.nextafter(a, torch.zeros_like(a)), a)   # (f64 -> f32 rounded up: step down)
    b = torch.where(b.double() < x + slack, torch.nextafter(b, torch.full_like(b, float("inf"))), b)
    lo = (a.view(torch.int32) & -65536).view(torch.float32)
    bb = b.view(torch.int32)
    hi = torch.where((bb & 0xFFFF) != 0, (bb & -65536) + 65536, bb).view(torch.float32)
    return lo, hi


def bf16_state_ok(stored, model, scale):
    """Per element: is the stored bf16 moment (widened) one the model admits?  Its magnitude lies in the bracket of the model's
    unrounded moment widened by STATE_ULPS x ``scale``, and its sign is the model's unless the model's value is inside that slack."""
    stored, model = stored.detach().cpu().float(), model.detach().cpu().double()
    slack = STATE_ULPS * scale.detach().cpu().double() + 1e-45
    lo, hi = bf16_bracket(model, slack)
    mag = stored.abs()
    sign_ok = (torch.sign(stored.double()) == torch.sign(model)) | (model.abs() <= slack) | (stored == 0)
    return (mag >= lo) & (mag <= hi) & sign_ok


# ---- synthetic inputs at the matrix's sizes, for the tests without a GPU -----------------------------------------------------------
FLAT_N = 1 << 14  # elements of the synthetic flat buffers: five segments of three groups and the log_var slot behind them


def synthetic_loss_inputs(row, seed=0):
    """Logits, labels, task weights and node counts of one step at the row's size: AR on its labelled rows (one per sequence),
    LTA and PNR on every node; a few ignored labels; log-variances away from 0."""
    _, batch = row["size"]
    g = torch.Generator().manual_seed(100 + seed + batch)
    n = batch * T_NODES
    logits, labels = {}, {}
    for t, rows_ in (("ar", batch), ("lta", n)):
        logits[t] = [3 * torch.randn(rows_, c, generator=g) for c in HEADS]
        y = torch.stack([torch.randint(0, c, (rows_,), generator=g) for c in HEADS], 1)
        if t == "lta":
            y[1::5, 0], y[2::7, 1] = -1, -1
        labels[t] = y
    logits["pnr"] = 3 * torch.randn(n, generator=g)
    y = torch.zeros(n, dtype=torch.int64)
    y[torch.arange(batch) * T_NODES + torch.randint(0, T_NODES, (batch,), generator=g)] = 1
    labels["pnr"] = y
    weights = {"ar": 1.0, "lta": 1.0, "pnr": 1.0}
    log_var = torch.tensor([0.4, -0.3, 0.2]) if row["task_weighting"] == "uncertainty" else None
    return dict(logits=logits, labels=labels, weights=weights, n_full={"ar": n, "lta": n, "pnr": n}, log_var=log_var, batch=batch)


def synthetic_update_inputs(row, ds=None, seed=0):
    """A snapshot in front of optimizer step t = 3: parameters, gradient, the rule's state, the average, the group table (the
    backbone at lr x 0.5, the heads at lr x 2, their 1-D parameters without decay, log_var in its own group) and a bound at half
    the gradient's norm.  ``ds``: d J / d log_var of the loss half, the gradient of the log_var slot."""
    g = torch.Generator().manual_seed(200 + seed)
    n = FLAT_N
    p, gr = 0.5 * torch.randn(n, generator=g), 1e-2 * torch.randn(n, generator=g)
    slot = None
    groups = uniform_groups(n)
    if on(row, "param_groups"):
        cuts = [0, 6000, 6400, 15000, 16000, n]
        for (b, e), (sc, bare) in zip(zip(cuts[:-1], cuts[1:]), [(0.5, False), (0.5, True), (2.0, False), (2.0, True), (2.0, False)]):
            groups["lr"][b:e], groups["scale"][b:e], groups["bare"][b:e] = TW.fl32(LR * sc), sc, bare
            if bare:
                groups["wd"][b:e] = 0.0
    if row["task_weighting"] == "uncertainty":
        slot = (n - 8, n)
        p[slot[0]:], gr[slot[0]:] = 0.0, 0.0
        p[slot[0]:slot[0] + 3] = torch.tensor([0.4, -0.3, 0.2])
        gr[slot[0]:slot[0] + 3] = torch.tensor(ds if ds is not None else [0.7, -0.9, 0.5], dtype=torch.float32)
        groups["lr"][slot[0]:], groups["wd"][slot[0]:], groups["scale"][slot[0]:], groups["bare"][slot[0]:] = TW.fl32(LR), 0.0, 1.0, False
        groups["log_var"] = slot
    n_state = 1 if row["rule"] == "sgd" else 2
    state = [1e-2 * torch.randn(n, generator=g), 1e-4 * torch.rand(n, generator=g)][:n_state]
    if on(row, "optimizer_state"):
        state = [s.to(BF).float() for s in state]
    ema = p + 0.05 * torch.randn(n, generator=g) if on(row, "ema") else None
    clip = 0.5 * float(gr.double().norm()) if on(row, "grad_clip_norm") else 0.0
    return dict(p=p, g=gr, state=state, ema=ema, t=3, groups=groups, clip=clip)
