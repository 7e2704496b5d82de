"""Shared pieces of the two entry points (main_temporal.py / main_egopack.py): config loading, dataset
and loader construction, checkpoints with the reference's key layout, schedulers, per-epoch loops."""
from __future__ import annotations

import logging
import math
import sys
from pathlib import Path
from typing import Dict, Optional

import torch

from . import data as D
from . import ops
from .config import Cfg, compose, instantiate
from .criterion import BCEWithLogitsNone, CrossEntropyNone, MetricSelectorWrapper
from .optim import STATE_DTYPES, STATE_ROUNDINGS, TASK_WEIGHTING_GROUP, TASK_WEIGHTING_MODES, FlatAdam, FlatAdamW, FlatLAMB, FlatSGD

logger = logging.getLogger("egopack")
TASKS = ("ar", "oscc", "lta", "pnr")
CKPT_KEYS = {"ar": "task/recognition", "oscc": "task/oscc", "lta": "task/lta", "pnr": "task/pnr"}
DSET_GROUP = {"ar": "dataset_recognition", "oscc": "dataset_oscc", "lta": "dataset_lta", "pnr": "dataset_pnr"}


def load_config(argv=None, config_dir: Optional[Path] = None) -> Cfg:
    """``python main_*.py key=value group/sub=name ...`` (Hydra override syntax)."""
    argv = sys.argv[1:] if argv is None else argv
    config_dir = config_dir or Path(__file__).resolve().parents[1] / "configs"
    return compose(config_dir, "defaults", [a for a in argv if "=" in a])


def cap_host_threads(n: int = 8) -> int:
    """The training process does no arithmetic on the host: what its intra-op thread pool runs is the memcpy of the
    step's feature block into the page-locked staging buffer.  With the default pool of one thread per core (128 on the
    MI355X host) that copy stalls for ~90 ms every few steps (per-step host time: median 83 ms, mean 60 ms); with 4-16
    threads it takes < 1 ms (3.0 ms per step for staging + replay bookkeeping, no stalls) -- tools/exp/loop_trace.py."""
    prev = torch.get_num_threads()
    if prev > n:
        torch.set_num_threads(n)
    return prev


def seed_everything(cfg, rank: int):
    if cfg.seed > 0:
        import numpy as np
        np.random.seed(cfg.seed)
        torch.manual_seed(cfg.seed)  # identical parameter init on every rank
        # dropout streams differ per rank; ``dropout_seed_offset`` (the noise-floor runs of the metric comparison) is mixed in with a
        # stride no rank count reaches, so offset k on rank r is not rank r + k's stream of the base run
        ops.manual_seed(cfg.seed * 7919 + rank + int(cfg.get("dropout_seed_offset", 0) or 0) * 1000003)


def task_weights(cfg) -> Dict[str, float]:
    return {t: float(cfg[f"weight_{t}"]) if t in cfg.enabled_tasks else 0.0 for t in TASKS}


def build_datasets(cfg, split: str):
    """One dataset per task with the reference's transforms: RadiusGraph(r=k+0.5) for AR / OSCC / PNR,
    LTATemporalConnectivity(r=k+0.5) for LTA (main_temporal.py:168-235)."""
    out = {}
    for t in TASKS:
        tf = D.LTATemporalConnectivity(r=cfg.k + 0.5, loop=False) if t == "lta" else D.RadiusGraph(r=cfg.k + 0.5, loop=False)
        dcfg = dict(cfg[DSET_GROUP[t]])
        if dcfg["_target_"].endswith(("SyntheticTaskDataset", "SyntheticResidentDataset", "LearnableSyntheticDataset")):
            n_val = int(cfg.get("synthetic_val_samples", 0)) or max(cfg.synthetic_samples // 4, 1)
            dcfg.update(length=cfg.synthetic_samples if split == "train" else n_val,
                        seed=cfg.seed + (0 if split == "train" else 10_000), k=cfg.k)
            if dcfg["_target_"].endswith("SyntheticResidentDataset"):
                dcfg["split"] = split
            out[t] = instantiate(dcfg, transform=tf)
        else:
            out[t] = instantiate(dcfg, split=split, transform=tf)
    return out


def build_feature_store(dsets, device):
    """ONE device-resident feature table for the tasks' datasets when they index one (datasets that expose ``videos``:
    uid -> [frames, F] and deliver ``x_idx``): the reference's four datasets read the same Omnivore file per video, so do
    these.  None for datasets that deliver features themselves."""
    from .feature_store import FeatureStore
    have = [ds for ds in dsets.values() if getattr(ds, "videos", None) is not None]
    if not have:
        return None
    if len(have) != len(dsets):
        raise ValueError("either every task dataset indexes the resident feature table or none does")
    ref = have[0].videos
    for ds in have[1:]:
        if ds.videos.keys() != ref.keys() or any(ds.videos[k].shape != ref[k].shape for k in ref):
            raise ValueError("the task datasets must index ONE feature table (same videos)")
    from . import ops
    # the table is stored in the activation type of the compute mode: f32 under compute=f32 (the reference-precision mode
    # must not round its inputs to bf16 before the first contraction), bf16 otherwise
    return FeatureStore(ref, device=device, dtype=ops.act_dtype())


def resident_batches(loader, store, device, dtype=None):
    """Evaluation-side adapter: the loader's batches on the device with their features gathered from the store."""
    from .feature_store import materialise_features
    for b in loader:
        yield materialise_features(b.to(device), store, dtype)


class ResidentLoader:
    """A loader of index-only batches (``x_idx``) seen as a loader of device batches with features: every batch is moved to
    the device and its rows are gathered from the resident table (evaluation passes, the prototype-bank pass)."""

    def __init__(self, loader, store, device, dtype=None):
        self.loader, self.store, self.device, self.dtype = loader, store, device, dtype

    def __iter__(self):
        return resident_batches(self.loader, self.store, self.device, self.dtype)

    def __len__(self):
        return len(self.loader)


def build_loaders(cfg, dsets, train: bool, rank: int, world: int, batch_size: Optional[int] = None):
    """Training loaders shard by sample (equal steps per rank); evaluation loaders shard by batch, so that every batch
    -- and with it every graph-LayerNorm statistic -- is the one the single-process pass sees."""
    bs = batch_size or cfg.batch_size
    out = {t: D.build_dataloader(ds, bs, train, cfg.num_workers, train, seed=cfg.seed, rank=rank, world_size=world,
                                 shard="samples" if train else "batches",
                                 workers=int(cfg.get("loader_workers", 0)) if train else 0)
           for t, ds in dsets.items()}
    mx = mixup_config(cfg)
    if train and mx["alpha"] > 0:  # (validation batches carry none of the fields)
        for t in mx["tasks"]:
            if t in out:
                out[t].mixup = dict(task=t, alpha=mx["alpha"], per_sequence=mx["per_sequence"], prob=mx["prob"],
                                    seed=int(cfg.seed if mx["seed"] is None else mx["seed"]))
    return out


# ---- sequence mixup of the AR / LTA heads (``mixup:`` of the config; include/egopack_mixup.h) ---------------------------
MIXUP_DEFAULTS = {"alpha": 0.0, "tasks": ["ar", "lta"], "per_sequence": True, "prob": 1.0, "seed": None}


def mixup_config(cfg) -> dict:
    """The ``mixup:`` block with its defaults filled in.  A ValueError names the key: an unknown key, alpha < 0 or not finite, prob
    outside [0, 1], a task outside [ar, lta]."""
    raw = cfg.get("mixup") if hasattr(cfg, "get") else None
    raw = dict(raw or {})
    unknown = set(raw) - set(MIXUP_DEFAULTS)
    if unknown:
        raise ValueError(f"mixup: unknown key(s) {sorted(unknown)} ({', '.join(MIXUP_DEFAULTS)})")
    mx = {**MIXUP_DEFAULTS, **raw}
    mx["alpha"], mx["prob"] = float(mx["alpha"]), float(mx["prob"])
    if not (mx["alpha"] >= 0.0 and mx["alpha"] < float("inf")):
        raise ValueError(f"mixup.alpha: {mx['alpha']} is not a finite value >= 0")
    if not (0.0 <= mx["prob"] <= 1.0):
        raise ValueError(f"mixup.prob: {mx['prob']} is outside [0, 1]")
    mx["tasks"] = [str(t) for t in (mx["tasks"] or [])]
    bad = [t for t in mx["tasks"] if t not in D.MIX_TASKS]
    if bad:
        raise ValueError(f"mixup.tasks: {bad} outside {list(D.MIX_TASKS)}")
    mx["per_sequence"] = bool(mx["per_sequence"])
    mx["seed"] = None if mx["seed"] is None else int(mx["seed"])
    return mx


def check_mixup(cfg, enable_graphone: bool = False, entry: str = "main_temporal.py") -> dict:
    """The ``mixup:`` block checked against the rest of the configuration at build time; returns it.  With alpha > 0 refused, each
    ValueError naming both keys: a mixed task with class_balance.mode != none or with ce_shape margins / gamma (the weighted and shaped
    two-target losses do not exist), and the EgoPack step (enable_graphone / main_egopack.py: MTLStep only, like task weighting)."""
    mx = mixup_config(cfg)
    if mx["alpha"] <= 0 or not mx["tasks"]:
        return mx
    if enable_graphone:
        raise ValueError(f"mixup.alpha = {mx['alpha']} with enable_graphone=True ({entry}): the EgoPack step trains one primary task "
                         "through GraphONE and has no mixed input -- mixup is for main_temporal.py (MTLStep)")
    cb = class_balance_config(cfg)
    if cb["mode"] != "none":
        both = [t for t in mx["tasks"] if t in cb["tasks"]]
        if both:
            raise ValueError(f"mixup.tasks {both} with class_balance.mode = {cb['mode']}: there is no class-balanced two-target cross "
                             "entropy -- take the task out of mixup.tasks or of class_balance.tasks")
    sh = ce_shape_config(cfg)
    if sh["margin"] != "none" or sh["gamma"] > 0:
        both = [t for t in mx["tasks"] if t in sh["tasks"]]
        if both:
            raise ValueError(f"mixup.tasks {both} with ce_shape.margin = {sh['margin']} / ce_shape.gamma = {sh['gamma']}: there is no "
                             "shaped two-target cross entropy -- take the task out of mixup.tasks or of ce_shape.tasks")
    return mx


def log_mixup(logger, epoch: int, loaders) -> None:
    """The mean lambda per mixed task over the batches of the epoch; nothing with the feature off."""
    means = {t: l.mix_lam_mean() for t, l in loaders.items() if getattr(l, "mixup", None)}
    means = {t: round(m, 4) for t, m in means.items() if m is not None}
    if means:
        logger.info("epoch %d: mixup mean lambda %s", epoch, means)


# ---- DropEdge of the backbone's SAGE means (``edge_drop:`` of the config) ------------------------------------------
EDGE_DROP_DEFAULTS = {"p": 0.0, "symmetric": True, "keep_self": True, "per_layer": True}


def edge_drop_config(cfg) -> dict:
    """The ``edge_drop:`` block with its defaults filled in.  A ValueError names the key: an unknown key, p outside [0, 1) or NaN."""
    raw = cfg.get("edge_drop") if hasattr(cfg, "get") else None
    raw = dict(raw or {})
    unknown = set(raw) - set(EDGE_DROP_DEFAULTS)
    if unknown:
        raise ValueError(f"edge_drop: unknown key(s) {sorted(unknown)} ({', '.join(EDGE_DROP_DEFAULTS)})")
    ed = {**EDGE_DROP_DEFAULTS, **raw}
    ed["p"] = float(ed["p"])
    if not (0.0 <= ed["p"] < 1.0):
        raise ValueError(f"edge_drop.p: {ed['p']} is outside [0, 1)")
    for k in ("symmetric", "keep_self", "per_layer"):
        ed[k] = bool(ed[k])
    return ed


def check_edge_drop(cfg, enable_graphone: bool = False, entry: str = "main_temporal.py") -> dict:
    """The ``edge_drop:`` block checked against the rest of the configuration at build time; returns it.  With p > 0 the EgoPack step
    is refused (enable_graphone / main_egopack.py): the dual-replay tape of its SAGE layers knows nothing of dropped edges -- MTLStep
    only, like mixup and task weighting."""
    ed = edge_drop_config(cfg)
    if ed["p"] > 0 and enable_graphone:
        raise ValueError(f"edge_drop.p = {ed['p']} with enable_graphone=True ({entry}): the EgoPack step replays its SAGE layers from a "
                         "tape that knows nothing of dropped edges -- edge_drop is for main_temporal.py (MTLStep)")
    return ed


def apply_edge_drop(model, ed: dict) -> None:
    """Set ``model.edge_drop`` / ``model.edge_drop_per_layer`` (models.graph.Graph) from a checked ``edge_drop:`` block; p == 0 leaves
    the attribute None -- every launch is the one of before."""
    from . import ops
    model.edge_drop = ops.EdgeDrop(ed["p"], ed["symmetric"], ed["keep_self"]) if ed["p"] > 0 else None
    model.edge_drop_per_layer = ed["per_layer"]


def log_edge_drop(logger, epoch: int, model) -> None:
    """One line with the configured p and flags; nothing with the feature off.  (No device statistic: the masks are never stored.)"""
    ed = getattr(model, "edge_drop", None)
    if ed:
        logger.info("epoch %d: edge_drop p %s symmetric %s keep_self %s per_layer %s", epoch, ed.p, ed.symmetric, ed.keep_self,
                    bool(getattr(model, "edge_drop_per_layer", True)))


def env_ranks() -> tuple:
    """(rank, local_rank, world) of the launcher environment, without initialising anything."""
    import os
    return int(os.environ.get("RANK", "0")), int(os.environ.get("LOCAL_RANK", "0")), int(os.environ.get("WORLD_SIZE", "1"))


def start_loader_workers(loaders) -> None:
    """Create the collation processes of every loader that asks for some (``loader_workers`` > 0).  The entry points call
    this BEFORE anything touches the GPU: the pool is then a plain fork of a process without HIP state (no runtime locks,
    threads or pinned mappings inherited, the dataset shared copy-on-write instead of pickled to every worker)."""
    for dl in loaders.values():
        if getattr(dl, "workers", 0) > 0:
            dl.start_workers()


def build_criteria(dsets, class_balance=None, pnr_balance=None, ce_shape=None):
    """``class_balance``: what ``build_class_balance`` returns -- the AR / LTA wrappers then carry its per-class vectors.
    ``pnr_balance``: what ``build_pnr_balance`` returns -- the PNR criterion then carries its pos / neg / gamma.
    ``ce_shape``: what ``build_ce_shape`` returns -- the AR / LTA wrappers then carry its margins and focal exponent."""
    cb, sh = class_balance or {}, ce_shape or {}
    kw = {t: dict(class_weights=cb[t]["weights"], class_offsets=cb[t]["offsets"]) if t in cb else {} for t in ("ar", "lta")}
    for t in ("ar", "lta"):
        if t in sh:
            kw[t].update(class_margins=sh[t]["margins"], focal_gamma=sh[t]["gamma"])
    pb = {k: pnr_balance[k] for k in ("pos", "neg", "gamma")} if pnr_balance else {}
    return {"ar": MetricSelectorWrapper(CrossEntropyNone(), dsets["ar"], **kw["ar"]),
            "lta": MetricSelectorWrapper(CrossEntropyNone(), dsets["lta"], **kw["lta"]),
            "oscc": CrossEntropyNone(), "pnr": BCEWithLogitsNone(**pb)}


# ---- class-balanced cross entropy of the AR / LTA heads (``class_balance:`` of the config) ---------------------------------------
# OSCC (two balanced classes) is not part of it; PNR (a BCE) has its own block, ``pnr_balance:`` (below).
CLASS_BALANCE_MODES = ("none", "weight", "logit_adjust")
CLASS_BALANCE_SCHEMES = ("effective_number", "inverse_frequency")
CLASS_BALANCE_TASKS = ("ar", "lta")
CLASS_BALANCE_DEFAULTS = {"mode": "none", "scheme": "effective_number", "beta": 0.999, "power": 1.0, "tau": 1.0, "normalize": True,
                          "tasks": ["ar", "lta"]}


def class_balance_config(cfg) -> dict:
    """The ``class_balance:`` block with its defaults filled in; an unknown key, mode, scheme or task is a ValueError naming it."""
    raw = cfg.get("class_balance") if hasattr(cfg, "get") else None
    raw = dict(raw or {})
    unknown = set(raw) - set(CLASS_BALANCE_DEFAULTS)
    if unknown:
        raise ValueError(f"class_balance: unknown key(s) {sorted(unknown)} ({', '.join(CLASS_BALANCE_DEFAULTS)})")
    cb = {**CLASS_BALANCE_DEFAULTS, **raw}
    cb["mode"], cb["scheme"] = str(cb["mode"]).lower(), str(cb["scheme"]).lower()
    if cb["mode"] not in CLASS_BALANCE_MODES:
        raise ValueError(f"class_balance.mode: unknown mode '{cb['mode']}' ({' | '.join(CLASS_BALANCE_MODES)})")
    if cb["scheme"] not in CLASS_BALANCE_SCHEMES:
        raise ValueError(f"class_balance.scheme: unknown scheme '{cb['scheme']}' ({' | '.join(CLASS_BALANCE_SCHEMES)})")
    cb["tasks"] = [str(t) for t in (cb["tasks"] or [])]
    unknown = set(cb["tasks"]) - set(CLASS_BALANCE_TASKS)
    if unknown:
        raise ValueError(f"class_balance.tasks: unknown task(s) {sorted(unknown)} ({', '.join(CLASS_BALANCE_TASKS)})")
    cb["beta"], cb["power"], cb["tau"], cb["normalize"] = float(cb["beta"]), float(cb["power"]), float(cb["tau"]), bool(cb["normalize"])
    if not 0.0 <= cb["beta"] < 1.0:
        raise ValueError(f"class_balance.beta: {cb['beta']} is outside [0, 1)")
    return cb


def label_counts(dataset) -> list:
    """Per head the number of labels >= 0 of every class over all nodes of all samples of ``dataset`` (int64, length C).  The
    WHOLE split, not a rank's shard: every rank computes the same vectors without a collective.  A dataset that holds its label
    table (the resident datasets' ``_tables()['y']``) is counted from it; otherwise one pass over the samples.
    That pass reads ``dataset[i]``, features included: it costs one read of the split at start-up, and on a dataset whose
    ``__getitem__`` is stateful (one that draws from a random stream per call) it advances that state once per sample before
    training starts, so a run with ``class_balance`` on and one with it off then see different samples.  The datasets of this
    project are pure functions of the index or hold a label table; a dataset that is neither should offer ``_tables``."""
    Cs = tuple(dataset.num_class_labels)
    if hasattr(dataset, "_tables"):
        y = torch.as_tensor(dataset._tables()["y"])
        ys = [y.reshape(-1, y.shape[-1]) if y.dim() >= 2 else y.reshape(-1, 1)]
    else:
        # (``dataset[i]``, the sample the loaders deliver: the synthetic datasets draw their labels behind their features from one
        #  random stream, so ``__getitem__(i, with_x=False)`` is another sample's labels there -- it is the resident datasets'
        #  label source only, and those are counted from their table above)
        ys = []
        for i in range(len(dataset)):
            y = torch.as_tensor(dataset[i].y)
            ys.append(y.reshape(-1, y.shape[-1]) if y.dim() >= 2 else y.reshape(-1, 1))
    y = torch.cat(ys).to(torch.int64) if ys else torch.zeros((0, len(Cs)), dtype=torch.int64)
    if y.shape[1] < len(Cs):
        raise ValueError(f"class_balance: the dataset's labels have {y.shape[1]} columns, its heads are {Cs}")
    counts = []
    for h, Cn in enumerate(Cs):
        col = y[:, h]
        col = col[(col >= 0) & (col < Cn)]
        counts.append(torch.bincount(col, minlength=Cn).to(torch.int64))
    return counts


def class_weights(counts, scheme: str = "effective_number", beta: float = 0.999, power: float = 1.0,
                  normalize: bool = True) -> torch.Tensor:
    """Per-class weights from label counts, float64.  With n' = max(n, 1) (a class without a label weighs what a class with one
    does): effective_number (Cui et al. 2019) w = (1 - beta) / (1 - beta ** n'); inverse_frequency w = n' ** -power.
    ``normalize``: w *= sum(n) / sum(n * w) -- the mean weight over the training labels is 1, so the objective keeps its scale
    and the task weights keep their meaning."""
    n = torch.as_tensor(counts).to(torch.float64)
    n1 = n.clamp(min=1.0)
    if scheme == "effective_number":
        w = (1.0 - beta) / (1.0 - torch.pow(torch.tensor(beta, dtype=torch.float64), n1)) if beta > 0 else torch.ones_like(n1)
    elif scheme == "inverse_frequency":
        w = torch.pow(n1, -power)
    else:
        raise ValueError(f"class_balance.scheme: unknown scheme '{scheme}' ({' | '.join(CLASS_BALANCE_SCHEMES)})")
    if normalize and float((n * w).sum()) > 0:
        w = w * (n.sum() / (n * w).sum())
    return w


def logit_offsets(counts, tau: float = 1.0) -> torch.Tensor:
    """Logit adjustment (Menon et al. 2021), float64: a_c = tau * log(n'_c / sum(n')), n' = max(n, 1)."""
    n1 = torch.as_tensor(counts).to(torch.float64).clamp(min=1.0)
    return tau * torch.log(n1 / n1.sum())


def build_class_balance(cfg, dsets_train, device=None, tasks=None) -> dict:
    """{task: {"weights": [f32 vector per head] | None, "offsets": [...] | None, "counts": [int64 vector per head]}} for the tasks
    of ``class_balance.tasks`` -- {} with ``mode: none`` (nothing is counted, nothing is built: the criteria and the launches are
    the ones without the feature).  ``tasks``: the tasks the caller trains (None: all) -- the labels of the others are not
    counted.  Formulas in float64, rounded once to f32."""
    cb = class_balance_config(cfg)
    if cb["mode"] == "none":
        return {}
    out = {}
    for t in CLASS_BALANCE_TASKS:
        if t not in cb["tasks"] or t not in dsets_train or (tasks is not None and t not in tasks):
            continue
        counts = label_counts(dsets_train[t])
        if cb["mode"] == "weight":
            vecs = [class_weights(c, cb["scheme"], cb["beta"], cb["power"], cb["normalize"]) for c in counts]
        else:
            vecs = [logit_offsets(c, cb["tau"]) for c in counts]
        vecs = [v.to(torch.float32) if device is None else v.to(torch.float32).to(device) for v in vecs]
        out[t] = {"weights": vecs if cb["mode"] == "weight" else None, "offsets": vecs if cb["mode"] == "logit_adjust" else None,
                  "counts": counts}
    return out


def log_class_balance(logger, cfg, class_balance) -> None:
    """One line per head: mode, smallest and largest weight or offset, classes without a label."""
    if not class_balance:
        return
    cb = class_balance_config(cfg)
    for t, entry in class_balance.items():
        vecs = entry["weights"] if entry["weights"] is not None else entry["offsets"]
        what = "weight" if entry["weights"] is not None else "offset"
        for h, (v, n) in enumerate(zip(vecs, entry["counts"])):
            logger.info("class balance %s head %d (%d classes): mode %s, %s in [%.6g, %.6g], %d zero-count classes, %d labels",
                        t, h, v.numel(), cb["mode"] + ("/" + cb["scheme"] if cb["mode"] == "weight" else ""), what,
                        float(v.min()), float(v.max()), int((n == 0).sum()), int(n.sum()))


def class_balance_state(cfg, class_balance) -> Optional[dict]:
    """The checkpoint's top-level ``"class_balance"`` entry: the config block and the vectors (host tensors); None when off."""
    if not class_balance:
        return None
    host = lambda vs: None if vs is None else [v.detach().cpu().clone() for v in vs]
    return {"config": class_balance_config(cfg),
            "vectors": {t: {"weights": host(e["weights"]), "offsets": host(e["offsets"])} for t, e in class_balance.items()}}


def check_class_balance(logger, ckpt: dict, cfg, class_balance) -> bool:
    """On resume: the vectors rebuilt from the config and the training split against the ones the checkpoint stores, bit for bit.
    A difference (or one side without vectors) is ONE warning line; returns whether they agree."""
    stored, now = ckpt.get("class_balance"), class_balance_state(cfg, class_balance)
    same = (stored is None) == (now is None)
    if same and now is not None:
        a, b = stored.get("vectors", {}), now["vectors"]
        same = a.keys() == b.keys()
        for t in (a if same else ()):
            for kind in ("weights", "offsets"):
                va, vb = a[t].get(kind), b[t].get(kind)
                if (va is None) != (vb is None) or (va is not None and (len(va) != len(vb) or any(
                        x.shape != y_.shape or not torch.equal(x.cpu().view(torch.int32), y_.view(torch.int32)) for x, y_ in zip(va, vb)))):
                    same = False
    if not same:
        logger.warning("class balance: the vectors built for this run differ from the checkpoint's (config %s, stored %s): "
                       "the run continues with the ones built now", class_balance_config(cfg),
                       None if stored is None else stored.get("config"))
    return same


# ---- shaped cross entropy of the AR / LTA heads (``ce_shape:`` of the config): LDAM margin, focal term, deferred re-weighting -------
# The terms ride in the tail of the fused launch's task argument (egk_ce_task, include/egopack_hip.h) next to the vectors of
# ``class_balance``.  Training loss only, like them.
CE_SHAPE_MARGINS = ("none", "ldam")
CE_SHAPE_DEFAULTS = {"margin": "none", "max_margin": 0.5, "power": 0.25, "gamma": 0.0, "tasks": ["ar", "lta"], "reweight_after": 0}


def ce_shape_config(cfg) -> dict:
    """The ``ce_shape:`` block with its defaults filled in; an unknown key, margin mode or task is a ValueError naming it."""
    raw = cfg.get("ce_shape") if hasattr(cfg, "get") else None
    raw = dict(raw or {})
    unknown = set(raw) - set(CE_SHAPE_DEFAULTS)
    if unknown:
        raise ValueError(f"ce_shape: unknown key(s) {sorted(unknown)} ({', '.join(CE_SHAPE_DEFAULTS)})")
    sh = {**CE_SHAPE_DEFAULTS, **raw}
    sh["margin"] = str(sh["margin"]).lower()
    if sh["margin"] not in CE_SHAPE_MARGINS:
        raise ValueError(f"ce_shape.margin: unknown mode '{sh['margin']}' ({' | '.join(CE_SHAPE_MARGINS)})")
    sh["tasks"] = [str(t) for t in (sh["tasks"] or [])]
    unknown = set(sh["tasks"]) - set(CLASS_BALANCE_TASKS)
    if unknown:
        raise ValueError(f"ce_shape.tasks: unknown task(s) {sorted(unknown)} ({', '.join(CLASS_BALANCE_TASKS)})")
    sh["max_margin"], sh["power"], sh["gamma"] = float(sh["max_margin"]), float(sh["power"]), float(sh["gamma"])
    for k in ("max_margin", "power", "gamma"):
        if not (math.isfinite(sh[k]) and sh[k] >= 0.0):
            raise ValueError(f"ce_shape.{k}: {sh[k]} is not a finite value >= 0")
    if isinstance(sh["reweight_after"], bool) or int(sh["reweight_after"]) != sh["reweight_after"] or int(sh["reweight_after"]) < 0:
        raise ValueError(f"ce_shape.reweight_after: {sh['reweight_after']} is not an epoch number >= 0")
    sh["reweight_after"] = int(sh["reweight_after"])
    return sh


def ldam_margins(counts, max_margin: float = 0.5, power: float = 0.25) -> torch.Tensor:
    """Label-distribution-aware margins (Cao et al. 2019) from label counts, float64: m_c = max_margin * n'_c^-power /
    max_c(n'_c^-power), n' = max(n, 1) -- the class with the fewest labels (a class without one counts as one) gets max_margin."""
    n1 = torch.as_tensor(counts).to(torch.float64).clamp(min=1.0)
    r = torch.pow(n1, -power)
    return max_margin * (r / r.max())


def build_ce_shape(cfg, dsets_train, device=None, tasks=None, class_balance=None) -> dict:
    """{task: {"margins": [f32 vector per head] | None, "gamma": float, "counts": [...] | None}} for the tasks of
    ``ce_shape.tasks`` -- {} when the block asks for nothing (no margin, gamma 0: nothing is counted, the criteria and the launches
    are the ones without the feature).  The labels of the WHOLE training split are counted as ``class_balance`` counts them
    (``label_counts``; its counts are reused when it has them).  ``reweight_after`` > 0 needs ``class_balance.mode=weight``."""
    sh = ce_shape_config(cfg)
    if sh["reweight_after"] > 0 and class_balance_config(cfg)["mode"] != "weight":
        raise ValueError("ce_shape.reweight_after defers the class weights: it needs class_balance.mode=weight")
    if sh["margin"] == "none" and sh["gamma"] == 0.0:
        return {}
    out = {}
    for t in CLASS_BALANCE_TASKS:
        if t not in sh["tasks"] or t not in dsets_train or (tasks is not None and t not in tasks):
            continue
        margins = counts = None
        if sh["margin"] == "ldam":
            counts = class_balance[t]["counts"] if class_balance and t in class_balance else label_counts(dsets_train[t])
            margins = [ldam_margins(c, sh["max_margin"], sh["power"]).to(torch.float32) for c in counts]
            margins = margins if device is None else [m.to(device) for m in margins]
        out[t] = {"margins": margins, "gamma": sh["gamma"], "counts": counts}
    return out


def log_ce_shape(logger, cfg, ce_shape) -> None:
    """The mode, once: one line per task (margin range per head, focal exponent, the epoch the class weights start at)."""
    sh = ce_shape_config(cfg)
    if sh["reweight_after"] > 0:
        logger.info("ce shape: deferred re-weighting -- the class weights are all ones before epoch %d", sh["reweight_after"])
    for t, e in (ce_shape or {}).items():
        rng = "none" if e["margins"] is None else ", ".join(f"head {h} in [{float(m.min()):.6g}, {float(m.max()):.6g}]"
                                                              for h, m in enumerate(e["margins"]))
        logger.info("ce shape %s: margin %s (%s), focal gamma %.6g", t, sh["margin"], rng, e["gamma"])


def reweight_side(cfg, epoch: int) -> str:
    """Deferred re-weighting: which class weights epoch ``epoch`` (1-based, as the epoch loops and the checkpoints count) trains
    with -- "ones" before ``ce_shape.reweight_after``, "weights" from it on (and always with ``reweight_after: 0``)."""
    return "ones" if int(epoch) < ce_shape_config(cfg)["reweight_after"] else "weights"


def apply_reweight(logger, cfg, class_balance, holders, epoch: int) -> Optional[str]:
    """At an epoch boundary: rewrite the class-weight buffers of ``holders`` (task -> the wrapper or task module that carries
    ``class_weight_<h>``) IN PLACE to the side of ``reweight_side`` -- the pointers a captured step holds stand, no new capture.
    The vectors of ``class_balance`` themselves (what a checkpoint stores) stay the full weights.  None with the feature off."""
    if ce_shape_config(cfg)["reweight_after"] <= 0 or not class_balance:
        return None
    side = reweight_side(cfg, epoch)
    for t, e in class_balance.items():
        if e.get("weights") is None or t not in holders:
            continue
        for h, w in enumerate(e["weights"]):
            buf = getattr(holders[t], f"class_weight_{h}", None)
            if buf is not None:
                with torch.no_grad():
                    buf.copy_(torch.ones_like(w) if side == "ones" else w)
    if epoch == ce_shape_config(cfg)["reweight_after"]:  # (the switch, once; ``log_ce_shape`` announced it at start-up)
        logger.info("ce shape: from epoch %d on the class weights apply", epoch)
    return side


# ---- positive-class weighting / focal loss of the PNR head (``pnr_balance:`` of the config) ---------------------------------------
# One positive node per sequence of T candidates: three scalars (pos, neg, gamma) shape the BCE inside the kernels of the step
# (include/egopack_bce_balanced.h).  Training loss only, like ``class_balance``.
PNR_BALANCE_MODES = ("none", "pos_weight", "focal")
PNR_BALANCE_DEFAULTS = {"mode": "none", "pos_weight": "auto", "power": 1.0, "normalize": True, "alpha": 0.25, "gamma": 2.0}


def pnr_balance_config(cfg) -> dict:
    """The ``pnr_balance:`` block with its defaults filled in; an unknown key or mode is a ValueError naming it."""
    raw = cfg.get("pnr_balance") if hasattr(cfg, "get") else None
    raw = dict(raw or {})
    unknown = set(raw) - set(PNR_BALANCE_DEFAULTS)
    if unknown:
        raise ValueError(f"pnr_balance: unknown key(s) {sorted(unknown)} ({', '.join(PNR_BALANCE_DEFAULTS)})")
    pb = {**PNR_BALANCE_DEFAULTS, **raw}
    pb["mode"] = str(pb["mode"]).lower()
    if pb["mode"] not in PNR_BALANCE_MODES:
        raise ValueError(f"pnr_balance.mode: unknown mode '{pb['mode']}' ({' | '.join(PNR_BALANCE_MODES)})")
    if isinstance(pb["pos_weight"], str):
        if pb["pos_weight"].lower() != "auto":
            raise ValueError(f"pnr_balance.pos_weight: '{pb['pos_weight']}' is neither 'auto' nor a number > 0")
        pb["pos_weight"] = "auto"
    else:
        pb["pos_weight"] = float(pb["pos_weight"])
        if not (pb["pos_weight"] > 0.0 and pb["pos_weight"] < float("inf")):
            raise ValueError(f"pnr_balance.pos_weight: {pb['pos_weight']} is neither 'auto' nor a number > 0")
    pb["power"], pb["normalize"], pb["alpha"], pb["gamma"] = float(pb["power"]), bool(pb["normalize"]), float(pb["alpha"]), float(pb["gamma"])
    if not pb["alpha"] <= 1.0:
        raise ValueError(f"pnr_balance.alpha: {pb['alpha']} is above 1 (pos = alpha, neg = 1 - alpha; < 0: both 1)")
    if not (0.0 <= pb["gamma"] < float("inf")):
        raise ValueError(f"pnr_balance.gamma: {pb['gamma']} is not a finite number >= 0")
    return pb


def pnr_label_counts(dataset) -> tuple:
    """(n_pos, n_neg): the nodes labelled != 0 / == 0 over all samples of ``dataset``, the WHOLE split on every rank.  From the
    label table of a dataset that holds one (``_tables()['y']``), one pass over ``dataset[i].y`` otherwise: the caveats of
    ``label_counts`` apply."""
    if hasattr(dataset, "_tables"):
        y = torch.as_tensor(dataset._tables()["y"]).reshape(-1)
    else:
        ys = [torch.as_tensor(dataset[i].y).reshape(-1) for i in range(len(dataset))]
        y = torch.cat(ys) if ys else torch.zeros(0, dtype=torch.int64)
    n_pos = int((y != 0).sum())
    return n_pos, int(y.numel()) - n_pos


def pnr_scalars(pb: dict, n_pos: int, n_neg: int) -> tuple:
    """(pos, neg, gamma) of a validated ``pnr_balance`` block and the counts: float64 arithmetic, each rounded once to f32
    (returned as the Python float of that f32).  pos_weight: pw = (n_neg / max(n_pos, 1)) ** power (``auto``) or the number given;
    ``normalize``: pos = pw k, neg = k with k = N / (pw n_pos + n_neg) -- the mean factor over the training labels is 1, so the
    objective keeps its scale.  focal: pos = alpha, neg = 1 - alpha (alpha < 0: both 1), gamma as given."""
    if pb["mode"] == "pos_weight":
        pw = (n_neg / max(n_pos, 1)) ** pb["power"] if pb["pos_weight"] == "auto" else float(pb["pos_weight"])
        den = pw * n_pos + n_neg
        k = (n_pos + n_neg) / den if (pb["normalize"] and den > 0) else 1.0
        out = (pw * k, k, 0.0)
    elif pb["mode"] == "focal":
        out = (1.0, 1.0, pb["gamma"]) if pb["alpha"] < 0 else (pb["alpha"], 1.0 - pb["alpha"], pb["gamma"])
    else:
        raise ValueError(f"pnr_balance.mode: no scalars for mode '{pb['mode']}'")
    return tuple(float(torch.tensor(v, dtype=torch.float64).to(torch.float32)) for v in out)


def build_pnr_balance(cfg, dsets_train, tasks=None) -> Optional[dict]:
    """{"pos", "neg", "gamma": Python floats holding f32 values, "n_pos", "n_neg": the counts of the training split} -- None with
    ``mode: none`` (nothing is counted, nothing is built: the criterion and the launches are the ones without the feature) and
    when PNR is not among ``tasks`` (the tasks the caller trains; None: all)."""
    pb = pnr_balance_config(cfg)
    if pb["mode"] == "none" or (tasks is not None and "pnr" not in tasks) or "pnr" not in dsets_train:
        return None
    n_pos, n_neg = pnr_label_counts(dsets_train["pnr"])
    pos, neg, gamma = pnr_scalars(pb, n_pos, n_neg)
    return {"pos": pos, "neg": neg, "gamma": gamma, "n_pos": n_pos, "n_neg": n_neg}


def log_pnr_balance(logger, cfg, pnr_balance) -> None:
    """One line: mode, the counts, pos, neg, gamma."""
    if pnr_balance:
        logger.info("pnr balance: mode %s, %d positive / %d negative nodes, pos %.9g, neg %.9g, gamma %.9g", pnr_balance_config(cfg)["mode"],
                    pnr_balance["n_pos"], pnr_balance["n_neg"], pnr_balance["pos"], pnr_balance["neg"], pnr_balance["gamma"])


def pnr_balance_state(cfg, pnr_balance) -> Optional[dict]:
    """The checkpoint's top-level ``"pnr_balance"`` entry: the config block, the counts and the scalars (an f32 tensor
    [pos, neg, gamma]); None when off."""
    if not pnr_balance:
        return None
    return {"config": pnr_balance_config(cfg), "counts": {"n_pos": pnr_balance["n_pos"], "n_neg": pnr_balance["n_neg"]},
            "scalars": torch.tensor([pnr_balance[k] for k in ("pos", "neg", "gamma")], dtype=torch.float32)}


def check_pnr_balance(logger, ckpt: dict, cfg, pnr_balance) -> bool:
    """On resume: the scalars rebuilt from the config and the training split against the ones the checkpoint stores, bit for bit.
    A difference (or one side without scalars) is ONE warning line; returns whether they agree."""
    stored, now = ckpt.get("pnr_balance"), pnr_balance_state(cfg, pnr_balance)
    same = (stored is None) == (now is None)
    if same and now is not None:
        a = torch.as_tensor(stored.get("scalars", [])).cpu()
        same = a.dtype == torch.float32 and a.shape == now["scalars"].shape and torch.equal(a.view(torch.int32), now["scalars"].view(torch.int32))
    if not same:
        logger.warning("pnr balance: the scalars built for this run differ from the checkpoint's (now %s, stored %s): "
                       "the run continues with the ones built now", None if now is None else now["scalars"].tolist(),
                       None if stored is None else torch.as_tensor(stored.get("scalars", [])).tolist())
    return same


# ---- adjustable / learned task weights (``task_weighting:`` of the config; include/egopack_task_scale.h) ---------------
TASK_WEIGHTING_DEFAULTS = {"mode": "none", "lr_scale": 1.0}


def task_weighting_config(cfg) -> dict:
    """The ``task_weighting:`` block with its defaults filled in; an unknown key or mode is a ValueError that lists the known ones."""
    raw = cfg.get("task_weighting") if hasattr(cfg, "get") else None
    raw = dict(raw or {})
    unknown = set(raw) - set(TASK_WEIGHTING_DEFAULTS)
    if unknown:
        raise ValueError(f"task_weighting: unknown key(s) {sorted(unknown)} ({', '.join(TASK_WEIGHTING_DEFAULTS)})")
    tw = {**TASK_WEIGHTING_DEFAULTS, **raw}
    tw["mode"] = str(tw["mode"]).lower()
    if tw["mode"] not in TASK_WEIGHTING_MODES:
        raise ValueError(f"task_weighting.mode: unknown mode '{tw['mode']}' ({' | '.join(TASK_WEIGHTING_MODES)})")
    tw["lr_scale"] = float(tw["lr_scale"])
    if not (tw["lr_scale"] > 0.0 and tw["lr_scale"] < float("inf")):
        raise ValueError(f"task_weighting.lr_scale: {tw['lr_scale']} is not a finite number > 0")
    return tw


# ---- the seeded sampler of the LTA futures (``lta_sampling:`` of the config; include/egopack_sample.h) ------------------
LTA_SAMPLING_DEFAULTS = {"mode": "torch", "seed": 0}
LTA_SAMPLING_MODES = ("torch", "philox")


def lta_sampling_config(cfg) -> dict:
    """The ``lta_sampling:`` block with its defaults filled in; an unknown key or mode is a ValueError that lists the known ones."""
    raw = cfg.get("lta_sampling") if hasattr(cfg, "get") else None
    raw = dict(raw or {})
    unknown = set(raw) - set(LTA_SAMPLING_DEFAULTS)
    if unknown:
        raise ValueError(f"lta_sampling: unknown key(s) {sorted(unknown)} ({', '.join(LTA_SAMPLING_DEFAULTS)})")
    ls = {**LTA_SAMPLING_DEFAULTS, **raw}
    ls["mode"] = str(ls["mode"]).lower()
    if ls["mode"] not in LTA_SAMPLING_MODES:
        raise ValueError(f"lta_sampling.mode: unknown mode '{ls['mode']}' ({' | '.join(LTA_SAMPLING_MODES)})")
    if isinstance(ls["seed"], bool) or not isinstance(ls["seed"], int) or not 0 <= ls["seed"] < 2 ** 64:
        raise ValueError(f"lta_sampling.seed: {ls['seed']!r} is not an integer in [0, 2^64)")
    return ls


# ---- the per-class validation report (``log_confusion_matrices`` + ``class_report:`` of the config) ---------------------
CLASS_REPORT_DEFAULTS = {"shots": [20, 100], "top_confusions": 20, "save": True}
CLASS_REPORT_TASKS = ("ar", "lta", "oscc")  # (PNR is binary and reports tp / tn already)


def class_report_config(cfg) -> dict:
    """The ``class_report:`` block with its defaults filled in, plus ``enabled`` = ``log_confusion_matrices`` (the reference's
    key); an unknown key is a ValueError naming it, and so are shots that are not two increasing integers >= 0."""
    raw = cfg.get("class_report") if hasattr(cfg, "get") else None
    raw = dict(raw or {})
    unknown = set(raw) - set(CLASS_REPORT_DEFAULTS)
    if unknown:
        raise ValueError(f"class_report: unknown key(s) {sorted(unknown)} ({', '.join(CLASS_REPORT_DEFAULTS)})")
    cr = {**CLASS_REPORT_DEFAULTS, **raw}
    shots = list(cr["shots"]) if isinstance(cr["shots"], (list, tuple)) or hasattr(cr["shots"], "__iter__") else [cr["shots"]]
    if len(shots) != 2 or any(isinstance(v, bool) or not isinstance(v, int) for v in shots) or not 0 <= shots[0] < shots[1]:
        raise ValueError(f"class_report.shots: {shots!r} is not [lo, hi] with integers 0 <= lo < hi")
    cr["shots"] = (int(shots[0]), int(shots[1]))
    if isinstance(cr["top_confusions"], bool) or not isinstance(cr["top_confusions"], int) or cr["top_confusions"] < 0:
        raise ValueError(f"class_report.top_confusions: {cr['top_confusions']!r} is not an integer >= 0")
    cr["save"] = bool(cr["save"])
    cr["enabled"] = bool(cfg.get("log_confusion_matrices", False)) if hasattr(cfg, "get") else False
    return cr


def class_report_train_counts(cfg, dsets_train, tasks=None) -> dict:
    """{task: per-head training label counts} for the many / medium / few-shot accuracies of the report -- {} with the report off
    (nothing is counted).  AR / LTA: ``label_counts``; OSCC: its two classes over the labels of the split.  Counted once per run."""
    if not class_report_config(cfg)["enabled"]:
        return {}
    out = {}
    for t in CLASS_REPORT_TASKS:
        if t not in dsets_train or (tasks is not None and t not in tasks):
            continue
        if t == "oscc":
            ds = dsets_train[t]
            if hasattr(ds, "_tables"):  # (as ``pnr_label_counts``: the label table of a dataset that holds one)
                y = torch.as_tensor(ds._tables()["y"]).reshape(-1).to(torch.int64)
            else:
                ys = [torch.as_tensor(ds[i].y).reshape(-1) for i in range(len(ds))]
                y = torch.cat(ys).to(torch.int64) if ys else torch.zeros(0, dtype=torch.int64)
            out[t] = [torch.bincount(y[(y >= 0) & (y < 2)], minlength=2).to(torch.int64)]
        else:
            out[t] = label_counts(dsets_train[t])
    return out


def class_report_meter_args(cfg, train_counts, task: str) -> dict:
    """The keyword arguments of ``build_meter_for_dataset`` for ``task``: {} with the report off."""
    cr = class_report_config(cfg)
    if not cr["enabled"] or task not in CLASS_REPORT_TASKS:
        return {}
    return dict(class_report=True, train_counts=(train_counts or {}).get(task), shots=cr["shots"], top_confusions=cr["top_confusions"])


def save_class_reports(logger, cfg, directory: Path, reports: dict) -> list:
    """``class_report.save``: one ``class_report_<task>.pt`` per task under ``directory`` with the non-scalar entries of the last
    validation's report and the class names (``BaseMeter.report_tables``).  Returns the paths written."""
    cr = class_report_config(cfg)
    if not (cr["enabled"] and cr["save"]):
        return []
    paths = []
    for t, tables in (reports or {}).items():
        if not tables:
            continue
        directory.mkdir(parents=True, exist_ok=True)
        path = directory / f"class_report_{t}.pt"
        torch.save(tables, path)
        logger.info("class report of %s -> %s", t, path)
        paths.append(path)
    return paths


# ---- post-hoc temperature calibration of the heads (``calibration:`` of the config; include/egopack_calibrate.h) ---------
def calibration_config(cfg) -> dict:
    """The ``calibration:`` block with its defaults filled in and checked; an unknown key, mode, task or ``predict`` value is a
    ValueError that names it.  ``enabled`` = (mode == "temperature")."""
    from .calibration import DEFAULTS, MODES, TASKS as CAL_TASKS
    raw = cfg.get("calibration") if hasattr(cfg, "get") else None
    raw = dict(raw or {})
    unknown = set(raw) - set(DEFAULTS)
    if unknown:
        raise ValueError(f"calibration: unknown key(s) {sorted(unknown)} ({', '.join(DEFAULTS)})")
    cal = {**DEFAULTS, **raw}
    cal["mode"] = str(cal["mode"]).lower()
    if cal["mode"] not in MODES:
        raise ValueError(f"calibration.mode: unknown mode '{cal['mode']}' ({' | '.join(MODES)})")
    tasks = [str(t) for t in (cal["tasks"] if not isinstance(cal["tasks"], str) else [cal["tasks"]])]
    bad = [t for t in tasks if t not in CAL_TASKS]
    if bad:
        raise ValueError(f"calibration.tasks: {bad} take no temperature ({', '.join(CAL_TASKS)}; PNR is a one-logit head)")
    cal["tasks"] = tasks
    tr = list(cal["t_range"]) if hasattr(cal["t_range"], "__iter__") else [cal["t_range"]]
    if len(tr) != 2 or any(isinstance(v, bool) or not isinstance(v, (int, float)) for v in tr) or not 0.0 < tr[0] <= 1.0 <= tr[1] < float("inf"):
        raise ValueError(f"calibration.t_range: {tr!r} is not [T_min, T_max] with 0 < T_min <= 1 <= T_max")
    cal["t_range"] = [float(tr[0]), float(tr[1])]
    for key, least in (("iterations", 1), ("max_rows", 1)):
        if isinstance(cal[key], bool) or not isinstance(cal[key], int) or cal[key] < least:
            raise ValueError(f"calibration.{key}: {cal[key]!r} is not an integer >= {least}")
    if isinstance(cal["stop"], bool) or not isinstance(cal["stop"], (int, float)) or not cal["stop"] >= 0:
        raise ValueError(f"calibration.stop: {cal['stop']!r} is not a number >= 0")
    cal["stop"], cal["save"] = float(cal["stop"]), bool(cal["save"])
    pred = cal["predict"]
    pred = "true" if pred is True else "false" if pred is False else str(pred).lower()
    if pred not in ("auto", "true", "false"):
        raise ValueError(f"calibration.predict: unknown value '{cal['predict']}' (auto | true | false)")
    cal["predict"] = pred
    cal["enabled"] = cal["mode"] == "temperature"
    return cal


def calibration_meter_args(cfg, task: str) -> dict:
    """The keyword arguments of ``build_meter_for_dataset`` for ``task``: {} with calibration off (or a task that takes none)."""
    cal = calibration_config(cfg)
    if not cal["enabled"] or task not in cal["tasks"]:
        return {}
    return dict(calibration={k: cal[k] for k in ("t_range", "iterations", "stop", "max_rows")})


def calibration_path(directory, task: str) -> Path:
    return Path(directory) / f"calibration_{task}.pt"


def save_calibration(logger, cfg, directory: Path, fits: dict) -> list:
    """``calibration.save``: one ``calibration_<task>.pt`` per task under ``directory`` (beside the checkpoint, like
    ``class_report_<task>.pt``) with the per-head temperatures, status and row counts of the fit on all rows, the fold fits,
    ``t_range`` and the split it was fitted on.  ``fits``: task -> ``calibration.fit``'s result.  Returns the paths written."""
    cal = calibration_config(cfg)
    if not (cal["enabled"] and cal["save"]):
        return []
    paths = []
    for t, heads in (fits or {}).items():
        if not heads:
            continue
        Path(directory).mkdir(parents=True, exist_ok=True)
        path = calibration_path(directory, t)
        torch.save({"task": t, "heads": heads, "t_range": cal["t_range"], "split": str(cfg.get("validation_split", "")),
                    "iterations": cal["iterations"], "stop": cal["stop"]}, path)
        logger.info("calibration of %s -> %s (%s)", t, path, ", ".join(f"{h} T={v['temperature']:.4f} [{v['status']}]" for h, v in heads.items()))
        paths.append(path)
    return paths


def load_calibration(cfg, directory, task: str) -> Optional[dict]:
    """The calibration file of ``task`` under ``directory`` as ``calibration.predict`` asks for it: None with ``false`` and, with
    ``auto``, when there is no file; with ``true`` a missing file is a FileNotFoundError.  A file of another task or with a
    temperature that is not a finite positive number is a ValueError."""
    cal = calibration_config(cfg)
    if cal["predict"] == "false":
        return None
    path = calibration_path(directory, task)
    if not path.exists():
        if cal["predict"] == "true":
            raise FileNotFoundError(f"calibration.predict=true: {path} is missing (python calibrate.py resume_from=<checkpoint> writes it)")
        return None
    blob = torch.load(path, map_location="cpu", weights_only=False)
    if blob.get("task") != task or not blob.get("heads"):
        raise ValueError(f"{path}: not a calibration file of task {task}")
    for h, v in blob["heads"].items():
        if not 0.0 < float(v["temperature"]) < float("inf"):
            raise ValueError(f"{path}: head {h} holds the temperature {v['temperature']!r}")
    return blob


# ---- action-level scores (``action_scores:`` of the config; include/egopack_action.h) ---------------------------------
ACTION_SCORES_DEFAULTS = {"enabled": False, "tasks": ["ar", "lta"], "topk": 5, "calibrated": "auto", "seen_split": False}
ACTION_SCORES_TASKS = ("ar", "lta")  # (the tasks with a verb and a noun head)


def action_scores_config(cfg) -> dict:
    """The ``action_scores:`` block with its defaults filled in and checked (a config without the block: the defaults, off); an
    unknown key, task or ``calibrated`` value and a ``topk`` outside 1 .. 32 are ValueErrors that name it."""
    from ._lib import ACTION_MAX_K
    raw = cfg.get("action_scores") if hasattr(cfg, "get") else None
    raw = dict(raw or {})
    unknown = set(raw) - set(ACTION_SCORES_DEFAULTS)
    if unknown:
        raise ValueError(f"action_scores: unknown key(s) {sorted(unknown)} ({', '.join(ACTION_SCORES_DEFAULTS)})")
    ac = {**ACTION_SCORES_DEFAULTS, **raw}
    ac["enabled"], ac["seen_split"] = bool(ac["enabled"]), bool(ac["seen_split"])
    tasks = [str(t) for t in (ac["tasks"] if not isinstance(ac["tasks"], str) else [ac["tasks"]])]
    bad = [t for t in tasks if t not in ACTION_SCORES_TASKS]
    if bad:
        raise ValueError(f"action_scores.tasks: {bad} have no (verb, noun) pair ({', '.join(ACTION_SCORES_TASKS)})")
    ac["tasks"] = tasks
    if isinstance(ac["topk"], bool) or not isinstance(ac["topk"], int) or not 1 <= ac["topk"] <= ACTION_MAX_K:
        raise ValueError(f"action_scores.topk: an integer in 1 .. {ACTION_MAX_K} (got {ac['topk']!r})")
    cal = ac["calibrated"]
    cal = "true" if cal is True else "false" if cal is False else str(cal).lower()
    if cal not in ("auto", "true", "false"):
        raise ValueError(f"action_scores.calibrated: unknown value '{ac['calibrated']}' (auto | true | false)")
    ac["calibrated"] = cal
    return ac


def action_pair_codes(dataset) -> torch.Tensor:
    """The sorted distinct codes v * Cn + n (int64) of the (verb, noun) pairs the labels of ``dataset`` hold, over all nodes of all
    samples with both labels inside their heads: one pass over the split, like ``label_counts`` (from the label table where the
    dataset holds one)."""
    names = list(dataset.label_names)
    iv, inn = names.index("verbs"), names.index("nouns")
    Cv, Cn = dataset.num_class_labels[iv], dataset.num_class_labels[inn]
    if hasattr(dataset, "_tables"):
        y = torch.as_tensor(dataset._tables()["y"])
        ys = [y.reshape(-1, y.shape[-1])]
    else:
        ys = [torch.as_tensor(dataset[i].y).reshape(-1, len(names)) for i in range(len(dataset))]
    y = torch.cat(ys).to(torch.int64) if ys else torch.zeros((0, len(names)), dtype=torch.int64)
    v, n = y[:, iv], y[:, inn]
    ok = (v >= 0) & (v < Cv) & (n >= 0) & (n < Cn)
    return torch.unique(v[ok] * Cn + n[ok])  # (sorted)


def action_scores_seen(cfg, dsets_train, tasks=None) -> dict:
    """{task: ``action_pair_codes`` of its training split} with ``action_scores.seen_split`` on -- {} otherwise (nothing is read).
    Built once per run."""
    ac = action_scores_config(cfg)
    if not (ac["enabled"] and ac["seen_split"]):
        return {}
    return {t: action_pair_codes(dsets_train[t]) for t in ac["tasks"] if t in dsets_train and (tasks is None or t in tasks)}


def action_scores_meter_args(cfg, task: str, seen=None) -> dict:
    """The keyword arguments of ``build_meter_for_dataset`` for ``task``: {} with the block off (or a task without a pair).
    ``seen``: ``action_scores_seen``'s dict."""
    ac = action_scores_config(cfg)
    if not ac["enabled"] or task not in ac["tasks"]:
        return {}
    args = {"topk": ac["topk"]}
    if ac["seen_split"] and seen is not None and task in seen:
        args["seen"] = seen[task]
    return dict(action_scores=args)


# ---- the cluster bootstrap of the validation metrics (``bootstrap:`` of the config; include/egopack_bootstrap.h) --------
BOOTSTRAP_DEFAULTS = {"replicates": 0, "level": 0.95, "seed": 0, "save": True}


def bootstrap_config(cfg) -> dict:
    """The ``bootstrap:`` block with its defaults filled in and checked (a config without the block: the defaults, off); an unknown
    key, ``replicates`` outside 0 .. 65536, a ``level`` outside (0, 1) and a seed that is no integer are ValueErrors that name it."""
    from ._lib import BOOT_MAX_R
    raw = cfg.get("bootstrap") if hasattr(cfg, "get") else None
    raw = dict(raw or {})
    unknown = set(raw) - set(BOOTSTRAP_DEFAULTS)
    if unknown:
        raise ValueError(f"bootstrap: unknown key(s) {sorted(unknown)} ({', '.join(BOOTSTRAP_DEFAULTS)})")
    bc = {**BOOTSTRAP_DEFAULTS, **raw}
    if isinstance(bc["replicates"], bool) or not isinstance(bc["replicates"], int) or not 0 <= bc["replicates"] <= BOOT_MAX_R:
        raise ValueError(f"bootstrap.replicates: an integer in 0 .. {BOOT_MAX_R}, 0 = off (got {bc['replicates']!r})")
    if isinstance(bc["level"], bool) or not isinstance(bc["level"], (int, float)) or not 0.0 < float(bc["level"]) < 1.0:
        raise ValueError(f"bootstrap.level: a number inside (0, 1) (got {bc['level']!r})")
    if isinstance(bc["seed"], bool) or not isinstance(bc["seed"], int):
        raise ValueError(f"bootstrap.seed: an integer (got {bc['seed']!r})")
    bc["level"], bc["save"] = float(bc["level"]), bool(bc["save"])
    return bc


def bootstrap_meter_args(cfg, task: str = None) -> dict:
    """The keyword arguments of ``build_meter_for_dataset``: {} with ``bootstrap.replicates`` = 0 (every task's meter takes it)."""
    bc = bootstrap_config(cfg)
    if bc["replicates"] == 0:
        return {}
    return dict(bootstrap={"replicates": bc["replicates"], "level": bc["level"], "seed": bc["seed"]})


def save_bootstraps(logger, cfg, directory: Path, bootstraps: dict) -> list:
    """``bootstrap.save``: one ``bootstrap_<task>.pt`` per task under ``directory`` with the accumulators, the replicate values and
    point estimates per metric, seed, R, level, the split's name and the clusters seen of the last validation
    (``BaseMeter.bootstrap_tables``; ``compare_runs.py`` pairs two of them).  Returns the paths written."""
    bc = bootstrap_config(cfg)
    if not (bc["replicates"] > 0 and bc["save"]):
        return []
    paths = []
    for t, tables in (bootstraps or {}).items():
        if not tables:
            continue
        directory.mkdir(parents=True, exist_ok=True)
        path = directory / f"bootstrap_{t}.pt"
        torch.save(tables, path)
        logger.info("bootstrap of %s (%d replicates, seed %d, %d clusters) -> %s", t, tables["replicates"], tables["seed"],
                    tables["clusters"], path)
        paths.append(path)
    return paths


def action_scores_betas(cfg, directory, task: str, calibration=None):
    """What the export scores the joint at: (the task's calibration file or None, [1 / T of the verbs, 1 / T of the nouns] or None)
    as ``action_scores.calibrated`` asks.  ``calibration``: the file the caller loaded (``load_calibration``: what
    ``calibration.predict`` allows).  ``auto``: that file when it is loaded, else the raw logits; ``true``: the file is required --
    the one under ``directory`` is read when the caller loaded none, and a missing file is a FileNotFoundError; ``false`` (or the
    block off for ``task``): (None, None)."""
    ac = action_scores_config(cfg)
    if not ac["enabled"] or task not in ac["tasks"] or ac["calibrated"] == "false":
        return None, None
    blob = calibration
    if blob is None and ac["calibrated"] == "true":
        path = calibration_path(directory, task)
        if not path.exists():
            raise FileNotFoundError(f"action_scores.calibrated=true: {path} is missing (python calibrate.py resume_from=<checkpoint> writes it)")
        blob = torch.load(path, map_location="cpu", weights_only=False)
        if blob.get("task") != task or not blob.get("heads"):
            raise ValueError(f"{path}: not a calibration file of task {task}")
    if blob is None:
        return None, None
    betas = [1.0 / float(blob["heads"][p]["temperature"]) for p in ("verbs_", "nouns_")]
    if not all(0.0 < b < float("inf") for b in betas):
        raise ValueError(f"action_scores: the calibration file of task {task} holds the temperatures {[1 / b for b in betas]}")
    return blob, betas


def build_lta_sampler(cfg):
    """The ``ops.FutureSampler`` of ``lta_sampling.mode=philox`` (stateless: nothing of it goes into a checkpoint); None with
    ``mode: torch`` -- the validation loop then samples with torch's generator, as the reference does."""
    ls = lta_sampling_config(cfg)
    if ls["mode"] != "philox":
        return None
    from .ops import FutureSampler
    return FutureSampler(ls["seed"])


def build_task_weighting(cfg, enabled, device=None):
    """The models.TaskLogVariance of an ``uncertainty`` run over the enabled tasks (in the step's order), on ``device``; None in
    the other modes (nothing is built: the optimizer and the launches are the ones without the feature)."""
    if task_weighting_config(cfg)["mode"] != "uncertainty":
        return None
    from .models import TaskLogVariance
    lv = TaskLogVariance(enabled)
    return lv.to(device) if device is not None else lv


def log_task_weighting(logger, epoch: int, step) -> None:
    """One line per epoch: s_t and the effective weights w_t exp(-s_t) (uncertainty), or the scales set from the host and
    w_t scale_t (manual); nothing with the feature off.  One device synchronisation, like ``loss_sums``."""
    mode = getattr(step, "task_mode", "none")
    if mode == "uncertainty":
        eff = step.task_log_var.effective_weights(step.weights)
        logger.info("epoch %d: task weighting (uncertainty): %s", epoch,
                    {t: {"s": round(s_, 6), "weight": round(w_, 6)} for t, (s_, w_) in eff.items()})
    elif mode == "manual":
        logger.info("epoch %d: task weighting (manual): %s", epoch,
                    {t: {"scale": round(v, 6), "weight": round(step.weights[t] * v, 6)} for t, v in step.task_scales().items()})


def task_weighting_state(cfg, step) -> Optional[dict]:
    """The checkpoint's top-level ``"task_weighting"`` entry: the config block, the task order and ``log_var`` (uncertainty) or the
    scales (manual), as f32 tensors on the host; None when off."""
    mode = getattr(step, "task_mode", "none")
    if mode == "none":
        return None
    out = {"config": task_weighting_config(cfg), "tasks": list(step.enabled)}
    if mode == "uncertainty":
        out["log_var"] = step.task_log_var.log_var.detach().float().cpu().clone()
    else:
        out["scales"] = torch.tensor([step.task_scales()[t] for t in step.enabled], dtype=torch.float32)
    return out


def load_task_weighting(logger, ckpt: dict, step) -> bool:
    """On resume: ``log_var`` / the scales of the checkpoint's ``"task_weighting"`` entry go into the step (the optimizer state of
    ``log_var`` travels in the optimizer's state dict).  A checkpoint without the entry -- or one of another mode or task order --
    starts from s = 0 / scale 1 with ONE log line; that includes a checkpoint a fixed-weight run wrote with its optimizer state:
    optim.FlatOptimizer.load_state_dict takes a state that lacks exactly the trailing ``task_weighting`` group and starts its
    parameter with fresh moments.  Returns whether the entry was taken."""
    mode = getattr(step, "task_mode", "none")
    if mode == "none":
        return False
    stored = ckpt.get("task_weighting")
    key = "log_var" if mode == "uncertainty" else "scales"
    if not stored or list(stored.get("tasks", [])) != list(step.enabled) or stored.get(key) is None:
        logger.info("task weighting: the checkpoint has no '%s' for the tasks %s (stored: %s): starting from %s", key, list(step.enabled),
                    None if not stored else {"mode": stored.get("config", {}).get("mode"), "tasks": stored.get("tasks")},
                    "s = 0 (fresh optimizer moments for log_var)" if mode == "uncertainty" else "scale 1")
        return False
    vals = torch.as_tensor(stored[key]).float().reshape(-1)
    if mode == "uncertainty":
        with torch.no_grad():
            p = step.task_log_var.log_var
            p.copy_(vals.to(p.device))
    else:
        step.set_task_scale(dict(zip(step.enabled, vals.tolist())))
    return True


OPTIMIZERS = {"torch.optim.Adam": FlatAdam, "torch.optim.AdamW": FlatAdamW, "torch.optim.SGD": FlatSGD,
              "egopack_amd.optim.FlatLAMB": FlatLAMB}  # (LAMB has no torch class: the config names the flat-buffer one)

# ---- the element type of the optimizer state (``optimizer_state:`` of the config; include/egopack_optim.h) ---------------
OPTIMIZER_STATE_DEFAULTS = {"dtype": "f32", "rounding": "stochastic", "seed": None}


def optimizer_state_config(cfg) -> dict:
    """The ``optimizer_state:`` block with its defaults filled in (``dtype`` and ``rounding`` in lower case); an unknown key, dtype
    or rounding is a ValueError that lists the known ones.  ``seed``: None (the run's seed) or an integer in [0, 2^64)."""
    raw = cfg.get("optimizer_state") if hasattr(cfg, "get") else None
    raw = dict(raw or {})
    unknown = set(raw) - set(OPTIMIZER_STATE_DEFAULTS)
    if unknown:
        raise ValueError(f"optimizer_state: unknown key(s) {sorted(unknown)} ({', '.join(OPTIMIZER_STATE_DEFAULTS)})")
    st = {**OPTIMIZER_STATE_DEFAULTS, **raw}
    st["dtype"], st["rounding"] = str(st["dtype"]).lower(), str(st["rounding"]).lower()
    if st["dtype"] not in STATE_DTYPES:
        raise ValueError(f"optimizer_state.dtype: unknown dtype '{st['dtype']}' ({' | '.join(STATE_DTYPES)})")
    if st["rounding"] not in STATE_ROUNDINGS:
        raise ValueError(f"optimizer_state.rounding: unknown rounding '{st['rounding']}' ({' | '.join(sorted(STATE_ROUNDINGS, reverse=True))})")
    if st["seed"] is not None and (isinstance(st["seed"], bool) or not isinstance(st["seed"], int) or not 0 <= st["seed"] < 2 ** 64):
        raise ValueError(f"optimizer_state.seed: {st['seed']!r} is neither null nor an integer in [0, 2^64)")
    return st


def log_optimizer_state(logger, optimizer) -> None:
    """One line: which state the run keeps."""
    if getattr(optimizer, "bf16_state", False):
        logger.info("optimizer state: bf16, %s rounding%s (half the bytes of f32 moments)", optimizer.state_rounding,
                    f", seed {optimizer.state_seed}" if optimizer.state_rounding == "stochastic" else "")
    else:
        logger.info("optimizer state: f32")


PARAM_GROUP_MODULES = ("temporal_graph", "tasks", "graphone")  # the keys of ``param_groups.lr_scale``


def build_param_groups(cfg, model, tasks, graphone=None):
    """What the optimizer is built over.  With the defaults (``param_groups: {no_decay_1d: false, lr_scale: {}}``): the flat
    parameter list the entry points have always built -- the modules' ``configure_optimizers`` results spliced together, same
    order, same objects.  Otherwise at most six torch-style group dicts (module x decays-or-not, empty ones dropped):
    ``no_decay_1d`` gives the parameters with ``dim() <= 1`` (biases, LayerNorm weight and bias) ``weight_decay`` 0, and
    ``lr_scale.<temporal_graph | tasks | graphone>`` multiplies ``optimizer.lr`` for that module's parameters (missing: 1.0).
    ``param_groups:`` sits beside ``optimizer:``, not inside it, like ``grad_clip_norm``."""
    wd = cfg.optimizer.weight_decay
    parts = [("temporal_graph", list(model.configure_optimizers(wd))),
             ("tasks", [p for t in TASKS for p in tasks[t].configure_optimizers(wd)]),
             ("graphone", list(graphone.parameters()) if graphone is not None else [])]
    flat = [p for _, ps in parts for p in ps]
    pg = dict(cfg.get("param_groups") or {})
    unknown = set(pg) - {"no_decay_1d", "lr_scale"}
    if unknown:
        raise ValueError(f"param_groups: unknown key(s) {sorted(unknown)} (no_decay_1d, lr_scale)")
    no_decay = bool(pg.get("no_decay_1d", False))
    scale = {k: float(v) for k, v in dict(pg.get("lr_scale") or {}).items()}
    unknown = set(scale) - set(PARAM_GROUP_MODULES)
    if unknown:
        raise ValueError(f"param_groups.lr_scale: unknown key(s) {sorted(unknown)} ({', '.join(PARAM_GROUP_MODULES)})")
    scaled = any(v != 1.0 for v in scale.values())
    if not no_decay and not scaled:
        return flat
    groups, seen = {}, set()
    for module, ps in parts:
        for p in ps:
            if id(p) in seen:  # (the reference passes some parameters twice: the first mention decides)
                continue
            seen.add(id(p))
            bare = no_decay and p.dim() <= 1
            key = (module if scaled else "all", bare)
            if key not in groups:
                groups[key] = {"params": [], "name": key[0] + ("/no_decay" if bare else ""),
                               "lr": float(cfg.optimizer.lr) * scale.get(module, 1.0) if scaled else float(cfg.optimizer.lr),
                               "weight_decay": 0.0 if bare else float(wd)}
            groups[key]["params"].append(p)
    return [g for g in groups.values() if g["params"]]


def log_param_groups(logger, optimizer) -> None:
    """One line per parameter group: name, tensors, elements, lr, weight_decay."""
    for i, g in enumerate(optimizer.param_groups):
        logger.info("parameter group %d (%s): %d tensors, %d elements, lr %.6g, weight_decay %.6g", i, g.get("name", "all"),
                    len(g["params"]), sum(p.numel() for p in g["params"]), g["lr"], g.get("weight_decay", 0.0))


def build_optimizer(cfg, params, layout_order=None, log_var=None):
    """``_target_: torch.optim.Adam | AdamW | SGD`` of the config is served by the flat-buffer optimizer of the same rule (same
    arithmetic, same keyword arguments); ``torch.optim.Adam`` with ``decoupled_weight_decay: true`` is AdamW's rule.
    ``params``: a parameter list or the group dicts of ``build_param_groups``; ``layout_order``: with groups, the flat list they
    were cut from -- the flat buffers keep its order (optim.FlatOptimizer).
    ``log_var`` (``build_task_weighting``; None: nothing changes): its parameter becomes the LAST parameter, in a group of its own
    named ``task_weighting`` with weight_decay 0 and lr = optimizer.lr * task_weighting.lr_scale, through the parameter-group
    table; its slot follows the heads' slots in the flat buffers and is clipped and exchanged like any slot."""
    ocfg = dict(cfg.optimizer)
    target = ocfg.pop("_target_")
    if target not in OPTIMIZERS:
        raise ValueError(f"optimizer {target}: the flat-buffer kernels serve {', '.join(OPTIMIZERS)}")
    cls = OPTIMIZERS[target]
    if cls is FlatAdam and ocfg.pop("decoupled_weight_decay", False):
        cls = FlatAdamW
        ocfg.setdefault("weight_decay", 0.0)  # (torch.optim.Adam's default, not AdamW's)
    # (``grad_clip_norm`` sits beside ``optimizer:``, not inside it: that block is handed to Hydra's instantiate by the reference)
    grouped = bool(params) and isinstance(params[0], dict)
    if log_var is not None:
        own = list(log_var.parameters())
        flat = [p for g in params for p in g["params"]] if grouped else list(params)
        layout_order = [*(layout_order if (grouped and layout_order is not None) else flat), *own]
        params = [*(params if grouped else [{"params": flat, "name": "all"}]),
                  {"params": own, "name": TASK_WEIGHTING_GROUP, "lr": float(cfg.optimizer.lr) * task_weighting_config(cfg)["lr_scale"],
                   "weight_decay": 0.0}]
        grouped = True
    extra = {"layout_order": layout_order} if grouped and layout_order is not None else {}
    # (``ema:`` sits beside ``optimizer:`` for the same reason; decay 0 = off)
    ema = dict(cfg.get("ema") or {})
    unknown = set(ema) - {"decay", "warmup", "validate", "save"}
    if unknown:
        raise ValueError(f"ema: unknown key(s) {sorted(unknown)} (decay, warmup, validate, save)")
    # (``optimizer_state:`` likewise; the default block hands the constructors nothing they did not get before)
    st = optimizer_state_config(cfg)
    if st["dtype"] != "f32":
        extra.update(state_dtype=STATE_DTYPES[st["dtype"]], state_rounding=st["rounding"], state_seed=st["seed"])
    return cls(params, **ocfg, max_grad_norm=float(cfg.get("grad_clip_norm", 0) or 0), ema_decay=float(ema.get("decay", 0) or 0),
               ema_warmup=bool(ema.get("warmup", False)), **extra)


def ema_scope(cfg, optimizer):
    """The context a validation loop runs in: ``optimizer.ema_weights()`` with ``ema.decay`` > 0 and ``ema.validate`` set, otherwise
    one that does nothing."""
    import contextlib
    ema = dict(cfg.get("ema") or {})
    if getattr(optimizer, "ema", False) and bool(ema.get("validate", True)):
        return optimizer.ema_weights()
    return contextlib.nullcontext()


def ema_saved(cfg) -> bool:
    """``ema.save`` of the config (default true): ``save_checkpoint`` also writes the averaged weights when there is an average."""
    return bool(dict(cfg.get("ema") or {}).get("save", True))


def log_validation_weights(logger, cfg, optimizer, epoch: int) -> None:
    """One line per validation: which weights are scored."""
    ema = dict(cfg.get("ema") or {})
    if getattr(optimizer, "ema", False) and bool(ema.get("validate", True)):
        logger.info("epoch %d: validating the averaged weights (ema.decay %g%s)", epoch, optimizer.ema_decay,
                    ", warm-up" if optimizer.ema_warmup else "")
    else:
        logger.info("epoch %d: validating the raw weights%s", epoch,
                    " (ema.validate is off)" if getattr(optimizer, "ema", False) else "")


def log_grad_norms(logger, epoch: int, step) -> None:
    """With gradient clipping on: the epoch's gradient-norm figures, next to the task losses (nothing otherwise)."""
    if not getattr(step.optimizer, "clipping", False):
        return
    st = step.grad_norm_stats()
    logger.info("epoch %d: gradient norm mean %.9g, largest %.9g, clipped %d of %d steps (max norm %g), skipped %d (norm not finite)",
                epoch, st["mean_norm"], st["max_norm"], st["clipped"], st["steps"], step.optimizer.max_grad_norm, st["skipped"])


def log_trust_ratios(logger, epoch: int, step) -> None:
    """With LAMB: the smallest, median and largest trust ratio of the epoch's last step, next to the task losses (nothing otherwise)."""
    opt = step.optimizer
    if not hasattr(opt, "trust_ratios") or not getattr(opt, "materialised", False):
        return
    trust = sorted(t for t, _, _ in opt.trust_ratios().values())
    if trust:
        logger.info("epoch %d: trust ratio min %.6g, median %.6g, max %.6g over %d parameter tensors", epoch, trust[0],
                    trust[len(trust) // 2], trust[-1], len(trust))


def build_scheduler(cfg, optimizer):
    sched = instantiate(cfg.lr_scheduler, optimizer=optimizer)
    if cfg.use_warmup:
        sched = torch.optim.lr_scheduler.ChainedScheduler(
            [torch.optim.lr_scheduler.LinearLR(optimizer, 0.001, 1, 5), sched])
    return sched


def _module_states(model, tasks, epoch: int, graphone=None) -> dict:
    """The modules' state dicts on the host under the reference's keys."""
    ckpt = {"temporal_graph": {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}, "epoch": epoch}
    for t, key in CKPT_KEYS.items():
        ckpt[key] = {k: v.detach().cpu().clone() for k, v in tasks[t].state_dict().items()}
    if graphone is not None:
        ckpt["graphone"] = {k: v.detach().cpu().clone() for k, v in graphone.state_dict().items()}
    return ckpt


def _write(ckpt: dict, path: Path) -> None:
    tmp = path.with_suffix(path.suffix + ".tmp")
    torch.save(ckpt, tmp)
    tmp.replace(path)  # a killed run never leaves a half-written checkpoint behind
    logger.info("saved %s", path)


def ema_checkpoint_path(path: Path) -> Path:
    """``checkpoint.pth`` -> ``checkpoint_ema.pth``, beside it."""
    return path.with_name(path.stem + "_ema" + path.suffix)


def save_checkpoint(path: Path, model, tasks, epoch: int, graphone=None, optimizer=None, scheduler=None, loaders=None,
                    save_ema: bool = False, class_balance: Optional[dict] = None, pnr_balance: Optional[dict] = None,
                    task_weighting: Optional[dict] = None):
    """Reference key layout (main_temporal.py:410-417, main_egopack.py:453-460) + what the reference does not keep and
    a resumed run needs: the optimiser state (torch.optim.Adam's per-parameter layout) and the schedule state.
    ``save_ema`` (``ema.save`` of the config; an optimizer that keeps a weight average): a second file beside it,
    ``checkpoint_ema.pth``, with the reference's key layout alone and the AVERAGED weights in place of the parameters -- the
    modules' state dicts taken inside ``optimizer.ema_weights()``; any loader of the reference's layout and ``resume_from=``
    take it as it is.  The ordinary file keeps the raw weights and the average under the optimizer's ``"ema"`` key.
    ``class_balance`` (``class_balance_state``; None when off): stored under the top-level key ``"class_balance"``;
    ``pnr_balance`` (``pnr_balance_state``) likewise under ``"pnr_balance"``, ``task_weighting`` (``task_weighting_state``) under
    ``"task_weighting"``."""
    path.parent.mkdir(parents=True, exist_ok=True)
    if save_ema and getattr(optimizer, "ema", False):
        with optimizer.ema_weights():
            averaged = _module_states(model, tasks, epoch, graphone)
        _write(averaged, ema_checkpoint_path(path))
    ckpt = _module_states(model, tasks, epoch, graphone)
    if optimizer is not None:
        sd = optimizer.state_dict()
        sd["state"] = {i: {k: (v.cpu() if torch.is_tensor(v) else v) for k, v in st.items()} for i, st in sd["state"].items()}
        if sd.get("ema") is not None:
            sd["ema"] = {**sd["ema"], "values": {i: v.cpu() for i, v in sd["ema"]["values"].items()}}
        ckpt["optimizer"] = sd
    if scheduler is not None:
        ckpt["scheduler"] = scheduler.state_dict()
    if class_balance is not None:
        ckpt["class_balance"] = class_balance
    if pnr_balance is not None:
        ckpt["pnr_balance"] = pnr_balance
    if task_weighting is not None:
        ckpt["task_weighting"] = task_weighting
    if loaders is not None:  # shuffle generators of the training loaders + dropout streams: exact continuation
        ckpt["rng"] = {"loaders": {t: dl.state_dict() for t, dl in loaders.items() if hasattr(dl, "state_dict")},
                       "dropout": ops.get_rng_state(), "torch": torch.get_rng_state()}
    _write(ckpt, path)


def load_checkpoint(path, model, tasks, strict_tasks: bool = True, device="cpu", graphone=None, optimizer=None,
                    scheduler=None, loaders=None):
    """Weights (reference layout; a reference checkpoint loads as it is) and, when given and present, GraphONE,
    optimiser and schedule state.  Returns the checkpoint dict (``["epoch"]`` = last finished epoch)."""
    ckpt = torch.load(path, map_location=device, weights_only=False)
    model.load_state_dict(ckpt["temporal_graph"])
    for t, key in CKPT_KEYS.items():
        if ckpt.get(key) is not None:
            tasks[t].load_state_dict(ckpt[key], strict=strict_tasks)
    if graphone is not None and ckpt.get("graphone") is not None:
        graphone.load_state_dict(ckpt["graphone"])
    if optimizer is not None and ckpt.get("optimizer") is not None:
        optimizer.load_state_dict(ckpt["optimizer"])
        if getattr(optimizer, "materialised", False):
            optimizer.refresh_shadows()  # the bf16 operand copies follow the f32 parameters just loaded
    if scheduler is not None and ckpt.get("scheduler") is not None:
        scheduler.load_state_dict(ckpt["scheduler"])
    if loaders is not None and ckpt.get("rng") is not None:
        for t, st in ckpt["rng"]["loaders"].items():
            if t in loaders and hasattr(loaders[t], "load_state_dict"):
                loaders[t].load_state_dict(st)
        ops.set_rng_state(ckpt["rng"]["dropout"])
        torch.set_rng_state(ckpt["rng"]["torch"].cpu())
    return ckpt


def setup_logging(rank: int):
    logging.basicConfig(level=logging.INFO if rank == 0 else logging.WARNING,
                        format="[%(asctime)s][%(name)s][%(levelname)s] %(message)s")
