"""Prediction export: what a trained model predicts, per sample, as plain CPU tensors.

One ``@torch.no_grad()`` loop per kind of task.  Each reuses ``validate._eval_mode`` and ``validate._logits`` as they are, so a
prediction is made from the very logits validation scores; there are no meters and no loss.  The classes a head chose and their
probabilities come from ONE ``egk_topk_softmax`` launch per batch for all heads (``ops.topk_softmax``: the meters' order, the
log-sum-exp of the loss kernels), the LTA futures from the seeded sampler only (``ops.FutureSampler``, keyed by the batch ordinal
exactly as ``validate_lta`` does it), the PNR key frame from ``egk_segment_max_fwd`` exactly as ``PNRMeter.update`` calls it.

Every row carries its provenance: ``sample`` is the sample's index in the dataset (batch ordinal * the loader's batch size + the
row's entry in ``data.batch`` / its sequence number; the loader is unshuffled and unsharded), ``pos`` the node's ``data.pos``.

``main`` is the entry point behind ``python predict.py resume_from=<checkpoint> ...`` (the ``predict:`` block of the config)."""
from __future__ import annotations

import json
import logging
import time
from pathlib import Path
from typing import List, Optional

import torch

from . import _lib, ops
from .validate import _eval_mode, _logits

logger = logging.getLogger("predict")

PREDICT_DEFAULTS = {"split": "validation", "topk": 5, "out": None, "json": True}
HEADS = ("verb", "noun")


def predict_config(cfg) -> dict:
    """The ``predict:`` block with its defaults filled in; an unknown key or a ``topk`` outside 1 .. 64 is a ValueError naming it."""
    raw = cfg.get("predict") if hasattr(cfg, "get") else None
    raw = dict(raw or {})
    unknown = set(raw) - set(PREDICT_DEFAULTS)
    if unknown:
        raise ValueError(f"predict: unknown key(s) {sorted(unknown)} ({', '.join(PREDICT_DEFAULTS)})")
    pc = {**PREDICT_DEFAULTS, **raw}
    if "split" not in raw and hasattr(cfg, "get") and cfg.get("validation_split"):
        pc["split"] = cfg.get("validation_split")
    pc["split"], pc["json"] = str(pc["split"]), bool(pc["json"])
    if isinstance(pc["topk"], bool) or not isinstance(pc["topk"], int) or not 1 <= pc["topk"] <= _lib.TOPK_MAX_K:
        raise ValueError(f"predict.topk: an integer in 1 .. {_lib.TOPK_MAX_K} (got {pc['topk']!r})")
    pc["out"] = None if pc["out"] in (None, "", "null") else str(pc["out"])
    return pc


# ---- provenance ---------------------------------------------------------------------------------------------------------------------
def _batch_size(dataloader) -> int:
    """The batch size of a ``data.BatchLoader``, also behind an adapter that wraps one (``train.ResidentLoader``)."""
    dl = dataloader
    while not hasattr(dl, "batch_size") and hasattr(dl, "loader"):
        dl = dl.loader
    bs = getattr(dl, "batch_size", None)
    if bs is None:
        raise ValueError("predict: the loader has no batch_size (a data.BatchLoader with shuffle=False on rank 0 of 1 is expected)")
    if getattr(dl, "shuffle", False) or int(getattr(dl, "world_size", 1)) > 1:
        raise ValueError("predict: the loader must be unshuffled and unsharded (sample = ordinal * batch_size + row's sequence)")
    return int(bs)


def _first_sample(data, bs: int) -> int:
    ordinal = getattr(data, "ordinal", None)
    if ordinal is None:
        raise ValueError("predict: the batch carries no ordinal (data.BatchLoader stamps it on every batch)")
    return int(ordinal) * bs


def _node_samples(data, bs: int) -> torch.Tensor:
    return data.batch.to(torch.int64) + _first_sample(data, bs)


def _seq_samples(data, bs: int, n_seq: int, device) -> torch.Tensor:
    return torch.arange(n_seq, dtype=torch.int64, device=device) + _first_sample(data, bs)


class _Fields:
    """Per-batch device tensors, one device-to-host copy per field and batch, concatenated at the end."""

    def __init__(self):
        self.parts = {}

    def add(self, **fields):
        for k, v in fields.items():
            if v is not None:
                self.parts.setdefault(k, []).append(v.detach().cpu())

    def result(self) -> dict:
        return {k: torch.cat(v) for k, v in self.parts.items()}


# ---- the fitted temperatures of a calibration file (train.load_calibration) ------------------------------------------
def beta_words(calibration: Optional[dict], prefixes, device):
    """Per head of ``prefixes`` (the meters' key prefixes: "verbs_", "nouns_", "" for OSCC) the device word fl(1 / T) the
    temperature launches read; None without a calibration file."""
    if not calibration:
        return None
    return [torch.tensor([1.0 / float(calibration["heads"][p]["temperature"])], dtype=torch.float32, device=device) for p in prefixes]


def temperatures(calibration: Optional[dict]) -> dict:
    """What a prediction file records of the calibration it was written with: {} without one (the file is then today's)."""
    if not calibration:
        return {}
    return {"temperature": {(p.rstrip("_") or "oscc"): float(v["temperature"]) for p, v in calibration["heads"].items()}}


# ---- AR and LTA: the verb / noun heads, per node ------------------------------------------------------------------------------------
def action_args(action: Optional[dict], device):
    """``action`` ({"topk": k, "betas": [1 / T verbs, 1 / T nouns] | None}; None: the export is off) as the loops use it: (k, the
    two-word device tensor ``ops.action_topk`` reads, or None)."""
    if not action:
        return None
    betas = action.get("betas")
    return int(action["topk"]), None if betas is None else torch.tensor([float(b) for b in betas], dtype=torch.float32, device=device)


def _heads_batch(out: _Fields, data, logits, k: int, bs: int, head_index, betas=None, action=None):
    from .meters import label_rank
    heads = [logits[i] for i in head_index]
    (vi, vp, vl), (ni, np_, nl) = ops.topk_softmax(heads, k, want_prob=True, want_lse=True)  # both heads, one launch
    if betas is not None:  # calibrated: the probabilities of the SAME order at the fitted temperatures (the order is never recomputed)
        vp, vl = ops.temp_topk_prob(heads[0], vi, betas[0], want_lse=True)
        np_, nl = ops.temp_topk_prob(heads[1], ni, betas[1], want_lse=True)
    y = getattr(data, "y", None)
    label = rank = None
    if y is not None:
        label = torch.stack([y[:, i].to(torch.int64) for i in head_index], 1)
        rank = torch.stack([label_rank(h.detach(), y[:, i]) for h, i in zip(heads, head_index)], 1)
    out.add(sample=_node_samples(data, bs), pos=data.pos, verb_topk=vi, verb_prob=vp, noun_topk=ni, noun_prob=np_, verb_lse=vl,
            noun_lse=nl, label=label, rank=rank)
    if action is not None:  # the best pairs under the product of both heads' softmaxes, one launch (action_scores)
        a = ops.action_topk(heads[0], heads[1], action[0], beta=action[1], want_prob=True)
        out.add(action_topk=a["pair"], action_logp=a["logp"], action_prob=a["prob"])


@torch.no_grad()
def predict_heads(temporal_graph_model, dataloader, primary_task, k: int = 5, other_tasks: Optional[List] = None, graphone=None,
                  late_fusion: bool = True, device: str = "cuda", head_index=(0, 1), calibration=None, action=None) -> dict:
    """The verb / noun heads of the AR task (or of any multi-head task), per node: ``sample``, ``pos``, ``verb_topk``, ``verb_prob``,
    ``noun_topk``, ``noun_prob`` [rows, k], ``verb_lse``, ``noun_lse`` [rows] and, when the split has labels, ``label`` [rows, 2] and
    ``rank`` int32 [rows, 2] (``egk_label_rank``; -1 for an ignored row).  ``late_fusion``: as ``validate.validate``.
    ``calibration`` (``train.load_calibration``): ``*_prob`` and ``*_lse`` at the fitted temperatures, over the raw order.
    ``action`` ({"topk": k, "betas": [1 / T verbs, 1 / T nouns] | None}): also ``action_topk`` int64 [rows, k, 2], ``action_logp`` and
    ``action_prob`` [rows, k], the best (verb, noun) pairs of ``ops.action_topk``; with betas the joint is SCORED AND ORDERED at
    them, so its order may differ from the raw one (two temperatures make another product distribution)."""
    other_tasks = other_tasks or []
    bs = _batch_size(dataloader)
    betas = beta_words(calibration, ("verbs_", "nouns_"), device)
    action = action_args(action, device)
    _eval_mode(temporal_graph_model, primary_task, other_tasks, graphone)
    out = _Fields()
    for data in dataloader:
        data = data.to(device)
        logits, _ = _logits(temporal_graph_model, data, primary_task, other_tasks, graphone, late_fusion, needs_batch=True)
        _heads_batch(out, data, logits, k, bs, head_index, betas, action)
    return out.result()


@torch.no_grad()
def predict_lta(temporal_graph_model, dataloader, primary_task, k: int = 5, seed: int = 0, n_nodes: int = 22, n_futures: int = 5,
                other_tasks: Optional[List] = None, graphone=None, late_fusion: bool = False, device: str = "cuda",
                head_index=(0, 1), calibration=None, action=None) -> dict:
    """The LTA task: the per-node fields of ``predict_heads`` and the sampled futures ``verb_futures`` / ``noun_futures``, int64
    [sequences, Z, K] (``futures_sample`` [sequences]: their samples), after dropping the observed nodes as ``meters.LTAMeter``
    does (sequences of ``n_nodes`` nodes -- the dataset's ``lta_nodes`` --, the first ``LTAMeter.SKIP`` dropped).  The futures come
    from ``ops.FutureSampler(seed)`` keyed by the batch ordinal, exactly as ``validate.validate_lta`` draws them with
    ``lta_sampling.mode=philox``: a function of the weights and the seed alone."""
    from .meters import LTAMeter
    other_tasks = other_tasks or []
    bs = _batch_size(dataloader)
    sampler = ops.FutureSampler(seed)
    betas = beta_words(calibration, ("verbs_", "nouns_"), device)  # (the per-node probabilities; the futures are the raw logits')
    action = action_args(action, device)  # (``action``: as ``predict_heads``)
    _eval_mode(temporal_graph_model, primary_task, other_tasks, graphone)
    out = _Fields()
    for data in dataloader:
        data = data.to(device)
        logits, _ = _logits(temporal_graph_model, data, primary_task, other_tasks, graphone, late_fusion, needs_batch=True)
        predictions, logits = primary_task.generate_from_logits(logits, K=n_futures, sampler=sampler,
                                                                ordinal=getattr(data, "ordinal", None))
        _heads_batch(out, data, logits, k, bs, head_index, betas, action)
        fut = [predictions[i].reshape(-1, n_nodes, n_futures)[:, LTAMeter.SKIP:] for i in head_index]
        out.add(verb_futures=fut[0], noun_futures=fut[1], futures_sample=_seq_samples(data, bs, fut[0].shape[0], fut[0].device))
    return out.result()


# ---- OSCC: one state-change probability per sequence --------------------------------------------------------------------------------
@torch.no_grad()
def predict_oscc(temporal_graph_model, dataloader, primary_task, other_tasks: Optional[List] = None, graphone=None,
                 late_fusion: bool = True, device: str = "cuda", calibration=None) -> dict:
    """Per sequence: ``sample``, ``pred`` (the first class of the order), ``prob_change`` (the probability of class 1), ``lse`` and,
    when the split has labels, ``label``.  One ``topk_softmax`` launch with k = 2 per batch.  ``calibration``: ``prob_change`` and
    ``lse`` at the fitted temperature, over the raw order."""
    other_tasks = other_tasks or []
    bs = _batch_size(dataloader)
    betas = beta_words(calibration, ("",), device)
    _eval_mode(temporal_graph_model, primary_task, other_tasks, graphone)
    out = _Fields()
    for data in dataloader:
        data = data.to(device)
        logits, _ = _logits(temporal_graph_model, data, primary_task, other_tasks, graphone, late_fusion, needs_batch=True)
        (idx, prob, lse), = ops.topk_softmax([logits], 2, want_prob=True, want_lse=True)
        if betas is not None:
            prob, lse = ops.temp_topk_prob(logits, idx, betas[0], want_lse=True)
        change = torch.where(idx[:, 0] == 1, prob[:, 0], prob[:, 1])
        y = getattr(data, "y", None)
        out.add(sample=_seq_samples(data, bs, idx.shape[0], idx.device), pred=idx[:, 0], prob_change=change, lse=lse,
                label=None if y is None else y.to(torch.int64).view(-1))
    return out.result()


# ---- PNR: one key frame per sequence ------------------------------------------------------------------------------------------------
@torch.no_grad()
def predict_pnr(temporal_graph_model, dataloader, primary_task, other_tasks: Optional[List] = None, graphone=None,
                late_fusion: bool = False, device: str = "cuda") -> dict:
    """Per sequence: ``sample``, ``node`` (the arg-max node's position inside the sequence, ``egk_segment_max_fwd`` on the sigmoid
    of the logits exactly as ``meters.PNRMeter.update`` calls it), ``prob`` (the sigmoid of the winning logit),
    ``frame = start_frame + (end_frame - start_frame) / 16 * node`` in float64 (the meter's formula) and ``pnr_frame`` when the
    split has it."""
    from .models.tasks.oscc import sequence_ptr
    other_tasks = other_tasks or []
    bs = _batch_size(dataloader)
    _eval_mode(temporal_graph_model, primary_task, other_tasks, graphone)
    out = _Fields()
    for data in dataloader:
        data = data.to(device)
        logits, _ = _logits(temporal_graph_model, data, primary_task, other_tasks, graphone, late_fusion, needs_batch=False)
        probs = torch.sigmoid(logits.detach().float())
        ptr = sequence_ptr(data if getattr(data, "ptr32", None) is not None else data.batch)
        n_seg = ptr.numel() - 1
        col = probs.contiguous().view(-1, 1)
        best = torch.empty((n_seg, 1), dtype=torch.float32, device=col.device)
        arg = torch.empty((n_seg, 1), dtype=torch.int32, device=col.device)
        ops._ck(_lib.load().egk_segment_max_fwd(ops._stream(), ops._p(col), ops._p(ptr), ops._p(best), ops._p(arg), n_seg, 1, 0),
                "egk_segment_max_fwd")
        node = (arg.view(-1) - ptr[:-1]).to(torch.int64)
        sf, ef = (torch.as_tensor(v).to(col.device).double() for v in (data.start_frame, data.end_frame))
        pf = getattr(data, "pnr_frame", None)
        out.add(sample=_seq_samples(data, bs, n_seg, col.device), node=node, prob=best.view(-1),
                frame=sf + (ef - sf) / 16 * node.double(), pnr_frame=None if pf is None else torch.as_tensor(pf).to(col.device))
    return out.result()


# ---- the files ----------------------------------------------------------------------------------------------------------------------
def _key(dataset, i: int) -> str:
    fn = getattr(dataset, "sample_id", None)
    return str(fn(int(i))) if callable(fn) else str(int(i))


def _by_sample(sample: torch.Tensor):
    """sample value -> the rows that carry it, in row order."""
    rows = {}
    for r, s in enumerate(sample.tolist()):
        rows.setdefault(s, []).append(r)
    return rows


def to_json(task: str, pred: dict, dataset) -> dict:
    """The JSON document of a task's predictions, keyed by ``dataset.sample_id(i)`` when the dataset has such a method, else
    ``str(i)``.  LTA: {"verb": K lists of Z ints, "noun": K lists of Z ints} (the challenge's shape); AR: the per-node top-k lists;
    OSCC: {"state_change", "prob"}; PNR: {"pnr_frame", "node", "prob"}.  A file with retrieval fields (predict_egopack.py) also gets
    ``"retrieval"`` per sample: {"pos": its nodes, <aux task>: {"index", "dist", "wins"[, "label"]} per node}."""
    doc = {}
    act = [f for f in ("action_topk", "action_logp", "action_prob") if f in pred]  # (action_scores.enabled: per node of the sample)
    if task == "lta":
        for s, v, n in zip(pred["futures_sample"].tolist(), pred["verb_futures"], pred["noun_futures"]):
            doc[_key(dataset, s)] = {"verb": v.t().tolist(), "noun": n.t().tolist()}
        if act:
            for s, rows in _by_sample(pred["sample"]).items():
                doc.setdefault(_key(dataset, s), {}).update({f: pred[f][rows].tolist() for f in act})
    elif task == "ar":
        for s, rows in _by_sample(pred["sample"]).items():
            doc[_key(dataset, s)] = {"pos": pred["pos"][rows].tolist(),
                                     **{f: pred[f][rows].tolist() for f in ("verb_topk", "verb_prob", "noun_topk", "noun_prob", *act)}}
    elif task == "oscc":
        for s, p, c in zip(pred["sample"].tolist(), pred["pred"].tolist(), pred["prob_change"].tolist()):
            doc[_key(dataset, s)] = {"state_change": bool(p == 1), "prob": float(c)}
    elif task == "pnr":
        for s, f, n, p in zip(pred["sample"].tolist(), pred["frame"].tolist(), pred["node"].tolist(), pred["prob"].tolist()):
            doc[_key(dataset, s)] = {"pnr_frame": float(f), "node": int(n), "prob": float(p)}
    else:
        raise ValueError(f"to_json: unknown task {task!r}")
    if "retrieval_sample" in pred:  # (a file of predict_egopack.py: what every node of the sample retrieved, per auxiliary task)
        aux = sorted(f[len("retrieval_"):-len("_index")] for f in pred if f.startswith("retrieval_") and f.endswith("_index"))
        for s, rows in _by_sample(pred["retrieval_sample"]).items():
            entry = {"pos": pred["retrieval_pos"][rows].tolist()}
            for a in aux:
                entry[a] = {f: pred[f"retrieval_{a}_{f}"][rows].tolist() for f in ("index", "dist", "wins", "label")
                            if f"retrieval_{a}_{f}" in pred}
            doc.setdefault(_key(dataset, s), {})["retrieval"] = entry
    return doc


def _class_names(task: str, dataset):
    if task in ("ar", "lta") and getattr(dataset, "class_labels", None) is not None and getattr(dataset, "label_names", None):
        names = dataset.label_names
        return {"verb": list(dataset.class_labels[names.index("verbs")]), "noun": list(dataset.class_labels[names.index("nouns")])}
    if task == "oscc" and getattr(dataset, "oscc_class_labels", None) is not None:
        return list(dataset.oscc_class_labels)
    return None


def action_export(cfg, directory, t: str, calibration=None):
    """(``action`` of the loops, what the document records) for task ``t`` as the ``action_scores:`` block asks: (None, {}) with the
    block off -- the file is then today's.  The record: ``action_topk_k`` and ``action_betas`` ({"verb", "noun"}: the 1 / T the
    joint was scored at, or None: the raw logits)."""
    from . import train as T
    ac = T.action_scores_config(cfg)
    if not ac["enabled"] or t not in ac["tasks"]:
        return None, {}
    _, betas = T.action_scores_betas(cfg, directory, t, calibration=calibration)
    return ({"topk": ac["topk"], "betas": betas},
            {"action_topk_k": ac["topk"], "action_betas": None if betas is None else {"verb": betas[0], "noun": betas[1]}})


def predict_task(t: str, model, dataloader, dataset, task, pc: dict, ls: dict, device, calibration=None, action=None, **fusion) -> dict:
    """The loop of task ``t`` with the entry points' arguments (``pc``: ``predict_config``, ``ls``: ``train.lta_sampling_config``).
    ``calibration``: the task's calibration file (``train.load_calibration``; PNR takes none).  ``fusion``: ``other_tasks`` /
    ``graphone`` / ``late_fusion`` of the loops, for a model with a GraphONE."""
    names = getattr(dataset, "label_names", None)
    heads = (names.index("verbs"), names.index("nouns")) if names else (0, 1)
    if t != "pnr" and calibration:
        fusion = {**fusion, "calibration": calibration}
    if t in ("ar", "lta") and action:  # (``action``: ``action_export``'s first entry)
        fusion = {**fusion, "action": action}
    if t == "ar":
        return predict_heads(model, dataloader, task, k=pc["topk"], device=device, head_index=heads, **fusion)
    if t == "lta":
        from .meters import LTAMeter
        return predict_lta(model, dataloader, task, k=pc["topk"], seed=ls["seed"], n_nodes=int(getattr(dataset, "lta_nodes", LTAMeter.N_NODES)),
                           n_futures=LTAMeter.N_SAMPLES, device=device, head_index=heads, **fusion)
    if t == "oscc":
        return predict_oscc(model, dataloader, task, device=device, **fusion)
    return predict_pnr(model, dataloader, task, device=device, **fusion)


def write_predictions(t: str, pred: dict, dataset, pc: dict, ls: dict, ck: dict, out_dir: Path, seconds: float, **extra):
    """``predictions_<t>.pt`` (and ``.json``): (the saved document, its path).  ``extra``: further entries of the document."""
    doc = {**pred, "topk": pc["topk"], "seed": ls["seed"], "split": pc["split"], "epoch": ck.get("epoch"), **extra}
    names = _class_names(t, dataset)
    if names is not None:
        doc["class_names"] = names
    path = out_dir / f"predictions_{t}.pt"
    torch.save(doc, path)
    if pc["json"]:
        with open(out_dir / f"predictions_{t}.json", "w") as f:
            json.dump(to_json(t, pred, dataset), f)
    n = next(iter(pred.values())).shape[0] if pred else 0
    logger.info("[predict %s] %d rows of split '%s' in %.1f ms -> %s", t, n, pc["split"], seconds * 1e3, path)
    return doc, path


def main(argv=None):
    """``python predict.py resume_from=<checkpoint> enabled_tasks=[ar,lta,oscc,pnr] predict.split=validation predict.topk=5
    predict.out=<dir>``: ``predictions_<task>.pt`` (and ``.json``) per enabled task."""
    from . import train as T
    from .config import instantiate
    from .models.tasks import LTATask, OSCCTask, PNRTask, RecognitionTask
    cfg = T.load_config(argv)
    pc = predict_config(cfg)
    rank, local_rank, world = T.env_ranks()
    if world > 1:
        raise ValueError("predict: one process only (a prediction file lists the split in the single-process batch order; got "
                         f"WORLD_SIZE={world})")
    if not cfg.get("resume_from"):
        raise ValueError("predict: resume_from=<checkpoint> is required (there is nothing to predict with untrained weights)")
    if cfg.get("enable_graphone", False):
        raise ValueError("predict: enable_graphone=True is not served here (this entry point builds no GraphONE): an EgoPack "
                         "checkpoint is exported by predict_egopack.py")
    T.setup_logging(rank)
    T.cap_host_threads(int(cfg.get("host_threads", 8)))
    T.seed_everything(cfg, rank)
    ops.set_compute(cfg.compute)
    enabled = [t for t, w in T.task_weights(cfg).items() if w > 0]
    ls = T.lta_sampling_config(cfg)
    if "lta" in enabled and ls["mode"] != "philox":
        logger.info("lta_sampling.mode=%s: the exported futures come from the seeded sampler all the same (seed %d) -- futures that "
                    "depend on a generator's state are not exported", ls["mode"], ls["seed"])

    dsets = T.build_datasets(cfg, pc["split"])
    loaders = T.build_loaders(cfg, dsets, False, 0, 1)
    device = torch.device("cuda", local_rank)
    torch.cuda.set_device(device)
    store = T.build_feature_store(dsets, device)
    if store is not None:
        loaders = {t: T.ResidentLoader(l, store, device, ops.act_dtype()) for t, l in loaders.items()}
    H = cfg.model.hidden_size
    model = instantiate(cfg.model, input_size=dsets["ar"].features_size, num_segments=cfg.dataset_recognition.num_segments,
                        _recursive_=False).to(device)
    tasks = {
        "ar": RecognitionTask(H, H, heads=dsets["ar"].num_class_labels, dropout=cfg.task_dropout, head_dropout=cfg.task_head_dropout),
        "oscc": OSCCTask(H, cfg.oscc_feat_size, dropout=cfg.task_dropout, head_dropout=cfg.task_head_dropout, loss_func=cfg.oscc_loss),
        "lta": LTATask(H, H, heads=dsets["lta"].num_class_labels, dropout=cfg.task_dropout, head_dropout=cfg.task_head_dropout),
        "pnr": PNRTask(H, H, dropout=cfg.task_dropout, head_dropout=cfg.task_head_dropout),
    }
    for t in tasks.values():
        t.to(device)
    ck = T.load_checkpoint(cfg.resume_from, model, tasks, strict_tasks=True, device=device)  # (weights only: no optimizer is built)
    out_dir = Path(pc["out"]) if pc["out"] else Path(cfg.resume_from).resolve().parent / "predictions"
    out_dir.mkdir(parents=True, exist_ok=True)

    results, paths, seconds = {}, {}, {}
    for t in enabled:
        t0 = time.perf_counter()
        # calibration.predict: the file calibrate.py (or a validation with calibration.mode=temperature) wrote beside the checkpoint
        cal = T.load_calibration(cfg, Path(cfg.resume_from).resolve().parent, t) if t != "pnr" else None
        action, action_doc = action_export(cfg, Path(cfg.resume_from).resolve().parent, t, calibration=cal)
        pred = predict_task(t, model, loaders[t], dsets[t], tasks[t], pc, ls, device, calibration=cal, action=action)
        torch.cuda.synchronize()
        seconds[t] = time.perf_counter() - t0
        results[t], paths[t] = write_predictions(t, pred, dsets[t], pc, ls, ck, out_dir, seconds[t], **temperatures(cal), **action_doc)
    return {"predictions": results, "paths": paths, "out": out_dir, "seconds": seconds, "model": model, "tasks": tasks,
            "datasets": dsets, "loaders": loaders}


if __name__ == "__main__":
    main()
