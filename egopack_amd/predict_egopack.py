"""Prediction export of an EgoPack checkpoint, with what every node retrieved.

``main`` is the entry point behind ``python predict_egopack.py enable_graphone=True resume_from=<checkpoint of main_egopack.py> ...``.
It builds what ``main_egopack.main`` builds -- the backbone, the task heads with their auxiliary classifiers, a GraphONE over banks
of the checkpoint's shapes -- loads the checkpoint into all of it (no prototype-bank pass), and runs the loops of
``egopack_amd.predict`` as they are, every enabled task with the auxiliary tasks and the GraphONE ``main_egopack.validate_metrics``
gives it: a prediction is made from the very logits the EgoPack validation scores.

The loops are not told about the retrieval.  ``RetrievalTap`` stands where they expect the GraphONE and the loader: it remembers
the batch the loader handed out, runs the real ``interact`` inside ``GraphONE.record_retrieval`` and follows it with ONE
``egk_retrieval_report`` launch for all auxiliary tasks, on the tensors the interaction used.  Per node and auxiliary task ``a``:
``retrieval_<a>_index`` int64 [rows, k] (the prototypes, nearest first), ``retrieval_<a>_dist`` f32 [rows, k] (their distances),
``retrieval_<a>_wins`` int32 [rows, k + 1] (channels of the first stage's max aggregation each prototype, and last the node itself,
supplies) and, when the bank rows' labels are known, ``retrieval_<a>_label`` int64 [rows, k, 2] (verb, noun);
``retrieval_sample`` / ``retrieval_pos`` are the rows' provenance, as ``sample`` / ``pos`` of ``egopack_amd.predict``."""
from __future__ import annotations

import logging
import time
from pathlib import Path

import torch

from . import ops
from . import predict as P
from .graphone import bank_labels

logger = logging.getLogger("predict_egopack")

PREDICT_EGOPACK_DEFAULTS = {"retrieval": True, "labels": True}
# other_tasks of every task's validation call, in order (main_egopack.AUX_ORDER: tests/test_retrieval_cpu.py holds the two equal)
AUX_ORDER = {"ar": ("lta", "oscc", "pnr"), "oscc": ("ar", "lta", "pnr"), "lta": ("ar", "oscc", "pnr"), "pnr": ("ar", "lta", "oscc")}
BANK_BATCH = 256  # the prototype-bank pass of main_egopack.main: the AR training split, batch 256, unshuffled, drop_last


def predict_egopack_config(cfg) -> dict:
    """The ``predict_egopack:`` block with its defaults filled in; an unknown key is a ValueError naming it."""
    raw = cfg.get("predict_egopack") if hasattr(cfg, "get") else None
    raw = dict(raw or {})
    unknown = set(raw) - set(PREDICT_EGOPACK_DEFAULTS)
    if unknown:
        raise ValueError(f"predict_egopack: unknown key(s) {sorted(unknown)} ({', '.join(PREDICT_EGOPACK_DEFAULTS)})")
    return {k: bool(v) for k, v in {**PREDICT_EGOPACK_DEFAULTS, **raw}.items()}


class RetrievalTap:
    """The GraphONE and the loader as a prediction loop sees them (``eval`` / ``interact``; iteration, ``loader``), with the
    retrieval of every batch collected on the side.  ``interact`` returns what the GraphONE returns."""

    def __init__(self, graphone, loader):
        self.graphone, self.loader = graphone, loader
        self.task_labels = graphone.task_labels
        self.fields, self.current, self.bs = P._Fields(), None, P._batch_size(loader)

    def __iter__(self):
        for data in self.loader:
            self.current = data
            yield data

    def __len__(self):
        return len(self.loader)

    def eval(self):
        self.graphone.eval()
        return self

    def interact(self, features):
        g = self.graphone
        with g.record_retrieval() as kept:
            out = g.interact(features)
        aux = list(features)
        got = [kept[a] for a in aux]
        reports = ops.retrieval_report([r["features"] for r in got], [r["features_act"] for r in got], [g.embeddings[a].weight for a in aux],
                                       [r["nn"] for r in got], g.distance_func)  # every auxiliary task, one launch
        data = self.current
        self.fields.add(retrieval_sample=P._node_samples(data, self.bs), retrieval_pos=data.pos)
        for a, r, (dist, wins) in zip(aux, got, reports):
            self.fields.add(**{f"retrieval_{a}_index": r["nn"], f"retrieval_{a}_dist": dist, f"retrieval_{a}_wins": wins})
        return out

    def result(self, labels=None, n_nouns: int = 0) -> dict:
        """The collected fields on the host; ``labels`` (``bank_labels``): also the (verb, noun) of every retrieved prototype."""
        out = self.fields.result()
        if labels is not None:
            for f in [f for f in out if f.endswith("_index")]:
                lab = labels[out[f]]
                out[f[:-len("_index")] + "_label"] = torch.stack([lab // n_nouns, lab % n_nouns], dim=-1)
        return out


def inspect_checkpoint(path) -> dict:
    """{task: (K, H)} of the prototype banks of the checkpoint, read on the host; a ValueError when it holds no GraphONE."""
    ck = torch.load(path, map_location="cpu", weights_only=False)
    state = ck.get("graphone") if isinstance(ck, dict) else None
    if not state:
        raise ValueError(f"predict_egopack: {path} has no 'graphone' entry (a checkpoint of main_egopack.py is expected; a checkpoint "
                         "of main_temporal.py is exported by predict.py)")
    banks = {k[len("embeddings."):-len(".weight")]: tuple(v.shape) for k, v in state.items()
             if k.startswith("embeddings.") and k.endswith(".weight")}
    if not banks:
        raise ValueError(f"predict_egopack: the 'graphone' entry of {path} holds no prototype bank (embeddings.<task>.weight)")
    return banks


def main(argv=None):
    """``python predict_egopack.py enable_graphone=True resume_from=<EgoPack checkpoint> enabled_tasks=[oscc] graphone.k=4 ...
    predict.out=<dir>``: ``predictions_<task>.pt`` (and ``.json``) per enabled task, with the retrieval fields."""
    from . import train as T
    from .config import instantiate
    from .data import build_dataloader
    from .models.graphONE.graphONE import GraphONE
    from .models.tasks import LTATask, OSCCTask, PNRTask, RecognitionTask
    cfg = T.load_config(argv)
    pc, ec = P.predict_config(cfg), predict_egopack_config(cfg)
    rank, local_rank, world = T.env_ranks()
    if world > 1:
        raise ValueError("predict_egopack: one process only (a prediction file lists the split in the single-process batch order; got "
                         f"WORLD_SIZE={world})")
    if not cfg.get("resume_from"):
        raise ValueError("predict_egopack: resume_from=<checkpoint> is required (there is nothing to predict with untrained weights)")
    if not cfg.get("enable_graphone", False):
        raise ValueError("predict_egopack: enable_graphone=True is required (a model without a GraphONE is exported by predict.py)")
    bank_shapes = inspect_checkpoint(cfg.resume_from)  # (before any dataset or device is touched)
    T.setup_logging(rank)
    T.cap_host_threads(int(cfg.get("host_threads", 8)))
    T.seed_everything(cfg, rank)
    ops.set_compute(cfg.compute)
    enabled = [t for t, w in T.task_weights(cfg).items() if w > 0]
    ls = T.lta_sampling_config(cfg)

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
    kw = dict(dropout=cfg.task_dropout, head_dropout=cfg.task_head_dropout)
    tasks = {  # (as main_egopack.main builds them)
        "ar": RecognitionTask(H, H, heads=dsets["ar"].num_class_labels, aux_tasks=("oscc", "lta", "pnr"), **kw),
        "oscc": OSCCTask(H, H, aux_tasks=("ar", "lta", "pnr"), average_logits=True, **kw),
        "lta": LTATask(H, H, heads=dsets["lta"].num_class_labels, aux_tasks=("ar", "oscc", "pnr"), **kw),
        "pnr": PNRTask(H, H, aux_tasks=("ar", "oscc", "lta"), **kw),
    }
    for t in tasks.values():
        t.to(device)
    graphone = GraphONE({t: torch.zeros(shape) for t, shape in bank_shapes.items()}, **cfg.graphone).to(device)
    ck = T.load_checkpoint(cfg.resume_from, model, tasks, strict_tasks=True, device=device, graphone=graphone)
    out_dir = Path(pc["out"]) if pc["out"] else Path(cfg.resume_from).resolve().parent / "predictions"
    out_dir.mkdir(parents=True, exist_ok=True)

    labels, n_nouns = None, 0
    if ec["retrieval"] and ec["labels"]:
        n_classes = tuple(c[-1].out_features for c in tasks["ar"].classifiers)
        ar_train = T.build_datasets(cfg, "train")["ar"]
        labels = bank_labels(build_dataloader(ar_train, BANK_BATCH, False, cfg.num_workers, True, cfg.seed, rank=0, world_size=1,
                                              shard="batches"), n_classes)
        n_nouns = n_classes[1]
        rows = {t: shape[0] for t, shape in bank_shapes.items()}
        if any(K != labels.numel() for K in rows.values()):
            logger.warning("the AR training split gives %d labels, the banks have %s rows: the indices are exported without labels "
                           "(the banks were built from another split?)", labels.numel(), rows)
            labels = None

    results, paths, seconds = {}, {}, {}
    for t in enabled:
        others = [tasks[o] for o in AUX_ORDER[t] if o in graphone.task_labels]  # (main_egopack.validate_metrics)
        tap = RetrievalTap(graphone, loaders[t]) if ec["retrieval"] and others else None
        t0 = time.perf_counter()
        # calibration.predict: the file calibrate.py enable_graphone=True wrote beside the checkpoint (PNR takes none)
        cal = T.load_calibration(cfg, Path(cfg.resume_from).resolve().parent, t) if t != "pnr" else None
        action, action_doc = P.action_export(cfg, Path(cfg.resume_from).resolve().parent, t, calibration=cal)  # (action_scores)
        pred = P.predict_task(t, model, loaders[t] if tap is None else tap, dsets[t], tasks[t], pc, ls, device, calibration=cal,
                              action=action, other_tasks=others, graphone=graphone if tap is None else tap, late_fusion=cfg.late_fusion)
        if tap is not None:
            pred.update(tap.result(labels, n_nouns))
        torch.cuda.synchronize()
        seconds[t] = time.perf_counter() - t0
        extra = {"retrieval_tasks": [o.name for o in others], "retrieval_k": int(graphone.k),
                 "retrieval_distance": graphone.distance_func} if tap is not None else {}
        extra.update(P.temperatures(cal))
        extra.update(action_doc)
        results[t], paths[t] = P.write_predictions(t, pred, dsets[t], pc, ls, ck, out_dir, seconds[t], **extra)
    return {"predictions": results, "paths": paths, "out": out_dir, "seconds": seconds, "model": model, "tasks": tasks,
            "graphone": graphone, "datasets": dsets, "loaders": loaders, "bank_labels": labels}


if __name__ == "__main__":
    main()
