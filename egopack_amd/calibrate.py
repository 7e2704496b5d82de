"""Temperature calibration of a trained checkpoint: one validation pass over ``validation_split`` per enabled task
that takes a temperature (AR, LTA, OSCC), the fit on the device over the logits the meters scored (include/egopack_calibrate.h,
egopack_amd/calibration.py), and ``calibration_<task>.pt`` beside the checkpoint -- where predict.py / predict_egopack.py look for
it (``calibration.predict``).  ``calibration.mode`` is taken as ``temperature`` whatever the config says: that is what this entry
point is for.  No weight, no prediction and no accuracy changes; the meters' lines show the NLL and the calibration error before
and after."""
from __future__ import annotations

import logging
from pathlib import Path

import torch

from . import ops
from .meters import build_meter_for_dataset
from .validate import validate, validate_lta

logger = logging.getLogger(__name__)


def calibrate_tasks(cfg, model, tasks, dsets, loaders, enabled, device, sampler=None, graphone=None, aux_order=None,
                    late_fusion=None) -> dict:
    """task -> ``calibration.fit``'s result (with the cross-fitted scores) for every task of ``enabled`` that takes a temperature:
    the validation loops of the entry points with a meter that stores what it scores.  ``graphone`` / ``aux_order`` /
    ``late_fusion``: the EgoPack form (``main_egopack.validate_metrics``)."""
    from . import train as T
    fits = {}
    for t in enabled:
        args = T.calibration_meter_args(cfg, t)
        if not args:
            continue
        meter = build_meter_for_dataset(dsets[t], device=device, **args)
        fusion = {}
        if graphone is not None:
            fusion = dict(other_tasks=[tasks[o] for o in aux_order[t] if o in graphone.task_labels], graphone=graphone,
                          late_fusion=late_fusion)
        if t == "lta":
            validate_lta(model, loaders[t], meter, tasks[t], device=device, sampler=sampler, **fusion)
        else:
            validate(0, model, loaders[t], meter, tasks[t], device=device, **fusion)
        for line in meter.print_logs():
            logger.info("[calibrate %s] %s", t, line)
        fits[t] = meter.temperature_fit()
    return fits


def main(argv=None):
    """``python calibrate.py resume_from=<checkpoint> enabled_tasks=[ar,lta,oscc]`` (a checkpoint of main_temporal.py), or with
    ``enable_graphone=True`` a checkpoint of main_egopack.py: ``calibration_<task>.pt`` per task beside the checkpoint."""
    from . import train as T
    from .config import instantiate
    from .models.tasks import LTATask, OSCCTask, PNRTask, RecognitionTask
    cfg = T.load_config(argv)
    cfg["calibration"] = type(cfg)({**dict(cfg.get("calibration") or {}), "mode": "temperature"})
    cal = T.calibration_config(cfg)
    rank, local_rank, world = T.env_ranks()
    if world > 1:
        raise ValueError(f"calibrate: one process only (got WORLD_SIZE={world}); a sharded validation with calibration.mode=temperature "
                         "fits over all ranks' rows")
    if not cfg.get("resume_from"):
        raise ValueError("calibrate: resume_from=<checkpoint> is required (there is nothing to calibrate with untrained weights)")
    egopack = bool(cfg.get("enable_graphone", False))
    T.setup_logging(rank)
    T.cap_host_threads(int(cfg.get("host_threads", 8)))
    T.seed_everything(cfg, rank)
    ops.set_compute(cfg.compute)
    enabled = [t for t, w in T.task_weights(cfg).items() if w > 0 and t in cal["tasks"]]
    if not enabled:
        raise ValueError(f"calibrate: none of the enabled tasks takes a temperature (calibration.tasks = {cal['tasks']})")

    dsets = T.build_datasets(cfg, cfg.validation_split)
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
    graphone, fusion = None, {}
    if egopack:  # (as main_egopack.main and predict_egopack.main build them)
        from .models.graphONE.graphONE import GraphONE
        from .predict_egopack import AUX_ORDER, inspect_checkpoint
        bank_shapes = inspect_checkpoint(cfg.resume_from)
        tasks = {
            "ar": RecognitionTask(H, H, heads=dsets["ar"].num_class_labels, aux_tasks=("oscc", "lta", "pnr"), **kw),
            "oscc": OSCCTask(H, H, aux_tasks=("ar", "lta", "pnr"), average_logits=True, **kw),
            "lta": LTATask(H, H, heads=dsets["lta"].num_class_labels, aux_tasks=("ar", "oscc", "pnr"), **kw),
            "pnr": PNRTask(H, H, aux_tasks=("ar", "oscc", "lta"), **kw),
        }
        graphone = GraphONE({t: torch.zeros(shape) for t, shape in bank_shapes.items()}, **cfg.graphone).to(device)
        fusion = dict(graphone=graphone, aux_order=AUX_ORDER, late_fusion=cfg.late_fusion)
    else:
        tasks = {
            "ar": RecognitionTask(H, H, heads=dsets["ar"].num_class_labels, **kw),
            "oscc": OSCCTask(H, cfg.oscc_feat_size, loss_func=cfg.oscc_loss, **kw),
            "lta": LTATask(H, H, heads=dsets["lta"].num_class_labels, **kw),
            "pnr": PNRTask(H, H, **kw),
        }
    for t in tasks.values():
        t.to(device)
    T.load_checkpoint(cfg.resume_from, model, tasks, strict_tasks=True, device=device, **({"graphone": graphone} if egopack else {}))
    fits = calibrate_tasks(cfg, model, tasks, dsets, loaders, enabled, device, sampler=T.build_lta_sampler(cfg), **fusion)
    directory = Path(cfg.resume_from).resolve().parent
    paths = T.save_calibration(logger, cfg, directory, fits)
    return {"calibration": fits, "paths": paths, "model": model, "tasks": tasks, "datasets": dsets, "loaders": loaders}


if __name__ == "__main__":
    main()
