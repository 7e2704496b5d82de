#!/usr/bin/env python3
"""Multi-task pre-training of the temporal backbone (entry point of the reference's main_temporal.py).

    python main_temporal.py k=1 batch_size=16 num_epochs=40 model.temporal_pooling.hidden_size=1024 \
        enabled_tasks=[ar,lta,pnr] save_model=True
    torchrun --nproc-per-node 8 --master-addr 127.0.0.1 main_temporal.py ...      # data parallel

Same configuration keys and training semantics as the reference (zero_grad -> backbone forward for
every enabled task batch -> head -> weight * loss.mean() summed -> backward -> Adam; cosine schedule
stepped per epoch; ``multiloader`` restarts exhausted loaders).  In the last epochs every enabled task is
validated with its meter (``validate`` / ``validate_lta`` / ``validate_pnr`` + ``utils.meters``, reference
main_temporal.py:340-400); W&B logging is not reproduced, checkpoints are written locally with the reference's key
layout."""
from __future__ import annotations

import logging
import time
from pathlib import Path

import torch

from egopack_amd import dist as edist
from egopack_amd import engine, ops, train as T
from egopack_amd.config import instantiate
from egopack_amd.data import multiloader
from models.tasks import LTATask, OSCCTask, PNRTask, RecognitionTask
from utils.meters import build_meter_for_dataset
from validate import validate, validate_lta, validate_pnr

logger = logging.getLogger("main_temporal")
RATE_WARMUP_STEPS = 30  # steps of an epoch left out of its logged steady-state rate (eager steps, the capture, first replays)


def train(epoch, step: engine.MTLStep, loaders, weights, device="cuda", store=None):
    """One epoch (reference main_temporal.train :49-134)."""
    step.model.train()
    for t in step.tasks.values():
        t.train()
    for c in step.criteria.values():
        c.train()  # (class-balance vectors apply to the training loss only)
    order = ("ar", "lta", "oscc", "pnr")
    it = 0
    step.loss_sums()  # (clears the per-task loss sums: they accumulate inside the step, on the device, until the epoch ends)
    if step.optimizer.clipping:
        step.grad_norm_stats()  # (and the gradient-norm statistics of grad_clip_norm)
    for l in loaders.values():
        if getattr(l, "mixup", None):
            l.mix_epoch = epoch  # (mixup: the draws are keyed by the epoch -- a resumed run draws what the uninterrupted one draws)
    hosts = (dict(zip(order, batch)) for batch in multiloader([loaders[t] for t in order], [weights[t] for t in order]))
    # batch i + 1 is built and copied to the device (staging thread, copy stream) while step i runs
    mark = None  # (iteration, wall clock, sequences so far) once the eager steps and the capture are behind: steady-state rate
    seqs = 0
    for batches, merged in engine.StagedBatches(hosts, device, order, fused=step.fused, store=store, dtype=ops.act_dtype(), step=step):
        step.train_step(batches, merged)  # eager for the first steps, then the captured step (no launch of this loop between two)
        seqs += sum(int(b.num_graphs) for b in batches.values() if b is not None)
        it += 1
        if it == RATE_WARMUP_STEPS and torch.cuda.is_available():
            torch.cuda.synchronize()
            mark = (it, time.perf_counter(), seqs)
    if mark is not None and it > mark[0]:
        torch.cuda.synchronize()
        dt = time.perf_counter() - mark[1]
        logger.info("epoch %d: steady state %.3f ms/step, %.0f clip-seqs/s on this rank (%d steps after the first %d); "
                    "device memory %.0f MB allocated, %.0f MB reserved", epoch, dt * 1e3 / (it - mark[0]), (seqs - mark[2]) / dt,
                    it - mark[0], mark[0], torch.cuda.memory_allocated() / 2 ** 20, torch.cuda.memory_reserved() / 2 ** 20)
    logger.info("epoch %d: %d iterations, train loss %s", epoch, it,
                {t: round(s_ / max(n_, 1), 4) for t, (s_, n_) in step.loss_sums().items() if n_})
    T.log_grad_norms(logger, epoch, step)
    T.log_trust_ratios(logger, epoch, step)  # (LAMB: min / median / max trust ratio)
    T.log_mixup(logger, epoch, loaders)  # (the mean lambda per mixed task; nothing with the feature off)
    T.log_edge_drop(logger, epoch, step.model)  # (the configured p and flags; nothing with the feature off)
    T.log_task_weighting(logger, epoch, step)  # (s_t and w_t exp(-s_t), or the manual scales; nothing with the feature off)
    lc = getattr(step, "loop_counts", None)
    if lc is not None:  # how many steps replayed the captured graph and how many ran eagerly (shape changes, warm-up)
        logger.info("epoch %d: %d steps replayed the captured step, %d ran eagerly", epoch, lc["replayed"], lc["eager"])
        step.loop_counts = {"replayed": 0, "eager": 0}
    return it


@torch.no_grad()
def validate_losses(step: engine.MTLStep, loaders, device="cuda"):
    step.model.eval()
    for t in step.tasks.values():
        t.eval()
    for c in step.criteria.values():
        c.eval()  # (validation losses are the plain cross entropy whatever ``class_balance`` says: curves compare across runs)
    out = {}
    for t in step.enabled:
        s, n = 0.0, 0
        for b in loaders[t]:
            _, vectors, _ = step.losses({t: b.to(device)})
            s += float(vectors[t].sum())
            n += vectors[t].numel()
        if torch.distributed.is_initialized() and torch.distributed.get_world_size() > 1:  # batch-sharded split
            tot = torch.tensor([s, n], dtype=torch.float64, device=device)
            torch.distributed.all_reduce(tot)
            s, n = float(tot[0]), int(tot[1])
        out[t] = s / max(n, 1)
    return out


def validate_metrics(epoch, model, tasks, enabled, dsets_val, loaders, device="cuda", sampler=None, report=None, reports=None,
                     calibrations=None, bootstraps=None, split=None):
    """Task metrics of every enabled task (reference main_temporal.py:340-400).  ``sampler``: the seeded sampler of the LTA futures
    (``T.build_lta_sampler``, lta_sampling.mode=philox); None: torch's generator.  ``report``: task -> the meter's per-class report
    arguments (``T.class_report_meter_args``, log_confusion_matrices) and its temperature-fit arguments
    (``T.calibration_meter_args``, calibration.mode) and its action-score arguments (``T.action_scores_meter_args``); ``reports``: a dict that receives every task's tables; ``calibrations``: a dict
    that receives every task's fitted temperatures (``BaseMeter.temperature_fit``); ``bootstraps``: a dict that receives every
    task's bootstrap tables (``BaseMeter.bootstrap_tables``, bootstrap.replicates > 0; ``split``: the split's name, stored there)."""
    out = {}
    for t in enabled:
        meter = build_meter_for_dataset(dsets_val[t], device=device, **(report(t) if report else {}))
        if t == "lta":
            validate_lta(model, loaders[t], meter, tasks[t], device=device, sampler=sampler)
        elif t == "pnr":
            validate_pnr(model, loaders[t], meter, tasks[t], device=device)
        else:
            validate(epoch, model, loaders[t], meter, tasks[t], device=device)
        meter.all_reduce()  # ranks validated disjoint batches of the split: every rank ends with the totals
        for line in meter.print_logs():
            logger.info("[val %s] %s", t, line)
        out[t] = {k: v for k, v in meter.get_logs().items() if isinstance(v, (int, float))}
        if reports is not None and meter.reports:
            reports[t] = meter.report_tables()
        if calibrations is not None and meter.temp_store is not None:
            calibrations[t] = meter.temperature_fit()
        if bootstraps is not None and meter.boot is not None:
            bootstraps[t] = meter.bootstrap_tables(split)
    return out


def main(argv=None):
    cfg = T.load_config(argv)
    rank, local_rank, world = T.env_ranks()
    T.setup_logging(rank)
    T.cap_host_threads(int(cfg.get("host_threads", 8)))
    T.seed_everything(cfg, rank)
    ops.set_compute(cfg.compute)
    weights = T.task_weights(cfg)
    logger.info("task weights: %s", weights)
    artifact = f"{cfg.artifact_prefix}_" + "-".join(sorted(t for t, w in weights.items() if w > 0))

    # datasets, loaders and their collation processes come first: nothing has touched the GPU yet, so the workers are a
    # plain fork of a process without HIP state (data.BatchLoader.start_workers)
    T.check_mixup(cfg, enable_graphone=bool(cfg.get("enable_graphone", False)))  # (mixup with class_balance / ce_shape / GraphONE: refused here)
    T.bootstrap_config(cfg)  # (an unknown key of the bootstrap block is refused here, by name)
    edge_drop = T.check_edge_drop(cfg, enable_graphone=bool(cfg.get("enable_graphone", False)))  # (edge_drop.p > 0 with GraphONE: refused here)
    dsets_train, dsets_val = T.build_datasets(cfg, "train"), T.build_datasets(cfg, cfg.validation_split)
    assert len({d.features_size for d in dsets_train.values()}) == 1, "all tasks must share the input feature size"
    dl_train = T.build_loaders(cfg, dsets_train, True, rank, world)
    dl_val = T.build_loaders(cfg, dsets_val, False, rank, world)  # batch-sharded; meters are summed across ranks
    T.start_loader_workers(dl_train)
    rank, local_rank, world = edist.init_from_env()
    device = torch.device("cuda", local_rank)
    torch.cuda.set_device(device)
    # datasets that index a device-resident feature table (dataset_*=synthetic_resident; the reference's .npy files
    # loaded into HBM): one table per split, the training step gathers its rows on the device, evaluation batches get
    # theirs through an adapter
    store, store_val = T.build_feature_store(dsets_train, device), T.build_feature_store(dsets_val, device)
    if store_val is not None:
        dl_val = {t: T.ResidentLoader(l, store_val, device, ops.act_dtype()) for t, l in dl_val.items()}

    H = cfg.model.hidden_size
    model = instantiate(cfg.model, input_size=dsets_train["ar"].features_size,
                        num_segments=cfg.dataset_recognition.num_segments, _recursive_=False).to(device)
    T.apply_edge_drop(model, edge_drop)  # (DropEdge of the SAGE means in training mode; p = 0: the attribute stays None)
    tasks = {
        "ar": RecognitionTask(H, H, heads=dsets_train["ar"].num_class_labels, dropout=cfg.task_dropout, head_dropout=cfg.task_head_dropout),
        "oscc": OSCCTask(H, cfg.oscc_feat_size, dropout=cfg.task_dropout, head_dropout=cfg.task_head_dropout, loss_func=cfg.oscc_loss),
        "lta": LTATask(H, H, heads=dsets_train["lta"].num_class_labels, dropout=cfg.task_dropout, head_dropout=cfg.task_head_dropout),
        "pnr": PNRTask(H, H, dropout=cfg.task_dropout, head_dropout=cfg.task_head_dropout),
    }
    for t in tasks.values():
        t.to(device)
    wd = cfg.optimizer.weight_decay
    params = [*model.configure_optimizers(wd), *(p for t in ("ar", "oscc", "lta", "pnr") for p in tasks[t].configure_optimizers(wd))]
    if world > 1:
        for p in params:  # same start everywhere (seeded identically; broadcast makes it unconditional)
            torch.distributed.broadcast(p.data, src=0)
    # task_weighting: the balance between the tasks, adjustable (manual) or learned (uncertainty) inside the captured step
    tw_mode = T.task_weighting_config(cfg)["mode"]
    log_var = T.build_task_weighting(cfg, [t for t in engine.MTLStep.order if weights.get(t, 0) > 0 and t in tasks], device)
    if world > 1 and log_var is not None:
        torch.distributed.broadcast(log_var.log_var.data, src=0)
    optimizer = T.build_optimizer(cfg, T.build_param_groups(cfg, model, tasks), layout_order=params, log_var=log_var)
    T.log_param_groups(logger, optimizer)
    T.log_optimizer_state(logger, optimizer)
    scheduler = T.build_scheduler(cfg, optimizer)
    compress = str(cfg.get("grad_compress", "none"))  # element type of the gradient all-reduce: none (f32) | bf16
    sync = edist.GradSync(world, compress=compress) if world > 1 else None
    dry = int(cfg.get("exchange_dry_run", 0))
    if world == 1 and dry > 1:
        # development / test knob: run the N-rank exchange path (conversion, RCCL all-reduce on a 1-rank group, 1/N gradient
        # scale, staged backward) on ONE GPU -- everything of the N-GPU step except the peers' contributions
        edist.init_single_rank_group()  # (no-op when the caller already owns a group; free rendezvous port otherwise)
        sync = edist.GradSync(dry, compress=compress)
    # class_balance: per-class weights / logit offsets of the AR and LTA heads from the label counts of the whole training split
    balance = T.build_class_balance(cfg, dsets_train, device=device)
    T.log_class_balance(logger, cfg, balance)
    # ce_shape: LDAM margins from the same counts, the focal exponent, deferred re-weighting of the class weights
    shape = T.build_ce_shape(cfg, dsets_train, device=device, class_balance=balance)
    T.log_ce_shape(logger, cfg, shape)
    # pnr_balance: pos / neg / gamma of the PNR head's BCE from the positive and negative node counts of the whole training split
    pnr_balance = T.build_pnr_balance(cfg, dsets_train, tasks=[t for t, w in weights.items() if w > 0])
    T.log_pnr_balance(logger, cfg, pnr_balance)
    step = engine.MTLStep(model, tasks, T.build_criteria(dsets_train, balance, pnr_balance, shape), weights, optimizer,
                          fused_backbone=cfg.fused_backbone, sync=sync, task_weighting=tw_mode, log_var=log_var)
    step.use_graph = bool(cfg.get("use_graph", True))
    step.exact_graph_ln = bool(cfg.get("exact_graph_ln", False))  # several ranks: graph-LN statistics over the GLOBAL batch

    first_epoch = 1
    ckpt_path = Path(cfg.checkpoint_dir) / artifact / "checkpoint.pth"
    if cfg.resume_from:  # continue an interrupted run: weights, Adam moments, schedule, epoch counter
        ck = T.load_checkpoint(cfg.resume_from, model, tasks, strict_tasks=True, device=device, optimizer=optimizer,
                               scheduler=scheduler, loaders=dl_train)
        first_epoch = int(ck.get("epoch", 0)) + 1
        T.check_class_balance(logger, ck, cfg, balance)  # (rebuilt above; compared bit for bit with the stored vectors)
        T.check_pnr_balance(logger, ck, cfg, pnr_balance)  # (likewise the PNR scalars)
        T.load_task_weighting(logger, ck, step)  # (log_var / the manual scales; without the entry: s = 0, one log line)
        logger.info("resumed from %s at epoch %d", cfg.resume_from, first_epoch)
    sampler = T.build_lta_sampler(cfg)  # (lta_sampling.mode=philox: the LTA futures from the seeded launch; None: torch's generator)
    # log_confusion_matrices: the per-class report of the validation meters; the training labels are counted once, here
    train_counts = T.class_report_train_counts(cfg, dsets_train, tasks=step.enabled)
    seen_pairs = T.action_scores_seen(cfg, dsets_train, tasks=step.enabled)  # (action_scores.seen_split: the training split's pairs, once)
    report, reports = (lambda t: {**T.class_report_meter_args(cfg, train_counts, t), **T.calibration_meter_args(cfg, t),
                                  **T.action_scores_meter_args(cfg, t, seen_pairs), **T.bootstrap_meter_args(cfg, t)}), {}
    bootstraps = {}  # (bootstrap.replicates > 0: task -> the accumulators and replicate values of the last validation)
    calibrations = {}  # (calibration.mode=temperature: task -> the temperatures fitted in the last validation)
    metrics = None
    for epoch in range(first_epoch, cfg.num_epochs + 1):
        # (ce_shape.reweight_after: the class-weight buffers are rewritten in place -- a captured step keeps its pointers; after a
        #  resume the side follows the checkpoint's epoch)
        T.apply_reweight(logger, cfg, balance, step.criteria, epoch)
        train(epoch, step, dl_train, weights, device, store=store)
        scheduler.step()
        logger.info("learning rate -> %.6g", scheduler.get_last_lr()[0])
        if cfg.save_model and cfg.get("save_every", 0) and epoch % cfg.save_every == 0 and sync is not None:
            sync.gather_moments(optimizer)  # (sharded update: a collective, every rank; a no-op otherwise)
        if cfg.save_model and cfg.get("save_every", 0) and epoch % cfg.save_every == 0 and rank == 0:
            T.save_checkpoint(ckpt_path, model, tasks, epoch, optimizer=optimizer, scheduler=scheduler, loaders=dl_train,
                              save_ema=T.ema_saved(cfg), class_balance=T.class_balance_state(cfg, balance),
                              pnr_balance=T.pnr_balance_state(cfg, pnr_balance), task_weighting=T.task_weighting_state(cfg, step))
        if epoch >= cfg.num_epochs - 5:  # all ranks: the validation split is sharded by batch
            T.log_validation_weights(logger, cfg, optimizer, epoch)
            with T.ema_scope(cfg, optimizer):  # (ema.decay > 0 and ema.validate: the averaged weights are scored)
                logger.info("validation losses: %s", validate_losses(step, dl_val, device))
                metrics = validate_metrics(epoch, model, tasks, step.enabled, dsets_val, dl_val, device, sampler=sampler,
                                           report=report, reports=reports, calibrations=calibrations, bootstraps=bootstraps,
                                           split=str(cfg.validation_split))
    if cfg.num_epochs < first_epoch and cfg.get("validate_untrained", False):  # (num_epochs=0: metrics of the initial state)
        T.log_validation_weights(logger, cfg, optimizer, 0)
        with T.ema_scope(cfg, optimizer):
            metrics = validate_metrics(0, model, tasks, step.enabled, dsets_val, dl_val, device, sampler=sampler, report=report,
                                       reports=reports, calibrations=calibrations, bootstraps=bootstraps, split=str(cfg.validation_split))
    if rank == 0:
        T.save_class_reports(logger, cfg, ckpt_path.parent, reports)  # (class_report.save: the tables of the last validation)
        T.save_calibration(logger, cfg, ckpt_path.parent, calibrations)  # (calibration.save: the temperatures of the last validation)
        T.save_bootstraps(logger, cfg, ckpt_path.parent, bootstraps)  # (bootstrap.save: the replicates of the last validation)
    if cfg.save_model and sync is not None:
        sync.gather_moments(optimizer)
    if cfg.save_model and rank == 0:
        T.save_checkpoint(ckpt_path, model, tasks, cfg.num_epochs, optimizer=optimizer, scheduler=scheduler, loaders=dl_train,
                          save_ema=T.ema_saved(cfg), class_balance=T.class_balance_state(cfg, balance),
                          pnr_balance=T.pnr_balance_state(cfg, pnr_balance), task_weighting=T.task_weighting_state(cfg, step))
    if world > 1:
        torch.distributed.destroy_process_group()
    # (callers that drive main() from Python -- the tests -- get the last validation metrics and the trained modules)
    return {"metrics": metrics, "model": model, "tasks": tasks, "step": step, "loaders": dl_train, "val_datasets": dsets_val,
            "val_loaders": dl_val, "optimizer": optimizer}


if __name__ == "__main__":
    main()
