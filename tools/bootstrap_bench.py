#!/usr/bin/env python3
"""The cluster bootstrap of the validation metrics, timed -- profiles/bootstrap_cost.txt.
1. The launch: ``egk_bootstrap_accumulate`` at the headline validation batch -- 2048 rows (64 sequences of 32 nodes, the cluster of
   a row is its sequence), M = 5 columns (the row count and top-1/2/3/5), the class part on, C = 115 (verbs) and 478 (nouns),
   R = 1000 -- beside ``egk_class_report`` for one head on the same [2048, C] logits, the figure to read it against.  Device time per
   launch from one replay of a captured graph of ``iters`` launches (tools/_timing.py), three rounds, the launches alternating.
2. The pass: ``validate`` over the synthetic AR validation split with B = 64 and the RecognitionMeter, ``bootstrap.replicates`` 0 and
   1000 alternated three times in this one process (host clock, device synchronised before and after; the batches are collated
   before the timed region; one warm-up pass each); ``get_logs()`` -- where the intervals are formed on the host -- timed separately.
Usage: python tools/bootstrap_bench.py [iters] [config overrides, e.g. synthetic_val_samples=4096]"""
import os
import sys
import time

sys.path.insert(0, os.getcwd())
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import torch

from _timing import time_us
from egopack_amd import meters, ops, train as T
from egopack_amd.config import instantiate
from models.tasks import RecognitionTask
from validate import validate

iters = int(sys.argv[1]) if len(sys.argv) > 1 else 20
extra = sys.argv[2:]
dev = torch.device("cuda", 0)
ROWS, SEQ, M, R = 2048, 32, 5, 1000
g = torch.Generator().manual_seed(0)
key = ops.bootstrap_key(0)
cluster = (torch.arange(ROWS) // SEQ).to(dev)
runs = {}
for C in (115, 478):
    logits = torch.randn(ROWS, C, generator=g).to(dev)
    labels = torch.randint(0, C, (ROWS,), generator=g).to(dev)
    rank = meters.label_rank(logits, labels)
    ok = rank >= 0
    num = torch.stack([torch.ones_like(ok), *(ok & (rank < k) for k in meters.KS)], 1).to(torch.int64)
    den = torch.stack([torch.ones_like(ok), *(ok for _ in meters.KS)], 1).to(torch.int64)
    acc = [torch.zeros((R, M), dtype=torch.int64, device=dev) for _ in range(2)]
    cls = [torch.zeros((R, C), dtype=torch.int64, device=dev) for _ in range(2)]
    state = meters._ClassReport(C, dev)
    runs[f"egk_bootstrap_accumulate C={C} (class part on)"] = lambda a=acc, c=cls, n=num, d=den, y=labels: ops.bootstrap_accumulate(
        cluster, n, d, a[0], a[1], key, max_cluster=ROWS // SEQ, label=y, class_col=1, cls_num=c[0], cls_den=c[1])
    runs[f"egk_bootstrap_accumulate C={C} (class part off)"] = lambda a=acc, n=num, d=den: ops.bootstrap_accumulate(
        cluster, n, d, a[0], a[1], key, max_cluster=ROWS // SEQ)
    runs[f"egk_class_report C={C} (one head)"] = lambda z=logits, y=labels, s=state: meters.class_report([(z, y, s)])
for rnd in range(3):
    for name, fn in runs.items():
        print(f"[{ROWS} rows, M = {M}, R = {R}] round {rnd}: {name}: {time_us(fn, iters):.2f} us", flush=True)


class Batches(list):
    """Collated batches that still say what the loader's batch size was (the cluster ids are ordinal * batch_size + sequence)."""
    batch_size = 64


cfg = T.load_config(["batch_size=64", "num_workers=0"] + extra)
T.seed_everything(cfg, 0)
ops.set_compute(cfg.compute)
dv = T.build_datasets(cfg, cfg.validation_split)
dl = T.build_loaders(cfg, dv, False, 0, 1)
H = cfg.model.hidden_size
model = instantiate(cfg.model, input_size=dv["ar"].features_size, num_segments=cfg.dataset_recognition.num_segments, _recursive_=False).to(dev)
task = RecognitionTask(H, H, heads=dv["ar"].num_class_labels, dropout=cfg.task_dropout, head_dropout=cfg.task_head_dropout).to(dev)
batches = Batches(b for b in dl["ar"])
print(f"validation pass: {len(batches)} batches of {batches[0].y.shape[0]} rows, heads {tuple(dv['ar'].num_class_labels)}", flush=True)


def one_pass(replicates):
    kw = dict(bootstrap={"replicates": replicates, "level": 0.95, "seed": 0}) if replicates else {}
    meter = meters.build_meter_for_dataset(dv["ar"], device=dev, **kw)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    validate(0, model, batches, meter, task, device=dev)
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    logs = meter.get_logs()
    torch.cuda.synchronize()
    return (t1 - t0) * 1e3, (time.perf_counter() - t1) * 1e3, len(logs)


for replicates in (0, R):
    one_pass(replicates)  # warm-up
for rnd in range(3):
    for replicates in (0, R):
        v, l, n = one_pass(replicates)
        print(f"round {rnd}: bootstrap.replicates={replicates}: validate {v:.3f} ms, get_logs {l:.3f} ms, {n} keys", flush=True)
