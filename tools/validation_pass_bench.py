#!/usr/bin/env python3
"""One validation pass of the AR task, timed: ``validate`` over the synthetic validation split with B = 64 and the RecognitionMeter,
with the per-class report (``log_confusion_matrices``) off or on -- profiles/class_report.txt.  The batches are
collated before the timed region; two warm-up passes, then ``repeats`` timed ones (host clock, device synchronised before and
after); ``get_logs()`` is timed separately.  Runs on the tree it is started in (also one without the report, with ``0``).
Usage: python tools/validation_pass_bench.py <0|1> [repeats] [config overrides, e.g. synthetic_val_samples=4096]"""
import os
import sys
import time

sys.path.insert(0, os.getcwd())
import torch

from egopack_amd import ops, train as T
from egopack_amd.config import instantiate
from models.tasks import RecognitionTask
from utils.meters import build_meter_for_dataset
from validate import validate

report, reps = int(sys.argv[1]), int(sys.argv[2]) if len(sys.argv) > 2 else 5
extra = sys.argv[3:]
cfg = T.load_config(["batch_size=64", "num_workers=0"] + extra + (["log_confusion_matrices=true"] if report else []))
T.seed_everything(cfg, 0)
ops.set_compute(cfg.compute)
dv = T.build_datasets(cfg, cfg.validation_split)
dl = T.build_loaders(cfg, dv, False, 0, 1)
dev = torch.device("cuda", 0)
H = cfg.model.hidden_size
model = instantiate(cfg.model, input_size=dv["ar"].features_size, num_segments=cfg.dataset_recognition.num_segments, _recursive_=False).to(dev)
task = RecognitionTask(H, H, heads=dv["ar"].num_class_labels, dropout=cfg.task_dropout, head_dropout=cfg.task_head_dropout).to(dev)
kw = {}
if report:
    dt = T.build_datasets(cfg, "train")
    tc = T.class_report_train_counts(cfg, dt, tasks=["ar"])
    kw = T.class_report_meter_args(cfg, tc, "ar")
batches = [b for b in dl["ar"]]
times = []
for r in range(reps + 2):
    meter = build_meter_for_dataset(dv["ar"], device=dev, **kw)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    validate(0, model, batches, meter, task, device=dev)
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    logs = meter.get_logs()
    torch.cuda.synchronize()
    t2 = time.perf_counter()
    if r >= 2:
        times.append(((t1 - t0) * 1e3, (t2 - t1) * 1e3))
v = sorted(t[0] for t in times)
print(f"report={report} batches={len(batches)} validate ms: median {v[len(v)//2]:.3f} min {v[0]:.3f} max {v[-1]:.3f}; get_logs ms median {sorted(t[1] for t in times)[len(times)//2]:.3f}; keys {len(logs)}", flush=True)
