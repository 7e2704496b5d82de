#!/usr/bin/env python3
"""One AR validation pass with the temperature calibration off and on, timed -- profiles/calibration.txt.  Trains one epoch
(``enabled_tasks=[ar]``), then runs ``main_temporal.validate_metrics`` on the trained model and its validation loader ``repeats``
times each way, alternating (host clock, device synchronised; the first pair warms up), and last times the fit alone --
``calibration.fit`` over the rows the last pass stored -- and prints the library profiler's lines of the new launches.
Usage: python tools/calibration_pass_bench.py <dir> [repeats] [config overrides, e.g. synthetic_samples=256 batch_size=64]"""
import os
import sys
import time
from pathlib import Path

sys.path.insert(0, os.getcwd())
import torch

import main_temporal
from egopack_amd import calibration as CAL
from egopack_amd import ops
from egopack_amd import train as T
from egopack_amd.meters import build_meter_for_dataset
from egopack_amd.validate import validate

root, reps = Path(sys.argv[1]), int(sys.argv[2]) if len(sys.argv) > 2 else 3
extra = sys.argv[3:]
common = ["num_epochs=1", f"checkpoint_dir={root}", "enabled_tasks=[ar]"] + extra
r = main_temporal.main(common)
cfg = T.load_config(common + ["calibration.mode=temperature"])
args = lambda on: (lambda t: T.calibration_meter_args(cfg, t)) if on else None
rows = []
for i in range(reps + 1):
    t = []
    for on in (False, True):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        main_temporal.validate_metrics(0, r["model"], r["tasks"], ["ar"], r["val_datasets"], r["val_loaders"], "cuda", report=args(on))
        torch.cuda.synchronize()
        t.append(time.perf_counter() - t0)
    if i:
        rows.append(t)
for off, on in rows:
    print(f"validate_metrics [ar]: calibration off {off * 1e3:.1f} ms, on {on * 1e3:.1f} ms", flush=True)

meter = build_meter_for_dataset(r["val_datasets"]["ar"], device="cuda", **T.calibration_meter_args(cfg, "ar"))
validate(0, r["model"], r["val_loaders"]["ar"], meter, r["tasks"]["ar"], device="cuda")
store = meter.temp_store
print("rows stored per head and fold:", {h: {f: store.folds[h][f].n for f in CAL.FOLDS} for h in store.heads}, flush=True)
for i in range(reps + 1):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    res = CAL.fit(store, meter.temp_cfg)
    torch.cuda.synchronize()
    if i:
        print(f"calibration.fit (two heads, three fits each, {meter.temp_cfg['iterations']} iterations + the two NLL passes): "
              f"{(time.perf_counter() - t0) * 1e3:.2f} ms", flush=True)
print({h: {k: v for k, v in r_.items() if k != "folds"} for h, r_ in res.items()}, flush=True)
ops.prof_enable(True)
ops.prof_reset()
CAL.fit(store, meter.temp_cfg)
CAL.cross_scores(store, res)
torch.cuda.synchronize()
for name, line in ops.prof_report().items():
    if name.startswith("temp_") or name in ("topk_softmax",):
        print(f"profile: {name} launches {line['launches']} total {line['total_ms'] * 1e3:.1f} us "
              f"({line['total_ms'] * 1e3 / line['launches']:.2f} us per launch), {line['bytes'] / 1e6:.2f} MB modelled", flush=True)
ops.prof_enable(False)
