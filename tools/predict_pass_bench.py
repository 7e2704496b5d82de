#!/usr/bin/env python3
"""The prediction export against the validation pass on the same split and checkpoint, timed -- profiles/predict.txt.  Trains one
epoch into ``<dir>`` when it holds no checkpoint yet, then runs ``predict.main`` (all four tasks, JSON on) and
``main_temporal.validate_metrics`` on the model, datasets and loaders that ``predict.main`` built, ``repeats`` times each
(alternating; host clock, device synchronised), and last one more ``predict.main`` under the library's profiler for the
``topk_softmax`` line.
Usage: python tools/predict_pass_bench.py <dir> [repeats] [config overrides, e.g. synthetic_samples=256 batch_size=64]"""
import os
import sys
import time
from pathlib import Path

sys.path.insert(0, os.getcwd())
import torch

import main_temporal
import predict
from egopack_amd import ops

root, reps = Path(sys.argv[1]), int(sys.argv[2]) if len(sys.argv) > 2 else 3
extra = sys.argv[3:]
common = ["num_epochs=1", "save_model=True", f"checkpoint_dir={root}", "enabled_tasks=[ar,lta,oscc,pnr]", "lta_sampling.mode=philox"] + extra
ckpt = root / "MTL_ar-lta-oscc-pnr" / "checkpoint.pth"
if not ckpt.exists():
    main_temporal.main(common)
args = common + [f"resume_from={ckpt}", f"predict.out={root / 'predictions'}"]
rows = []
for r in range(reps + 1):  # (the first pair warms up)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = predict.main(args)
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    main_temporal.validate_metrics(0, out["model"], out["tasks"], ["ar", "lta", "oscc", "pnr"], out["datasets"], out["loaders"], "cuda",
                                   sampler=ops.FutureSampler(0))
    torch.cuda.synchronize()
    t2 = time.perf_counter()
    if r:
        rows.append((t1 - t0, sum(out["seconds"].values()), t2 - t1, dict(out["seconds"])))
for whole, loops, val, per in rows:
    print(f"predict.main {whole * 1e3:.1f} ms (its four loops {loops * 1e3:.1f} ms: "
          + ", ".join(f"{t} {s * 1e3:.1f}" for t, s in per.items()) + f"); validate_metrics {val * 1e3:.1f} ms", flush=True)
n = {t: int(next(iter(p.values())).shape[0]) if p else 0 for t, p in ((t, {k: v for k, v in d.items() if torch.is_tensor(v)})
                                                                      for t, d in out["predictions"].items())}
print(f"rows per task: {n}; batches per task: { {t: len(l) for t, l in out['loaders'].items()} }", flush=True)
ops.prof_enable(True)
ops.prof_reset()
predict.main(args)
torch.cuda.synchronize()
for name, line in ops.prof_report().items():
    if name in ("topk_softmax", "categorical_sample", "segmax_fwd"):
        print(f"profile: {name} launches {line['launches']} total {line['total_ms'] * 1e3:.1f} us "
              f"({line['total_ms'] * 1e3 / line['launches']:.2f} us per launch), {line['bytes'] / 1e6:.2f} MB modelled", flush=True)
ops.prof_enable(False)
