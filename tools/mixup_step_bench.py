#!/usr/bin/env python3
"""The headline training step (bench.py's workload: AR + LTA + PNR, B = 64 x T = 32 per task, H = 1024, bf16) with sequence mixup
off and on, timed through the engine -- profiles/mixup.txt.  Three captured steps in ONE process, replayed in alternating blocks:
  off         the step as bench.py builds it
  no-compact  the same step with head compaction off (MTLStep.compact_heads = False): what a mixed task's heads give up
  on          mixup.alpha = 0.4 on AR and LTA: fields from data.mixup_fields, one mix launch in front of the backbone, the two-target
              cross entropy, head compaction off for the mixed tasks
so that (no-compact - off) is the lost compaction and (on - no-compact) the mix pass plus the second label.  ``rounds`` blocks of
``steps`` replays per arm, wall time by device events around a block; the median and the spread of the blocks per arm.
Usage: python tools/mixup_step_bench.py [steps] [rounds]"""
import os
import statistics
import sys

sys.path.insert(0, os.getcwd())
import torch

import bench
from egopack_amd import data as D
from egopack_amd import engine, ops
from egopack_amd.optim import FlatAdam

steps = int(sys.argv[1]) if len(sys.argv) > 1 else 200
rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 7
ORDER = ("ar", "oscc", "lta", "pnr")


def arm(name):
    args = bench.parse_args(["--workload", "mtl"])
    ops.set_compute(args.compute)
    ops.manual_seed(0)
    model, tasks, crit, weights, dev, merged = bench.build_workload(args, 0, torch.device("cuda"))
    model.to("cuda").train()
    for t in tasks.values():
        t.to("cuda").train()
    crit = {t: c.to("cuda").train() for t, c in crit.items()}
    wd = 1e-5
    params = [*model.configure_optimizers(wd), *(p for t in ORDER for p in tasks[t].configure_optimizers(wd))]
    step = engine.MTLStep(model, tasks, crit, weights, FlatAdam(params, lr=1e-5, weight_decay=1e-5), fused_backbone=True)
    if name == "no-compact":
        step.compact_heads = False
    if name == "on":
        for t in ("ar", "lta"):
            src, lam, my = D.mixup_fields(dev[t].ptr.cpu(), dev[t].y.cpu(), 0, 0, 0, t, 0.4)
            dev[t].mix_src, dev[t].mix_lam, dev[t].mix_y = src.cuda(), lam.cuda(), my.cuda()
    step.capture(dev, merged, warmup=2)
    for _ in range(20):
        step.replay()
    torch.cuda.synchronize()
    return step


def block(step):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(steps):
        step.replay()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / steps


arms = {name: arm(name) for name in ("off", "no-compact", "on")}
ms = {name: [] for name in arms}
for _ in range(rounds):
    for name, step in arms.items():
        ms[name].append(block(step))
for name, v in ms.items():
    print(f"{name}: median {statistics.median(v):.4f} ms/step, min {min(v):.4f}, max {max(v):.4f} ({rounds} blocks of {steps} replays)", flush=True)
off, nc, on = (statistics.median(ms[k]) for k in ("off", "no-compact", "on"))
print(f"on - off {1e3 * (on - off):+.1f} us = lost head compaction {1e3 * (nc - off):+.1f} us + mix pass and second label {1e3 * (on - nc):+.1f} us", flush=True)
