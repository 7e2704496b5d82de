#!/usr/bin/env python3
"""The headline training step (bench.py's workload: AR + LTA + PNR, B = 64 x T = 32 per task, H = 1024, bf16) with DropEdge off and
on, timed through the engine -- profiles/edge_drop.txt.  Two captured steps in ONE process, replayed in alternating blocks
(the method of tools/mixup_step_bench.py):
  off   the step as bench.py builds it (model.edge_drop None)
  on    model.edge_drop = EdgeDrop(p): the three forward gathers and the three transposed gathers become the drop launches
``rounds`` blocks of ``steps`` replays per arm, wall time by device events around a block; the median and the spread per arm.
Usage: python tools/edge_drop_step_bench.py [steps] [rounds] [p]"""
import os
import statistics
import sys

sys.path.insert(0, os.getcwd())
import torch

import bench
from egopack_amd import engine, ops
from egopack_amd.optim import FlatAdam

steps = int(sys.argv[1]) if len(sys.argv) > 1 else 200
rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 7
p = float(sys.argv[3]) if len(sys.argv) > 3 else 0.2
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
    params = [*model.configure_optimizers(wd), *(q for t in ORDER for q in tasks[t].configure_optimizers(wd))]
    step = engine.MTLStep(model, tasks, crit, weights, FlatAdam(params, lr=1e-5, weight_decay=1e-5), fused_backbone=True)
    if name == "on":
        model.edge_drop = ops.EdgeDrop(p)
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


arms = {name: arm(name) for name in ("off", "on")}
ms = {name: [] for name in arms}
for _ in range(rounds):
    for name, step in arms.items():
        ms[name].append(block(step))
for name, v in ms.items():
    print(f"{name}: median {statistics.median(v):.4f} ms/step, min {min(v):.4f}, max {max(v):.4f} ({rounds} blocks of {steps} replays)", flush=True)
off, on = (statistics.median(ms[k]) for k in ("off", "on"))
print(f"edge_drop.p = {p}: on - off {1e3 * (on - off):+.1f} us per step", flush=True)
