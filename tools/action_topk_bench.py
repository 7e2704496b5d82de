#!/usr/bin/env python3
"""``egk_action_topk`` beside ``egk_topk_softmax`` on the same two heads and rows, timed -- profiles/action_topk.txt.
6144 rows x (115, 478) classes, k = 5, bf16 and f32: the top-k launch over both heads (indices, probabilities, lse), the action
launch with ranks and labels (pairs, logp, prob, lse, rank), the action launch as the meters issue it (ranks only) and as the export
issues it (no labels).  Device events around ``iters`` back-to-back launches after a warm-up, alternating the launches, three
rounds; logits from a seed on a 2^-4 grid.
Usage: python tools/action_topk_bench.py [rows] [iters]"""
import os
import sys

sys.path.insert(0, os.getcwd())
import torch

from egopack_amd import ops

rows = int(sys.argv[1]) if len(sys.argv) > 1 else 6144
iters = int(sys.argv[2]) if len(sys.argv) > 2 else 200
Cv, Cn, k = 115, 478, 5
g = torch.Generator().manual_seed(0)


def timed(fn):
    for _ in range(10):
        fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / iters  # us per launch (the host's allocation of the outputs included)


for dt in (torch.bfloat16, torch.float32):
    zv = (torch.randint(-128, 129, (rows, Cv), generator=g).float() / 16).to(dt).cuda()
    zn = (torch.randint(-128, 129, (rows, Cn), generator=g).float() / 16).to(dt).cuda()
    yv, yn = torch.randint(0, Cv, (rows,), generator=g).cuda(), torch.randint(0, Cn, (rows,), generator=g).cuda()
    runs = {
        "topk_softmax (both heads, idx + prob + lse)": lambda: ops.topk_softmax([zv, zn], k, want_prob=True, want_lse=True),
        "action_topk (pairs + logp + prob + lse + rank)": lambda: ops.action_topk(zv, zn, k, labels=(yv, yn), want_lse=True),
        "action_topk (ranks only: the meters' launch)": lambda: ops.action_topk(zv, zn, k, labels=(yv, yn), want_prob=False, want_logp=False),
        "action_topk (no labels: the export's launch)": lambda: ops.action_topk(zv, zn, k),
    }
    for rnd in range(3):
        print(f"{str(dt).replace('torch.', '')} rows {rows} round {rnd}: " +
              "; ".join(f"{name} {timed(fn):.1f} us" for name, fn in runs.items()), flush=True)
    ops.prof_enable(True)
    ops.prof_reset()
    for fn in runs.values():
        for _ in range(20):
            fn()
    torch.cuda.synchronize()
    for name, line in ops.prof_report().items():
        if name in ("topk_softmax", "action_topk"):
            note = ", the three action variants together" if name == "action_topk" else ""
            print(f"profile ({str(dt).replace('torch.', '')}): {name} launches {line['launches']} total {line['total_ms'] * 1e3:.1f} us "
                  f"({line['total_ms'] * 1e3 / line['launches']:.2f} us per launch{note})", flush=True)
    ops.prof_enable(False)
