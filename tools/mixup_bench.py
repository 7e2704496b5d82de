#!/usr/bin/env python3
"""The two launches of include/egopack_mixup.h, timed -- profiles/mixup.txt.
``egk_mix_rows_multi`` over three segments of ``rows / 3`` rows x ``cols`` columns (the task batches of a merged input; the second
one unmixed: a copy), bf16 and f32, beside a plain device copy of the same buffer: device time per launch and achieved bytes per
second, counting what the launch moves -- two row reads and one row write for a mixed row, one read and one write for a copied one.
``egk_ce_mix_fused_multi`` beside ``egk_ce_fused_multi`` on the same two tasks x (115, 478) classes: the cost of the second label.
Device time from one replay of a captured graph of ``iters`` launches (tools/_timing.py), three rounds, the launches alternating.
Usage: python tools/mixup_bench.py [rows] [cols] [iters]"""
import os
import sys

sys.path.insert(0, os.getcwd())
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import torch

from _timing import time_us
from egopack_amd import ops

rows = int(sys.argv[1]) if len(sys.argv) > 1 else 6144
cols = int(sys.argv[2]) if len(sys.argv) > 2 else 1536
iters = int(sys.argv[3]) if len(sys.argv) > 3 else 20
g = torch.Generator().manual_seed(0)
per = rows // 3
offs = [0, per, 2 * per, 3 * per]

for dt in (torch.bfloat16, torch.float32):
    es = 2 if dt == torch.bfloat16 else 4
    x = torch.randn(3 * per, cols, generator=g).to(dt).cuda()
    out = torch.empty_like(x)
    seg = lambda t: [t[offs[i]:offs[i + 1]] for i in range(3)]
    src = [torch.randperm(per, generator=g).to(torch.int32).cuda() for _ in range(3)]
    lam = [torch.rand(per, generator=g).cuda() for _ in range(3)]
    one = [torch.ones(per).cuda() for _ in range(3)]
    runs = {
        "mix_rows (2 of 3 segments mixed)": (lambda: ops.mix_rows(seg(x), seg(out), [src[0], None, src[2]], [lam[0], None, lam[2]]), (3 + 2 + 3) * per),
        "mix_rows (every row mixed)": (lambda: ops.mix_rows(seg(x), seg(out), src, lam), 9 * per),
        "mix_rows (lam == 1: every row copied)": (lambda: ops.mix_rows(seg(x), seg(out), src, one), 6 * per),
        "device copy of the buffer": (lambda: out.copy_(x), 6 * per),
    }
    for rnd in range(3):
        parts = []
        for name, (fn, row_moves) in runs.items():
            us = time_us(fn, iters)
            parts.append(f"{name} {us:.2f} us, {row_moves * cols * es / us / 1e6:.2f} TB/s")
        print(f"{str(dt).replace('torch.', '')} [{3 * per}, {cols}] round {rnd}: " + "; ".join(parts), flush=True)


def banked(logits, dt):
    """The heads' logits with the hand-off record a classifier bank gives them (ops.classifier_bank): blocks of one gradient operand."""
    widths = [(l.shape[1] + 63) // 64 * 64 for l in logits]
    gbuf = torch.empty((logits[0].shape[0], sum(widths)), dtype=dt, device="cuda")
    state, col, outs = {"filled": set(), "pads": False}, 0, []
    for l, w in zip(logits, widths):
        d = l.detach().requires_grad_(True)
        d._egk_grad_dst = (gbuf, col, state)
        outs.append(d)
        col += w
    return tuple(outs)


n = rows // 3
for dt in (torch.bfloat16, torch.float32):
    tasks = []
    for _ in range(2):
        z = [(torch.randn(n, c, generator=g) * 3).cuda() for c in (115, 478)]
        y = torch.stack([torch.randint(0, c, (n,), generator=g) for c in (115, 478)], 1).cuda()
        yb = y[torch.randperm(n, generator=g).cuda()].contiguous()
        tasks.append((z, y, yb, torch.rand(n, generator=g).cuda()))

    def ce(mixed):
        with ops.bank_grad_handoff():
            ops.cross_entropy_multi([(banked(z, dt), y) for z, y, _, _ in tasks], [1.0 / n] * 2, 0.1,
                                    mixes=[(yb, lm) for _, _, yb, lm in tasks] if mixed else None)
    for rnd in range(3):
        print(f"{str(dt).replace('torch.', '')} 2 tasks x {n} rows x (115, 478) round {rnd}: ce_fused_multi {time_us(lambda: ce(False), iters):.2f} us; "
              f"ce_mix_fused_multi {time_us(lambda: ce(True), iters):.2f} us", flush=True)
