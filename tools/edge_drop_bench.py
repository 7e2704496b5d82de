#!/usr/bin/env python3
"""The two launches of include/egopack_edge_drop.h, timed -- profiles/edge_drop.txt.
On the graph of the headline batch (bench.py's workload: AR + LTA + PNR, 64 sequences x 32 nodes per task, 6144 rows) and a
[rows, cols] activation, bf16 and f32: the plain forward gather (the banded fast path) and the plain weighted, gated backward gather
beside ``egk_csr_mean_drop_fwd`` / ``_bwd`` at p in {0, 0.2, 0.5}.  Device time per launch from one replay of a captured graph of
``iters`` launches (tools/_timing.py), three rounds, the launches alternating, and the row bytes each launch moves: one neighbour
row read per (kept) edge, one row written per node, one gate row read per node in backward; the CSR arrays, 4 bytes per edge and per
row, are left out.  What to look at: whether the drop launches' time falls with p (only kept rows are requested), and what p = 0
costs over the banded fast path (index fetches and one Philox call per edge instead of a one-byte code per row).
Usage: python tools/edge_drop_bench.py [cols] [iters]"""
import os
import sys

sys.path.insert(0, os.getcwd())
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import torch

import bench
from _timing import time_us
from egopack_amd import ops

cols = int(sys.argv[1]) if len(sys.argv) > 1 else 1024
iters = int(sys.argv[2]) if len(sys.argv) > 2 else 20
args = bench.parse_args(["--workload", "mtl"])
ops.manual_seed(0)
_, _, _, _, _, merged = bench.build_workload(args, 0, torch.device("cuda"))
gr = merged.graph
rows, E = gr.num_nodes, int(gr.col.numel())
deg_in, deg_out = (gr.rowptr[1:] - gr.rowptr[:-1]), (gr.t_rowptr[1:] - gr.t_rowptr[:-1])
print(f"graph: {rows} rows, {E} edges, in-degree max {int(deg_in.max())}, out-degree max {int(deg_out.max())}, "
      f"banded rows {int((gr.band != 0xFF).sum())}", flush=True)
g = torch.Generator().manual_seed(0)

for dt in (torch.bfloat16, torch.float32):
    es = 2 if dt == torch.bfloat16 else 4
    x, d, gate = (torch.randn(rows, cols, generator=g).to(dt).cuda() for _ in range(3))
    out, dx = torch.empty_like(x), torch.empty_like(x)
    inv = torch.empty(rows, dtype=torch.float32, device="cuda")
    runs = {
        "plain fwd (banded)": (lambda: ops._csr_gather(x, gr.rowptr, gr.col, None, None, out, gr.heavy, gr.heavy_mode, gr.band), E + rows),
        "plain bwd (weighted, gated)": (lambda: ops._csr_gather(d, gr.t_rowptr, gr.t_col, gr.t_wgt, gate, dx, gr.t_heavy, gr.t_heavy_mode),
                                        E + 2 * rows),
    }
    for p in (0.0, 0.2, 0.5):
        drop = ops.EdgeDrop(p, rng=(1234, 4096))
        with ops.tap_edge_keep() as tap:
            inv_p, rng = ops._csr_mean_drop_fwd(x, gr.rowptr, gr.col, out, drop)
        kept = int(tap.fwd[0].sum())
        runs[f"drop fwd p={p} (kept {kept})"] = (lambda drop=drop: ops._csr_mean_drop_fwd(x, gr.rowptr, gr.col, out, drop), kept + rows)
        runs[f"drop bwd p={p}"] = (lambda drop=drop, inv_p=inv_p, rng=rng: ops._csr_mean_drop_bwd(d, gr.t_rowptr, gr.t_col, inv_p, gate, dx, drop, rng),
                                   kept + 2 * rows)
    for rnd in range(3):
        for name, (fn, row_moves) in runs.items():
            us = time_us(fn, iters)
            print(f"{str(dt).replace('torch.', '')} [{rows}, {cols}] round {rnd}: {name}: {us:.2f} us, {row_moves * cols * es / 1e6:.1f} MB of rows, "
                  f"{row_moves * cols * es / us / 1e6:.2f} TB/s", flush=True)
