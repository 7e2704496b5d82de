#!/usr/bin/env python3
"""What LAMB costs (profiles/lamb_cost.txt).

    python tools/lamb_bench.py [--kernels] [--loop] [--rounds 3] [--out FILE]

--kernels: the three launches of include/egopack_lamb.h at the layout of the headline model (bench.py's flagship model: its slot
lengths, 64-row padding included, cut into pieces) beside the Adam launch (egk_adam_step_gated, both bf16 copies) in the same
session.  Method of tools/optim_state_bench.py: the variants are ALTERNATED ``--rounds`` times in one process; per round 5 warm-up
steps, then 6 batches of 10 steps timed by the library's profile counters (HIP events around every launch; each batch is enqueued
behind one uncounted step); figure = the median of the batch means, per variant the median of its rounds.  A LAMB step is moments ->
trust -> apply, back to back as in the training step, so the apply launch finds in the cache what the moments launch left there.
LAMB runs under four cache policies: the family's mask (egk_tune 9) at 7 with and without "keep" (egk_lamb_tune 0), at 1 and at 0.
The bytes are the library's own counts; TB/s = counted bytes / median time.

--loop: main_temporal.py at the headline size with torch.optim.Adam and with egopack_amd.optim.FlatLAMB, alternated ``--rounds``
times, one child process per run; the figure is the loop's own steady-state line.

Needs a GPU; prints, and with --out appends to a file."""
import argparse
import ctypes as C
import re
import statistics
import subprocess
import sys
from pathlib import Path

REPO = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(REPO))
DEV = "cuda"
HEADLINE = ["dataset_recognition=synthetic_resident", "dataset_lta=synthetic_resident", "dataset_oscc=synthetic_resident",
            "dataset_pnr=synthetic_resident", "enabled_tasks=[ar,lta,pnr]", "k=1", "batch_size=64", "model.hidden_size=1024",
            "model.temporal_pooling.hidden_size=1024", "dataset_recognition.T=32", "dataset_lta.T=32", "dataset_oscc.T=32",
            "dataset_pnr.T=32", "num_epochs=1", "synthetic_samples=32768"]
RULES = {"adam": ["optimizer._target_=torch.optim.Adam"],
         "lamb": ["optimizer._target_=egopack_amd.optim.FlatLAMB", "+optimizer.eps=1e-6", "optimizer.weight_decay=1e-2"]}


def slot_sizes():
    """The slot lengths of the flat buffers of bench.py's flagship model (optim.FlatOptimizer._slot_len)."""
    import torch

    import bench
    from egopack_amd.optim import FlatOptimizer
    model, tasks, *_ = bench.build_workload(bench.parse_args([]), 0, torch.device(DEV))
    seen, sizes = set(), []
    for p in [*model.parameters(), *(q for t in tasks.values() for q in t.parameters())]:
        if id(p) not in seen and p.requires_grad:
            seen.add(id(p))
            sizes.append(FlatOptimizer._slot_len(p))
    return sizes


def prof(lib):
    """{profile id: (total ms, bytes)} since the last reset (synchronises)."""
    buf, out = C.create_string_buffer(64), {}
    n, ms, fl, by = C.c_int64(), C.c_double(), C.c_double(), C.c_double()
    for i in range(lib.egk_prof_count()):
        lib.egk_prof_get(i, buf, 64, C.byref(n), C.byref(ms), C.byref(fl), C.byref(by))
        out[buf.value.decode()] = (ms.value, by.value)
    return out


class Step:
    """One optimizer step over buffers of its own; ``ids``: the profile ids it is timed under."""

    def __init__(self, label, lib, sizes, rule, mask=7, keep=1):
        import torch

        from egopack_amd.optim import FlatLAMB
        self.label, self.lib, self.rule, self.mask, self.keep = label, lib, rule, mask, keep
        begin, piece0, pieces = FlatLAMB.piece_table(sizes)
        n = self.n = begin[-1]
        g = torch.Generator(device=DEV).manual_seed(1)
        self.p = torch.randn(n, device=DEV, generator=g)
        self.g = torch.randn(n, device=DEV, generator=g) * 1e-2
        self.m, self.v = torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)
        self.hi, self.lo = (torch.zeros(n, device=DEV, dtype=torch.bfloat16) for _ in range(2))
        self.hyper = torch.tensor([1e-3, 0.1, 0.0316, 1.0], device=DEV)
        self.slot_begin = torch.tensor(begin, dtype=torch.int64, device=DEV)
        self.slot_piece0 = torch.tensor(piece0, dtype=torch.int32, device=DEV)
        self.slot_group = torch.zeros(len(sizes), dtype=torch.int32, device=DEV)
        self.group_hyper = torch.tensor([[1e-3, 1e-2, 0.0, 0.0]], device=DEV)
        self.part = torch.zeros(piece0[-1] * 4, dtype=torch.float64, device=DEV)
        self.trust = torch.ones(len(sizes), device=DEV)
        self.norms = torch.zeros(2 * len(sizes), dtype=torch.float64, device=DEV)
        self.n_pieces, self.n_slots = piece0[-1], len(sizes)
        self.ids = ("adam",) if rule == "adam" else ("lamb_moments", "lamb_trust", "lamb_apply")
        self.medians, self.bytes = {k: [] for k in self.ids}, {}

    def launch(self):
        import torch
        lib, s = self.lib, C.c_void_p(torch.cuda.current_stream().cuda_stream)
        P = lambda t: C.c_void_p(t.data_ptr())
        if self.rule == "adam":
            rc = lib.egk_adam_step_gated(s, P(self.p), P(self.g), 0, P(self.m), P(self.v), self.n, P(self.hyper), 0.9, 0.999, 1e-8, 1e-2,
                                         P(self.hi), P(self.lo), None, 0, None)
        else:
            tables = (P(self.slot_piece0), P(self.slot_group), self.n_slots, P(self.group_hyper), 1)
            rc = lib.egk_lamb_moments(s, P(self.p), P(self.g), 0, P(self.m), P(self.v), 0, self.n, 0, self.n_pieces, 1, P(self.slot_begin),
                                      *tables, P(self.hyper), 0.9, 0.999, 1e-6, P(self.part), None, None, 0)
            rc = rc or lib.egk_lamb_trust(s, P(self.part), *tables, 0, 0, P(self.trust), P(self.norms), None)
            rc = rc or lib.egk_lamb_apply(s, P(self.p), P(self.m), P(self.v), self.n, self.n_pieces, P(self.slot_begin), *tables,
                                          P(self.hyper), 1e-6, P(self.trust), P(self.hi), P(self.lo), None, 0.0, 0, None, None)
        if rc:
            raise RuntimeError(f"{self.label}: a launch returned {rc}")

    def round(self, warm=5, batches=6, per_batch=10):
        import torch
        prev_mask, prev_keep = self.lib.egk_tune(9, self.mask), self.lib.egk_lamb_tune(0, self.keep)
        try:
            for _ in range(warm):
                self.launch()
            torch.cuda.synchronize()
            times = {k: [] for k in self.ids}
            for _ in range(batches):
                self.lib.egk_prof_enable(0)
                self.launch()
                self.lib.egk_prof_enable(1)
                self.lib.egk_prof_reset()
                for _ in range(per_batch):
                    self.launch()
                got = prof(self.lib)
                for k in self.ids:
                    times[k].append(got[k][0] * 1e3 / per_batch)
                    self.bytes[k] = got[k][1] / per_batch
            self.lib.egk_prof_enable(0)
            for k in self.ids:
                self.medians[k].append(statistics.median(times[k]))
        finally:
            self.lib.egk_tune(9, prev_mask)
            self.lib.egk_lamb_tune(0, prev_keep)


def kernels(rounds):
    import torch

    from egopack_amd import _lib
    lib = _lib.load()
    sizes = slot_sizes()
    variants = [Step("adam (mask 7, the default)", lib, sizes, "adam"), Step("lamb mask 7 keep", lib, sizes, "lamb", 7, 1),
                Step("lamb mask 7 stream all", lib, sizes, "lamb", 7, 0), Step("lamb mask 1 (g only)", lib, sizes, "lamb", 1, 1),
                Step("lamb mask 0", lib, sizes, "lamb", 0, 1)]
    for _ in range(rounds):
        for v in variants:
            v.round()
    n = variants[0].n
    lines = [f"flagship layout: {n} elements in {len(sizes)} slots, {variants[1].n_pieces} pieces; f32 gradient, both bf16 copies; "
             f"{rounds} alternated rounds of 6 x 10 steps; us = median of the rounds' medians (spread = max - min of the rounds)"]
    lines.append(f"  {'variant':28s} {'launch':14s} {'us':>8s} {'spread':>7s} {'B/param':>8s} {'TB/s':>6s}")
    for v in variants:
        total = 0.0
        for k in v.ids:
            us = statistics.median(v.medians[k])
            total += us
            tb = f"{v.bytes[k] / us / 1e6:6.2f}" if v.bytes[k] else "     -"
            lines.append(f"  {v.label:28s} {k:14s} {us:8.1f} {max(v.medians[k]) - min(v.medians[k]):7.1f} {v.bytes[k] / n:8.1f} {tb}")
        if len(v.ids) > 1:
            lines.append(f"  {v.label:28s} {'sum':14s} {total:8.1f}")
    del variants
    torch.cuda.empty_cache()
    return lines


def loop(rounds):
    lines = ["main_temporal.py " + " ".join(HEADLINE) + " + the rule's overrides, one child process per run"]
    for r in range(1, rounds + 1):
        for rule, over in RULES.items():
            out = subprocess.run([sys.executable, str(REPO / "main_temporal.py"), *HEADLINE, *over], capture_output=True, text=True, cwd=str(REPO),
                                 timeout=600)
            log = out.stdout + out.stderr
            if out.returncode:
                raise RuntimeError(f"{rule}: main_temporal.py ended with {out.returncode}\n{log[-3000:]}")
            steady = re.search(r"steady state ([0-9.]+) ms/step, ([0-9.]+) clip-seqs/s", log)
            trust = re.search(r"trust ratio min.*", log)
            lines.append(f"run {r} {rule}: steady state {steady.group(1)} ms/step, {steady.group(2)} clip-seqs/s  {trust.group(0) if trust else ''}")
    return lines


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--kernels", action="store_true")
    ap.add_argument("--loop", action="store_true")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    lines = []
    if args.loop:  # (first: its children must find the GPU uninitialised by this process's own kernels -- they are independent either way)
        lines += loop(args.rounds)
    if args.kernels or not args.loop:
        import torch
        if not torch.cuda.is_available():
            raise SystemExit("lamb_bench.py measures on the GPU: none found")
        lines += kernels(args.rounds)
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "a") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
