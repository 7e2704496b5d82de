#!/usr/bin/env python3
"""The optimizer launch alone with the state in f32, in bf16 rounded to nearest and in bf16 rounded stochastically.

    python tools/optim_state_bench.py [--n N ...] [--trn-hidden 4096] [--parent-lib PATH] [--rounds 3] [--out FILE]

Sizes: the flat buffers of the headline model (25 003 272 elements: profiles/optim_unified_cost.txt) and, with --trn-hidden, those
of the model bench.py builds for that width (counted from its parameters, slot padding included).  Per size and variant: AdamW
through egk_optim_step, f32 gradient, both bf16 copies written -- the launch of the captured step.  Method of
profiles/optim_unified_cost.txt: the variants are ALTERNATED ``--rounds`` times inside one process; per round 5 warm-up launches,
then 6 batches of 10 launches timed by the library's profile counters (HIP events around every launch: egk_prof_reset, the batch
enqueued back to back behind one uncounted launch, egk_prof_get); figure = the median of the 6 batch means, per variant the median
of its round medians and their spread.  --parent-lib: another
build of the library (the parent commit's) measured in the same alternation under "f32 (parent)": its f32 figure must not have
moved.  The bytes are the library's own count (optim_bytes: 30 / 22 B per parameter), so GB/s = counted bytes / median time.
Needs a GPU; prints a table and, with --out, appends it to a file."""
import argparse
import ctypes as C
import statistics
import sys
from pathlib import Path

REPO = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(REPO))
import torch  # noqa: E402

from egopack_amd import _lib  # noqa: E402

HEADLINE = 25_003_272
DEV = "cuda"


def model_elements(trn_hidden: int) -> int:
    """Elements of the flat buffers of bench.py's flagship model at ``--trn-hidden``: the slot lengths optim.FlatOptimizer gives
    its parameters (16-byte alignment, 64-row padding of the classifier matrices)."""
    import bench
    from egopack_amd.optim import FlatOptimizer
    args = bench.parse_args(["--trn-hidden", str(trn_hidden)])
    model, tasks, *_ = bench.build_workload(args, 0, torch.device(DEV))
    seen, total = set(), 0
    for p in [*model.parameters(), *(q for t in tasks.values() for q in t.parameters())]:
        if id(p) not in seen and p.requires_grad:
            seen.add(id(p))
            total += FlatOptimizer._slot_len(p)
    return total


def prof_time_ms(lib, name=b"optim"):
    """total_ms and bytes of the profile id ``name`` since the last reset (synchronises)."""
    buf = C.create_string_buffer(64)
    n, ms, fl, by = C.c_int64(), C.c_double(), C.c_double(), C.c_double()
    for i in range(lib.egk_prof_count()):
        lib.egk_prof_get(i, buf, 64, C.byref(n), C.byref(ms), C.byref(fl), C.byref(by))
        if buf.value == name:
            return ms.value, by.value
    raise RuntimeError("no profile id 'optim'")


class Variant:
    def __init__(self, label, lib, n, state_dtype, mode):
        self.label, self.lib, self.n = label, lib, n
        g = torch.Generator(device=DEV).manual_seed(1)
        self.p = torch.randn(n, device=DEV, generator=g)
        self.g = torch.randn(n, device=DEV, generator=g) * 1e-2
        self.m = torch.zeros(n, device=DEV, dtype=state_dtype)
        self.v = torch.zeros(n, device=DEV, dtype=state_dtype)
        self.hi, self.lo = torch.zeros(n, device=DEV, dtype=torch.bfloat16), torch.zeros(n, device=DEV, dtype=torch.bfloat16)
        self.hyper = torch.tensor([1e-3, 0.1, 0.0316, 1.0], device=DEV)
        self.t = torch.ones(1, dtype=torch.int64, device=DEV)
        d = self.d = _lib.OptimDesc()
        d.rule, d.g_dtype, d.n = _lib.OPT_ADAMW, 0, n
        d.p, d.g, d.state0, d.state1, d.hyper, d.t_dev = (x.data_ptr() for x in (self.p, self.g, self.m, self.v, self.hyper, self.t))
        d.beta1, d.beta2, d.eps, d.weight_decay = 0.9, 0.999, 1e-8, 1e-2
        d.bf16_shadow, d.bf16_lo_shadow = self.hi.data_ptr(), self.lo.data_ptr()
        if state_dtype == torch.bfloat16:
            d.state_dtype, d.state_round, d.state_seed = 1, mode, 0x1234567
        self.medians, self.bytes = [], 0.0

    def launch(self):
        self.t.add_(1)
        rc = self.lib.egk_optim_step(C.c_void_p(torch.cuda.current_stream().cuda_stream), C.byref(self.d))
        if rc:
            raise RuntimeError(f"egk_optim_step returned {rc}")

    def round(self, warm=5, batches=6, per_batch=10):
        """The events of the counters sit on the stream around each launch: on an idle stream the time between them holds the host's
        way from one to the other too (measured: up to 9 us of a 150 us launch, different for two loads of ONE binary).  So every
        timed launch is enqueued while the device is still busy with the one before it: an uncounted launch leads each batch."""
        for _ in range(warm):
            self.launch()
        torch.cuda.synchronize()
        times = []
        for _ in range(batches):
            self.lib.egk_prof_enable(0)
            self.launch()
            self.lib.egk_prof_enable(1)
            self.lib.egk_prof_reset()
            for _ in range(per_batch):
                self.launch()
            ms, total = prof_time_ms(self.lib)
            times.append(ms * 1e3 / per_batch)
            self.bytes = total / per_batch
        self.lib.egk_prof_enable(0)
        self.medians.append(statistics.median(times))


def bind(path):
    """Another build of the library under the signatures of THIS tree's headers (the descriptor of an older build is a prefix of
    today's: it reads what it knows)."""
    lib = C.CDLL(str(path))
    for table in _lib.signatures().values():
        for name, (res, args) in table.items():
            fn = getattr(lib, name, None)
            if fn is not None:
                fn.restype, fn.argtypes = res, args
    return lib


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--n", type=int, nargs="*", default=[HEADLINE])
    ap.add_argument("--trn-hidden", type=int, default=0)
    ap.add_argument("--parent-lib", default="")
    ap.add_argument("--parent-last", action="store_true", help="measure the parent library behind the three variants instead of in front")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("optim_state_bench.py measures on the GPU: none found")
    lib = _lib.load()
    parent = bind(args.parent_lib) if args.parent_lib else None
    sizes = [(f"n = {n}", n) for n in args.n]
    if args.trn_hidden:
        sizes.append((f"--trn-hidden {args.trn_hidden}", model_elements(args.trn_hidden)))
    lines = []
    for title, n in sizes:
        variants = [Variant("f32 state", lib, n, torch.float32, 0), Variant("bf16 nearest", lib, n, torch.bfloat16, 0),
                    Variant("bf16 stochastic", lib, n, torch.bfloat16, 1)]
        if parent is not None:  # (first in every round, or last: the place in the alternation is part of what is measured)
            variants.insert(len(variants) if args.parent_last else 0, Variant("f32 state (parent)", parent, n, torch.float32, 0))
        for _ in range(args.rounds):
            for v in variants:
                v.round()
        base = next(v for v in variants if v.label == "f32 state")
        f32 = statistics.median(base.medians)
        lines.append(f"{title}: {n} elements, AdamW, f32 gradient, both bf16 copies; {args.rounds} alternated rounds of 6 x 10 launches")
        lines.append(f"  {'variant':20s} {'us (median of medians)':>24s} {'spread':>8s} {'B/param':>8s} {'TB/s':>7s} {'vs f32':>7s} {'bytes ratio':>12s}")
        for v in variants:
            us = statistics.median(v.medians)
            lines.append(f"  {v.label:20s} {us:24.1f} {max(v.medians) - min(v.medians):8.1f} {v.bytes / n:8.1f} {v.bytes / us / 1e6:7.2f} "
                         f"{us / f32:7.3f} {v.bytes / base.bytes:12.3f}")
        del variants
        torch.cuda.empty_cache()
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "a") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
