"""Shared by the LAMB tests (tests/test_lamb_cpu.py, tests/test_gpu_lamb.py, tests/test_gpu_bounds_lamb.py): the float64 model of
include/egopack_lamb.h on f32-rounded inputs, its mutants, the piece-table builder, the raw-buffer problem the kernels are held to,
and the three launches over raw pointers.  Imports without a GPU."""
import ctypes as C
import math

import numpy as np
import torch

PIECE = 4096
TOL = dict(rtol=1e-5, atol=1e-6)   # p, m, v: tests/test_gpu_optim_rules.py
TRUST_RTOL = 1e-6                  # trust: the elementwise f32 error of u is a few ulps; at worst aligned ~3e-7 with the final rounding
B1, B2, EPS = 0.9, 0.999, 1e-6
GRAD_SCALE = 0.5                   # s = hyper[3]: not 1, so that where it is applied shows
# the raw-buffer problem: shorter than a quad per thread; three quads short of ...; exactly one piece; one piece + 8; two pieces + 8;
# a 64-row-padded [2, 72] classifier (144 live elements, zero padding)
SIZES = [8, 24, 4096, 4104, 8200, 4608]
LIVE = [8, 24, 4096, 4104, 8200, 144]
SLOT_GROUP = [0, 1, 0, 0, 1, 0]
GROUPS = [(1e-2, 1e-2), (3e-3, 0.0)]  # (lr, weight_decay): group 1 decays nothing
SEED = 0
MUTANTS = ("trust_from_g", "global_norms", "no_wd_in_norm", "adapt_at_wd0", "no_bias_correction", "scale_after_moments")


def f32(x) -> float:
    """``x`` rounded to f32 once, as a Python double."""
    return float(np.float32(x))


def piece_table(sizes):
    """(slot_begin [n + 1], slot_piece0 [n + 1], piece_begin [pieces + 1]): every slot cut into pieces of at most PIECE elements, the
    last one shorter; a piece never crosses a slot boundary."""
    begin, piece0, pieces = [0], [0], []
    for sz in sizes:
        b = begin[-1]
        pieces += list(range(b, b + sz, PIECE))
        begin.append(b + sz)
        piece0.append(len(pieces))
    return begin, piece0, pieces + [begin[-1]]


def hyper(t, lr=0.0, s=GRAD_SCALE, b1=B1, b2=B2):
    """{lr, 1 - b1^t, sqrt(1 - b2^t), s} as f32 values: what the launches read (the model takes exactly these)."""
    return np.array([lr, 1.0 - b1 ** t, math.sqrt(1.0 - b2 ** t), s], dtype=np.float32)


def problem(seed=SEED, sizes=SIZES, live=LIVE):
    """p, g (three steps), m, v as f32 numpy arrays over the flat layout of ``sizes``; the padding of every slot is zero."""
    rng = np.random.default_rng(seed)
    begin, _, _ = piece_table(sizes)
    total = begin[-1]
    mask = np.zeros(total, dtype=bool)
    for b, n in zip(begin, live):
        mask[b:b + n] = True
    zero = np.float32(0.0)  # (+0: a product with the mask would leave -0 in the padding)
    p = np.where(mask, (rng.standard_normal(total) * 0.1).astype(np.float32), zero)
    gs = [np.where(mask, (rng.standard_normal(total) * (10.0 ** rng.uniform(-3, 0, total))).astype(np.float32), zero) for _ in range(3)]
    z = np.zeros(total, dtype=np.float32)
    return dict(p=p, g=gs, m=z.copy(), v=z.copy(), mask=mask, begin=begin, total=total)


def lamb_model(p, g, m, v, begin, slot_group, groups, hy, b1=B1, b2=B2, eps=EPS, trust_clip=False, always_adapt=False, mutant=None,
               dtype=np.float64):
    """One LAMB step.  Inputs are f32 values (numpy arrays); ``dtype`` = float64: the model; float32: the restatement in the
    kernels' precision (numpy rounds every operation separately; the sums stay f64).  Returns (p, m, v, trust [slots], norms)."""
    D = dtype
    p, g, m, v = (np.asarray(x, dtype=np.float32).astype(D) for x in (p, g, m, v))
    h1, h2, s = D(hy[1]), D(hy[2]), D(hy[3])
    omb1, omb2, b2f, epsf = D(f32(1.0 - b1)), D(f32(1.0 - b2)), D(f32(b2)), D(f32(eps))
    if mutant == "no_bias_correction":
        h1 = h2 = D(1.0)
    gg = g if mutant == "scale_after_moments" else g * s
    m = m + (gg - m) * omb1
    v = v * b2f + omb2 * gg * gg
    mh = (m * s if mutant == "scale_after_moments" else m) / h1
    r = mh / (np.sqrt(v) / h2 + epsf)
    trust, norms = [], []
    p_new = p.copy()
    for k in range(len(begin) - 1):
        sl = slice(begin[k], begin[k + 1])
        lr, wd = (D(f32(x)) for x in groups[slot_group[k]])
        u = r[sl] + wd * p[sl]
        span = slice(None) if mutant == "global_norms" else sl
        wd_all = np.concatenate([np.full(begin[j + 1] - begin[j], f32(groups[slot_group[j]][1])) for j in range(len(begin) - 1)]).astype(D)
        u_norm = (r + wd_all * p)[span]
        if mutant == "no_wd_in_norm":
            u_norm = r[span]
        if mutant == "trust_from_g":
            u_norm = gg[span]
        P = float(np.sum(p[span].astype(np.float64) ** 2))
        U = float(np.sum(u_norm.astype(np.float64) ** 2))
        plain = (float(wd) == 0.0 and not always_adapt and mutant != "adapt_at_wd0") or P == 0.0 or U == 0.0
        tr = 1.0 if plain else f32(math.sqrt(P) / math.sqrt(U))
        if trust_clip:
            tr = min(tr, 1.0)
        step = D(lr) * D(tr)
        p_new[sl] = p[sl] - step * u
        trust.append(tr)
        norms.append((math.sqrt(P), math.sqrt(U)))
    return p_new, m, v, np.array(trust), np.array(norms)


def within(got, ref, rtol, atol):
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    return bool(np.all(np.abs(got - ref) <= atol + rtol * np.abs(ref)))


def excess(got, ref, rtol, atol):
    """max |got - ref| / (atol + rtol |ref|): above 1 is outside the tolerance."""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    return float(np.max(np.abs(got - ref) / (atol + rtol * np.abs(ref))))


# ---- the three launches over raw pointers (integers or None) -------------------------------------------------------------------------
def vp(x):
    return None if x is None else C.c_void_p(int(x))


def tables(dev, sizes, slot_group, groups):
    """The device tables of a layout: dict(slot_begin, slot_piece0, slot_group, group_hyper, part, trust, norms) + host copies."""
    begin, piece0, pieces = piece_table(sizes)
    gh = torch.zeros(len(groups), 4, dtype=torch.float32)
    gh[:, :2] = torch.tensor(groups, dtype=torch.float32)
    return dict(begin=begin, piece0=piece0, pieces=pieces,
                slot_begin=torch.tensor(begin, dtype=torch.int64, device=dev), slot_piece0=torch.tensor(piece0, dtype=torch.int32, device=dev),
                slot_group=torch.tensor(slot_group, dtype=torch.int32, device=dev), group_hyper=gh.to(dev),
                part=torch.zeros(piece0[-1] * 4, dtype=torch.float64, device=dev), trust=torch.ones(len(sizes), dtype=torch.float32, device=dev),
                norms=torch.zeros(len(sizes) * 2, dtype=torch.float64, device=dev))


def piece_range(pieces, lo, hi):
    import bisect
    q0, q1 = bisect.bisect_right(pieces, lo) - 1, bisect.bisect_right(pieces, hi - 1) - 1
    return q0, q1 - q0 + 1, int(q0 != q1 or pieces[q0] == lo or pieces[q1 + 1] == hi)  # ([lo, hi] holds a piece boundary)


def moments(lib, stream, ptr, T, lo, hi, g_dtype=0, gate=None, bump_word=None, bump=0, b1=B1, b2=B2, eps=EPS):
    """egk_lamb_moments over [lo, hi); ``ptr``: dict of integer pointers (p, g, m, v, hyper and the tables of ``T``)."""
    q0, nq, on = piece_range(T["pieces"], lo, hi)
    return lib.egk_lamb_moments(stream, vp(ptr["p"]), vp(ptr["g"]), g_dtype, vp(ptr["m"]), vp(ptr["v"]), lo, hi, q0, nq, on,
                                vp(ptr["slot_begin"]), vp(ptr["slot_piece0"]), vp(ptr["slot_group"]), len(T["begin"]) - 1,
                                vp(ptr["group_hyper"]), T["group_hyper"].shape[0], vp(ptr["hyper"]), b1, b2, eps, vp(ptr["part"]),
                                vp(gate), vp(bump_word), bump)


def trust(lib, stream, ptr, T, trust_clip=False, always_adapt=False, gate=None):
    return lib.egk_lamb_trust(stream, vp(ptr["part"]), vp(ptr["slot_piece0"]), vp(ptr["slot_group"]), len(T["begin"]) - 1,
                              vp(ptr["group_hyper"]), T["group_hyper"].shape[0], int(trust_clip), int(always_adapt), vp(ptr["trust"]),
                              vp(ptr["norms"]), vp(gate))


def apply(lib, stream, ptr, T, gate=None, ema=None, ema_decay=0.0, ema_warmup=0, t_dev=None, eps=EPS):
    return lib.egk_lamb_apply(stream, vp(ptr["p"]), vp(ptr["m"]), vp(ptr["v"]), T["begin"][-1], T["piece0"][-1], vp(ptr["slot_begin"]),
                              vp(ptr["slot_piece0"]), vp(ptr["slot_group"]), len(T["begin"]) - 1, vp(ptr["group_hyper"]),
                              T["group_hyper"].shape[0], vp(ptr["hyper"]), eps, vp(ptr["trust"]), vp(ptr["w16"]), vp(ptr.get("w16lo")),
                              vp(ema), ema_decay, ema_warmup, vp(t_dev), vp(gate))
