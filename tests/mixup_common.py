"""What the mixup tests share (host only: no GPU, no library): a float64 model of the two launches of include/egopack_mixup.h, a
pure-numpy restatement of the loader's draw (egopack_amd.data.mixup_fields), and thin ctypes callers of the two entry points.

The row mix: out = lam a + (1 - lam) b with lam the f32 value, in float64 -- "exact" at the precision of the checks.  The launch forms
u = fl(1 - lam), t = fl(lam a), fma(u, b, t): three f32 roundings, each at most 2^-24 relative, of quantities bounded by |lam a| and
|(1 - lam) b|, hence ``mix_bound``.

The two-target loss: lam CE(z, a) + (1 - lam) CE(z, b) with ignored labels contributing 0, through F.cross_entropy and autograd in
float64."""
import ctypes as C

import numpy as np
import torch
import torch.nn.functional as F

F32, BF16 = 0, 1  # EGK_F32 / EGK_BF16
TASK_IDS = {"ar": 1, "lta": 2}  # egopack_amd.data.MIX_TASK_IDS


def gen(seed):
    return torch.Generator().manual_seed(seed)


# ---- the row mix ------------------------------------------------------------------------------------------------------------------
def mix_model(x, src, lam):
    """float64 [rows, cols]: lam x + (1 - lam) x[src]; ``x`` any float tensor, ``lam`` f32, ``src`` integer (None, None: a copy)."""
    x = x.double()
    if src is None:
        return x.clone()
    l = lam.double()[:, None]
    return l * x + (1.0 - l) * x[src.long()]


def mix_bound(x, src, lam):
    """3 * 2^-24 * (|lam a| + |(1 - lam) b|), float64 [rows, cols]."""
    x = x.double()
    if src is None:
        return torch.zeros_like(x)
    l = lam.double()[:, None]
    return 3.0 * 2.0 ** -24 * ((l * x).abs() + ((1.0 - l) * x[src.long()]).abs())


def copied_rows(src, lam):
    """(rows whose output is their own bits, rows whose output is the partner's bits) as bool masks."""
    own = (lam == 1.0) | (src.long() == torch.arange(src.numel()))
    return own, (lam == 0.0) & ~own


def call_mix_rows(lib, segs, cols, dtype, stream):
    """``segs``: [(x_in ptr, x_out ptr, ld_in, ld_out, rows, src ptr or None, lam ptr or None)]."""
    n = len(segs)
    vp = lambda xs: (C.c_void_p * max(n, 1))(*xs)
    return lib.egk_mix_rows_multi(stream, n, vp([s[0] for s in segs]), vp([s[1] for s in segs]),
                                  (C.c_int64 * max(n, 1))(*[s[2] for s in segs]), (C.c_int64 * max(n, 1))(*[s[3] for s in segs]),
                                  (C.c_int32 * max(n, 1))(*[s[4] for s in segs]), vp([s[5] for s in segs]), vp([s[6] for s in segs]),
                                  cols, dtype)


# ---- the two-target cross entropy -------------------------------------------------------------------------------------------------
def ce_mix_model(logits, y, y_b, lam, smoothing, g):
    """(loss float64 [rows], [gradient float64 [rows, C] per head]) of
    sum_h lam CE(z_h, y[:, h]) + (1 - lam) CE(z_h, y_b[:, h]), back-propagated with the seed ``g`` on every row."""
    zs = [l.double().clone().requires_grad_(True) for l in logits]
    lm = lam.double()
    total = torch.zeros(y.shape[0], dtype=torch.float64)
    for h, z in enumerate(zs):
        Cn = z.shape[1]
        ya = torch.where((y[:, h] >= 0) & (y[:, h] < Cn), y[:, h], torch.full_like(y[:, h], -1))
        yb = torch.where((y_b[:, h] >= 0) & (y_b[:, h] < Cn), y_b[:, h], torch.full_like(y_b[:, h], -1))
        total = total + lm * F.cross_entropy(z, ya, ignore_index=-1, reduction="none", label_smoothing=smoothing) \
            + (1.0 - lm) * F.cross_entropy(z, yb, ignore_index=-1, reduction="none", label_smoothing=smoothing)
    if total.numel():
        (total * float(g)).sum().backward()
    return total.detach(), [z.grad if z.grad is not None else torch.zeros_like(z) for z in zs]


def call_ce_mix(lib, tasks, smoothing, dtype, stream):
    """``tasks``: [dict(logits=[(ptr, ld, C, pad, dcol)], y=ptr, y_b=ptr, y_stride, lam=ptr, loss=ptr, dlogits=ptr, ldd, rows, gscale,
    scale=ptr or None)]."""
    n = len(tasks)
    m = max(n, 1)
    lg, ld, Cs, pad, dcol = (C.c_void_p * (4 * m))(), (C.c_int64 * (4 * m))(), (C.c_int32 * (4 * m))(), (C.c_int32 * (4 * m))(), (C.c_int64 * (4 * m))()
    for i, t in enumerate(tasks):
        for h, (p, l, c, pd, dc) in enumerate(t["logits"]):
            lg[4 * i + h], ld[4 * i + h], Cs[4 * i + h], pad[4 * i + h], dcol[4 * i + h] = p, l, c, pd, dc
    vp = lambda key: (C.c_void_p * m)(*[t[key] for t in tasks])
    scales = vp("scale") if any(t.get("scale") is not None for t in tasks) else None
    return lib.egk_ce_mix_fused_multi(stream, n, lg, ld, Cs, pad, dcol, (C.c_int32 * m)(*[len(t["logits"]) for t in tasks]), vp("y"), vp("y_b"),
                                      (C.c_int64 * m)(*[t["y_stride"] for t in tasks]), vp("lam"), vp("loss"), vp("dlogits"),
                                      (C.c_int64 * m)(*[t["ldd"] for t in tasks]), (C.c_int32 * m)(*[t["rows"] for t in tasks]),
                                      (C.c_float * m)(*[t["gscale"] for t in tasks]), scales, float(smoothing), dtype)


def mix_labels(rows, Cs, g):
    """(y, y_b) int64 [rows, heads + 1] (y_stride = heads + 1, the last column a poison): random labels with the four label cases of
    a row in turn -- a ignored with b live, b ignored, both ignored, a == b -- and plain rows between them."""
    n = len(Cs)
    y = torch.stack([torch.randint(0, c, (rows,), generator=g) for c in Cs] + [torch.zeros(rows, dtype=torch.int64)], 1)
    yb = torch.stack([torch.randint(0, c, (rows,), generator=g) for c in Cs] + [torch.zeros(rows, dtype=torch.int64)], 1)
    for h in range(n):
        y[0 + h::7, h] = -1        # a ignored, b live
        yb[1 + h::7, h] = -1       # b ignored
        y[2::7, h] = -1            # both ignored, in every head
        yb[2::7, h] = -1
        yb[3::7, h] = y[3::7, h]   # a == b
    if rows > 5:
        yb[5, 0] = Cs[0]           # a label at C is ignored too
    return y, yb


def lam_vector(kind, rows, g):
    if kind == "random":
        return torch.rand(rows, generator=g)
    return torch.full((rows,), float(kind))


# ---- the loader's draw, restated ----------------------------------------------------------------------------------------------------
def draw_key(seed, epoch, ordinal, task):
    """The Philox key of one batch's draw: a function of (seed, epoch, batch ordinal, task) alone."""
    return np.array([(int(seed) & 0xFFFFFFFFFFFFFFFF), ((int(epoch) & 0xFFFFFFFF) << 32) | (int(ordinal) & 0xFFFFFFFF)], dtype=np.uint64), \
        np.array([TASK_IDS[task], 0x6D697875, 0, 0], dtype=np.uint64)


def draw(lengths, y, seed, epoch, ordinal, task, alpha, per_sequence=True, prob=1.0):
    """(mix_src int32 [N], mix_lam float32 [N], mix_y) of a batch whose sequences have ``lengths`` nodes each (rows in order), as
    egopack_amd.data.mixup_fields draws them: one uniform for the batch's coin, then per group of equal-length sequences in ascending
    length a permutation, then the Beta(alpha, alpha) draws (one per sequence, or one for the batch), clipped to [0, 1]."""
    key, ctr = draw_key(seed, epoch, ordinal, task)
    rng = np.random.Generator(np.random.Philox(key=key, counter=ctr))
    lengths = np.asarray(lengths, dtype=np.int64)
    B = len(lengths)
    starts = np.concatenate([[0], np.cumsum(lengths)[:-1]]).astype(np.int64) if B else np.zeros(0, np.int64)
    mixed = bool(rng.random() < prob)
    partner = np.arange(B, dtype=np.int64)
    for L in np.unique(lengths):
        members = np.nonzero(lengths == L)[0]
        partner[members] = members[rng.permutation(len(members))]
    lam_seq = np.clip(rng.beta(alpha, alpha, size=B if per_sequence else 1), 0.0, 1.0).astype(np.float32)
    if not per_sequence:
        lam_seq = np.repeat(lam_seq, B)
    if not mixed:
        lam_seq = np.ones(B, dtype=np.float32)
    N = int(lengths.sum())
    src, lam = np.empty(N, dtype=np.int32), np.empty(N, dtype=np.float32)
    for s in range(B):
        a, b, L = starts[s], starts[partner[s]], lengths[s]
        src[a:a + L] = np.arange(b, b + L, dtype=np.int32)
        lam[a:a + L] = lam_seq[s]
    y = np.asarray(y)
    return src, lam, y[src]
