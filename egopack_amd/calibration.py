"""Post-hoc temperature calibration of the classification heads, fitted on the device (include/egopack_calibrate.h).

One scalar T > 0 per head divides the logits before the softmax (Guo et al. 2017).  An arg-max does not move under a division by
T > 0, so what is predicted stays; only the confidence moves.  The objective -- the NLL of the scaled logits over the stored
validation rows, written in beta = 1 / T -- is convex in beta, and a safeguarded Newton iteration on its derivative runs in a dozen
launches with beta in device memory: per iteration one ``egk_zero_fill`` of the accumulators, the ``egk_temp_stats`` launches and
one ``egk_temp_newton``; the host reads the state once, at the end.  The sums are integers, so ranks that all-reduce them between
the statistics and the Newton launch hold the same bits, and those are the bits of the single pass.

``LogitStore`` keeps what a meter scored, per head in two folds (even / odd batch ordinal); ``fit`` runs three fits per head on the
same launches -- fold A, fold B, all rows -- and ``cross_scores`` gives the cross-fitted confidences: fold A's rows at beta_B and
fold B's at beta_A, from the raw top-1 (``egk_topk_softmax``) and ``egk_temp_topk_prob`` -- the order is never recomputed.
"""
from __future__ import annotations

import logging
from typing import Callable, Dict, Optional

import torch

from . import _lib, ops

logger = logging.getLogger(__name__)

Q24 = float(1 << 24)
STATUS = {0: "running", 1: "converged", 2: "at_beta_min", 3: "at_beta_max", 4: "no_rows"}
FOLDS = ("A", "B")
DEFAULTS = {"mode": "none", "tasks": ["ar", "lta", "oscc"], "t_range": [0.05, 20.0], "iterations": 16, "stop": 1e-6,
            "max_rows": 1048576, "save": True, "predict": "auto"}
MODES = ("none", "temperature")
TASKS = ("ar", "lta", "oscc")  # (PNR is a one-logit BCE head and its export is a frame index: it takes no temperature)


class _Fold:
    """The rows of one fold of one head: f32 [capacity, ld] logits and int64 labels, grown by doubling up to the store's limit."""

    def __init__(self, C: int, device):
        self.C, self.ld, self.n, self.device = C, (C + 3) // 4 * 4, 0, device
        self.logits = torch.empty((0, self.ld), dtype=torch.float32, device=device)
        self.labels = torch.empty((0,), dtype=torch.int64, device=device)

    def reserve(self, rows: int) -> None:
        cap = self.logits.shape[0]
        if rows <= cap:
            return
        new = max(rows, 2 * cap, 1024)
        logits = torch.zeros((new, self.ld), dtype=torch.float32, device=self.device)
        labels = torch.full((new,), -1, dtype=torch.int64, device=self.device)
        logits[: self.n].copy_(self.logits[: self.n])
        labels[: self.n].copy_(self.labels[: self.n])
        self.logits, self.labels = logits, labels

    def rows(self):
        """(logits [n, C] -- a view with row stride ld --, labels [n])"""
        return self.logits[: self.n, : self.C], self.labels[: self.n]


class LogitStore:
    """Per head the logits a meter scored, as f32, with their int64 labels, in two folds: the rows of a batch go into fold A for an
    even batch ordinal and into fold B for an odd one (``data.BatchLoader`` stamps ``ordinal``), so the folds do not depend on how
    the batches are dealt to ranks.  ``append`` stores by device copies.  At ``max_rows`` rows of a head the store stops collecting
    for it and logs once."""

    def __init__(self, heads: Dict[str, int], max_rows: int = DEFAULTS["max_rows"], device="cuda"):
        if not 1 <= len(heads) <= 2:
            raise ValueError(f"LogitStore: 1 or 2 heads (three fits per head share one Newton launch of at most "
                             f"{_lib.TEMP_MAX_HEADS}), got {list(heads)}")
        self.heads = {h: int(c) for h, c in heads.items()}
        self.max_rows, self.device = int(max_rows), torch.device(device)
        self.folds = {h: {f: _Fold(c, self.device) for f in FOLDS} for h, c in self.heads.items()}
        self.full = {h: False for h in self.heads}
        self._auto = 0  # the ordinal of a batch that carries none: the count of appends

    def count(self, head: str) -> int:
        return sum(f.n for f in self.folds[head].values())

    @torch.no_grad()
    def append(self, head: str, logits: torch.Tensor, y: torch.Tensor, ordinal: Optional[int] = None) -> int:
        """Store ``logits`` [N, C] and ``y`` [N] of ``head``; returns the rows stored (fewer than N once the limit is reached)."""
        C = self.heads[head]
        if logits.dim() != 2 or logits.shape[1] != C or y.dim() != 1 or y.shape[0] != logits.shape[0]:
            raise ValueError(f"LogitStore.append: head {head} takes [N, {C}] logits and [N] labels (got {tuple(logits.shape)}, {tuple(y.shape)})")
        ops._need_gpu(logits, y)
        if ordinal is None:
            ordinal = self._auto
        self._auto += 1
        room = self.max_rows - self.count(head)
        n = min(int(logits.shape[0]), max(room, 0))
        if n < logits.shape[0] and not self.full[head]:
            self.full[head] = True
            logger.warning("calibration: the store of head %s is full at %d rows (calibration.max_rows): later rows are not collected",
                           head, self.max_rows)
        if n == 0:
            return 0
        fold = self.folds[head][FOLDS[int(ordinal) & 1]]
        fold.reserve(fold.n + n)
        fold.logits[fold.n: fold.n + n, :C].copy_(logits.detach()[:n])  # (widens bf16: what the meters score is logits.float())
        fold.labels[fold.n: fold.n + n].copy_(y[:n])
        fold.n += n
        return n


def _zero(acc: torch.Tensor) -> None:
    ops._ck(_lib.load().egk_zero_fill(ops._stream(), ops._p(acc), acc.numel() * acc.element_size()), "egk_zero_fill")


def _stats_pass(store: LogitStore, beta: torch.Tensor, acc: torch.Tensor) -> None:
    """The statistics of every head at the betas of its three fits: slot 3h = fold A, 3h + 1 = fold B, 3h + 2 = all rows (both folds
    into one accumulator: the iterates of the three fits differ, so acc_A + acc_B is not the third)."""
    for h, head in enumerate(store.heads):
        for i, f in enumerate(FOLDS):
            z, y = store.folds[head][f].rows()
            if z.shape[0]:
                ops.temp_stats(z, y, beta[3 * h + i:], acc[3 * h + i])
                ops.temp_stats(z, y, beta[3 * h + 2:], acc[3 * h + 2])


@torch.no_grad()
def fit(store: LogitStore, cfg: dict, reduce: Optional[Callable[[torch.Tensor], None]] = None) -> Dict[str, dict]:
    """The temperature of every head of ``store``: {head: {temperature, beta, status, iterations, rows, left_out, nll,
    nll_calibrated, folds: {A: {...}, B: {...}}}} -- the outer entries are the fit on all rows, ``folds`` holds the two fold fits
    (the cross-fitted scores read their betas).  ``nll`` / ``nll_calibrated``: the mean NLL per counted row at T = 1 and at the
    fitted T.  ``cfg``: ``t_range`` = [T_min, T_max] (beta runs over the reciprocals), ``iterations``, ``stop``.  ``reduce``: called
    with the int64 accumulators between the statistics launches and the Newton launch -- a SUM all-reduce when a process group
    exists, so every rank holds the same bits and they equal the single pass's.  One host read, at the end."""
    t_lo, t_hi = (float(v) for v in cfg.get("t_range", DEFAULTS["t_range"]))
    if not 0.0 < t_lo <= 1.0 <= t_hi < float("inf"):
        raise ValueError(f"calibration.t_range: [T_min, T_max] with 0 < T_min <= 1 <= T_max (got {[t_lo, t_hi]})")
    iterations, stop = int(cfg.get("iterations", DEFAULTS["iterations"])), float(cfg.get("stop", DEFAULTS["stop"]))
    if iterations < 1 or not stop >= 0.0:
        raise ValueError(f"calibration: iterations >= 1 and stop >= 0 (got {iterations}, {stop})")
    dev, H = store.device, len(store.heads)
    lim = torch.tensor([1.0 / t_hi, 1.0 / t_lo], dtype=torch.float32)  # (the f32 words the launches take)
    bmin, bmax = float(lim[0]), float(lim[1])
    beta = torch.ones(3 * H, dtype=torch.float32, device=dev)
    state = torch.tensor([[1.0, bmin, bmax, 0.0, 0.0, 0.0, 0.0, 0.0]] * (3 * H), dtype=torch.float64, device=dev)
    acc = torch.zeros((3 * H, 8), dtype=torch.int64, device=dev)
    for _ in range(iterations):
        _zero(acc)
        _stats_pass(store, beta, acc)
        if reduce is not None:
            reduce(acc)
        ops.temp_newton(acc, state, beta, bmin, bmax, stop)
    # the NLL at the fitted betas and at T = 1 (the same launches; the raw sums of the two folds add up to the third: one beta)
    final, raw, one = torch.zeros_like(acc), torch.zeros_like(acc), torch.ones_like(beta)
    _stats_pass(store, beta, final)
    _stats_pass(store, one, raw)
    if reduce is not None:
        reduce(final)
        reduce(raw)
    st, fin, rw, bt = state.cpu().tolist(), final.cpu().tolist(), raw.cpu().tolist(), beta.cpu().tolist()

    def entry(slot):
        counted = fin[slot][3] - fin[slot][5]
        raw_counted = rw[slot][3] - rw[slot][5]
        status = int(st[slot][5])
        if status == 0:
            logger.warning("calibration: a fit is still running after %d iterations (last relative step %.3g)", iterations, st[slot][7])
        return dict(temperature=1.0 / bt[slot], beta=bt[slot], status=STATUS[status], iterations=int(st[slot][6]), rows=int(fin[slot][3]),
                    left_out=int(fin[slot][5]), nll=rw[slot][0] / Q24 / max(raw_counted, 1), nll_calibrated=fin[slot][0] / Q24 / max(counted, 1))

    out = {}
    for h, head in enumerate(store.heads):
        out[head] = entry(3 * h + 2)
        out[head]["folds"] = {f: entry(3 * h + i) for i, f in enumerate(FOLDS)}
    return out


@torch.no_grad()
def cross_scores(store: LogitStore, result: Dict[str, dict]):
    """{head: (in_sample, [(conf f32 [n], pred int64 [n], labels int64 [n]) per non-empty fold])}: the cross-fitted confidences.
    Fold A's rows are scored at beta_B and fold B's at beta_A; with an empty fold (its fit has no rows) both are scored at the
    beta of all rows and ``in_sample`` is True.  ``pred`` is the RAW top-1 (``egk_topk_softmax``), ``conf`` its probability at the
    temperature (``egk_temp_topk_prob``, k = 1)."""
    out = {}
    for head in store.heads:
        folds, res = store.folds[head], result[head]
        in_sample = any(res["folds"][f]["status"] == "no_rows" for f in FOLDS)
        parts = []
        for f, other in (("A", "B"), ("B", "A")):
            z, y = folds[f].rows()
            if not z.shape[0]:
                continue
            b = res["beta"] if in_sample else res["folds"][other]["beta"]
            word = torch.tensor([b], dtype=torch.float32, device=z.device)
            idx, _, _ = ops.topk_softmax([z], 1, want_prob=False)[0]
            prob, _ = ops.temp_topk_prob(z, idx, word)
            parts.append((prob[:, 0], idx[:, 0], y))
        out[head] = (in_sample, parts)
    return out


def all_reduce_sum(group=None) -> Optional[Callable[[torch.Tensor], None]]:
    """The ``reduce`` of ``fit`` for the current process group: None without one (or with a single rank)."""
    import torch.distributed as dist
    if not (dist.is_available() and dist.is_initialized()) or dist.get_world_size(group) == 1:
        return None
    return lambda t: dist.all_reduce(t, group=group)
