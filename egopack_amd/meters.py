"""Validation meters: the core metrics of reference utils/meters/ego4d.py without torchmetrics,
editdistance, W&B tables or t-SNE plots.

Every ``update`` works on the logits / labels where they are (HBM): one ``egk_label_rank`` launch per head gives
the rank of the ground-truth class, and all top-k accuracies, per-class recalls and supports are integer counts of
it kept in small device tensors -- nothing is copied to the host before ``compute`` / ``get_logs``.

    reference class (ego4d.py)        here                 keys kept
    Ego4dRecognitionMeter :34-203     RecognitionMeter     verbs/nouns_top{1,2,3,5}, verbs/nouns_mc, *_class_acc,
                                                           *_calibration_erorr (the reference's spelling), *_brier_score, loss
    Ego4dAnticipationMeter :206-289   AnticipationMeter    *_accuracy_top{1,2,3,5}, *_recall_top{1,2,3,5}, loss
    Ego4dOSCCMeter :292-318           OSCCMeter            accuracy, loss
    Ego4dPNRMeter :321-377            PNRMeter             accuracy, recall, auroc, localization_error, loss
    Ego4dLTAMeter :380-453            LTAMeter             verbs_ed, nouns_ed (+ verbs/nouns_top1), loss
    utils/confusion.py + ego4d.py:125-170   class_report=True   per head: *_confusion, *_top2_confusion, *_class_loss,
                                                           *_class_precision / _recall / _f1, *_top_confusions,
                                                           *_macro_precision / _recall / _f1, *_acc_many / _medium / _few
    action_scores (config block)   action_scores=  actions_top{1,2,3,5} (AR, anticipation), actions_top1 + actions_ed
                                                           (LTA), actions_seen_top1 / actions_unseen_top1 with their supports
    bootstrap (config block)       bootstrap=       <key>_ci_lo / _ci_hi / _se beside every ratio key: top-k, mean-class
                                                           top-1, action top-k, edit distances, OSCC accuracy, PNR localization_error
Dropped: feature dumps, W&B tables and plots (reporting only).

The per-class report (``class_report=True``; ``log_confusion_matrices`` of the config) is one ``egk_class_report`` launch per
``update`` for all heads of the meter (include/egopack_class_report.h), beside the counting above, which it leaves as it is.  Its
state is four int64 tensors per head -- confusion [C, C], top-2 confusion [C, C], per-class loss sums in 2^-24 fixed point [C],
counts [4] -- that join ``_sums()``: integers only, so shards merge to the bits of the single pass.  With the report off a meter
has the keys and values it had before.

Several ranks (SURVEY §8(e) caveat 5): every meter is a set of SUMS (integer counts, float64 loss / distance sums) plus,
for the PNR AUROC, a list of scores.  ``merge`` adds another meter's state, ``all_reduce`` does the same across the
process group (sum all-reduce of the packed counts, all-gather of the scores), so a validation split sharded batch by
batch (data.BatchLoader ``shard="batches"``) reports exactly the numbers of the single-process pass.
"""
from __future__ import annotations

import logging
import math
from typing import Dict, List, Optional, Sequence

import numpy as np
import torch
import torch.distributed as dist

from . import _lib, ops

logger = logging.getLogger(__name__)

KS = (1, 2, 3, 5)


def label_rank(logits: torch.Tensor, labels: torch.Tensor) -> torch.Tensor:
    """int32 [N]: rank of labels[n] inside logits[n, :] (0 = top-1; ties to the lower class index), -1 where the
    label is negative (ignore_index) -- ``egk_label_rank``."""
    ops._need_gpu(logits, labels)
    if logits.dtype != torch.float32:
        logits = logits.float()
    if logits.stride(1) != 1:
        logits = logits.contiguous()
    labels = labels.to(torch.int64)
    n, c = logits.shape
    rank = torch.empty(n, dtype=torch.int32, device=logits.device)
    ops._ck(_lib.load().egk_label_rank(ops._stream(), ops._p(logits), logits.stride(0), ops._p(labels), labels.stride(0),
                                       ops._p(rank), n, c), "egk_label_rank")
    return rank


def edit_distances(pred: torch.Tensor, label: torch.Tensor) -> torch.Tensor:
    """int32 [N, K] Levenshtein distances between pred[n, :, k] and label[n, :] -- ``egk_edit_distance``."""
    ops._need_gpu(pred, label)
    pred, label = pred.to(torch.int64), label.to(torch.int64)
    n, z, k = pred.shape
    out = torch.zeros((n, k), dtype=torch.int32, device=pred.device)
    if n == 0 or z == 0 or k == 0:  # empty sequences are at distance 0
        return out
    ops._ck(_lib.load().egk_edit_distance(ops._stream(), ops._p(pred), pred.stride(0), pred.stride(1), pred.stride(2),
                                          ops._p(label), label.stride(0), label.stride(1), ops._p(out), n, z, k),
            "egk_edit_distance")
    return out


def action_edit_distances(pred_v: torch.Tensor, pred_n: torch.Tensor, label_v: torch.Tensor, label_n: torch.Tensor) -> torch.Tensor:
    """int32 [N, K, 3]: the Levenshtein distances between the futures pred[n, :, k] and label[n, :] of the verbs ([., ., 0]), of the
    nouns ([., ., 1]: both the integers of ``edit_distances``) and of the actions ([., ., 2]: a position matches only if verb AND
    noun do), in one launch -- ``egk_edit_distance_pairs``."""
    ops._need_gpu(pred_v, pred_n, label_v, label_n)
    if pred_v.shape != pred_n.shape or label_v.shape != label_n.shape or pred_v.dim() != 3 or label_v.shape != pred_v.shape[:2]:
        raise ValueError(f"action_edit_distances: pred [N, Z, K] and label [N, Z] of both heads (got {tuple(pred_v.shape)}, "
                         f"{tuple(pred_n.shape)}, {tuple(label_v.shape)}, {tuple(label_n.shape)})")
    pred_v, pred_n, label_v, label_n = (t.to(torch.int64) for t in (pred_v, pred_n, label_v, label_n))
    if pred_n.stride() != pred_v.stride():  # (the launch reads both heads through one set of strides)
        pred_v, pred_n = pred_v.contiguous(), pred_n.contiguous()
    if label_n.stride() != label_v.stride():
        label_v, label_n = label_v.contiguous(), label_n.contiguous()
    n, z, k = pred_v.shape
    out = torch.zeros((n, k, 3), dtype=torch.int32, device=pred_v.device)
    if n == 0 or z == 0 or k == 0:  # empty sequences are at distance 0
        return out
    ops._ck(_lib.load().egk_edit_distance_pairs(ops._stream(), ops._p(pred_v), ops._p(pred_n), pred_v.stride(0), pred_v.stride(1),
                                                pred_v.stride(2), ops._p(label_v), ops._p(label_n), label_v.stride(0),
                                                label_v.stride(1), ops._p(out), n, z, k), "egk_edit_distance_pairs")
    return out


def class_report(heads) -> None:
    """One ``egk_class_report`` launch for ``heads``, a list of ``(logits [N, C], labels [N] -- a column view is read through its
    stride --, state)`` with ``state`` a ``_ClassReport`` of C classes: the state's tensors are added to.  f32 logits with unit
    column stride are read where they lie; anything else is converted first."""
    if not heads:
        return
    if len(heads) > _lib.CLASS_REPORT_MAX_TASKS:
        raise ValueError(f"class_report: at most {_lib.CLASS_REPORT_MAX_TASKS} heads per launch, got {len(heads)}")
    tasks = (_lib.ClassReportTask * len(heads))()
    keep = []  # (converted tensors stay alive until the launch is issued)
    for t, (logits, labels, state) in zip(tasks, heads):
        ops._need_gpu(logits, labels)
        logits = logits.detach()
        if logits.dtype != torch.float32:
            logits = logits.float()
        if logits.dim() != 2 or labels.dim() != 1 or labels.shape[0] != logits.shape[0]:
            raise ValueError(f"class_report: logits {tuple(logits.shape)} / labels {tuple(labels.shape)}")
        if (logits.shape[1] > 1 and logits.stride(1) != 1) or (logits.shape[0] > 1 and logits.stride(0) < logits.shape[1]):
            logits = logits.contiguous()
        if labels.dtype != torch.int64:
            labels = labels.to(torch.int64)
        if logits.shape[1] != state.C:
            raise ValueError(f"class_report: {logits.shape[1]} logits per row, the state has {state.C} classes")
        keep += [logits, labels]
        t.logits, t.ld, t.labels, t.label_stride = logits.data_ptr(), max(logits.stride(0), logits.shape[1]), labels.data_ptr(), labels.stride(0)
        t.rows, t.C = logits.shape[0], state.C
        t.confusion, t.top2, t.loss_q24, t.counts = (x.data_ptr() for x in state.tensors())
    ops._ck(_lib.load().egk_class_report(ops._stream(), tasks, len(heads)), "egk_class_report")


Q24 = float(1 << 24)  # the fixed point of the per-class loss sums


class _ClassReport:
    """Confusion [C, C] (+1 at [label, top-1]), top-2 confusion [C, C] (+1 at [label, top-1] where the label was the runner-up),
    per-class loss sums in 2^-24 fixed point [C] and counts [4] (valid, ignored, non-finite loss, 0) of one head: int64, on the
    device, added to by ``class_report``."""

    def __init__(self, n_classes: int, device):
        self.C = int(n_classes)
        self.confusion = torch.zeros((self.C, self.C), dtype=torch.int64, device=device)
        self.top2 = torch.zeros((self.C, self.C), dtype=torch.int64, device=device)
        self.loss_q24 = torch.zeros(self.C, dtype=torch.int64, device=device)
        self.counts = torch.zeros(4, dtype=torch.int64, device=device)

    def tensors(self) -> List[torch.Tensor]:
        return [self.confusion, self.top2, self.loss_q24, self.counts]


def report_metrics(confusion, top2, loss_q24, names=None, train_counts=None, shots=(20, 100), top_confusions: int = 20) -> dict:
    """What a head's report derives from its integer state, on the host in float64 (keys without the head's prefix).

    support_c = row sum, predicted_c = column sum, tp_c = diagonal.  recall_c = tp / support (0 without support), precision_c =
    tp / predicted (0 for a class never predicted), f1_c = 2 p r / (p + r) (0 when both are 0); the macro figures are means over
    the classes with support > 0.  class_loss_c = loss_q24 / 2^24 / support (NaN without support).  top_confusions: the largest
    non-zero off-diagonal cells of the top-2 matrix as (label name, confused-with name, count), ties by the lower flat index.
    With ``train_counts`` (training labels per class) and shots = (lo, hi): top-1 accuracy over the validation samples whose
    class has > hi (many), lo .. hi inclusive (medium), < lo (few) training labels, with each bucket's class and sample counts."""
    conf, top2 = torch.as_tensor(confusion).cpu().to(torch.int64), torch.as_tensor(top2).cpu().to(torch.int64)
    C = conf.shape[0]
    names = list(names) if names is not None else [str(c) for c in range(C)]
    tp, support, predicted = conf.diagonal(), conf.sum(1), conf.sum(0)
    tpd = tp.double()
    recall = torch.where(support > 0, tpd / support.clamp(min=1).double(), torch.zeros(C, dtype=torch.float64))
    precision = torch.where(predicted > 0, tpd / predicted.clamp(min=1).double(), torch.zeros(C, dtype=torch.float64))
    pr = precision + recall
    f1 = torch.where(pr > 0, 2 * precision * recall / pr.clamp(min=1e-300), torch.zeros(C, dtype=torch.float64))
    seen = support > 0
    macro = (lambda v: float(v[seen].mean())) if bool(seen.any()) else (lambda v: 0.0)
    loss = torch.as_tensor(loss_q24).cpu().double() / Q24
    class_loss = torch.where(seen, loss / support.clamp(min=1).double(), torch.full((C,), float("nan"), dtype=torch.float64))
    off = top2.clone()
    off.fill_diagonal_(0)
    flat = off.reshape(-1)
    val, idx = torch.sort(flat, descending=True, stable=True)
    pairs = [(names[i // C], names[i % C], v) for v, i in zip(val[:max(int(top_confusions), 0)].tolist(),
                                                                 idx[:max(int(top_confusions), 0)].tolist()) if v > 0]
    out = {"macro_precision": macro(precision), "macro_recall": macro(recall), "macro_f1": macro(f1),
           "confusion": conf, "top2_confusion": top2, "class_loss": class_loss, "class_precision": precision,
           "class_recall": recall, "class_f1": f1, "top_confusions": pairs}
    if train_counts is not None:
        n = torch.as_tensor(train_counts).cpu().to(torch.int64)
        if n.shape != (C,):
            raise ValueError(f"class_report: {tuple(n.shape)} training counts for {C} classes")
        lo, hi = shots
        for name, mask in (("many", n > hi), ("medium", (n >= lo) & (n <= hi)), ("few", n < lo)):
            samples = int(support[mask].sum())
            out[f"acc_{name}"] = int(tp[mask].sum()) / samples if samples else 0.0
            out[f"classes_{name}"] = int(mask.sum())
            out[f"samples_{name}"] = samples
    return out


def _report_line(name: str, m: dict, names) -> str:
    """The report's line of ``print_logs``: macro F1, the bucket accuracies, the five classes with the lowest recall (support >= 1)."""
    support = m["confusion"].sum(1)
    order = sorted((c for c in range(len(support)) if int(support[c]) >= 1), key=lambda c: (float(m["class_recall"][c]), c))[:5]
    worst = ", ".join(f"{names[c]} {float(m['class_recall'][c]) * 100:.1f} (n={int(support[c])})" for c in order)
    shots = "".join(f", {b} {m[f'acc_{b}'] * 100:.2f}" for b in ("many", "medium", "few") if f"acc_{b}" in m)
    return f"{name} macro F1: {m['macro_f1'] * 100:.2f}{shots}; lowest recall: {worst or '-'}"


class _HeadCounts:
    """hits@k, valid count, per-class hits@k and support of one classification head, on the device."""

    def __init__(self, n_classes: int, device, ks: Sequence[int] = KS):
        self.ks, self.C = tuple(ks), n_classes
        self.hits = torch.zeros(len(self.ks), dtype=torch.int64, device=device)
        self.valid = torch.zeros((), dtype=torch.int64, device=device)
        self.class_hits = torch.zeros((len(self.ks), n_classes), dtype=torch.int64, device=device)
        self.support = torch.zeros(n_classes, dtype=torch.int64, device=device)

    def update(self, logits: torch.Tensor, labels: torch.Tensor):
        rank = label_rank(logits, labels)
        ok = rank >= 0
        lab = torch.where(ok, labels.to(torch.int64), torch.zeros_like(labels, dtype=torch.int64))
        self.valid += ok.sum()
        self.support += torch.bincount(lab, weights=ok.to(torch.float64), minlength=self.C).to(torch.int64)
        for i, k in enumerate(self.ks):
            hit = ok & (rank < k)
            self.hits[i] += hit.sum()
            self.class_hits[i] += torch.bincount(lab, weights=hit.to(torch.float64), minlength=self.C).to(torch.int64)
        return rank  # (what was counted: the bootstrap's columns are built from it)

    def tensors(self) -> List[torch.Tensor]:
        return [self.hits, self.valid, self.class_hits, self.support]

    def accuracy(self, k: int) -> float:  # MulticlassAccuracy(top_k=k, average="micro", ignore_index=-1)
        return float(self.hits[self.ks.index(k)]) / max(int(self.valid), 1)

    def class_accuracy(self, k: int) -> torch.Tensor:  # average=None
        return self.class_hits[self.ks.index(k)].double() / self.support.clamp(min=1).double()

    def mean_class(self, k: int = 1) -> float:
        """average="macro" (= utils/meters/utils.py topk_recall): mean over the classes that occurred."""
        seen = self.support > 0
        return float(self.class_accuracy(k)[seen].mean()) if bool(seen.any()) else 0.0


class _ActionCounts:
    """hits@k and the valid count of the ACTION, the (verb, noun) pair, of a meter with both heads, on the device: integer counts
    of the exact rank of the labelled pair among all Cv * Cn pairs (``ops.action_topk``: one launch per batch, k = the largest of
    ``ks``, ranks only).  A row counts when both labels lie inside their heads.  ``seen`` (a sorted int64 vector of
    the codes v * Cn + n of the training split's pairs, on the device; None: off) splits the top-1 counts into pairs that occur in
    the training split and pairs that do not: ``split`` = [seen hits, seen rows, unseen hits, unseen rows]."""

    def __init__(self, n_verbs: int, n_nouns: int, device, ks: Sequence[int] = KS, seen=None):
        self.ks, self.Cv, self.Cn = tuple(ks), int(n_verbs), int(n_nouns)
        self.hits = torch.zeros(len(self.ks), dtype=torch.int64, device=device)
        self.valid = torch.zeros((), dtype=torch.int64, device=device)
        self.seen = None if seen is None else torch.as_tensor(seen, dtype=torch.int64).to(device)
        self.split = torch.zeros(4, dtype=torch.int64, device=device)

    def update(self, verb_logits, noun_logits, verb_labels, noun_labels):
        yv, yn = verb_labels.to(torch.int64), noun_labels.to(torch.int64)
        rank = ops.action_topk(verb_logits, noun_logits, max(self.ks), labels=(yv, yn), want_prob=False, want_logp=False)["rank"]
        self.count(rank, yv, yn)
        return rank

    def count(self, rank: torch.Tensor, yv: torch.Tensor, yn: torch.Tensor):
        """The integer arithmetic on a rank vector (-1: the row does not count)."""
        ok = rank >= 0
        self.valid += ok.sum()
        for i, k in enumerate(self.ks):
            self.hits[i] += (ok & (rank < k)).sum()
        if self.seen is not None:
            code = torch.where(ok, yv.to(torch.int64) * self.Cn + yn.to(torch.int64), torch.full_like(yv, -1, dtype=torch.int64))
            known = torch.zeros_like(ok)
            if self.seen.numel():
                at = torch.searchsorted(self.seen, code).clamp(max=self.seen.numel() - 1)
                known = ok & (self.seen[at] == code)
            hit = ok & (rank < 1)
            self.split += torch.stack([(hit & known).sum(), known.sum(), (hit & ~known).sum(), (ok & ~known).sum()])

    def tensors(self) -> List[torch.Tensor]:
        return [self.hits, self.valid, self.split]

    def accuracy(self, k: int) -> float:
        return float(self.hits[self.ks.index(k)]) / max(int(self.valid), 1)

    def split_logs(self) -> dict:
        if self.seen is None:
            return {}
        sh, sn, uh, un = (int(v) for v in self.split)
        return {"actions_seen_top1": sh / max(sn, 1), "actions_seen_support": sn, "actions_unseen_top1": uh / max(un, 1),
                "actions_unseen_support": un}


class _Calibration:
    """torchmetrics MulticlassCalibrationError(num_classes, n_bins, norm, ignore_index=-1) as the reference builds it
    (utils/meters/ego4d.py:52-53, :66-67: 15 bins / l1 = the expected calibration error; 1 bin / l2 = its "Brier score") as
    per-bin SUMS on the device -- count, confidence sum, hit count -- so that it merges across shards like every other meter
    (torchmetrics keeps the confidence of every sample and bins at compute time: the same bins, the same sums)."""

    def __init__(self, n_bins: int, norm: str, device):
        if norm not in ("l1", "l2", "max"):
            raise ValueError(norm)
        self.n_bins, self.norm = n_bins, norm
        self.bounds = torch.linspace(0, 1, n_bins + 1, dtype=torch.float32, device=device)
        self.count = torch.zeros(n_bins + 1, dtype=torch.int64, device=device)  # (+1: a confidence of exactly 1 has its own bin)
        self.hits = torch.zeros(n_bins + 1, dtype=torch.int64, device=device)
        self.conf = torch.zeros(n_bins + 1, dtype=torch.float64, device=device)

    def update(self, logits: torch.Tensor, labels: torch.Tensor):
        p = logits.detach().float()
        labels = labels.to(torch.int64)
        in_unit = ((p >= 0) & (p <= 1)).all()  # (scores that already are probabilities are taken as they are)
        p = torch.where(in_unit, p, p.softmax(1))
        conf, pred = p.max(dim=1)
        ok = labels != -1
        w = ok.to(torch.float64)
        idx = (torch.bucketize(conf, self.bounds, right=True) - 1).clamp_(0, self.n_bins)
        self.count += torch.bincount(idx, weights=w, minlength=self.n_bins + 1).to(torch.int64)
        self.hits += torch.bincount(idx, weights=w * (pred == labels).to(torch.float64), minlength=self.n_bins + 1).to(torch.int64)
        self.conf += torch.bincount(idx, weights=w * conf.double(), minlength=self.n_bins + 1)

    def update_conf(self, conf: torch.Tensor, pred: torch.Tensor, labels: torch.Tensor):
        """The same bins and sums from a confidence and a prediction formed elsewhere: the calibrated scores (the raw top-1 with its
        probability at the fitted temperature, ``calibration.cross_scores``)."""
        conf, labels = conf.detach().float(), labels.to(torch.int64)
        w = (labels != -1).to(torch.float64)
        idx = (torch.bucketize(conf, self.bounds, right=True) - 1).clamp_(0, self.n_bins)
        self.count += torch.bincount(idx, weights=w, minlength=self.n_bins + 1).to(torch.int64)
        self.hits += torch.bincount(idx, weights=w * (pred == labels).to(torch.float64), minlength=self.n_bins + 1).to(torch.int64)
        self.conf += torch.bincount(idx, weights=w * conf.double(), minlength=self.n_bins + 1)

    def tensors(self) -> List[torch.Tensor]:
        return [self.count, self.hits, self.conf]

    def compute(self) -> float:
        cnt = self.count.double()
        total = float(cnt.sum())
        if total == 0:
            return 0.0
        acc = torch.nan_to_num(self.hits.double() / cnt)
        conf = torch.nan_to_num(self.conf / cnt)
        share = cnt / total
        if self.norm == "l1":
            return float((acc - conf).abs().mul(share).sum())
        if self.norm == "max":
            return float((acc - conf).abs().max())
        ce = float(((acc - conf) ** 2 * share).sum())
        return ce ** 0.5 if ce > 0 else 0.0


# ---- the cluster bootstrap of the ratio metrics (include/egopack_bootstrap.h) -----------------------------------------
def bootstrap_ratio(acc_num: torch.Tensor, acc_den: torch.Tensor):
    """float64 [R]: ``acc_num / acc_den`` per replicate, NaN where the denominator is 0 (the replicate is dropped)."""
    num, den = torch.as_tensor(acc_num).cpu().to(torch.int64), torch.as_tensor(acc_den).cpu().to(torch.int64)
    ok = den != 0
    nan = torch.full((), float("nan"), dtype=torch.float64)
    return torch.where(ok, num.double() / torch.where(ok, den, torch.ones_like(den)).double(), nan)


def bootstrap_mean_class(cls_num: torch.Tensor, cls_den: torch.Tensor):
    """float64 [R]: per replicate the mean over the classes it drew (``cls_den > 0``) of ``cls_num / cls_den`` -- what
    ``_HeadCounts.mean_class`` divides; NaN for a replicate that drew no class (it is dropped)."""
    num, den = torch.as_tensor(cls_num).cpu().to(torch.int64), torch.as_tensor(cls_den).cpu().to(torch.int64)
    seen = den > 0
    acc = torch.where(seen, num.double() / den.clamp(min=1).double(), torch.zeros((), dtype=torch.float64))
    n = seen.sum(1)
    nan = torch.full((), float("nan"), dtype=torch.float64)
    return torch.where(n > 0, acc.sum(1) / n.clamp(min=1).double(), nan)


def bootstrap_interval(values: torch.Tensor, level: float, replicates: int):
    """{"lo", "hi", "se", "valid", "dropped"} of the valid (not NaN) replicate values, or None with fewer than ``replicates`` / 2 of
    them: the values sorted, j = floor((1 - level) / 2 * n) (1e-9 is added before the floor, so that a product that is an integer in decimal is not
    rounded below it), lo = v[j], hi = v[n - 1 - j]; se = the standard deviation with divisor n - 1 (0 for n = 1)."""
    v = torch.as_tensor(values, dtype=torch.float64).reshape(-1)
    total = int(v.numel())
    v = torch.sort(v[~torch.isnan(v)]).values
    n = int(v.numel())
    if n == 0 or 2 * n < int(replicates):
        return None
    j = int(math.floor((1.0 - float(level)) / 2.0 * n + 1e-9))
    se = float(np.std(v.numpy(), ddof=1)) if n > 1 else 0.0
    return {"lo": float(v[j]), "hi": float(v[n - 1 - j]), "se": se, "valid": n, "dropped": total - n}


class _BootGroup:
    """The accumulators of ONE launch per batch: M columns of (numerator, denominator) sums per replicate and, optionally, the
    per-class (hit, support) pair of one column.  ``keys``: the log key of every column -- column 0 is the row count (num = den = 1
    on every row, key None): its ``acc_den`` is the sum of the weights, the same for every run that saw the same samples."""

    def __init__(self, R: int, keys, device, class_key=None, class_col: int = -1, n_classes: int = 0):
        self.keys, self.class_key, self.class_col = list(keys), class_key, int(class_col)
        self.acc_num = torch.zeros((R, len(self.keys)), dtype=torch.int64, device=device)
        self.acc_den = torch.zeros_like(self.acc_num)
        self.cls_num = self.cls_den = None
        if class_key is not None:
            self.cls_num = torch.zeros((R, int(n_classes)), dtype=torch.int64, device=device)
            self.cls_den = torch.zeros_like(self.cls_num)

    def tensors(self) -> List[torch.Tensor]:
        return [self.acc_num, self.acc_den, *([self.cls_num, self.cls_den] if self.cls_num is not None else ())]

    def values(self) -> Dict[str, torch.Tensor]:
        """log key -> the replicate values, float64 [R] (NaN: dropped)."""
        out = {k: bootstrap_ratio(self.acc_num[:, m], self.acc_den[:, m]) for m, k in enumerate(self.keys) if k is not None}
        if self.class_key is not None:
            out[self.class_key] = bootstrap_mean_class(self.cls_num, self.cls_den)
        return out


class _Bootstrap:
    """The seeded Poisson cluster bootstrap of a meter (``bootstrap:`` of the config with replicates > 0), in the manner of
    ``_ClassReport``: int64 accumulators on the device that join ``_sums()`` -- integers with one writer per word, so shards merge
    to the bits of the single pass -- added to by ONE ``ops.bootstrap_accumulate`` launch per group and batch.  The validation loop
    stamps the batch's cluster ids (``stamp``) before ``update``: cluster = batch ordinal * loader batch size + the row's sequence in
    the batch, ``predict.py``'s ``sample``.  ``trace`` (a list, for tests): every launch's (group, cluster, num, den, label)."""

    def __init__(self, cfg: dict, device):
        self.R, self.level, self.seed = int(cfg["replicates"]), float(cfg.get("level", 0.95)), int(cfg.get("seed", 0))
        if not 1 <= self.R <= _lib.BOOT_MAX_R:
            raise ValueError(f"bootstrap.replicates: an integer in 1 .. {_lib.BOOT_MAX_R} (got {self.R})")
        self.key, self.device = ops.bootstrap_key(self.seed), device
        self.groups: Dict[str, _BootGroup] = {}
        self.clusters = torch.zeros((), dtype=torch.int64, device=device)  # clusters seen (a sum: it merges like the rest)
        self.first = self.bound = self.nodes = None
        self.trace = None

    def add(self, name: str, keys, class_key=None, n_classes: int = 0) -> None:
        """A group with the row-count column and one column per key; ``class_key``: the mean-class key of the FIRST keyed column."""
        self.groups[name] = _BootGroup(self.R, [None, *keys], self.device, class_key, 1 if class_key is not None else -1, n_classes)

    def tensors(self) -> List[torch.Tensor]:
        return [self.clusters, *(t for g in self.groups.values() for t in g.tensors())]

    def stamp(self, first: int, batch_size: int, n_clusters: int, nodes=None) -> None:
        """The cluster ids of the next ``update``: ``first`` = ordinal * batch size, ``nodes`` = the sequence of every node."""
        self.first, self.bound = int(first), int(first) + max(int(batch_size), int(n_clusters), 1) - 1
        self.nodes = None if nodes is None else nodes.to(self.device, torch.int64) + self.first
        self.clusters += int(n_clusters)

    def node_clusters(self, rows: int) -> torch.Tensor:
        if self.nodes is None or self.nodes.shape[0] != rows:
            raise ValueError("bootstrap: the meter has no cluster id per node of this batch (the validation loops stamp them: "
                             f"{None if self.nodes is None else self.nodes.shape[0]} ids, {rows} rows)")
        return self.nodes

    def sequence_clusters(self, rows: int) -> torch.Tensor:
        if self.first is None:
            raise ValueError("bootstrap: the meter has no cluster ids of this batch (the validation loops stamp them)")
        return torch.arange(rows, dtype=torch.int64, device=self.device) + self.first

    def accumulate(self, name: str, cluster: torch.Tensor, num: torch.Tensor, den: torch.Tensor, label=None) -> None:
        g = self.groups[name]
        if self.trace is not None:
            self.trace.append((name, cluster.cpu(), num.cpu().to(torch.int64), den.cpu().to(torch.int64),
                               None if label is None or g.class_key is None else label.cpu().to(torch.int64)))
        ops.bootstrap_accumulate(cluster, num, den, g.acc_num, g.acc_den, self.key, max_cluster=self.bound,
                                 label=label if g.class_key is not None else None, class_col=g.class_col, cls_num=g.cls_num,
                                 cls_den=g.cls_den)

    def ranks(self, name: str, rank: torch.Tensor, ks, cluster: torch.Tensor, label=None) -> None:
        """Columns from a rank vector (-1: the row does not count): num = rank < k, den = rank >= 0."""
        ok = rank >= 0
        one = torch.ones_like(ok)
        num = torch.stack([one, *(ok & (rank < k) for k in ks)], 1).to(torch.int64)
        den = torch.stack([one, *(ok for _ in ks)], 1).to(torch.int64)
        self.accumulate(name, cluster, num, den, label)

    def sums(self, name: str, cluster: torch.Tensor, nums, dens) -> None:
        """Columns from integer per-row terms: ``nums`` / ``dens`` are lists of int64 [rows] (or Python ints for a constant)."""
        rows = cluster.shape[0]
        col = lambda v: v.to(torch.int64) if torch.is_tensor(v) else torch.full((rows,), int(v), dtype=torch.int64, device=self.device)  # noqa: E731
        self.accumulate(name, cluster, torch.stack([col(1), *(col(v) for v in nums)], 1), torch.stack([col(1), *(col(v) for v in dens)], 1))

    def values(self) -> Dict[str, torch.Tensor]:
        return {k: v for g in self.groups.values() for k, v in g.values().items()}

    def intervals(self) -> Dict[str, Optional[dict]]:
        """log key -> ``bootstrap_interval`` (None: fewer than R / 2 valid replicates, which a log line says)."""
        out = {}
        for k, v in self.values().items():
            out[k] = bootstrap_interval(v, self.level, self.R)
            if out[k] is None:
                logger.warning("bootstrap: %s has %d valid of %d replicates (fewer than half): no interval", k,
                               int((~torch.isnan(v)).sum()), self.R)
        return out

    def tables(self, point: dict, split=None) -> dict:
        """What ``bootstrap.save`` writes: the accumulators per group, the replicate values and the point estimate per metric,
        seed, R, level, the split's name and the number of clusters seen."""
        groups = {n: {"keys": list(g.keys), "class_key": g.class_key, "acc_num": g.acc_num.cpu(), "acc_den": g.acc_den.cpu(),
                      **({"cls_num": g.cls_num.cpu(), "cls_den": g.cls_den.cpu()} if g.cls_num is not None else {})}
                  for n, g in self.groups.items()}
        vals = self.values()
        return {"seed": self.seed, "replicates": self.R, "level": self.level, "split": split, "clusters": int(self.clusters),
                "groups": groups, "values": vals,
                "point": {k: float(point[k]) for k in vals if k in point}}


class BaseMeter:
    """utils/meters/base.py: running mean of the per-batch loss + sample counter."""

    def __init__(self, save_features: bool = False, device="cuda", class_report: bool = False, train_counts=None,
                 shots=(20, 100), top_confusions: int = 20, calibration=None, action_scores=None, bootstrap=None) -> None:
        self.device = torch.device(device)
        # the cluster bootstrap of the ratio metrics (``bootstrap``: replicates, level, seed of the config block; None or
        # replicates = 0: no state, no launch, no key): the meters register their groups of columns on ``boot``
        self.boot = _Bootstrap(bootstrap, self.device) if bootstrap and int(bootstrap.get("replicates", 0)) > 0 else None
        # action-level scores (``action_scores``: topk and the seen pairs of the config block; None: no state, no launch, no key):
        # the verb / noun meters build an ``_ActionCounts`` from it
        self.action_cfg = dict(action_scores) if action_scores else None
        # temperature calibration (``calibration``: t_range, iterations, stop, max_rows of the config block; None: no state, no
        # launch, no key): the meters that have heads fill ``temp_store`` with what they score, ``get_logs`` fits once
        self.temp_cfg = dict(calibration) if calibration else None
        self.temp_store, self._temp, self._temp_batches = None, None, 0
        self.batch_ordinal = None  # the validation loop stamps the batch's ordinal here before ``update`` (the folds follow it)
        self.loss_sum = torch.zeros((), dtype=torch.float64, device=self.device)
        self.loss_n = 0
        self.counter = 0
        # the per-class report (off: no state, no launch, no key); the meters that have heads fill ``reports``
        self.class_report, self.train_counts = bool(class_report), train_counts
        self.shots, self.top_confusions = (int(shots[0]), int(shots[1])), int(top_confusions)
        self.reports: Dict[str, tuple] = {}  # key prefix -> (_ClassReport, class names, training counts of the head or None)

    def _add_report(self, prefix: str, names, head: int) -> None:
        if not self.class_report:
            return
        tc = self.train_counts
        if tc is not None and not torch.is_tensor(tc):
            tc = tc[head]  # (the per-head list of train.label_counts)
        self.reports[prefix] = (_ClassReport(len(names), self.device), list(names), tc)

    def _report_sums(self) -> List[torch.Tensor]:
        return [t for st, _, _ in self.reports.values() for t in st.tensors()]

    def _report_metrics(self) -> Dict[str, dict]:
        return {p: report_metrics(st.confusion, st.top2, st.loss_q24, names, tc, self.shots, self.top_confusions)
                for p, (st, names, tc) in self.reports.items()}

    def _report_logs(self) -> dict:
        return {f"{p}{k}": v for p, m in self._report_metrics().items() for k, v in m.items()}

    def _report_lines(self) -> List[str]:
        return [_report_line(p.rstrip("_") or "classes", m, self.reports[p][1]) for p, m in self._report_metrics().items()]

    def report_tables(self) -> dict:
        """The non-scalar entries of the report plus the class names and the counts: what ``class_report.save`` writes."""
        out = {}
        for p, (st, names, tc) in self.reports.items():
            out.update({k: v for k, v in self._report_logs().items() if k.startswith(p) and not isinstance(v, (int, float))})
            out[f"{p}class_names"], out[f"{p}counts"] = names, st.counts.cpu()
            if tc is not None:
                out[f"{p}train_counts"] = torch.as_tensor(tc).cpu()
        return out

    # ---- temperature calibration (egopack_amd/calibration.py) -------------------------------------
    def _add_temperature(self, heads: Dict[str, int]) -> None:
        """``heads``: key prefix -> class count of every head that takes a temperature."""
        if self.temp_cfg is None:
            return
        from .calibration import LogitStore
        self.temp_store = LogitStore(heads, self.temp_cfg.get("max_rows", 1048576), self.device)

    def _temperature_append(self, heads) -> None:
        """``heads``: (key prefix, logits [N, C], labels [N]) of one batch, stored as the meter scores them."""
        if self.temp_store is None:
            return
        ordinal = self.batch_ordinal if self.batch_ordinal is not None else self._temp_batches
        self._temp_batches += 1
        for prefix, logits, labels in heads:
            self.temp_store.append(prefix, logits.detach(), labels.to(torch.int64), ordinal)
        self._temp = None

    def temperature_fit(self) -> Dict[str, dict]:
        """``calibration.fit`` over the stored rows (once; the accumulators are summed over the ranks of a process group), with the
        cross-fitted calibration error and Brier score added per head: {} with calibration off."""
        if self.temp_store is None:
            return {}
        if self._temp is None:
            from . import calibration as CAL
            reduce = CAL.all_reduce_sum()
            res = CAL.fit(self.temp_store, self.temp_cfg, reduce=reduce)
            for prefix, (in_sample, parts) in CAL.cross_scores(self.temp_store, res).items():
                ece, brier = _Calibration(15, "l1", self.device), _Calibration(1, "l2", self.device)
                for conf, pred, y in parts:
                    ece.update_conf(conf, pred, y)
                    brier.update_conf(conf, pred, y)
                if reduce is not None:
                    for t in (*ece.tensors(), *brier.tensors()):
                        reduce(t)
                res[prefix].update(calibration_error_calibrated=ece.compute(), brier_score_calibrated=brier.compute(), in_sample=bool(in_sample))
            self._temp = res
        return self._temp

    def _temperature_logs(self) -> dict:
        out = {}
        for p, r in self.temperature_fit().items():
            out.update({f"{p}temperature": r["temperature"], f"{p}nll": r["nll"], f"{p}nll_calibrated": r["nll_calibrated"],
                        f"{p}calibration_erorr_calibrated": r["calibration_error_calibrated"],  # (the spelling of the raw key)
                        f"{p}brier_score_calibrated": r["brier_score_calibrated"]})
            if r["in_sample"]:
                out[f"{p}calibration_in_sample"] = 1
        return out

    def _temperature_lines(self) -> List[str]:
        return [f"{p.rstrip('_') or 'head'} temperature: {r['temperature']:.4f} [{r['status']}, {r['iterations']} iterations, {r['rows']} rows], "
                f"NLL {r['nll']:.4f} -> {r['nll_calibrated']:.4f}, calibration error (cross-fitted{', IN SAMPLE' if r['in_sample'] else ''}) "
                f"{r['calibration_error_calibrated']:.4f}" for p, r in self.temperature_fit().items()]

    # ---- the cluster bootstrap ---------------------------------------------------------------------
    def _boot_logs(self) -> dict:
        """<key>_ci_lo / _ci_hi / _se of every covered key that has an interval: {} with the bootstrap off."""
        if self.boot is None:
            return {}
        out = {}
        for k, ci in self.boot.intervals().items():
            if ci is not None:
                out.update({f"{k}_ci_lo": ci["lo"], f"{k}_ci_hi": ci["hi"], f"{k}_se": ci["se"]})
        return out

    @staticmethod
    def _ci(logs: dict, key: str, scale: float = 1.0, digits: int = 4) -> str:
        """" [lo, hi]" of a covered key for a line of ``print_logs`` ("" without an interval)."""
        if f"{key}_ci_lo" not in logs:
            return ""
        return f" [{logs[f'{key}_ci_lo'] * scale:.{digits}f}, {logs[f'{key}_ci_hi'] * scale:.{digits}f}]"

    def bootstrap_tables(self, split=None) -> dict:
        """What ``bootstrap.save`` writes for this meter (``_Bootstrap.tables``): {} with the bootstrap off."""
        if self.boot is None:
            return {}
        return self.boot.tables({k: v for k, v in self.get_logs().items() if isinstance(v, (int, float))}, split)

    def update(self, labels, loss, *args, **kwargs) -> None:
        loss = loss.detach().double()
        if bool(torch.isnan(loss).any()):
            raise RuntimeError("Encountered `nan` values in tensor")  # MeanMetric(nan_strategy="error")
        self.loss_sum += loss.sum().to(self.device)
        self.loss_n += loss.numel()
        self.counter += labels.shape[0]

    def loss(self) -> float:
        return float(self.loss_sum) / max(self.loss_n, 1)

    # ---- combining meters (other shards of the same split) ----------------------------------------------------
    _INTS = ("loss_n", "counter")  # python-int counters
    _LISTS = ()  # attributes holding lists of 1-D tensors that concatenate across shards

    def _sums(self) -> List[torch.Tensor]:
        """Device tensors that add across shards (updated in place)."""
        return [self.loss_sum, *self._report_sums(), *(self.boot.tensors() if self.boot is not None else ())]

    def merge(self, other: "BaseMeter") -> "BaseMeter":
        """Add the state of a meter that saw another shard of the split."""
        for a, b in zip(self._sums(), other._sums()):
            a += b.to(a.device)
        for n in self._INTS:
            setattr(self, n, getattr(self, n) + getattr(other, n))
        for n in self._LISTS:
            getattr(self, n).extend(t.to(self.device) for t in getattr(other, n))
        return self

    def all_reduce(self, group=None) -> "BaseMeter":
        """Combine the meters of all ranks (every rank ends with the totals).  Two collectives for the sums (one int64,
        one float64 buffer) and, for list state, a size exchange plus one padded all-gather per list."""
        if not (dist.is_available() and dist.is_initialized()) or dist.get_world_size(group) == 1:
            return self
        world = dist.get_world_size(group)
        sums = self._sums()
        ints = torch.tensor([getattr(self, n) for n in self._INTS], dtype=torch.int64, device=self.device)
        for dtype in (torch.int64, torch.float64):
            parts = [t for t in sums if t.dtype == dtype] + ([ints] if dtype == torch.int64 else [])
            if not parts:
                continue
            flat = torch.cat([t.reshape(-1) for t in parts])
            dist.all_reduce(flat, group=group)
            o = 0
            for t in parts:
                t.copy_(flat[o: o + t.numel()].view(t.shape))
                o += t.numel()
        for n, v in zip(self._INTS, ints.tolist()):
            setattr(self, n, v)
        for n in self._LISTS:
            mine = torch.cat(getattr(self, n)) if getattr(self, n) else None
            count = torch.tensor([0 if mine is None else mine.numel()], dtype=torch.int64, device=self.device)
            counts = [torch.zeros_like(count) for _ in range(world)]
            dist.all_gather(counts, count, group=group)
            counts = [int(c) for c in counts]
            if max(counts) == 0:
                continue
            dtype = self._list_dtype(n)
            pad = torch.zeros(max(counts), dtype=dtype, device=self.device)
            if mine is not None:
                pad[: mine.numel()] = mine.to(dtype)
            got = [torch.empty_like(pad) for _ in range(world)]
            dist.all_gather(got, pad, group=group)
            setattr(self, n, [torch.cat([g[:c] for g, c in zip(got, counts)])])
        return self

    def _list_dtype(self, name: str) -> torch.dtype:
        return torch.float32

    def print_logs(self) -> List[str]:
        return [*self._report_lines(), *self._temperature_lines(), f"Loss: {self.loss():.4f}"]

    def get_logs(self, *args, **kwargs) -> Dict[str, float]:
        return {"loss": self.loss(), **self._report_logs(), **self._temperature_logs(), **self._boot_logs()}


class _VerbNounMeter(BaseMeter):
    # what the bootstrap covers of a head: the key of top-k per k, the ks, the key of mean-class top-1 (None: not logged here)
    BOOT_TOPK, BOOT_KS, BOOT_MC, BOOT_ACTION_KS = "{name}_top{k}", KS, "{name}_mc", KS

    def __init__(self, dataset, *args, **kwargs) -> None:
        super().__init__(*args, **kwargs)
        self.dataset = dataset
        self.idx_verbs, self.idx_nouns = dataset.label_names.index("verbs"), dataset.label_names.index("nouns")
        self.verb_labels, self.noun_labels = dataset.class_labels[self.idx_verbs], dataset.class_labels[self.idx_nouns]
        self.verbs = _HeadCounts(len(self.verb_labels), self.device)
        self.nouns = _HeadCounts(len(self.noun_labels), self.device)
        # (the reference builds its noun table from the VERB matrix, utils/meters/ego4d.py:148; here the nouns get the nouns' matrix)
        self._add_report("verbs_", self.verb_labels, self.idx_verbs)
        self._add_report("nouns_", self.noun_labels, self.idx_nouns)
        self._add_temperature({"verbs_": len(self.verb_labels), "nouns_": len(self.noun_labels)})
        self.actions = None  # (action_scores off: no state, no launch, no key)
        if self.action_cfg is not None:
            self.actions = _ActionCounts(len(self.verb_labels), len(self.noun_labels), self.device, seen=self.action_cfg.get("seen"))
        if self.boot is not None:  # one group (= one launch per batch) per head, one for the action ranks
            for name, names in (("verbs", self.verb_labels), ("nouns", self.noun_labels)):
                self.boot.add(name, [self.BOOT_TOPK.format(name=name, k=k) for k in self.BOOT_KS],
                              self.BOOT_MC.format(name=name) if self.BOOT_MC else None, len(names))
            if self.actions is not None:
                self.boot.add("actions", [f"actions_top{k}" for k in self.BOOT_ACTION_KS])

    def _sums(self):
        return [*super()._sums(), *self.verbs.tensors(), *self.nouns.tensors(), *(self.actions.tensors() if self.actions else ())]

    def _action_logs(self, ks=KS, fmt: str = "actions_top{k}") -> dict:
        if self.actions is None:
            return {}
        return {**{fmt.format(k=k): self.actions.accuracy(k) for k in ks}, **self.actions.split_logs()}

    def _action_lines(self, ks=KS) -> List[str]:
        if self.actions is None:
            return []
        a = self.actions
        ci = self._boot_logs()
        line = "Actions " + ", ".join(f"Top-{k}: {a.accuracy(k) * 100:.2f}{self._ci(ci, f'actions_top{k}', 100, 2)}" for k in ks)
        sp = a.split_logs()
        if sp:
            line += (f"; seen pairs Top-1: {sp['actions_seen_top1'] * 100:.2f} (n={sp['actions_seen_support']}), "
                     f"unseen Top-1: {sp['actions_unseen_top1'] * 100:.2f} (n={sp['actions_unseen_support']})")
        return [line]

    @torch.no_grad()
    def _count(self, logits, labels):
        rank_v = self.verbs.update(logits[self.idx_verbs].detach(), labels[:, self.idx_verbs])
        rank_n = self.nouns.update(logits[self.idx_nouns].detach(), labels[:, self.idx_nouns])
        if self.boot is not None:  # the ranks just counted, weighted per replicate: one launch per head
            nodes = self.boot.node_clusters(labels.shape[0])
            self.boot.ranks("verbs", rank_v, self.BOOT_KS, nodes, labels[:, self.idx_verbs])
            self.boot.ranks("nouns", rank_n, self.BOOT_KS, nodes, labels[:, self.idx_nouns])
        if self.class_report:  # both heads in one launch, beside the counting above
            class_report([(logits[self.idx_verbs], labels[:, self.idx_verbs], self.reports["verbs_"][0]),
                          (logits[self.idx_nouns], labels[:, self.idx_nouns], self.reports["nouns_"][0])])
        self._temperature_append([("verbs_", logits[self.idx_verbs], labels[:, self.idx_verbs]),
                                  ("nouns_", logits[self.idx_nouns], labels[:, self.idx_nouns])])
        if self.actions is not None:  # the joint of both heads: one launch, ranks only
            rank_a = self.actions.update(logits[self.idx_verbs], logits[self.idx_nouns], labels[:, self.idx_verbs], labels[:, self.idx_nouns])
            if self.boot is not None:
                self.boot.ranks("actions", rank_a, self.BOOT_ACTION_KS, self.boot.node_clusters(labels.shape[0]))


class RecognitionMeter(_VerbNounMeter):
    def __init__(self, dataset, *args, **kwargs) -> None:
        super().__init__(dataset, *args, **kwargs)
        # ego4d.py:52-53 / :66-67: calibration error (15 bins, l1) and "Brier score" (1 bin, l2) per head
        self.calibration = {h: (_Calibration(15, "l1", self.device), _Calibration(1, "l2", self.device)) for h in ("verbs", "nouns")}

    def _sums(self):
        return [*super()._sums(), *(t for h in ("verbs", "nouns") for c in self.calibration[h] for t in c.tensors())]

    @torch.no_grad()
    def update(self, logits, labels, *args, **kwargs) -> None:
        super().update(labels, *args, **kwargs)
        self._count(logits, labels)
        for h, i in (("verbs", self.idx_verbs), ("nouns", self.idx_nouns)):
            for c in self.calibration[h]:
                c.update(logits[i], labels[:, i])

    def print_logs(self):
        v, n = self.verbs, self.nouns
        ci = self._boot_logs()
        top = lambda name, h: ", ".join(f"Top-{k}: {h.accuracy(k) * 100:.2f}{self._ci(ci, f'{name}_top{k}', 100, 2)}" for k in KS)  # noqa: E731
        return [f"Verbs {top('verbs', v)}", f"Nouns {top('nouns', n)}",
                f"Verbs Mean class: {v.mean_class() * 100:.2f}{self._ci(ci, 'verbs_mc', 100, 2)}",
                f"Nouns Mean class: {n.mean_class() * 100:.2f}{self._ci(ci, 'nouns_mc', 100, 2)}",
                f"Verbs Brier score: {self.calibration['verbs'][1].compute():.4f}",
                f"Nouns Brier score: {self.calibration['nouns'][1].compute():.4f}",
                *self._action_lines(), *super().print_logs()]

    def get_logs(self, *args, **kwargs):
        out = {}
        for name, h in (("verbs", self.verbs), ("nouns", self.nouns)):
            out.update({f"{name}_top{k}": h.accuracy(k) for k in KS})
            out[f"{name}_mc"] = h.mean_class()
            out[f"{name}_class_acc"] = {"top-1": h.class_accuracy(1).cpu(), "top-2": h.class_accuracy(2).cpu(),
                                        "top-5": h.class_accuracy(5).cpu(), "support": h.support.cpu()}
            out[f"{name}_calibration_erorr"] = self.calibration[name][0].compute()  # (sic: the reference's key, ego4d.py:174)
            out[f"{name}_brier_score"] = self.calibration[name][1].compute()
        return {**out, **self._action_logs(), **super().get_logs()}


class AnticipationMeter(_VerbNounMeter):
    BOOT_TOPK, BOOT_MC = "{name}_accuracy_top{k}", "{name}_recall_top1"

    @torch.no_grad()
    def update(self, logits, labels, *args, **kwargs) -> None:
        super().update(labels, *args, **kwargs)
        self._count(logits, labels)

    def get_logs(self, *args, **kwargs):
        out = {}
        for name, h in (("verbs", self.verbs), ("nouns", self.nouns)):
            out.update({f"{name}_accuracy_top{k}": h.accuracy(k) for k in KS})
            out.update({f"{name}_recall_top{k}": h.mean_class(k) for k in KS})  # topk_recall_fast: classes that occur
        return {**out, **self._action_logs(), **super().get_logs()}

    def print_logs(self):
        logs = self.get_logs()
        mine = [k for k in logs if k.startswith(("verbs_accuracy_top", "verbs_recall_top", "nouns_accuracy_top", "nouns_recall_top"))]
        return [", ".join(f"{k}: {logs[k] * 100:.2f}{self._ci(logs, k, 100, 2)}" for k in mine), *self._action_lines(), *super().print_logs()]


class OSCCMeter(BaseMeter):
    def __init__(self, dataset=None, *args, **kwargs) -> None:
        super().__init__(*args, **kwargs)
        self.dataset = dataset
        self.counts = _HeadCounts(2, self.device, ks=(1,))
        if self.class_report:  # one head of two classes, keys without a prefix
            tc = self.train_counts
            if tc is not None and not torch.is_tensor(tc):
                tc = tc[0]
            self.reports[""] = (_ClassReport(2, self.device), list(getattr(dataset, "oscc_class_labels", ("no_change", "change"))), tc)
        self._add_temperature({"": 2})
        if self.boot is not None:
            self.boot.add("oscc", ["accuracy"])

    def _sums(self):
        return [*super()._sums(), *self.counts.tensors()]

    @torch.no_grad()
    def update(self, logits, labels, *args, **kwargs) -> None:
        super().update(labels, *args, **kwargs)
        rank = self.counts.update(logits.detach(), labels)
        if self.boot is not None:  # (a row is a sequence)
            self.boot.ranks("oscc", rank, (1,), self.boot.sequence_clusters(labels.shape[0]))
        if self.class_report:
            class_report([(logits, labels, self.reports[""][0])])
        self._temperature_append([("", logits, labels)])

    def print_logs(self):
        return [f"Accuracy: {self.counts.accuracy(1) * 100:.2f}{self._ci(self._boot_logs(), 'accuracy', 100, 2)}", *super().print_logs()]

    def get_logs(self, *args, **kwargs):
        return {"accuracy": self.counts.accuracy(1), **super().get_logs()}


class PNRMeter(BaseMeter):
    """BinaryAccuracy / BinaryRecall at threshold 0.5 on sigmoid(logits), exact AUROC, key-frame localisation error."""

    def __init__(self, dataset=None, *args, **kwargs) -> None:
        super().__init__(*args, **kwargs)
        self.dataset = dataset
        self.stats = torch.zeros(4, dtype=torch.int64, device=self.device)  # tp, tn, positives, total
        self.probs: List[torch.Tensor] = []
        self.targets: List[torch.Tensor] = []
        self.loc_err_sum = torch.zeros((), dtype=torch.float64, device=self.device)
        self.loc_n = 0
        if self.boot is not None:  # (accuracy / recall count nodes and the AUROC is no sum of per-sample terms: no interval)
            self.boot.add("pnr", ["localization_error"])

    _INTS = (*BaseMeter._INTS, "loc_n")
    _LISTS = ("probs", "targets")

    def _sums(self):
        return [*super()._sums(), self.stats, self.loc_err_sum]

    def _list_dtype(self, name):
        return torch.float32 if name == "probs" else torch.uint8

    @torch.no_grad()
    def update(self, logits, labels, batch, start_frame, end_frame, pnr_frame, *args, **kwargs) -> None:
        super().update(labels, *args, **kwargs)
        from .models.tasks.oscc import sequence_ptr
        probs = torch.sigmoid(logits.detach().float())
        t = labels.to(torch.bool)
        pred = probs > 0.5
        self.stats += torch.stack([(pred & t).sum(), (~pred & ~t).sum(), t.sum(), torch.tensor(t.numel(), device=t.device)])
        self.probs.append(probs)
        self.targets.append(t)
        # per-sequence arg-max node (first maximum) by the segment-max kernel on the [N, 1] probabilities
        ptr = sequence_ptr(batch)
        n_seg = ptr.numel() - 1
        col = probs.contiguous().view(-1, 1)
        best = torch.empty((n_seg, 1), dtype=torch.float32, device=col.device)
        arg = torch.empty((n_seg, 1), dtype=torch.int32, device=col.device)
        ops._ck(_lib.load().egk_segment_max_fwd(ops._stream(), ops._p(col), ops._p(ptr), ops._p(best), ops._p(arg), n_seg, 1, 0),
                "egk_segment_max_fwd")
        loc = (arg.view(-1) - ptr[:-1]).double()
        sf, ef, pf = (v.to(col.device).double() for v in (start_frame, end_frame, pnr_frame))
        err_sec = ((ef - sf) / 16 * loc - (pf - sf)).abs() / 30
        self.loc_err_sum += err_sec.sum()
        self.loc_n += n_seg
        if self.boot is not None:  # seconds in 2^-24 fixed point, rounded to nearest, over 1 in the same fixed point: a row is a sequence
            self.boot.sums("pnr", self.boot.sequence_clusters(n_seg), [torch.round(err_sec * Q24).to(torch.int64)], [1 << 24])

    def auroc(self) -> float:
        """Exact area under the ROC curve (Mann-Whitney U, ties count 1/2) over everything seen."""
        if not self.probs:
            return 0.0
        p, t = torch.cat(self.probs).double(), torch.cat(self.targets).to(torch.bool)
        n_pos, n_neg = int(t.sum()), int((~t).sum())
        if n_pos == 0 or n_neg == 0:
            return 0.0
        vals, inv, counts = torch.unique(p, return_inverse=True, return_counts=True)
        ends = torch.cumsum(counts, 0).double()
        mid_rank = ends - (counts.double() - 1) / 2  # average 1-based rank of each distinct value
        r_pos = mid_rank[inv][t].sum()
        return float((r_pos - n_pos * (n_pos + 1) / 2) / (n_pos * n_neg))

    def get_logs(self, *args, **kwargs):
        tp, tn, pos, tot = (int(v) for v in self.stats)
        return {"accuracy": (tp + tn) / max(tot, 1), "recall": tp / max(pos, 1), "auroc": self.auroc(),
                "localization_error": float(self.loc_err_sum) / max(self.loc_n, 1), **super().get_logs()}

    def print_logs(self):
        l = self.get_logs()
        return [f"accuracy: {l['accuracy']:.4f}", f"recall: {l['recall']:.4f}", f"auroc: {l['auroc']:.4f}",
                f"localization_error: {l['localization_error']:.4f}{self._ci(l, 'localization_error')}", *super().print_logs()]


class LTAMeter(_VerbNounMeter):
    """Edit distance @ Z = 20 over K = 5 sampled futures (ego4d.py:410-433: sequences of 22 nodes, the 2 observed
    nodes dropped), plus top-1 accuracy on the labelled nodes."""

    N_NODES, N_SAMPLES, SKIP = 22, 5, 2
    BOOT_KS, BOOT_MC, BOOT_ACTION_KS = (1,), None, (1,)  # (the keys this meter logs: verbs_top1 / nouns_top1, actions_top1)

    def __init__(self, dataset, *args, **kwargs) -> None:
        super().__init__(dataset, *args, **kwargs)
        self.N_NODES = int(getattr(dataset, "lta_nodes", self.N_NODES))  # synthetic datasets use their own T
        self.ed_sum = torch.zeros(2, dtype=torch.float64, device=self.device)
        self.ed_n = 0
        self.action_ed_sum = torch.zeros((), dtype=torch.float64, device=self.device) if self.actions is not None else None
        self._ed_min = []  # the smallest of the K integer distances per sequence of the current update, per column, with Z
        if self.boot is not None:
            self.boot.add("ed", ["verbs_ed", "nouns_ed", *(["actions_ed"] if self.actions is not None else [])])

    _INTS = (*BaseMeter._INTS, "ed_n")

    def _sums(self):
        return [*super()._sums(), self.ed_sum, *([self.action_ed_sum] if self.action_ed_sum is not None else ())]

    def _pair_distances(self, preds, labels):
        """(verb, noun, action) distances per sequence -- the minimum over the futures of each column, divided by Z -- from ONE
        ``egk_edit_distance_pairs`` launch; ``last_pair_distances``: its int32 [N, K, 3] result."""
        pv, pn = (preds[i].reshape(-1, self.N_NODES, self.N_SAMPLES)[:, self.SKIP:] for i in (self.idx_verbs, self.idx_nouns))
        lv, ln = (labels[:, i].reshape(-1, self.N_NODES)[:, self.SKIP:] for i in (self.idx_verbs, self.idx_nouns))
        d = action_edit_distances(pv, pn, lv, ln)
        self.last_pair_distances = d
        dmin = d.min(dim=1).values
        self._ed_min += [(dmin[:, c], pv.shape[1]) for c in range(3)]
        best = dmin.double() / pv.shape[1]
        return best[:, 0], best[:, 1], best[:, 2]

    def _edit_distance(self, preds: torch.Tensor, labels: torch.Tensor) -> torch.Tensor:
        p = preds.reshape(-1, self.N_NODES, self.N_SAMPLES)[:, self.SKIP:]
        l = labels.reshape(-1, self.N_NODES)[:, self.SKIP:]
        dmin = edit_distances(p, l).min(dim=1).values
        self._ed_min.append((dmin, p.shape[1]))
        return dmin.double() / p.shape[1]

    @torch.no_grad()
    def update(self, logits, labels, predictions, *args, **kwargs) -> None:
        super().update(labels, *args, **kwargs)
        self._count(logits, labels)  # rows with negative labels are skipped by the rank kernel (labels >= 0 filter)
        self._ed_min = []
        if self.actions is not None:  # all three distances from the pair launch (the verb / noun columns are egk_edit_distance's integers)
            dv, dn, da = self._pair_distances(predictions, labels)
            self.action_ed_sum += da.sum()
        else:
            dv = self._edit_distance(predictions[self.idx_verbs], labels[:, self.idx_verbs])
            dn = self._edit_distance(predictions[self.idx_nouns], labels[:, self.idx_nouns])
        self.ed_sum += torch.stack([dv.sum(), dn.sum()])
        self.ed_n += dv.numel()
        self.last_distances = (dv, dn)
        if self.boot is not None:  # the integers behind dv / dn (/ da) over Z: a row is a sequence
            self.boot.sums("ed", self.boot.sequence_clusters(dv.numel()), [d for d, _ in self._ed_min], [z for _, z in self._ed_min])

    def get_logs(self, *args, **kwargs):
        v, n = (float(x) / max(self.ed_n, 1) for x in self.ed_sum)
        act = {}
        if self.actions is not None:
            act = {"actions_ed": float(self.action_ed_sum) / max(self.ed_n, 1), **self._action_logs(ks=(1,))}
        return {"verbs_ed": v, "nouns_ed": n, "verbs_top1": self.verbs.accuracy(1), "nouns_top1": self.nouns.accuracy(1), **act,
                **super().get_logs()}

    def print_logs(self):
        l = self.get_logs()
        return [*(f"{k}: {l[k]:.4f}{self._ci(l, k)}" for k in ("verbs_ed", "nouns_ed", "verbs_top1", "nouns_top1")),
                *([f"actions_ed: {l['actions_ed']:.4f}{self._ci(l, 'actions_ed')}", *self._action_lines(ks=(1,))] if self.actions is not None else []),
                *super().print_logs()]


def build_meter_for_dataset(dataset, save_features: bool = False, device="cuda", class_report: bool = False, train_counts=None,
                            shots=(20, 100), top_confusions: int = 20, calibration=None, action_scores=None, bootstrap=None) -> BaseMeter:
    """utils/meters/__init__.py:10-22, keyed on the dataset's ``task`` name (synthetic and Ego4D datasets alike).
    ``class_report``: the per-class report of the verb / noun and OSCC meters (PNR is binary and reports tp / tn already: it
    takes no report); ``calibration``: the temperature fit of the same meters (``train.calibration_meter_args``; PNR takes none:
    a one-logit BCE head whose export is a frame index); ``train_counts``: per head the training labels of every class (``train.label_counts``) for the
    many / medium / few-shot accuracies, ``shots`` their (lo, hi) borders, ``top_confusions`` the length of the confusion list;
    ``action_scores``: the action-level scores of the verb / noun meters (``train.action_scores_meter_args``; OSCC and PNR have no
    pair and take none); ``bootstrap``: the cluster bootstrap of every meter's ratio metrics (``train.bootstrap_meter_args``: replicates,
    level, seed; None or replicates = 0: off)."""
    kind = getattr(dataset, "task", None) or type(dataset).__name__.lower()
    rep = dict(class_report=class_report, train_counts=train_counts, shots=shots, top_confusions=top_confusions, calibration=calibration,
               bootstrap=bootstrap)
    if "pnr" in kind:
        return PNRMeter(dataset, device=device, bootstrap=bootstrap)
    if "oscc" in kind:
        return OSCCMeter(dataset, device=device, **rep)
    if "lta" in kind:
        return LTAMeter(dataset, device=device, action_scores=action_scores, **rep)
    if "anticipation" in kind:
        return AnticipationMeter(dataset, device=device, action_scores=action_scores, **rep)
    if "ar" in kind or "recognition" in kind:
        return RecognitionMeter(dataset, save_features=save_features, device=device, action_scores=action_scores, **rep)
    raise NotImplementedError(f"no meter for dataset {type(dataset).__name__}")
