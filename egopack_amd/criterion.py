"""Loss selection wrapper (reference criterion/wrapper.py:11-82)."""
from __future__ import annotations

import logging
from typing import Optional, Sequence, Tuple

import torch

from . import ops

logger = logging.getLogger(__name__)


def _class_vector(v, what: str) -> Optional[torch.Tensor]:
    """A per-class vector as the f32 tensor the kernels read (None stays None)."""
    if v is None:
        return None
    v = torch.as_tensor(v)
    if v.dim() != 1 or not (v.is_floating_point() or v.numel() == 0):
        raise ValueError(f"{what}: expected a 1-D floating-point vector with one entry per class, got {v.dtype} {tuple(v.shape)}")
    return v.detach().to(torch.float32).contiguous().clone()


def _focal_gamma(gamma, what: str) -> float:
    gamma = 0.0 if gamma is None else float(gamma)
    if not (gamma >= 0.0 and gamma != float("inf")):
        raise ValueError(f"{what}: the focal exponent must be finite and >= 0, got {gamma}")
    return gamma


class CrossEntropyNone(torch.nn.Module):
    """nn.CrossEntropyLoss(reduction='none', ignore_index=-1[, label_smoothing][, weight]) on the HIP path.  ``offset``: a
    per-class vector added to the logits inside the loss only (logit adjustment).  Both are non-persistent buffers (single-head
    use; ``MetricSelectorWrapper`` carries one pair per head).  ``margin`` / ``gamma``: the per-class margin subtracted from the
    target's logit and the focal exponent (``ops.cross_entropy(margin=, gamma=)``), training mode only like the vectors."""

    def __init__(self, ignore_index: int = -1, label_smoothing: float = 0.0, weight=None, offset=None, margin=None, gamma: float = 0.0):
        super().__init__()
        if ignore_index != -1:
            raise ValueError("the hot path uses ignore_index=-1")
        self.label_smoothing = label_smoothing
        self.register_buffer("weight", _class_vector(weight, "CrossEntropyNone: weight"), persistent=False)
        self.register_buffer("offset", _class_vector(offset, "CrossEntropyNone: offset"), persistent=False)
        self.register_buffer("margin", _class_vector(margin, "CrossEntropyNone: margin"), persistent=False)
        self.gamma = _focal_gamma(gamma, "CrossEntropyNone")

    def forward(self, logits, target):
        if not self.training:  # (``eval()``: the plain cross entropy)
            return ops.cross_entropy(logits, target, self.label_smoothing)
        # (no vector, no margin, gamma 0: the plain launches)
        return ops.cross_entropy(logits, target, self.label_smoothing, weight=self.weight, offset=self.offset, margin=self.margin,
                                 gamma=self.gamma)


class BCEWithLogitsNone(torch.nn.Module):
    """nn.BCEWithLogitsLoss(reduction='none'); the caller passes ``y.float()`` as the reference does.
    ``pos`` / ``neg`` / ``gamma``: the class factor of a positive / a negative node and the focal exponent, applied inside the
    kernels (``ops.bce_with_logits``) while the module is in training mode; plain attributes, all None: the plain loss."""

    def __init__(self, pos=None, neg=None, gamma=None):
        super().__init__()
        self._balance = ops.bce_shape(pos, neg, gamma, "BCEWithLogitsNone")

    def balance(self):
        """(pos, neg, gamma), or None when the criterion carries no scalar or is in ``eval()`` mode (the scalars shape the
        training loss only)."""
        return self._balance if self.training else None

    def forward(self, logits, target):
        pos, neg, gamma = self.balance() or (None, None, None)
        return ops.bce_with_logits(logits, target, pos, neg, gamma)  # (no scalar: the plain launches)


class MetricSelectorWrapper(torch.nn.Module):
    """Apply a per-head criterion to the heads selected by the dataset's label structure and sum the
    per-head loss vectors.  Needs only ``dataset.has_joint_label`` and ``dataset.num_labels``."""

    def __init__(self, criterion: torch.nn.Module, dataset, joint_label_training: bool = False, *,
                 class_weights: Optional[Sequence] = None, class_offsets: Optional[Sequence] = None,
                 class_margins: Optional[Sequence] = None, focal_gamma: float = 0.0) -> None:
        """``class_weights`` / ``class_offsets``: one per-class vector or None per head of the task (label column), applied inside
        the cross entropy of that head (``ops.cross_entropy(weight=, offset=)``); kept as non-persistent buffers.
        ``class_margins`` (one vector or None per head, buffers like them) / ``focal_gamma``: the LDAM margins and the focal
        exponent of ``ops.cross_entropy(margin=, gamma=)``."""
        super().__init__()
        if not dataset.has_joint_label and joint_label_training:
            logger.warning("The flag join_labels is set to True but the dataset has no joint label")
            joint_label_training = False
        self.criterion, self.dataset, self.joint_label = criterion, dataset, joint_label_training
        self.n_balance = 0
        for name, vecs in (("class_weight", class_weights), ("class_offset", class_offsets)):
            vecs = list(vecs) if vecs is not None else []
            if vecs and self.n_balance and len(vecs) != self.n_balance:
                raise ValueError(f"MetricSelectorWrapper: {len(vecs)} {name} entries, {self.n_balance} of the other kind")
            self.n_balance = max(self.n_balance, len(vecs))
            for h, v in enumerate(vecs):
                self.register_buffer(f"{name}_{h}", _class_vector(v, f"MetricSelectorWrapper: {name} of head {h}"), persistent=False)
        self.n_margin = len(class_margins) if class_margins is not None else 0
        for h, v in enumerate(class_margins or []):
            self.register_buffer(f"class_margin_{h}", _class_vector(v, f"MetricSelectorWrapper: class_margin of head {h}"), persistent=False)
        self.focal_gamma = _focal_gamma(focal_gamma, "MetricSelectorWrapper")

    def _heads(self, n_logits: int):
        if self.dataset.has_joint_label:
            return [n_logits - 1] if self.joint_label else list(range(self.dataset.num_labels - 1))
        return list(range(self.dataset.num_labels))

    def select_balance(self, logits: Tuple[torch.Tensor, ...]):
        """(weights, offsets) of the heads ``select`` chooses, one vector or None per chosen head -- (None, None) when the wrapper
        carries no vector or is in ``eval()`` mode (the vectors shape the training loss only)."""
        if not self.n_balance or not self.training:  # (``eval()``: the plain cross entropy, e.g. validation losses)
            return None, None
        heads = self._heads(len(logits))
        if heads and max(heads) >= self.n_balance:
            raise ValueError(f"MetricSelectorWrapper: class-balance vectors for {self.n_balance} heads, head {max(heads)} is selected")
        out = tuple(tuple(getattr(self, f"{name}_{h}", None) for h in heads) for name in ("class_weight", "class_offset"))
        return tuple(None if all(v is None for v in vecs) else vecs for vecs in out)

    def select_shape(self, logits: Tuple[torch.Tensor, ...]):
        """(margins, gamma) of the heads ``select`` chooses -- a tuple with one vector or None per chosen head (None when there is
        none) and the focal exponent -- or (None, 0.0) in ``eval()`` mode: the terms shape the training loss only."""
        if not self.training or (not self.n_margin and not self.focal_gamma):
            return None, 0.0
        margins = None
        if self.n_margin:
            heads = self._heads(len(logits))
            if heads and max(heads) >= self.n_margin:
                raise ValueError(f"MetricSelectorWrapper: margins for {self.n_margin} heads, head {max(heads)} is selected")
            margins = tuple(getattr(self, f"class_margin_{h}", None) for h in heads)
            margins = None if all(m is None for m in margins) else margins
        return margins, self.focal_gamma

    def select(self, logits: Tuple[torch.Tensor, ...], ground_truths: torch.Tensor):
        """(logits of the heads that count, their label columns, label smoothing): what ``forward`` hands to the cross
        entropy (the engine batches the cross entropies of several tasks into one launch from these)."""
        if len(logits) != ground_truths.shape[1]:
            raise ValueError("The number of predictions must match the number of ground truth labels")
        heads = self._heads(len(logits))
        smoothing = getattr(self.criterion, "label_smoothing", 0.0)
        if heads == list(range(ground_truths.shape[1])):
            return tuple(logits), ground_truths, smoothing  # all heads: the common case on the path
        return tuple(logits[h] for h in heads), ground_truths[:, heads].contiguous(), smoothing

    def select_mix(self, logits: Tuple[torch.Tensor, ...], mix):
        """The two-target argument of ``ops.cross_entropy(mix=)`` for the heads ``select`` chooses: (the partner labels' columns,
        lam) -- or None without one or in ``eval()`` mode (mixup shapes the training loss only)."""
        if mix is None or not self.training:
            return None
        y_b, lam = mix
        heads = self._heads(len(logits))
        if heads == list(range(y_b.shape[1])):
            return y_b, lam
        return y_b[:, heads].contiguous(), lam

    def forward(self, logits: Tuple[torch.Tensor, ...], ground_truths: torch.Tensor, mix=None) -> torch.Tensor:
        """``mix``: None, or (partner labels of ground_truths' shape, f32 lam per row) -- sequence mixup, training mode only."""
        sel, gt, smoothing = self.select(logits, ground_truths)
        weights, offsets = self.select_balance(logits)
        margins, gamma = self.select_shape(logits)
        mix = self.select_mix(logits, mix)
        if mix is not None:
            return ops.cross_entropy(sel, gt, smoothing, weight=weights, offset=offsets, margin=margins, gamma=gamma, mix=mix)
        # one fused per-row sum over the heads
        return ops.cross_entropy(sel, gt, smoothing, weight=weights, offset=offsets, margin=margins, gamma=gamma)
