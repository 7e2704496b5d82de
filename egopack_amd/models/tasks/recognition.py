"""Multi-head recognition task (AR): verb and noun classifiers over the projected clip feature.

Mirror of reference models/tasks/recognition.py:10-72 (constructor, ``classifiers`` /
``aux_classifiers`` layout, ``forward_logits`` / ``forward_aux_logits`` / ``compute_loss``)."""
from __future__ import annotations

from typing import Dict, Optional, Tuple

import torch
import torch.nn as nn

from ... import ops
from .task import ProjectionTask, TaskLiteral, apply_classifier, build_classifier, fuse_logits


class MultiHeadTask(ProjectionTask):
    """Common body of the AR and LTA heads (they differ in name and in LTA's sampler)."""

    def __init__(self, name: str, input_size: int, features_size: int, heads: Tuple[int, ...], dropout: float = 0,
                 head_dropout: float = 0, aux_tasks: Optional[Tuple[TaskLiteral, ...]] = None,
                 average_logits: bool = False):
        super().__init__(name, input_size, features_size, dropout)
        self.heads = tuple(heads)
        self.classifiers = self._build_classifier(head_dropout, heads)
        key = object()  # (identity of this bank; a deep copy of the task gets its own)
        for h, c in enumerate(self.classifiers):  # one bank: optim.FlatAdam lays their padded slots out as one matrix
            c[1].weight._egk_bank, c[1].bias._egk_bank = (key, "w", h), (key, "b", h)
        if aux_tasks:
            self.aux_classifiers = nn.ModuleDict({t: self._build_classifier(head_dropout, heads) for t in aux_tasks})
            self.average_logits = average_logits

    def _build_classifier(self, head_dropout, heads) -> nn.ModuleList:
        return nn.ModuleList([build_classifier(self.features_size, h, head_dropout) for h in heads])

    def forward_logits(self, features: torch.Tensor, batch: Optional[torch.Tensor] = None,
                       aux_features: Optional[Dict[TaskLiteral, torch.Tensor]] = None, *args, **kwargs):
        bank = getattr(self.classifiers[0][1].weight, "_egk_bank_views", None)
        if bank is not None and features.is_cuda and not (self.training and any(c[0].p > 0 for c in self.classifiers)):
            logits = ops.classifier_bank(features, self.classifiers[0][1].weight, bank)  # one contraction for all heads
        else:
            logits = tuple(apply_classifier(c, features) for c in self.classifiers)
        if aux_features is not None:
            aux = [self.forward_aux_logits(f, t) for t, f in aux_features.items()]
            logits = tuple(fuse_logits(p, [a[h] for a in aux], self.average_logits) for h, p in enumerate(logits))
        return logits

    def forward_aux_logits(self, features: torch.Tensor, t: TaskLiteral = "ar", *args, **kwargs):
        return tuple(apply_classifier(c, features) for c in self.aux_classifiers[t])

    def set_class_balance(self, weights=None, offsets=None) -> None:
        """Per-class vectors of the training loss, one entry (a vector of ``heads[h]`` values or None) per head: ``weights`` as
        nn.CrossEntropyLoss(weight=...), ``offsets`` added to the logits inside the loss only.  Non-persistent buffers: they follow
        ``.to(device)`` and stay out of the state dict, whose key layout is the reference's.  None, None removes them."""
        from ...criterion import _class_vector
        for name, vecs in (("class_weight", weights), ("class_offset", offsets)):
            vecs = list(vecs) if vecs is not None else [None] * len(self.heads)
            if len(vecs) != len(self.heads):
                raise ValueError(f"{self.name}: {len(vecs)} {name} entries for {len(self.heads)} heads")
            for h, v in enumerate(vecs):
                v = _class_vector(v, f"{self.name}: {name} of head {h}")
                if v is not None and v.numel() != self.heads[h]:
                    raise ValueError(f"{self.name}: {name} of head {h} has {v.numel()} entries, the head has {self.heads[h]} classes")
                if v is not None:
                    v = v.to(self.classifiers[h][1].weight.device)
                key = f"{name}_{h}"
                if key in self._buffers:
                    self._buffers[key] = v
                else:
                    self.register_buffer(key, v, persistent=False)

    def set_ce_shape(self, margins=None, gamma: float = 0.0) -> None:
        """The label-distribution-aware margins (one vector of ``heads[h]`` values or None per head, subtracted from the target's
        logit inside the loss) and the focal exponent of the training loss (``ops.cross_entropy(margin=, gamma=)``).  The margins
        are non-persistent buffers like the class-balance vectors.  None, 0 removes them."""
        from ...criterion import _class_vector, _focal_gamma
        vecs = list(margins) if margins is not None else [None] * len(self.heads)
        if len(vecs) != len(self.heads):
            raise ValueError(f"{self.name}: {len(vecs)} class_margin entries for {len(self.heads)} heads")
        for h, v in enumerate(vecs):
            v = _class_vector(v, f"{self.name}: class_margin of head {h}")
            if v is not None and v.numel() != self.heads[h]:
                raise ValueError(f"{self.name}: class_margin of head {h} has {v.numel()} entries, the head has {self.heads[h]} classes")
            if v is not None:
                v = v.to(self.classifiers[h][1].weight.device)
            key = f"class_margin_{h}"
            if key in self._buffers:
                self._buffers[key] = v
            else:
                self.register_buffer(key, v, persistent=False)
        self.focal_gamma = _focal_gamma(gamma, self.name)

    def ce_shape(self):
        """(margins, gamma) as ``ops.cross_entropy`` takes them: a tuple with one vector or None per head (or None), a float."""
        vecs = tuple(getattr(self, f"class_margin_{h}", None) for h in range(len(self.heads)))
        return (None if all(v is None for v in vecs) else vecs), getattr(self, "focal_gamma", 0.0)

    def class_balance(self):
        """(weights, offsets) as ``ops.cross_entropy`` takes them: a tuple with one vector or None per head, or None."""
        out = []
        for name in ("class_weight", "class_offset"):
            vecs = tuple(getattr(self, f"{name}_{h}", None) for h in range(len(self.heads)))
            out.append(None if all(v is None for v in vecs) else vecs)
        return tuple(out)

    def compute_loss(self, logits: Tuple[torch.Tensor, ...], targets: torch.Tensor, return_separate_losses: bool = False):
        """sum over heads of CrossEntropy(reduction='none', ignore_index=-1).  While training, with the class-balance vectors of
        ``set_class_balance``; a validation loss (``eval()``) is always the plain cross entropy, so curves compare across runs."""
        weights, offsets = self.class_balance() if self.training else (None, None)
        margins, gamma = self.ce_shape() if self.training else (None, 0.0)  # (``set_ce_shape``; training loss only, like the vectors)
        # (no vector, no margin, gamma 0: the plain launches)
        total = ops.cross_entropy(tuple(logits), targets, weight=weights, offset=offsets, margin=margins, gamma=gamma)
        if return_separate_losses:
            w, a, m = weights or [None] * len(logits), offsets or [None] * len(logits), margins or [None] * len(logits)
            return total, tuple(ops.cross_entropy(l, targets[:, i].contiguous(), weight=w[i], offset=a[i], margin=m[i], gamma=gamma)
                                for i, l in enumerate(logits))
        return total


class RecognitionTask(MultiHeadTask):
    def __init__(self, input_size: int, features_size: int, heads: Tuple[int, ...], dropout: float = 0,
                 head_dropout: float = 0, aux_tasks: Optional[Tuple[TaskLiteral, ...]] = None,
                 average_logits: bool = False):
        super().__init__("ar", input_size, features_size, heads, dropout, head_dropout, aux_tasks, average_logits)
