"""Flat-buffer optimizers: torch.optim.Adam (L2 weight decay), torch.optim.AdamW and torch.optim.SGD semantics in ONE kernel launch.

All trainable parameters that actually receive gradients are re-homed as views of one contiguous
fp32 buffer (``flat_p``); their ``.grad`` are views of ``flat_g``.  The backward kernels accumulate
weight gradients straight into those views (ops._grad_slot), ``zero_grad`` is one memset, the step
is one ``egk_adam_step`` launch and the data-parallel gradient exchange all-reduces slices of the
same buffer (dist.GradSync).  Mirrors ``_target_: torch.optim.Adam`` of configs/defaults.yaml:17-20.

Parameters whose gradient is None after the first backward (disabled tasks, detached aux heads,
frozen prototypes) are left alone, exactly as torch.optim.Adam skips ``grad is None``.

``FlatOptimizer`` holds everything that is not the update rule: the flat buffers, the bank ordering, the stored gradient
slots, the bf16 copies and low halves, the device-side step constants, clipping, ``launch(grads, lo, hi, bump)``.  A rule
(``FlatAdam``, ``FlatAdamW``, ``FlatSGD``) names its per-parameter state -- two buffers, one or none, in torch's
state-dict names -- and issues its launch: ``FlatAdam`` through the egk_adam_step* entry points, the others through
egk_optim_step (include/egopack_optim.h).

Parameter groups (a list of ``{"params": [...], "lr": ..., "weight_decay": ...}`` dicts, as torch.optim takes them) may differ in
``lr`` and ``weight_decay``.  The flat layout does not depend on the grouping; the groups become a segment table over it
(``group_segments``) that every launch resolves per element, in the one launch (egk_optim_step_groups,
include/egopack_optim_groups.h).  One group -- a plain list, or a single dict -- issues exactly what it always issued.

``ema_decay`` (None or 0: off) keeps an exponential moving average of the weights in ``flat_ema``, updated INSIDE the optimizer
launch (egk_optim_step_ema, include/egopack_ema.h): it follows the steps that happen, not the ones the clip gate skips, and costs
no launch.  ``ema_weights()`` swaps the average into the parameters (bf16 copies and low halves included) for validation and for
saving; the state dict carries it under a third top-level key, ``"ema"``."""
from __future__ import annotations

import bisect
import contextlib
import ctypes as C
import logging
import math
from typing import Iterable, List

import torch

from . import _lib, ops, switches
from .ops import _ck, _p, _stream

logger = logging.getLogger("egopack")


def _minus_ranges(ranges, lo, hi):
    """``ranges`` ([a, b) pairs) without [lo, hi)."""
    out = []
    for a, b in ranges:
        if b <= lo or hi <= a:
            out.append((a, b))
            continue
        if a < lo:
            out.append((a, lo))
        if hi < b:
            out.append((hi, b))
    return out


_STATE_NAMES = {frozenset(("exp_avg", "exp_avg_sq")): "Adam / AdamW state (exp_avg, exp_avg_sq)",
                frozenset(("momentum_buffer",)): "SGD state with momentum (momentum_buffer)",
                frozenset(): "no per-parameter buffers (SGD without momentum)"}


def _refuse_unbuilt(name: str, amsgrad, maximize) -> None:
    """``amsgrad`` / ``maximize`` have no kernel; foreach / fused / capturable / differentiable are execution hints without
    arithmetic and are accepted."""
    for key, val in (("amsgrad", amsgrad), ("maximize", maximize)):
        if val:
            raise ValueError(f"{name}: {key}=True is not built (the flat-buffer kernels implement the plain rule only)")


# keys of a parameter group that may differ between groups: the kernel looks these two up per element
_PER_GROUP_KEYS = ("lr", "weight_decay")
# ... and keys that select the rule or its constants for the whole launch: a group that sets one differently is refused by name
_SHARED_KEYS = ("betas", "eps", "momentum", "dampening", "nesterov", "decoupled_weight_decay", "amsgrad", "maximize")
MAX_GROUPS, MAX_SEGMENTS = 64, 4096  # (include/egopack_optim_groups.h)


def _unique(params):
    seen, uniq = set(), []
    for p in params:
        if id(p) not in seen:
            seen.add(id(p))
            uniq.append(p)
    return uniq


# the optimizer state's element type and the rounding of a bf16 state (include/egopack_optim.h): the names the config,
# the keyword arguments and the state dict use, and the descriptor's codes
STATE_DTYPES = {"f32": torch.float32, "bf16": torch.bfloat16}
STATE_ROUNDINGS = {"nearest": 0, "stochastic": 1}


# task weighting: the modes of ``task_weighting.mode`` and the name of the parameter group that holds the log-variances
# -- the one definition engine.MTLStep, train and dist read
TASK_WEIGHTING_MODES = ("none", "manual", "uncertainty")
TASK_WEIGHTING_GROUP = "task_weighting"


class FlatOptimizer(torch.optim.Optimizer):
    def __init__(self, params: Iterable[torch.Tensor], defaults: dict, state_keys=(), max_grad_norm=None, layout_order=None,
                 ema_decay=None, ema_warmup=False, state_dtype=torch.float32, state_rounding="stochastic", state_seed=None):
        """``layout_order``: the parameters in the order their slots take in the flat buffers (default: constructor order, groups one
        after the other).  A caller that splits one list into groups hands the list in here, and the layout -- backward order, the
        regions the step slices, the classifier banks -- stays what the ungrouped optimizer builds.
        ``state_keys``: torch's state-dict names of the rule's per-parameter buffers, in the order of ``state_buffers()``.
        ``max_grad_norm`` (None or 0: off): clip the global L2 norm of the gradient to it before every update --
        torch.nn.utils.clip_grad_norm_'s arithmetic, computed on the device inside the step (see ``norm_partials``).
        ``ema_decay`` (None or 0: off; otherwise inside (0, 1)): keep ``flat_ema``, the moving average of the weights, inside every
        launch: ema += (1 - d_t) * (p_new - ema) with d_t = ema_decay, or min(ema_decay, (1 + t) / (10 + t)) at step t with
        ``ema_warmup``.
        ``state_dtype`` (torch.float32, or torch.bfloat16): the element type of the state buffers.  A bf16 state is read widened,
        the update runs in f32 as ever and only what is stored is rounded: ``state_rounding`` = "stochastic" (unbiased; every
        rounding bit is a function of ``state_seed``, the counted step and the element's place in the flat buffers) or "nearest"
        (which stalls exp_avg_sq: DESIGN 3.16).  ``state_seed`` (None: the process seed of ``ops.manual_seed`` when the optimizer is
        built): the Philox key is ``ops.optim_state_key`` of it."""
        params = [p for p in params]
        if isinstance(state_dtype, str):
            state_dtype = STATE_DTYPES.get(state_dtype.lower(), state_dtype)
        if state_dtype not in STATE_DTYPES.values():
            raise ValueError(f"{type(self).__name__}: state_dtype must be torch.float32 or torch.bfloat16, got {state_dtype!r}")
        if state_rounding not in STATE_ROUNDINGS:
            raise ValueError(f"{type(self).__name__}: state_rounding must be one of {', '.join(STATE_ROUNDINGS)}, got {state_rounding!r}")
        if state_seed is not None and (isinstance(state_seed, bool) or not isinstance(state_seed, int) or not 0 <= state_seed < 2 ** 64):
            raise ValueError(f"{type(self).__name__}: state_seed must be None or an integer in [0, 2^64), got {state_seed!r}")
        if state_dtype is torch.bfloat16 and switches.enabled("sharded_update"):
            raise ValueError(f"{type(self).__name__}: state_dtype=torch.bfloat16 (optimizer_state.dtype: bf16) does not combine with the "
                             "sharded update (EGK_ENABLE=sharded_update): dist.GradSync slices and all-gathers the moments as f32 "
                             "buffers -- keep the state in f32, or use the all-reduce exchange (the default)")
        if ema_decay is not None and ema_decay != 0 and not 0.0 < float(ema_decay) < 1.0:
            raise ValueError(f"{type(self).__name__}: ema_decay must be None, 0 (off) or inside (0, 1), got {ema_decay!r}")
        if max_grad_norm is not None and not float(max_grad_norm) >= 0.0:
            raise ValueError(f"{type(self).__name__}: max_grad_norm must be None, 0 (off) or positive, got {max_grad_norm!r}")
        if params and all(isinstance(g, dict) for g in params):
            # parameter groups: a parameter listed twice INSIDE a group is kept once; one in two groups is torch's error
            params = [{**g, "params": _unique([g["params"]] if torch.is_tensor(g["params"]) else list(g["params"]))} for g in params]
        elif len({id(p) for p in params}) != len(params):  # the reference passes some parameters twice
            params = _unique(params)
        super().__init__(params, defaults)
        if len(self.param_groups) > MAX_GROUPS:
            raise ValueError(f"{type(self).__name__}: at most {MAX_GROUPS} parameter groups (got {len(self.param_groups)})")
        self._check_groups()
        self.layout_order = list(layout_order) if layout_order is not None else None
        self._segments = None       # [(begin, end, group)] over the flat buffers once materialised
        self._group_host = None     # the per-group (lr, weight_decay) last uploaded
        self.flat_p = self.flat_g = self.flat_w16 = None
        self._state_keys = tuple(state_keys)
        self._state_bufs: List[torch.Tensor] = []  # one flat buffer of ``state_dtype`` per state key
        self.active: List[torch.Tensor] = []
        self.step_count = 0
        self.grad_scale = 1.0
        self._hyper = None
        self.flat_w16lo = None      # bf16 LOW halves of the parameters (p - bf16(p)), built on demand: ensure_lo_shadows
        self._lo_fresh = []         # [lo, hi) ranges of flat_w16lo that match flat_p (cleared by every write to flat_p)
        self._moment_views = {}     # id(param) -> one view per state buffer once materialised
        self._slot_of = {}          # id(param) -> (first element, slot length) in the flat buffers
        self._pending_state = None  # a state dict loaded before the flat buffers exist
        self.max_grad_norm = float(max_grad_norm) if max_grad_norm else 0.0
        self.norm_regions = None    # [lo, hi) pieces the eager ``step`` takes the norm's partial sums over (None: one piece)
        self._norm_cursor = 0       # partial-sum slots written since the last ``norm_finalize``
        self.ema_decay = float(ema_decay) if ema_decay else 0.0
        self.ema_warmup = bool(ema_warmup)
        self.flat_ema = None        # the moving average of flat_p (same layout), with ``ema_decay`` only
        self._ema_swapped = False   # inside ``ema_weights()``: flat_p holds the average, flat_ema the raw weights
        self.task_weighting = "none"  # the step's task_weighting.mode (engine.MTLStep sets it; dist.GradSync reads it)
        self.state_dtype = state_dtype
        self.state_rounding = state_rounding
        self.state_seed = int(ops._rng["seed"] if state_seed is None else state_seed)  # (the seed itself; the key: ops.optim_state_key)

    @property
    def bf16_state(self) -> bool:
        """The state buffers hold bf16 (``state_dtype=torch.bfloat16``)."""
        return self.state_dtype is torch.bfloat16

    def _state_entries(self) -> dict:
        """The three top-level keys the state dict of a bf16 state carries beside torch's (torch.optim ignores them).  An f32 state
        writes the dict it always wrote: a dict without the keys IS an f32 state."""
        if not self.bf16_state:
            return {}
        return {"state_dtype": "bf16", "state_rounding": self.state_rounding, "state_seed": self.state_seed}

    @property
    def ema(self) -> bool:
        """A moving average of the weights is kept (``ema_decay`` > 0)."""
        return self.ema_decay > 0.0

    # -- parameter groups ---------------------------------------------------------------------------------------------------------
    @property
    def grouped(self) -> bool:
        """Several parameter groups: the launches resolve lr / weight_decay per element (one group: the plain entry points)."""
        return len(self.param_groups) > 1

    def _check_groups(self) -> None:
        """Groups may differ in ``lr`` and ``weight_decay``; any other key that differs is refused by name."""
        first = self.param_groups[0]
        for gi, g in enumerate(self.param_groups[1:], 1):
            for key in (*self.defaults, *(k for k in _SHARED_KEYS if k not in self.defaults)):
                if key not in _PER_GROUP_KEYS and g.get(key) != first.get(key):
                    raise ValueError(f"{type(self).__name__}: parameter groups 0 and {gi} differ in {key!r} ({first.get(key)!r} and "
                                     f"{g.get(key)!r}) -- only {' and '.join(_PER_GROUP_KEYS)} may differ between groups")

    def _all_params(self) -> list:
        """Every parameter in constructor order, groups one after the other: the indices of the state dict."""
        return [p for g in self.param_groups for p in g["params"]]

    def _live(self) -> list:
        """The parameters that have a gradient, in layout order."""
        live = [p for p in self._all_params() if p.requires_grad and p.grad is not None]
        if self.layout_order is not None:  # (stable: parameters the order does not name follow, in constructor order)
            pos = {id(p): i for i, p in reversed(list(enumerate(self.layout_order)))}
            live.sort(key=lambda p: pos.get(id(p), len(pos)))
        return live

    @staticmethod
    def _slot_len(p) -> int:
        # slots aligned to 16 bytes in the bf16 shadow (32 B in f32).  A matrix whose row count is not a multiple of
        # 64 (the classifier layers: 478, 115, 2 ... rows) gets its slot padded to whole 64-row blocks: the padding
        # stays zero under every rule (zero gradient, zero state, zero weight), and the padded bf16 copy is the K-major
        # operand of the layer's dX contraction on the pipelined kernel (ops._Linear.backward).
        if p.dim() == 2 and p.shape[0] % 64:
            n = (p.shape[0] + 63) // 64 * 64 * p.shape[1]
        elif p.dim() == 1 and getattr(p, "_egk_bank", None) is not None:
            n = (p.numel() + 63) // 64 * 64  # a bank's bias vector lines up with the padded rows of its weights
        else:
            n = p.numel()
        return (n + 7) // 8 * 8

    def _layout(self, live):
        """(parameters in flat order, slot lengths, segments) -- host arithmetic only.  The order is that of the live parameters of
        all groups, banks pulled together: it does not depend on the grouping.  A slot with its alignment and 64-row padding belongs
        to its parameter's group; adjacent slots of one group merge into one segment ``(begin, end, group)``."""
        group_of = {id(p): gi for gi, g in enumerate(self.param_groups) for p in g["params"]}
        live = self._bank_order(live)
        sizes = [self._slot_len(p) for p in live]
        segs, off = [], 0
        for p, sz in zip(live, sizes):
            gi = group_of[id(p)]
            if segs and segs[-1][2] == gi:
                segs[-1] = (segs[-1][0], off + sz, gi)
            else:
                segs.append((off, off + sz, gi))
            off += sz
        self._check_segments(segs, off)
        return live, sizes, segs

    def _check_segments(self, segs, total) -> None:
        at = 0
        for b, e, gi in segs:
            if b != at or e <= b or b % 4 or e % 4 or not 0 <= gi < len(self.param_groups):
                raise RuntimeError(f"{type(self).__name__}: bad segment table at [{b}, {e}) of group {gi} (expected begin {at}; "
                                   "boundaries are multiples of 4, sorted, without gaps)")
            at = e
        if at != total:
            raise RuntimeError(f"{type(self).__name__}: the segment table covers [0, {at}) of {total} elements")
        if self.grouped and len(segs) > MAX_SEGMENTS:
            raise RuntimeError(f"{type(self).__name__}: {len(segs)} segments of alternating parameter groups; one launch resolves at "
                               f"most {MAX_SEGMENTS}")

    def group_segments(self) -> list:
        """``[(begin, end, group)]``: which parameter group owns which elements of the flat buffers -- sorted, gap-free, boundaries
        multiples of 4.  Before the flat buffers exist: the table they would get from the parameters that have a gradient now."""
        if self._segments is not None:
            return list(self._segments)
        live = self._live()
        if not live:
            raise RuntimeError(f"{type(self).__name__}.group_segments(): no parameter has a gradient")
        return self._layout(live)[2]

    # -- construction of the flat buffers (first step, once the set of live gradients is known) -------
    def _materialise(self):
        live = self._live()
        if not live:
            raise RuntimeError(f"{type(self).__name__}.step(): no parameter has a gradient")
        dev = live[0].device
        if dev.type != "cuda":
            raise RuntimeError(f"{type(self).__name__} needs parameters on a ROCm device (no CPU fallback)")
        live, sizes, self._segments = self._layout(live)
        total = sum(sizes)
        self.flat_p = torch.zeros(total, dtype=torch.float32, device=dev)
        self.flat_g = torch.zeros(total, dtype=torch.float32, device=dev)
        self._state_bufs = [torch.zeros(total, dtype=self.state_dtype, device=dev) for _ in self._state_keys]
        self.flat_w16 = torch.zeros(total, dtype=torch.bfloat16, device=dev)  # bf16 operand copies of the weights
        off = 0
        with torch.no_grad():
            for p, sz in zip(live, sizes):
                n = p.numel()
                self.flat_p[off:off + n].copy_(p.data.reshape(-1))
                self.flat_g[off:off + n].copy_(p.grad.reshape(-1))
                p.data = self.flat_p[off:off + n].view(p.shape)
                p.grad = self.flat_g[off:off + n].view(p.shape)
                p._egk_shadow = self.flat_w16[off:off + n].view(p.shape)
                self._moment_views[id(p)] = tuple(b[off:off + n].view(p.shape) for b in self._state_bufs)
                self._slot_of[id(p)] = (off, sz)
                p._egk_lo_init = self.ensure_lo_shadows
                if p.dim() == 2 and p.shape[0] % 64 and p.shape[1] % 8 == 0:
                    rows64 = (p.shape[0] + 63) // 64 * 64
                    p._egk_shadow_rows64 = self.flat_w16[off:off + rows64 * p.shape[1]].view(rows64, p.shape[1])
                off += sz
        self.active = live
        if self.ema:  # (the average starts at the parameters; the padding of the slots is zero in both and stays zero)
            self.flat_ema = self.flat_p.clone()
        self._bank_views(live)
        self.refresh_shadows()
        self._hyper = torch.zeros(4, dtype=torch.float32, device=dev)
        self._hyper_src = torch.zeros(2, dtype=torch.float32, device=dev)  # {lr, grad_scale}: uploaded when they change
        self._t_dev = torch.zeros(1, dtype=torch.int64, device=dev)        # optimizer steps taken (device-side counter)
        self._src_host, self._t_mirror = None, 0
        if self.grouped or self._group_table_always:  # the tables every launch resolves lr / weight_decay from (group_hyper: uploaded by sync_hyper_source)
            segs = self._segments
            self._seg_begin = torch.tensor([b for b, _, _ in segs] + [segs[-1][1]], dtype=torch.int64, device=dev)
            self._seg_group = torch.tensor([gi for _, _, gi in segs], dtype=torch.int32, device=dev)
            self._group_hyper = torch.zeros(len(self.param_groups), 4, dtype=torch.float32, device=dev)
            self._group_host = None
        if self.clipping:
            self._norm_buffers()
        if self._pending_state is not None:
            self._apply_state(self._pending_state)
            self._pending_state = None

    # -- classifier banks: several Linear layers over the SAME input (verb / noun classifiers of a head) ---------------
    # Their parameters carry ``_egk_bank = (owner, "w" | "b", index)`` (models/tasks/task.py).  The weights of a bank get
    # adjacent slots, and so do its biases: the zero-padded 64-row blocks of the members then form ONE [sum rows64, K]
    # matrix in the flat buffers (weights, bf16 copies, gradients), and the bank runs as one contraction forward, one for
    # dX, one for dW (ops.classifier_bank) instead of one of each per member.
    @staticmethod
    def _bank_order(live):
        groups, out, done = {}, [], set()
        for p in live:
            b = getattr(p, "_egk_bank", None)
            if b is not None:
                groups.setdefault((b[0], b[1]), []).append((b[2], p))
        for p in live:
            b = getattr(p, "_egk_bank", None)
            if b is None:
                out.append(p)
            elif (b[0], b[1]) not in done:
                done.add((b[0], b[1]))
                out.extend(q for _, q in sorted(groups[(b[0], b[1])], key=lambda t: t[0]))
        return out

    def _bank_views(self, live):
        banks = {}
        for p in live:
            b = getattr(p, "_egk_bank", None)
            if b is not None:
                banks.setdefault(b[0], {}).setdefault(b[1], []).append((b[2], p))
                p._egk_bank_views = None
        for kinds in banks.values():
            ws = [q for _, q in sorted(kinds.get("w", []), key=lambda t: t[0])]
            bs = [q for _, q in sorted(kinds.get("b", []), key=lambda t: t[0])]
            if len(ws) < 2 or len(bs) != len(ws) or len({w.shape[1] for w in ws}) != 1 or ws[0].shape[1] % 64:
                continue
            cols = ws[0].shape[1]
            rows64 = [(w.shape[0] + 63) // 64 * 64 for w in ws]
            offs_w, offs_b = [self._slot_of[id(w)][0] for w in ws], [self._slot_of[id(b)][0] for b in bs]
            ok = all(offs_w[i + 1] == offs_w[i] + rows64[i] * cols for i in range(len(ws) - 1))
            ok = ok and all(offs_b[i + 1] == offs_b[i] + rows64[i] for i in range(len(bs) - 1))
            ok = ok and all(b.numel() == w.shape[0] for w, b in zip(ws, bs))
            if not ok:
                continue
            n, ow, ob = sum(rows64), offs_w[0], offs_b[0]
            starts = [sum(rows64[:i]) for i in range(len(ws))]
            ws[0]._egk_bank_views = {
                "rows": [(st, w.shape[0]) for st, w in zip(starts, ws)], "n": n, "k": cols,
                "w16": self.flat_w16[ow:ow + n * cols].view(n, cols), "wp": self.flat_p[ow:ow + n * cols].view(n, cols),
                "wg": self.flat_g[ow:ow + n * cols].view(n, cols), "b": self.flat_p[ob:ob + n], "bg": self.flat_g[ob:ob + n]}

    def region_of(self, params) -> tuple:
        """[lo, hi) of the flat buffers spanned by ``params`` (those that live there); (0, 0) if none does."""
        slots = [self._slot_of[id(p)] for p in params if id(p) in self._slot_of]
        if not slots:
            return (0, 0)
        return (min(o for o, _ in slots), max(o + n for o, n in slots))

    def state_buffers(self) -> List[torch.Tensor]:
        """The rule's flat state buffers (Adam, AdamW: exp_avg, exp_avg_sq; SGD with momentum: the momentum buffer; SGD without:
        none), each laid out like ``flat_p``; empty before the flat buffers exist."""
        return list(self._state_bufs)

    # -- checkpointing: the layout of the torch class's state dict (per-parameter ``step`` + the rule's buffers) -----
    def state_dict(self):
        """``{"state": {index: {"step", *state keys}}, "param_groups": [...]}`` with parameter indices in constructor order --
        loadable by the torch class of the rule over the same parameter list and vice versa.  (torch.optim.SGD keeps no
        ``step``; the entry is harmless to it and tells a resumed run that its first step has happened.)  The buffers are f32
        tensors whatever ``state_dtype`` is -- a bf16 state widened, which is exact -- and with a bf16 state ``state_dtype``,
        ``state_rounding`` and ``state_seed`` travel as three more top-level keys."""
        if getattr(self, "_moments_sharded", False):
            raise RuntimeError(f"{type(self).__name__}.state_dict(): the moments are sharded over the ranks (dist.GradSync shard_update: "
                               "every rank holds its own 1 / world slice, zeros elsewhere) -- call GradSync.gather_moments(optimizer) "
                               "on EVERY rank before saving")
        state, groups, i = {}, [], 0
        for group in self.param_groups:  # (torch's layout: the indices run on across the groups)
            pg = {k: v for k, v in group.items() if k != "params"}
            pg["params"] = list(range(i, i + len(group["params"])))
            groups.append(pg)
            for p in group["params"]:
                mv = self._moment_views.get(id(p))
                if mv is not None:
                    state[i] = {"step": torch.tensor(float(self._steps_taken())),
                                **{k: v.detach().float().clone() for k, v in zip(self._state_keys, mv)}}
                i += 1
        if self._pending_state is not None and not state:
            # (the loaded state, with THIS optimizer's groups: a state loaded without the trailing task_weighting group must not
            #  be written back as if this optimizer had none)
            return {**self._pending_state, "param_groups": groups, **self._state_entries()}
        out = {"state": state, "param_groups": groups, **self._state_entries()}
        if self.ema:
            if self._ema_swapped:
                raise RuntimeError(f"{type(self).__name__}.state_dict(): inside ema_weights() the parameters hold the average -- "
                                   "take the optimizer's state outside the context")
            values, params = {}, self._all_params()
            for i, p in enumerate(params):
                view = self._ema_view(p)
                if view is not None:
                    values[i] = view.detach().clone()
            out["ema"] = {"decay": self.ema_decay, "warmup": self.ema_warmup, "values": values}
        return out

    def _ema_view(self, p):
        """The slot of ``p`` in ``flat_ema`` in the parameter's shape (None: no slot, or no average)."""
        if self.flat_ema is None or id(p) not in self._slot_of:
            return None
        off = self._slot_of[id(p)][0]
        return self.flat_ema[off:off + p.numel()].view(p.shape)

    def load_state_dict(self, state_dict):
        """Hyper-parameters now; the state now if the flat buffers exist, otherwise when the first step builds them.  With a bf16
        state the incoming f32 buffers are rounded to nearest: exact for a dict a bf16 run wrote, a rounding (once, here) for one an
        f32 run or a torch optimizer wrote.  ``state_dtype`` / ``state_rounding`` / ``state_seed`` stay the constructor's: a state
        saved with another dtype loads, and one log line says so."""
        self._check_state_rule(state_dict)
        held = state_dict.get("state_dtype", "f32")
        if STATE_DTYPES.get(held) is not self.state_dtype and state_dict["state"]:
            logger.info("%s: the loaded optimizer state was kept in %s, this run keeps it in %s%s", type(self).__name__, held,
                        "bf16" if self.bf16_state else "f32", " (rounded to nearest once)" if self.bf16_state else " (widened, exact)")
        # A state saved WITHOUT learned task weights loads into an optimizer that has them: it lacks exactly the trailing
        # ``task_weighting`` group and its parameter (the last index), which then start with fresh moments -- an ``uncertainty`` run
        # warm-started from a fixed-weight run (train.load_task_weighting says so in its one log line).
        fresh = []
        if (len(state_dict["param_groups"]) == len(self.param_groups) - 1
                and self.param_groups[-1].get("name") == TASK_WEIGHTING_GROUP
                and sum(len(g["params"]) for g in state_dict["param_groups"]) == len(self._all_params()) - len(self.param_groups[-1]["params"])):
            fresh = list(self.param_groups[-1]["params"])
        elif len(state_dict["param_groups"]) != len(self.param_groups):  # (torch.optim.Optimizer.load_state_dict's message)
            raise ValueError("loaded state dict has a different number of parameter groups")
        ema = self._check_ema_state(state_dict)
        for group, pg in zip(self.param_groups, state_dict["param_groups"]):
            for k, v in pg.items():
                if k not in ("params", *self._fixed_keys) and k in group:
                    group[k] = v
        self._check_groups()
        if self.materialised:
            if self.ema and ema is None:
                with torch.no_grad():
                    self.flat_ema.copy_(self.flat_p)
            self._apply_state(state_dict)
        else:  # snapshot: the caller may keep using (or another optimizer may step) the tensors it handed in
            # (state buffers: as the flat buffers will hold them -- with a bf16 state rounded to nearest, f32 unchanged)
            keep = lambda k, v: v.detach().clone().to(self.state_dtype).float() if k in self._state_keys else v.detach().clone()
            self._pending_state = {"state": {i: {k: (keep(k, v) if torch.is_tensor(v) else v) for k, v in st.items()}
                                             for i, st in state_dict["state"].items()},
                                   "param_groups": state_dict["param_groups"]}
            if ema is not None:
                self._pending_state["ema"] = {"decay": ema["decay"], "warmup": ema["warmup"],
                                              "values": {i: v.detach().clone() for i, v in ema["values"].items()}}
            steps = [self._entry_steps(s) for s in state_dict["state"].values()]
            self.step_count = int(max(steps)) if steps else 0
            # The parameters with saved moments ARE the live set of the run that wrote the state: build the flat buffers
            # now, so that the first step after a resume runs on the layout (bf16 operand copies, classifier banks) every
            # later step of the interrupted run ran on -- a resumed run continues it bit for bit.
            params = self._all_params()
            live = [params[int(i)] for i in state_dict["state"] if int(i) < len(params)]
            live += [p for p in fresh if live]  # (they join the layout now: their slot follows the heads' slots as in a fresh run)
            if live and all(p.is_cuda and p.requires_grad for p in live):
                for p in live:
                    if p.grad is None:
                        p.grad = torch.zeros_like(p)
                self._materialise()

    def _check_ema_state(self, state_dict):
        """The ``"ema"`` entry of a loaded state dict that this optimizer restores (None: nothing to restore), checked before anything
        is changed.  The decay and the warm-up stay the constructor's: the entry's own are what the saved run used."""
        held = state_dict.get("ema")
        if held is None:
            if self.ema:
                logger.info("%s: the loaded optimizer state holds no weight average -- the average starts from the loaded parameters",
                            type(self).__name__)
            return None
        if not self.ema:
            logger.info("%s: the loaded optimizer state holds a weight average (decay %g) and ema_decay is off -- ignored",
                        type(self).__name__, float(held.get("decay", 0.0)))
            return None
        params = self._all_params()
        for i, v in held["values"].items():
            if int(i) >= len(params) or tuple(v.shape) != tuple(params[int(i)].shape):
                want = tuple(params[int(i)].shape) if int(i) < len(params) else None
                raise ValueError(f"{type(self).__name__}.load_state_dict(): the weight average of parameter {i} has shape "
                                 f"{tuple(v.shape)}, the parameter has {want}")
        return held

    # keys of a parameter group that select the kernel (the rule itself, the number of state buffers): a loaded state leaves them
    _fixed_keys = ()
    # a rule that resolves lr / weight_decay from the group table even with one group (FlatLAMB: per slot)
    _group_table_always = False
    # the keys only a LAMB state's parameter groups carry: what tells it from an Adam state, whose buffers have the same names
    _LAMB_KEYS = ("trust_clip", "always_adapt")

    @staticmethod
    def _entry_steps(st) -> float:
        """Steps a per-parameter state entry stands for; a torch.optim.SGD entry (a buffer, no ``step``) counts as one."""
        if "step" in st:
            return float(st["step"])
        return 1.0 if any(v is not None for v in st.values()) else 0.0

    def _check_state_rule(self, state_dict) -> None:
        """A state of another rule is refused by name, before anything is changed."""
        if not state_dict["state"]:
            return
        held = frozenset(k for st in state_dict["state"].values() for k, v in st.items() if k != "step" and v is not None)
        want = frozenset(self._state_keys)
        if held != want:
            name = lambda keys: _STATE_NAMES.get(keys, "per-parameter state (" + ", ".join(sorted(keys)) + ")")
            raise RuntimeError(f"{type(self).__name__}.load_state_dict(): the checkpoint holds {name(held)}, the configured optimizer "
                               f"is {type(self).__name__} and keeps {name(want)}")
        held_lamb = any(k in pg for pg in state_dict.get("param_groups", ()) for k in self._LAMB_KEYS)
        if held == want and held_lamb != isinstance(self, FlatLAMB):  # (Adam's and LAMB's buffers have the same names)
            raise RuntimeError(f"{type(self).__name__}.load_state_dict(): the checkpoint holds {'LAMB' if held_lamb else 'Adam / AdamW'} "
                               f"state (exp_avg, exp_avg_sq, {'with' if held_lamb else 'without'} the group keys "
                               f"{', '.join(self._LAMB_KEYS)}), the configured optimizer is {type(self).__name__}: the moments of one "
                               "rule do not continue the other")

    def _apply_state(self, state_dict):
        params = self._all_params()
        steps = []
        with torch.no_grad():
            for i, st in state_dict["state"].items():
                mv = self._moment_views.get(id(params[int(i)]))
                if mv is None:
                    continue  # saved for a parameter that receives no gradient in this run
                for k, view in zip(self._state_keys, mv):
                    view.copy_(st[k])
                steps.append(self._entry_steps(st))
            if self.ema and state_dict.get("ema") is not None:
                for i, v in state_dict["ema"]["values"].items():
                    view = self._ema_view(params[int(i)])
                    if view is not None:
                        view.copy_(v)
        if steps:
            self.step_count = int(max(steps))

    # -- low halves for the three-product ('bf16x3') contractions ---------------------------------------------------------
    # A weight enters such a contraction as hi + lo with hi = its bf16 shadow (kept by the Adam kernel) and lo = bf16(p - hi).
    # The lo buffer is allocated the first time it is asked for; ``refresh_lo_shadows(params)`` recomputes the region spanned
    # by ``params`` in ONE launch (the engine: the backbone's region at the start of the forward-only precise pass of a step),
    # and a parameter whose slot is not marked fresh when a contraction wants its lo half refreshes its own slot
    # (ops._x3_weight) -- correctness never depends on the caller having refreshed.
    def ensure_lo_shadows(self):
        if not self.materialised:
            return False
        if self.flat_w16lo is None:
            self.flat_w16lo = torch.zeros_like(self.flat_w16)
            self._lo_fresh = []
            for p in self.active:
                off, _ = self._slot_of[id(p)]
                n = p.numel()
                view = self.flat_w16lo[off:off + n].view(p.shape)
                p._egk_lo = (view, (lambda o=off, m=n: self._lo_is_fresh(o, m)), (lambda q=p: self.refresh_lo_shadows([q])))
        return True

    # Once the low halves exist the Adam launch keeps them: it writes bf16(p - bf16(p)) of the slice it updates beside the bf16
    # shadow (+ 2 B per parameter on a 30 B pass), so the precise pass at the head of the NEXT step finds them fresh instead of
    # splitting the backbone's 17 M parameters in a launch of its own at the head of the step's critical chain (38 us in BASELINE
    # config 4, profiles/r04_c4_replay_timeline.txt at 118 us).  False: the round-4 behaviour (tests: the reference).
    adam_writes_lo = True

    def _lo_is_fresh(self, off: int, n: int) -> bool:
        # (fresh ranges may have been cut by partial updates: a slot is fresh when the union of the ranges covers it)
        need = [(off, off + n)]
        for lo, hi in self._lo_fresh:
            need = [piece for a, b in need for piece in ((a, min(b, lo)), (max(a, hi), b)) if piece[1] > piece[0]]
            if not need:
                return True
        return not need

    def invalidate_lo_shadows(self):
        self._lo_fresh = []

    def refresh_lo_shadows(self, params=None):
        """flat_w16lo[lo:hi] = bf16(flat_p - bf16(flat_p)) over the region spanned by ``params`` (default: everything)."""
        if not self.ensure_lo_shadows():
            return
        lo, hi = (0, self.flat_p.numel()) if params is None else self.region_of(list(params))
        if hi <= lo or self._lo_is_fresh(lo, hi - lo):
            return
        _ck(_lib.load().egk_split_bf16(_stream(), _p(self.flat_p[lo:hi]), hi - lo, None, _p(self.flat_w16lo[lo:hi]), hi - lo, 1, hi - lo),
            "egk_split_bf16")
        self._lo_fresh.append((lo, hi))

    def refresh_shadows(self, lo: int = 0, hi=None):
        """Re-derive the bf16 operand copies of flat_p[lo:hi] (default: everything) from the f32 parameters: after
        load_state_dict, the all-gather of a sharded update, or any other write to the parameters that did not go through ``step``."""
        hi = self.flat_p.numel() if hi is None else hi
        if hi <= lo:
            return
        if self.flat_w16 is not None:
            _ck(_lib.load().egk_cast(_stream(), _p(self.flat_p[lo:hi]), 0, _p(self.flat_w16[lo:hi]), 1, hi - lo), "egk_cast")
        self._lo_fresh = _minus_ranges(self._lo_fresh, lo, hi)
        if self.flat_w16lo is not None and self.adam_writes_lo:
            # a captured step whose Adam launches keep the low halves holds NO split launch (engine.StepBase.capture): an
            # out-of-band write to the parameters (checkpoint load, a restored snapshot, gathered slices) leaves them fresh itself
            _ck(_lib.load().egk_split_bf16(_stream(), _p(self.flat_p[lo:hi]), hi - lo, None, _p(self.flat_w16lo[lo:hi]), hi - lo, 1, hi - lo),
                "egk_split_bf16")
            self._lo_fresh.append((lo, hi))

    @property
    def materialised(self) -> bool:
        return self.flat_p is not None

    def zero_grad(self, set_to_none: bool = False):
        if not self.materialised:
            return super().zero_grad(set_to_none=True)
        self.zero_flat_grads()

    def zero_flat_grads(self) -> None:
        """The flat gradient buffer cleared by one launch of the library (capturable)."""
        g = self.flat_g
        nbytes = g.numel() * g.element_size()
        if nbytes % 16 == 0 and g.data_ptr() % 16 == 0 and self._zero_all_but_stored():
            return
        if nbytes % 16 or g.data_ptr() % 16:
            g.zero_()
            return
        _ck(_lib.load().egk_zero_fill(_stream(), _p(g), nbytes), "egk_zero_fill")

    # The step constants {lr, 1-b1^t, sqrt(1-b2^t), grad_scale} are computed ON THE DEVICE (egk_adam_hyper) from a device-side
    # step counter and a two-float source {lr, grad_scale}: the launch is a node of a captured step, so a replay needs no
    # host -> device copy in front of it (4 us of copy + the gap behind it, 14 us per step of the headline workload) while lr
    # schedules and step counts keep advancing.  The host uploads the source only when lr / grad_scale change (per epoch) and
    # the counter only when ``step_count`` was set from outside (load_state_dict); ``_t_mirror`` is the value the device
    # counter will hold once everything enqueued so far has run.
    def sync_hyper_source(self) -> None:
        src = (float(self.param_groups[0]["lr"]), float(self.grad_scale))
        if src != self._src_host:
            # (a FRESH pinned staging buffer per upload: torch's caching host allocator does not hand a pinned block out again
            #  before the async copy that read it has completed)
            host = torch.empty(2, dtype=torch.float32, pin_memory=True)
            host[0], host[1] = src
            self._hyper_src.copy_(host, non_blocking=True)
            self._src_host = src
        if self.grouped or self._group_table_always:  # the per-group {lr, weight_decay, 0, 0} rows the grouped launch reads: uploaded when any of them changes
            rows = tuple((float(g["lr"]), float(g["weight_decay"])) for g in self.param_groups)
            if rows != self._group_host:
                host = torch.zeros(len(rows), 4, dtype=torch.float32, pin_memory=True)
                host[:, :2] = torch.tensor(rows, dtype=torch.float32)
                self._group_hyper.copy_(host, non_blocking=True)
                self._group_host = rows
        if self._t_mirror != self.step_count:
            host = torch.empty(1, dtype=torch.int64, pin_memory=True)
            host[0] = self.step_count
            self._t_dev.copy_(host, non_blocking=True)
            self._t_mirror = self.step_count

    def prepare_hyper(self, in_capture: bool = False):
        """The constants of the NEXT step (t = step_count + 1), on the current stream.  ``in_capture``: the launch is being
        recorded into a graph -- the caller has called ``sync_hyper_source`` before the capture and calls
        ``note_captured_step`` after every replay."""
        b1, b2 = self.param_groups[0].get("betas", (0.0, 0.0))  # (a rule without betas: both bias corrections come out as 1)
        self._norm_cursor, self._norm_covered = 0, 0  # (a step abandoned between its partial sums and its finalize leaves nothing behind)
        if not in_capture:
            self.sync_hyper_source()
        _ck(_lib.load().egk_adam_hyper(_stream(), _p(self._hyper_src), _p(self._t_dev), float(b1), float(b2), _p(self._hyper)),
            "egk_adam_hyper")
        if not in_capture:
            self._t_mirror += 1

    def note_captured_step(self) -> None:
        """A replayed graph that contains the constants launch has been enqueued: the device counter moves on with it."""
        self._t_mirror += 1

    # -- gradient slots with ONE writer per step: stored, not accumulated -----------------------------------------------------------
    # The flat gradient buffer is cleared every step (100-260 MB beside the forward pass) so that the weight-gradient launches can
    # ADD into it -- which also makes each of them read its zeros back.  A weight matrix whose gradient comes from exactly one
    # launch per step needs neither: that launch stores.  Which slots those are is LEARNT from an eager step (every dW-form launch
    # into a parameter's slot is counted; a slot counted once qualifies) and CHECKED in the capture: a stored slot written twice,
    # or not at all, is an error -- never a silently wrong gradient.  Every capture: one rank, the staged graphs, the one-graph exchange.
    def _matrix_index(self):
        idx = getattr(self, "_mat_index", None)
        if idx is None:
            idx = self._mat_index = {self._slot_of[id(p)][0]: tuple(p.shape) for p in self.active
                                     if p.dim() == 2 and getattr(p, "_egk_bank", None) is None}
        return idx

    def learn_begin(self):
        """Provider for ops.set_grad_slot_provider during an EAGER step: counts the launches per matrix slot, changes nothing."""
        idx, g0, counts = self._matrix_index(), self.flat_g.data_ptr(), {}
        self._learn_counts = counts

        def provider(out, M, N, ldc):
            d = out.data_ptr() - g0
            if d >= 0 and d % 4 == 0 and ldc == N and idx.get(d // 4) == (M, N):
                counts[d // 4] = counts.get(d // 4, 0) + 1
            return None
        return provider

    def learn_end(self):
        idx = self._matrix_index()
        self.store_slots = {off: idx[off][0] * idx[off][1] for off, c in (getattr(self, "_learn_counts", None) or {}).items() if c == 1}
        self._learn_counts = None

    def store_begin(self):
        """Provider for a CAPTURE: 'store' for the learnt single-writer slots; ``zero_flat_grads`` leaves them out meanwhile."""
        slots = getattr(self, "store_slots", None)
        if not slots:
            return None
        idx, g0 = self._matrix_index(), self.flat_g.data_ptr()
        self._store_claims, self._store_active = set(), True

        def provider(out, M, N, ldc):
            d = out.data_ptr() - g0
            if d < 0 or d % 4 or ldc != N or (d // 4) not in slots or idx.get(d // 4) != (M, N):
                return None
            if d // 4 in self._store_claims:
                raise RuntimeError("grad_store: a gradient slot learnt as written once per step is written twice in the captured step "
                                   "(set EGK_DISABLE=grad_store)")
            self._store_claims.add(d // 4)
            return "store"
        return provider

    def store_end(self, ok: bool = True):
        claims, self._store_active = getattr(self, "_store_claims", None), False
        self._store_claims = None
        if ok and claims is not None and claims != set(self.store_slots):
            raise RuntimeError(f"grad_store: {len(set(self.store_slots) - claims)} gradient slot(s) left uncleared were not written by the "
                               "captured step (set EGK_DISABLE=grad_store)")

    def _zero_all_but_stored(self) -> bool:
        if not getattr(self, "_store_active", False):
            return False
        total, at, rest = self.flat_g.numel(), 0, []
        for off in sorted(self.store_slots):
            n = self.store_slots[off]
            a, b = (off + 3) // 4 * 4, (off + n) // 4 * 4  # (whole 16-byte groups INSIDE the slot stay uncleared; its ragged ends are cleared)
            if b <= a:
                continue
            if a > at:
                rest.append((at, a - at))
            at = b
        if total > at:
            rest.append((at, total - at))
        for i in range(0, len(rest), 48):
            part = rest[i:i + 48]
            bg, ln = (C.c_int64 * len(part))(*[4 * b for b, _ in part]), (C.c_int64 * len(part))(*[4 * n for _, n in part])
            _ck(_lib.load().egk_zero_fill_ranges(_stream(), _p(self.flat_g), bg, ln, len(part)), "egk_zero_fill_ranges")
        return True

    # -- global-norm gradient clipping (max_grad_norm) -------------------------------------------------------------------------------
    # torch.nn.utils.clip_grad_norm_ needs the norm on the host and a scaling pass over the gradient between backward and the
    # optimizer.  Here both stay on the device: ``norm_partials`` sums the squares of a piece of the gradient buffer (f64, one partial
    # per workgroup, one writer each -- no atomics, the same bits every time) as soon as backward has finished that piece,
    # ``norm_finalize`` adds the partials, writes grad_scale * min(1, max_norm / (norm + 1e-6)) into the grad_scale word every Adam
    # launch multiplies the gradient by, and keeps the statistics ``grad_norm_stats`` reads once per epoch.  A norm that is not
    # finite closes the gate word the step's Adam launches check: the step is skipped (parameters, moments, bf16 copies and the
    # device step counter as before it) -- where torch would write NaN into every weight.
    NORM_SLOTS = 1 << 16  # partial sums per step (1 .. 1024 per piece)

    @property
    def clipping(self) -> bool:
        return self.max_grad_norm > 0.0

    def _norm_buffers(self) -> None:
        """Partial sums, statistics and the gate word (built with the flat buffers; on first use when ``max_grad_norm`` was set later)."""
        if getattr(self, "_gate", None) is None:
            dev = self.flat_p.device
            self._norm_partials = torch.zeros(self.NORM_SLOTS, dtype=torch.float64, device=dev)
            self._norm_stats = torch.zeros(6, dtype=torch.float64, device=dev)
            self._gate = torch.ones(1, dtype=torch.int32, device=dev)

    def _steps_taken(self) -> int:
        """Optimizer steps taken.  With clipping on, skipped steps make the host's count an upper bound: the device counter is
        the truth (one synchronisation, when a checkpoint is written), and the host's count follows it."""
        if self.clipping and self.materialised and self._t_mirror == self.step_count:
            self.step_count = self._t_mirror = int(self._t_dev.item())
        return self.step_count

    def norm_partials(self, grads=None, lo: int = 0, hi=None) -> None:
        """Partial sums of squares of ``grads[lo:hi]`` (default: the f32 flat gradient; dist.GradSync hands in what Adam will read)
        into the next free slots (capturable).  Every element of the buffer must be covered exactly once before ``norm_finalize``;
        the order of the calls fixes the order of the sum."""
        if not self.clipping:
            raise RuntimeError(f"{type(self).__name__}.norm_partials(): built without max_grad_norm")
        grads = self.flat_g if grads is None else grads
        hi = self.flat_p.numel() if hi is None else hi
        if hi <= lo:
            return
        lib = _lib.load()
        self._norm_buffers()
        k = int(lib.egk_grad_sumsq_slots(hi - lo))
        if self._norm_cursor + k > self.NORM_SLOTS:
            raise RuntimeError(f"{type(self).__name__}.norm_partials(): more than {self.NORM_SLOTS} partial sums in one step")
        _ck(lib.egk_grad_sumsq(_stream(), _p(grads[lo:hi]), 1 if grads.dtype == torch.bfloat16 else 0, hi - lo,
                               _p(self._norm_partials[self._norm_cursor:]), k), "egk_grad_sumsq")
        self._norm_cursor += k
        self._norm_covered = getattr(self, "_norm_covered", 0) + (hi - lo)

    def norm_finalize(self) -> None:
        """Norm, clip coefficient (into the grad_scale word of the step constants), gate and statistics from the partial sums taken
        since the last call (capturable; behind ``prepare_hyper`` and every ``norm_partials`` of the step, in front of its Adam launches)."""
        covered, self._norm_covered = getattr(self, "_norm_covered", 0), 0
        count, self._norm_cursor = self._norm_cursor, 0
        if covered != self.flat_p.numel():
            raise RuntimeError(f"{type(self).__name__}.norm_finalize(): the partial sums cover {covered} of {self.flat_p.numel()} gradient elements")
        _ck(_lib.load().egk_grad_norm_finalize(_stream(), _p(self._norm_partials), count, _p(self._hyper_src), self.max_grad_norm,
                                               _p(self._hyper), _p(self._t_dev), _p(self._gate), _p(self._norm_stats)),
            "egk_grad_norm_finalize")

    def grad_norm_stats(self, reset: bool = True) -> dict:
        """{"steps", "mean_norm", "max_norm", "clipped", "skipped", "last_norm"} over the steps since the last reset (one device
        synchronisation).  The norm is that of the gradient Adam steps on (averaged over the ranks); mean and largest are taken
        over the steps whose norm was finite, ``skipped`` counts the others."""
        if not self.clipping:
            raise RuntimeError(f"{type(self).__name__}.grad_norm_stats(): built without max_grad_norm")
        live = self.materialised and getattr(self, "_gate", None) is not None
        vals = self._norm_stats.tolist() if live else [0.0] * 6
        steps, skipped = int(vals[0]), int(vals[4])
        out = {"steps": steps, "mean_norm": vals[1] / max(steps - skipped, 1), "max_norm": vals[2], "clipped": int(vals[3]),
               "skipped": skipped, "last_norm": vals[5]}
        if reset and live:
            self._norm_stats.zero_()
        return out

    def launch(self, grads=None, lo: int = 0, hi=None, bump=None):
        """The kernel launch alone (capturable).  ``grads``: the buffer to read gradients from (default the f32
        flat buffer; dist.GradSync hands in its bf16 copy after a compressed all-reduce).  ``[lo, hi)``: element range
        of the flat buffers to update (multiples of 8; the pipelined gradient exchange steps chunk by chunk).
        ``bump`` = (int64 device word, stride): the word moves on by ``stride`` inside this launch."""
        if self._ema_swapped:
            raise RuntimeError(f"{type(self).__name__}.launch(): inside ema_weights() the parameters hold the average -- no step there")
        grads = self.flat_g if grads is None else grads
        hi = self.flat_p.numel() if hi is None else hi
        if hi <= lo:
            return
        sl = slice(lo, hi)
        lo16 = self.flat_w16lo[sl] if (self.flat_w16lo is not None and self.adam_writes_lo) else None
        if lo16 is not None:
            # the launch also writes the low halves of the slice it updates (egk_adam_step_bump): that slice is fresh, the rest as it was
            self._lo_fresh = _minus_ranges(self._lo_fresh, lo, hi) + [(lo, hi)]
        elif self._lo_fresh:
            self._lo_fresh = []  # (the parameters move: every low half is stale)
        if self.clipping:  # (behind ``norm_finalize``: its coefficient is in the step constants, its gate decides whether the step happens)
            self._norm_buffers()
        self._launch_rule(sl, grads, lo16, bump, self._gate if self.clipping else None)

    def _launch_rule(self, sl, grads, lo16, bump, gate) -> None:
        """The rule's launch over the slice ``sl`` of the flat buffers."""
        raise NotImplementedError

    def _optim_step(self, rule: int, sl, grads, lo16, bump, gate, **scalars) -> None:
        """One egk_optim_step launch (include/egopack_optim.h); ``scalars``: the descriptor's beta1 .. nesterov.  With several
        parameter groups: one egk_optim_step_groups launch (include/egopack_optim_groups.h) over the same descriptor, the segment
        table and ``base`` = the slice's first element -- lr and weight_decay come from the table, per element.  With ``ema_decay``:
        one egk_optim_step_ema launch (include/egopack_ema.h) over the same descriptor and table (or none), the same update and
        ``flat_ema`` moved towards the new parameters inside it."""
        d = _lib.OptimDesc()
        d.rule, d.g_dtype, d.n = rule, 1 if grads.dtype == torch.bfloat16 else 0, sl.stop - sl.start
        d.p, d.g, d.hyper, d.t_dev = self.flat_p[sl].data_ptr(), grads[sl].data_ptr(), self._hyper.data_ptr(), self._t_dev.data_ptr()
        for name, buf in zip(("state0", "state1"), self._state_bufs):
            setattr(d, name, buf[sl].data_ptr())
        for name, val in scalars.items():
            setattr(d, name, val)
        d.bf16_shadow = self.flat_w16[sl].data_ptr()
        d.bf16_lo_shadow = lo16.data_ptr() if lo16 is not None else None
        if bump is not None:
            d.bump_word, d.bump = bump[0].data_ptr(), int(bump[1])
        d.gate = gate.data_ptr() if gate is not None else None
        if self.bf16_state and self._state_bufs:  # (a zeroed tail: the f32 launch as it always was)
            d.state_dtype, d.state_round = 1, STATE_ROUNDINGS[self.state_rounding]
            d.state_seed, d.elem0 = ops.optim_state_key(self.state_seed), sl.start
        t = None
        if self.grouped:
            t = _lib.OptimGroups()
            t.base, t.n_seg, t.n_groups = sl.start, self._seg_group.numel(), len(self.param_groups)
            t.seg_begin, t.seg_group, t.group_hyper = self._seg_begin.data_ptr(), self._seg_group.data_ptr(), self._group_hyper.data_ptr()
        if self.ema:
            e = _lib.EmaDesc()
            e.ema, e.decay, e.warmup = self.flat_ema[sl].data_ptr(), self.ema_decay, int(self.ema_warmup)
            _ck(_lib.load().egk_optim_step_ema(_stream(), C.byref(d), C.byref(t) if t is not None else None, C.byref(e)),
                "egk_optim_step_ema")
            return
        if t is not None:
            _ck(_lib.load().egk_optim_step_groups(_stream(), C.byref(d), C.byref(t)), "egk_optim_step_groups")
            return
        _ck(_lib.load().egk_optim_step(_stream(), C.byref(d)), "egk_optim_step")

    # -- the moving average of the weights ---------------------------------------------------------------------------------------
    @contextlib.contextmanager
    def ema_weights(self):
        """The model computes with the averaged weights inside this context (validation, saving them): ``flat_p`` and ``flat_ema``
        are exchanged by one launch (egk_ema_swap) and the bf16 copies and low halves re-derived, so every compute mode sees the
        average; on exit the same again -- parameters, copies and low halves are bit for bit what they were.  Outside captures;
        no ``step`` / ``launch`` inside, no nesting.  Before the flat buffers exist the average IS the parameters: nothing to do."""
        if not self.ema:
            raise RuntimeError(f"{type(self).__name__}.ema_weights(): built without ema_decay")
        if self._ema_swapped:
            raise RuntimeError(f"{type(self).__name__}.ema_weights(): already inside the context (no nesting)")
        self._ema_swapped = True
        try:
            self._swap_ema()
            yield self
        finally:
            try:
                self._swap_ema()
            finally:
                self._ema_swapped = False

    def _swap_ema(self) -> None:
        if not self.materialised:
            return
        _ck(_lib.load().egk_ema_swap(_stream(), _p(self.flat_p), _p(self.flat_ema), self.flat_p.numel()), "egk_ema_swap")
        self.refresh_shadows()

    @torch.no_grad()
    def step(self, closure=None, grads=None):
        if self._ema_swapped:
            raise RuntimeError(f"{type(self).__name__}.step(): inside ema_weights() the parameters hold the average -- no step there")
        if not self.materialised:
            self._materialise()
        self.prepare_hyper()
        if self.clipping:
            for lo, hi in (self.norm_regions or [(0, self.flat_p.numel())]):
                self.norm_partials(grads, lo, hi)
            self.norm_finalize()
        self.launch(grads)
        self.step_count += 1


class FlatAdam(FlatOptimizer):
    """torch.optim.Adam (L2 weight decay) through the egk_adam_step* entry points; ``decoupled_weight_decay=True``: AdamW's rule
    (``p *= 1 - lr * wd`` in front of Adam's update on the bare gradient) through egk_optim_step."""

    def __init__(self, params: Iterable[torch.Tensor], lr: float = 1e-3, betas=(0.9, 0.999), eps: float = 1e-8,
                 weight_decay: float = 0.0, max_grad_norm=None, *, decoupled_weight_decay: bool = False, amsgrad: bool = False,
                 maximize: bool = False, foreach=None, fused=None, capturable: bool = False, differentiable: bool = False,
                 layout_order=None, ema_decay=None, ema_warmup=False, state_dtype=torch.float32, state_rounding="stochastic",
                 state_seed=None):
        _refuse_unbuilt(type(self).__name__, amsgrad, maximize)
        if not 0.0 <= lr:  # (torch.optim.Adam's checks and messages)
            raise ValueError(f"Invalid learning rate: {lr}")
        if not 0.0 <= eps:
            raise ValueError(f"Invalid epsilon value: {eps}")
        if not 0.0 <= betas[0] < 1.0:
            raise ValueError(f"Invalid beta parameter at index 0: {betas[0]}")
        if not 0.0 <= betas[1] < 1.0:
            raise ValueError(f"Invalid beta parameter at index 1: {betas[1]}")
        if not 0.0 <= weight_decay:
            raise ValueError(f"Invalid weight_decay value: {weight_decay}")
        defaults = dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay)
        self.decoupled_weight_decay = bool(decoupled_weight_decay)
        if self.decoupled_weight_decay:  # (what torch.optim.Adam needs to read the saved group as AdamW's; plain Adam's group as it was)
            defaults["decoupled_weight_decay"] = True
        super().__init__(params, defaults, state_keys=("exp_avg", "exp_avg_sq"), max_grad_norm=max_grad_norm,
                         layout_order=layout_order, ema_decay=ema_decay, ema_warmup=ema_warmup, state_dtype=state_dtype,
                         state_rounding=state_rounding, state_seed=state_seed)

    _fixed_keys = ("decoupled_weight_decay",)

    # (bench.py and the tests read the moments by these names)
    @property
    def flat_m(self):
        return self._state_bufs[0] if self._state_bufs else None

    @property
    def flat_v(self):
        return self._state_bufs[1] if self._state_bufs else None

    def _launch_rule(self, sl, grads, lo16, bump, gate) -> None:
        g = self.param_groups[0]
        b1, b2 = g["betas"]
        n = sl.stop - sl.start
        # (several groups, the weight average, or a bf16 state: Adam's rule too goes through the descriptor, same bits)
        if self.decoupled_weight_decay or self.grouped or self.ema or self.bf16_state:
            self._optim_step(_lib.OPT_ADAMW if self.decoupled_weight_decay else _lib.OPT_ADAM, sl, grads, lo16, bump, gate,
                             beta1=b1, beta2=b2, eps=g["eps"], weight_decay=g["weight_decay"])
            return
        # (no low halves, no offset word, no gate: null, which is what egk_adam_step / egk_adam_step_bump hand on)
        _ck(_lib.load().egk_adam_step_gated(_stream(), _p(self.flat_p[sl]), _p(grads[sl]), 1 if grads.dtype == torch.bfloat16 else 0,
                                            _p(self.flat_m[sl]), _p(self.flat_v[sl]), n, _p(self._hyper), b1, b2,
                                            g["eps"], g["weight_decay"], _p(self.flat_w16[sl]), _p(lo16),
                                            _p(bump[0]) if bump is not None else None, int(bump[1]) if bump is not None else 0,
                                            _p(gate)),
            "egk_adam_step_gated")


class FlatAdamW(FlatAdam):
    """torch.optim.AdamW: ``FlatAdam(decoupled_weight_decay=True)`` with AdamW's default ``weight_decay`` of 0.01."""

    def __init__(self, params: Iterable[torch.Tensor], lr: float = 1e-3, betas=(0.9, 0.999), eps: float = 1e-8,
                 weight_decay: float = 1e-2, max_grad_norm=None, **hints):
        hints.pop("decoupled_weight_decay", None)  # (the class IS the flag)
        super().__init__(params, lr, betas, eps, weight_decay, max_grad_norm, decoupled_weight_decay=True, **hints)


class FlatSGD(FlatOptimizer):
    """torch.optim.SGD: weight decay, momentum, dampening, nesterov.  With momentum one state buffer (``momentum_buffer``), none
    without; the first step that happens stores the gradient as the buffer (the kernel reads the device step counter)."""

    def __init__(self, params: Iterable[torch.Tensor], lr: float = 1e-3, momentum: float = 0.0, dampening: float = 0.0,
                 weight_decay: float = 0.0, nesterov: bool = False, max_grad_norm=None, *, maximize: bool = False, foreach=None,
                 fused=None, capturable: bool = False, differentiable: bool = False, layout_order=None, ema_decay=None,
                 ema_warmup=False, state_dtype=torch.float32, state_rounding="stochastic", state_seed=None):
        _refuse_unbuilt(type(self).__name__, False, maximize)
        if lr < 0.0:  # (torch.optim.SGD's checks and messages)
            raise ValueError(f"Invalid learning rate: {lr}")
        if momentum < 0.0:
            raise ValueError(f"Invalid momentum value: {momentum}")
        if weight_decay < 0.0:
            raise ValueError(f"Invalid weight_decay value: {weight_decay}")
        if nesterov and (momentum <= 0 or dampening != 0):
            raise ValueError("Nesterov momentum requires a momentum and zero dampening")
        defaults = dict(lr=lr, momentum=momentum, dampening=dampening, weight_decay=weight_decay, nesterov=bool(nesterov))
        super().__init__(params, defaults, state_keys=("momentum_buffer",) if momentum != 0 else (), max_grad_norm=max_grad_norm,
                         layout_order=layout_order, ema_decay=ema_decay, ema_warmup=ema_warmup, state_dtype=state_dtype,
                         state_rounding=state_rounding, state_seed=state_seed)

    _fixed_keys = ("momentum",)  # (zero or not decides whether there is a buffer: the constructor's value stands)

    def _launch_rule(self, sl, grads, lo16, bump, gate) -> None:
        g = self.param_groups[0]
        self._optim_step(_lib.OPT_SGD, sl, grads, lo16, bump, gate, weight_decay=g["weight_decay"], momentum=g["momentum"],
                         dampening=g["dampening"], nesterov=int(bool(g["nesterov"])))


class FlatLAMB(FlatAdam):
    """LAMB (You et al. 2020; include/egopack_lamb.h): Adam's moments, the update u = m_hat / (sqrt(v_hat) + eps) + wd * p
    and, per slot of the flat layout (one parameter with its alignment and 64-row padding), p -= lr * trust * u with trust = ||p|| / ||u||.
    Three launches: ``launch`` issues egk_lamb_moments over its slice; the call that completes the coverage of the buffers issues
    egk_lamb_trust and egk_lamb_apply over everything.  ``trust_clip``: trust <= 1.  ``always_adapt``: the ratio also where
    weight_decay is 0 (default: trust 1 there).  lr and weight_decay come per slot from the parameter-group table, with one group too."""

    _fixed_keys = ("decoupled_weight_decay", *FlatOptimizer._LAMB_KEYS)
    _group_table_always = True

    def __init__(self, params: Iterable[torch.Tensor], lr: float = 1e-3, betas=(0.9, 0.999), eps: float = 1e-8,
                 weight_decay: float = 0.0, max_grad_norm=None, *, trust_clip: bool = False, always_adapt: bool = False, **hints):
        name = type(self).__name__
        if hints.pop("decoupled_weight_decay", False):
            raise ValueError(f"{name}: decoupled_weight_decay=True is not built -- LAMB's weight decay is part of the update whose norm "
                             "the trust ratio divides by")
        dt = hints.get("state_dtype", torch.float32)
        if (STATE_DTYPES.get(dt.lower(), dt) if isinstance(dt, str) else dt) is torch.bfloat16:
            raise ValueError(f"{name}: state_dtype=torch.bfloat16 (optimizer_state.dtype: bf16) is not built -- the norm launch and the "
                             "apply launch would have to agree on the rounded moments; keep the state in f32")
        if not eps > 0.0:
            raise ValueError(f"{name}: eps must be positive (got {eps}): the zero padding of a slot has exp_avg_sq = 0")
        super().__init__(params, lr, betas, eps, weight_decay, max_grad_norm, **hints)
        self.trust_clip, self.always_adapt = bool(trust_clip), bool(always_adapt)
        for g in (self.defaults, *self.param_groups):  # (the state dict's groups carry them: what tells a LAMB state from Adam's)
            g.setdefault("trust_clip", self.trust_clip)
            g.setdefault("always_adapt", self.always_adapt)
        self._check_groups()
        self._lamb_covered, self._lamb_events = 0, []

    @staticmethod
    def piece_table(sizes) -> tuple:
        """(slot_begin [n + 1], slot_piece0 [n + 1], piece_begin [pieces + 1]) of slots of ``sizes`` elements: every slot cut into
        pieces of at most ``_lib.LAMB_PIECE`` elements, the last one shorter; a piece never crosses a slot boundary."""
        begin, piece0, pieces = [0], [0], [0]
        for sz in sizes:
            if sz <= 0 or sz % 8:
                raise ValueError(f"FlatLAMB.piece_table(): a slot of {sz} elements (slots are positive multiples of 8)")
            b = begin[-1]
            pieces.extend(min(b + k + _lib.LAMB_PIECE, b + sz) for k in range(0, sz, _lib.LAMB_PIECE))
            begin.append(b + sz)
            piece0.append(len(pieces) - 1)
        return begin, piece0, pieces

    def _materialise(self):
        super()._materialise()
        dev = self.flat_p.device
        slots = sorted(self._slot_of[id(p)] for p in self.active)
        group_of = {id(p): gi for gi, g in enumerate(self.param_groups) for p in g["params"]}
        by_off = {self._slot_of[id(p)][0]: p for p in self.active}
        begin, piece0, self._piece_begin = self.piece_table([sz for _, sz in slots])
        if [off for off, _ in slots] != begin[:-1] or begin[-1] != self.flat_p.numel():
            raise RuntimeError(f"{type(self).__name__}: the slots do not tile the flat buffers")
        self._slot_params = [by_off[off] for off, _ in slots]
        self._slot_begin = torch.tensor(begin, dtype=torch.int64, device=dev)
        self._slot_piece0 = torch.tensor(piece0, dtype=torch.int32, device=dev)
        self._slot_group = torch.tensor([group_of[id(p)] for p in self._slot_params], dtype=torch.int32, device=dev)
        self._lamb_part = torch.zeros(piece0[-1], 2, 2, dtype=torch.float64, device=dev)
        self._lamb_trust = torch.ones(len(slots), dtype=torch.float32, device=dev)
        self._lamb_norms = torch.zeros(len(slots), 2, dtype=torch.float64, device=dev)
        self._lamb_covered, self._lamb_events = 0, []

    def prepare_hyper(self, in_capture: bool = False):
        super().prepare_hyper(in_capture)
        self._lamb_covered, self._lamb_events = 0, []  # (a step abandoned between two slices leaves nothing behind)

    def _piece_range(self, lo: int, hi: int) -> tuple:
        """(first piece that meets [lo, hi), how many do) from the host copy of the piece table; a range strictly inside one piece
        is refused."""
        pb = self._piece_begin
        q0, q1 = bisect.bisect_right(pb, lo) - 1, bisect.bisect_right(pb, hi - 1) - 1
        if lo % 8 or hi % 8 or lo < 0 or hi > pb[-1]:
            raise ValueError(f"{type(self).__name__}.launch(): [{lo}, {hi}) must be multiples of 8 inside [0, {pb[-1]})")
        if q0 == q1 and pb[q0] < lo and hi < pb[q0 + 1]:
            raise ValueError(f"{type(self).__name__}.launch(): [{lo}, {hi}) lies strictly inside the piece [{pb[q0]}, {pb[q0 + 1]}) of a "
                             f"parameter's slot -- the per-slot norms take a piece cut at most once per step: a gradient-exchange chunk "
                             f"(chunk_mb) must hold at least {_lib.LAMB_PIECE} elements")
        return q0, q1 - q0 + 1

    def _launch_rule(self, sl, grads, lo16, bump, gate) -> None:
        g = self.param_groups[0]
        b1, b2 = g["betas"]
        lib, lo, hi, total = _lib.load(), sl.start, sl.stop, self.flat_p.numel()
        q0, nq = self._piece_range(lo, hi)  # (not strictly inside a piece: [lo, hi] holds a piece boundary)
        if self._lamb_covered + (hi - lo) > total:
            raise RuntimeError(f"{type(self).__name__}.launch(): the slices of this step cover more than the {total} elements of the "
                               "flat buffers (prepare_hyper starts a step)")
        n_slots, n_groups = self._slot_group.numel(), len(self.param_groups)
        tables = (_p(self._slot_piece0), _p(self._slot_group), n_slots, _p(self._group_hyper), n_groups)
        _ck(lib.egk_lamb_moments(_stream(), _p(self.flat_p), _p(grads), 1 if grads.dtype == torch.bfloat16 else 0, _p(self.flat_m),
                                 _p(self.flat_v), lo, hi, q0, nq, 1, _p(self._slot_begin), *tables, _p(self._hyper),
                                 b1, b2, g["eps"], _p(self._lamb_part), _p(gate), _p(bump[0]) if bump is not None else None,
                                 int(bump[1]) if bump is not None else 0), "egk_lamb_moments")
        self._lamb_covered += hi - lo
        if self._lamb_covered < total:  # (more slices to come, maybe on other streams: the completing call waits for this one)
            ev = torch.cuda.Event()
            ev.record()
            self._lamb_events.append(ev)
            return
        for ev in self._lamb_events:
            torch.cuda.current_stream().wait_event(ev)
        self._lamb_covered, self._lamb_events = 0, []
        _ck(lib.egk_lamb_trust(_stream(), _p(self._lamb_part), *tables, int(self.trust_clip), int(self.always_adapt),
                               _p(self._lamb_trust), _p(self._lamb_norms), _p(gate)), "egk_lamb_trust")
        lo_all = self.flat_w16lo if lo16 is not None else None
        _ck(lib.egk_lamb_apply(_stream(), _p(self.flat_p), _p(self.flat_m), _p(self.flat_v), total, len(self._piece_begin) - 1,
                               _p(self._slot_begin), *tables, _p(self._hyper), g["eps"], _p(self._lamb_trust), _p(self.flat_w16),
                               _p(lo_all), _p(self.flat_ema) if self.ema else None, self.ema_decay, int(self.ema_warmup),
                               _p(self._t_dev), _p(gate)), "egk_lamb_apply")
        if lo_all is not None:
            self._lo_fresh = [(0, total)]

    def trust_ratios(self, names=None) -> dict:
        """``{name or index: (trust, ||p||, ||u||)}`` of the last step that happened, per parameter that has a slot (one device
        synchronisation).  ``names``: ``{parameter: name}`` (e.g. from ``named_parameters``); otherwise the parameter's index in
        constructor order, the state dict's."""
        if not self.materialised:
            return {}
        vals = torch.cat([self._lamb_trust.double(), self._lamb_norms.reshape(-1)]).tolist()
        n = len(self._slot_params)
        index = {id(p): i for i, p in enumerate(self._all_params())}
        names = {id(p): nm for p, nm in (names or {}).items()}
        return {names.get(id(p), index[id(p)]): (vals[s], vals[n + 2 * s], vals[n + 2 * s + 1]) for s, p in enumerate(self._slot_params)}
