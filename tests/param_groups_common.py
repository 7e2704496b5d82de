"""Shared by tests/test_gpu_param_groups.py and tests/test_gpu_bounds_param_groups.py: the problems of egk_optim_step_groups and
their references -- one egk_optim_step launch per segment with that segment's group's lr / weight_decay (the bits the grouped
launch must reproduce).  Imports without a GPU."""
import ctypes as C
import math

import torch

DEV = "cuda"
BF = torch.bfloat16
# kernel kind -> (rule code, the descriptor's scalars)
KINDS = {"adam": (0, dict()), "adamw": (1, dict()), "sgd": (2, dict()),
         "sgd_momentum": (2, dict(momentum=0.9, dampening=0.1))}
GROUP_HYPER = [(1e-2, 1e-2), (1e-2, 0.0), (1e-3, 1e-2)]  # (lr, weight_decay) of the three groups
SEG_GROUPS = [0, 1, 2, 1, 0]
# five segments: boundaries at multiples of 4, inside one wave's 256 elements, inside one 1024-element block, and (300007) whole
# workgroup blocks inside one segment beside blocks that straddle
SEG_BEGINS = {1003: [0, 100, 256, 260, 700, 1004], 4099: [0, 1028, 1032, 2048, 4000, 4100],
              300007: [0, 1000, 5120, 131076, 200000, 300008]}
ONE_GROUP = (3e-3, 2e-2)


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def problem(n, kind, gdt, seed=0):
    """CPU tensors of one launch: p, g (representable in ``gdt``), the rule's state, the step constants, the step counter."""
    gn = torch.Generator().manual_seed(1000 * seed + n + 13 * len(kind))
    p, g = torch.randn(n, generator=gn), torch.randn(n, generator=gn).to(BF).float()
    a, b = torch.randn(n, generator=gn) * 0.1, torch.rand(n, generator=gn) * 0.01
    hyper = torch.tensor([float("nan"), 1 - 0.9 ** 3, math.sqrt(1 - 0.999 ** 3), 0.5])  # (hyper[0]: per launch, or ignored)
    n_state = {"adam": 2, "adamw": 2, "sgd": 0, "sgd_momentum": 1}[kind]
    return dict(n=n, kind=kind, gdt=gdt, p=p, g=g.to(gdt), a=a, b=b, hyper=hyper, t=torch.tensor([3]), n_state=n_state)


def descriptor(kind, gdt, n, p, g, s0, s1, hyper, t_dev, hi, lo, word, gate, off=0, weight_decay=float("nan")):
    """egk_optim_desc over the elements [off, off + n) of the given device pointers (ints; 0 / None: absent)."""
    from egopack_amd import _lib
    d = _lib.OptimDesc()
    rule, scalars = KINDS[kind]
    d.rule, d.g_dtype, d.n = rule, 1 if gdt == BF else 0, n
    d.p, d.g = p + 4 * off, g + (2 if gdt == BF else 4) * off
    d.state0 = s0 + 4 * off if s0 else None
    d.state1 = s1 + 4 * off if s1 else None
    d.hyper, d.t_dev = hyper, t_dev
    d.beta1, d.beta2, d.eps, d.weight_decay = 0.9, 0.999, 1e-8, weight_decay
    for k, v in scalars.items():
        setattr(d, k, v)
    d.bf16_shadow = hi + 2 * off if hi else None
    d.bf16_lo_shadow = lo + 2 * off if lo else None
    d.bump_word, d.bump = (word, 7) if word else (None, 0)
    d.gate = gate
    return d


def group_table(base, seg_begin, seg_group, group_hyper, n_groups=None, n_seg=None):
    """egk_optim_groups over device tensors / pointers (pointers: ``n_seg`` and ``n_groups`` are given)."""
    from egopack_amd import _lib
    t = _lib.OptimGroups()
    ptr = lambda x: x.data_ptr() if torch.is_tensor(x) else x
    t.base, t.n_seg = base, (n_seg if n_seg is not None else seg_group.numel())
    t.n_groups = n_groups if n_groups is not None else group_hyper.numel() // 4
    t.seg_begin, t.seg_group, t.group_hyper = ptr(seg_begin), ptr(seg_group), ptr(group_hyper)
    return t


def hyper_rows(rows):
    out = torch.zeros(len(rows), 4)
    out[:, :2] = torch.tensor(rows, dtype=torch.float32)
    return out


_REFS = {}


def reference(prob, seg_begin, seg_group, rows, gate=None, lo=True, base=0):
    """{name: CPU tensor} after one egk_optim_step launch per segment (clipped to [base, base + n)), each with its group's lr
    (``hyper[0]``) and weight_decay; the offset word moves on once.  Computed once per problem and shared."""
    key = (prob["n"], prob["kind"], prob["gdt"], tuple(seg_begin), tuple(seg_group), tuple(rows), gate, lo, base)
    if key in _REFS:
        return _REFS[key]
    from egopack_amd import _lib
    lib = _lib.load()
    n, ns = prob["n"], prob["n_state"]
    p, g, a, b = (prob[k].to(DEV).clone() for k in ("p", "g", "a", "b"))
    t = prob["t"].to(DEV)
    hi, low = torch.zeros(n, dtype=BF, device=DEV), torch.zeros(n, dtype=BF, device=DEV)
    word = torch.tensor([100], dtype=torch.int64, device=DEV)
    gt = torch.tensor([gate], dtype=torch.int32, device=DEV) if gate is not None else None
    hypers, keep, first = [], [], True
    for k, gi in enumerate(seg_group):
        s, e = max(seg_begin[k] - base, 0), min(seg_begin[k + 1] - base, n)
        if e <= s:
            continue
        h = prob["hyper"].clone()
        h[0] = rows[gi][0]
        hypers.append(h.to(DEV))
        d = descriptor(prob["kind"], prob["gdt"], e - s, p.data_ptr(), g.data_ptr(), a.data_ptr() if ns >= 1 else 0,
                       b.data_ptr() if ns >= 2 else 0, hypers[-1].data_ptr(), t.data_ptr(), hi.data_ptr(), low.data_ptr() if lo else 0,
                       word.data_ptr() if first else 0, gt.data_ptr() if gt is not None else None, off=s, weight_decay=rows[gi][1])
        # (a plain launch wants its gradient 16-byte aligned; a bf16 sub-range that begins at a multiple of 4 is only 8-byte aligned:
        #  the gradient is read-only, so the launch reads an aligned copy of the sub-range -- the same values, the same bits out)
        keep.append(g[s:e].clone())
        d.g = keep[-1].data_ptr()
        assert lib.egk_optim_step(stream(), C.byref(d)) == 0, _lib.last_error()
        first = False
    torch.cuda.synchronize()
    out = dict(p=p.cpu(), hi=hi.view(torch.int16).cpu(), word=word.cpu())
    if ns >= 1:
        out["state0"] = a.cpu()
    if ns >= 2:
        out["state1"] = b.cpu()
    if lo:
        out["lo"] = low.view(torch.int16).cpu()
    _REFS[key] = out
    return out
