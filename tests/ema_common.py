"""Shared by tests/test_gpu_ema.py and tests/test_gpu_bounds_ema.py: the host model of the weight average of
include/egopack_ema.h and the segment tables of the sizes the tests use.  Imports without a GPU."""
import numpy
import torch


def ema_weight(decay, warmup, t):
    """w = (float)(1.0 - d_t): d_t in Python doubles, rounded to f32 once."""
    d_t = min(decay, (1.0 + t) / (10.0 + t)) if warmup else decay
    return numpy.float32(1.0 - d_t)


def ema_model(ema, p_new, w):
    """ema + w * (p_new - ema) as three separately rounded f32 torch operations on CPU tensors (no torch.lerp: its CPU path may
    contract)."""
    assert ema.dtype == p_new.dtype == torch.float32 and ema.device.type == p_new.device.type == "cpu"
    wt = torch.full((), float(w), dtype=torch.float32)
    assert float(wt) == float(w)  # (w is an f32 value: handing it over rounds nothing)
    diff = p_new - ema
    move = wt * diff
    return ema + move


def segments(n, base=0):
    """(seg_begin, seg_group) of up to three segments over the absolute elements [base, base + n rounded up to 4): cuts at multiples
    of 4 near the thirds (empty segments dropped) -- for n = 3080 one cut on a 1024-element block boundary and one inside a block."""
    end = (n + 3) // 4 * 4
    cuts = sorted({0, (end // 3) // 4 * 4, (2 * end // 3) // 4 * 4, end})
    return [base + c for c in cuts], [0, 1, 2][:len(cuts) - 1]
