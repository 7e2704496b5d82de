"""Host side of the task-weighting tests (include/egopack_task_scale.h): a float64 model of the objective with task scales, of the
gradient of the log-variances and of the scaled seeds.  Plain torch on the CPU; imports without a GPU.

    J       = sum_t w_t (exp(-s_t) L_t + s_t),   L_t = sum(loss_t) / count_t                    (``uncertainty``)
    dJ/ds_t = w_t (1 - exp(-s_t) L_t)
    J       = sum_t w_t scale_t L_t                                                             (``manual``: fixed scales)
    seed_t  = fl32(c_t * scale_t) with c_t = w_t / N_t as f32: ONE f32 product

``autograd_objective`` is the same J written for torch autograd in float64 (``torch.exp(-s) * L + s``): the model is held to it
in tests/test_task_weighting_cpu.py."""
import numpy as np
import torch

SCALES = (1.0, 0.5, 0.3, 1.7)                      # the scales of the bit-for-bit cases (1: the sibling itself; 0.3, 1.7: inexact products)
LOG_VARS = (0.0, 1e-3, -1e-3, 3.0, -3.0, -10.0, 10.0)


def fl32(x) -> float:
    """x rounded to f32 once, as a Python float."""
    return float(np.float32(x))


def scaled_seed(c, scale) -> float:
    """fl32(fl32(c) * fl32(scale)): the one separately rounded f32 product of the _s launches."""
    return float(np.float32(c) * np.float32(scale))


def prepared_scale(s) -> float:
    """What egk_task_scale_prepare stores for the f32 log-variance ``s``: exp(-s) in f64, rounded to f32 once."""
    return float(np.float32(np.exp(-np.float64(np.float32(s)))))


def ulp32(x) -> float:
    return float(np.spacing(np.float32(abs(x))))


def means(vectors, counts=None):
    """[L_t] in float64; a None vector (the task is absent from the step) gives None."""
    counts = counts or [None] * len(vectors)
    out = []
    for v, c in zip(vectors, counts):
        if v is None:
            out.append(None)
            continue
        n = c if c else max(v.numel(), 1)
        out.append(float(v.double().sum()) / n)
    return out


def objective(vectors, w, scale, s=None, counts=None):
    """(J, [dJ/ds_t] or None, [sum(loss_t)]) in float64.  ``scale``: the scales as the caller has them -- the f32 values the kernels
    read (``prepared_scale``) for a comparison with the kernels, exp(-s) in float64 for the comparison with autograd; ``s`` None:
    fixed scales, no gradient.  Absent tasks add nothing and have gradient 0."""
    L = means(vectors, counts)
    J, ds = 0.0, []
    for t, Lt in enumerate(L):
        if Lt is None:
            ds.append(0.0)
            continue
        sc = float(scale[t])
        J += float(w[t]) * (sc * Lt + (float(s[t]) if s is not None else 0.0))
        ds.append(float(w[t]) * (1.0 - sc * Lt))
    sums = [0.0 if v is None else float(v.double().sum()) for v in vectors]
    return J, (ds if s is not None else None), sums


def autograd_objective(L, w, s):
    """J of the ``uncertainty`` mode for torch autograd: L, w float64 tensors, s a float64 leaf."""
    return (w * (torch.exp(-s) * L + s)).sum()


def adam_first_step(g, lr, beta1=0.9, beta2=0.999, eps=1e-8):
    """The flat optimizer's Adam rule (csrc/optim_rules.hip: adam_update; include/egopack_hip.h: egk_adam_hyper) for ONE element at step
    t = 1 from p = m = v = 0 with weight_decay 0 and gradient scale 1, in float64 -- with the hyperparameters at the precision the
    launch receives them: lr, beta1, beta2, eps and the bias corrections 1 - beta1^t and sqrt(1 - beta2^t) are f32 numbers (the last
    two formed in double and rounded once).  They are the rule's inputs, not its error: 1 - fl32(0.999) differs from 0.001 by
    1.3e-5 relative, which moves the first update by 6.5e-6 relative -- far above the 1e-6 the comparison is made at.
        m = g (1 - b1);  v = (1 - b2) g^2;  p = -(lr / bc1) * m / (sqrt(v) / bc2s + eps)"""
    f = lambda x: float(np.float32(x))
    b1, b2, lr, eps = f(beta1), f(beta2), f(lr), f(eps)
    bc1, bc2s = f(1.0 - float(beta1) ** 1), f(np.sqrt(1.0 - float(beta2) ** 1))
    g = float(g)
    m, v = g * (1.0 - b1), (1.0 - b2) * g * g
    return -(lr / bc1) * (m / (np.sqrt(v) / bc2s + eps))
