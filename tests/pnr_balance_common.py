"""Host model of the shaped BCE-with-logits (include/egopack_bce_balanced.h) in float64, as plain torch operations, its two torch
references, and the tolerances, stated once.  Shared by tests/test_pnr_balance_cpu.py, tests/test_gpu_pnr_balance.py and
tests/test_gpu_bounds_pnr_balance.py.

    t = float(y),  c = pos if y != 0 else neg,  s = 2 t - 1,  u = s z,  softplus(x) = max(x, 0) + log1p(exp(-|x|))
    gamma == 0:  loss = c [(1 - t) z + max(-z, 0) + log1p(exp(-|z|))]          dz = c (sigma(z) - t) g
    gamma  > 0:  ce = softplus(-u), mod = exp(-gamma softplus(u)), p_t = sigma(u)
                 loss = c mod ce                                                dz = s c mod (gamma p_t (-ce) - (1 - p_t)) g

Tolerances.  Loss: the plain kernels' bar (tests/class_balance_common.py LOSS_TOL).  Gradient: rtol 1e-4 with an absolute term of
1e-6 * max(1, pos, neg) -- sigma(z) - t cancels in f32, so the absolute error of the gradient scales with the class factor: an f32
evaluation of the formulas against float64 needs 2.2e-6 at pos = 31 and nothing beyond the relative term at factors <= 1, for
gamma in [0, 5] and |z| <= 100.  bf16 outputs: the bounds suite's OUT16 (the final rounding of a bf16 value)."""
import torch

from tests.class_balance_common import LOSS_TOL  # noqa: F401  (rtol 1e-5, atol 1e-5)

OUT16 = dict(rtol=8e-3, atol=8e-3)  # tests/test_gpu_bounds.py
TRIPLES = [(31.0, 1.0, 0.0), (0.25, 0.75, 2.0), (1.0, 1.0, 0.5)]
EXTREMES = [0.0, 30.0, -30.0, 88.0, -88.0, 100.0, -100.0]


def grad_tol(pos, neg):
    return dict(rtol=1e-4, atol=1e-6 * max(1.0, pos, neg))


def gen(seed):
    return torch.Generator().manual_seed(seed)


def labels(n, g):
    """int64 labels with one positive in 8: both classes occur (n >= 8)."""
    return (torch.rand(n, generator=g) < 0.125).to(torch.int64)


def problem(n, seed):
    """(logits f32 [n], y int64 [n], gloss f32 [n]): logits ~ N(0, 3^2) with the fixed values 0, +-30, +-88, +-100 in front --
    each once with a positive and once with a negative label when n allows it."""
    g = gen(seed)
    x = 3 * torch.randn(n, generator=g)
    y = labels(n, g)
    k = min(n, 2 * len(EXTREMES))
    x[:k] = torch.tensor(EXTREMES + EXTREMES)[:k]
    y[:k] = torch.tensor([1] * len(EXTREMES) + [0] * len(EXTREMES))[:k]
    return x, y, torch.randn(n, generator=g)


def _softplus(x):
    return x.clamp(min=0) + torch.log1p(torch.exp(-x.abs()))


def model(z, y, pos=1.0, neg=1.0, gamma=0.0, gloss=None):
    """(loss, dz or None) in float64 from the formulas above, the shape of ``z``.  ``gloss``: a tensor like z or a number."""
    z = z.detach().double().cpu()
    y = y.detach().cpu()
    t = (y != 0).double()
    c = torch.where(y != 0, torch.tensor(float(pos), dtype=torch.float64), torch.tensor(float(neg), dtype=torch.float64))
    g = None if gloss is None else (gloss.detach().double().cpu() if torch.is_tensor(gloss) else float(gloss))
    if gamma == 0:
        loss = c * ((1 - t) * z + (-z).clamp(min=0) + torch.log1p(torch.exp(-z.abs())))
        return loss, None if g is None else c * (torch.sigmoid(z) - t) * g
    s = 2 * t - 1
    u = s * z
    ce, mod, pt = _softplus(-u), torch.exp(-gamma * _softplus(u)), torch.sigmoid(u)
    loss = c * mod * ce
    return loss, None if g is None else s * c * mod * (gamma * pt * (-ce) - (1 - pt)) * g


def torch_pos_weight(z, y, pos, neg, gloss):
    """neg * F.binary_cross_entropy_with_logits(z, t, pos_weight=pos / neg, reduction='none') in float64, gradient by autograd."""
    import torch.nn.functional as F
    x = z.detach().double().cpu().clone().requires_grad_(True)
    t = (y != 0).double()
    loss = neg * F.binary_cross_entropy_with_logits(x, t, pos_weight=torch.tensor(pos / neg, dtype=torch.float64), reduction="none")
    (loss * gloss.double()).sum().backward()
    return loss.detach(), x.grad


def torch_focal(z, y, pos, neg, gamma, gloss):
    """torchvision's sigmoid_focal_loss written out, alpha_t (1 - p_t) ** gamma * bce with alpha_t = pos t + neg (1 - t), in
    float64, gradient by autograd."""
    import torch.nn.functional as F
    x = z.detach().double().cpu().clone().requires_grad_(True)
    t = (y != 0).double()
    p = torch.sigmoid(x)
    ce = F.binary_cross_entropy_with_logits(x, t, reduction="none")
    p_t = p * t + (1 - p) * (1 - t)
    loss = (pos * t + neg * (1 - t)) * ((1 - p_t) ** gamma) * ce
    (loss * gloss.double()).sum().backward()
    return loss.detach(), x.grad
