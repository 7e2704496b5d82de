"""Host model of the class-balanced cross entropy (include/egopack_ce_balanced.h) in float64, as plain torch operations, and the
known answers of the vector builders (egopack_amd/train.py).  Shared by tests/test_class_balance_cpu.py,
tests/test_gpu_class_balance.py and tests/test_gpu_bounds_class_balance.py.

    x' = x + a,  lse = logsumexp(x'),  W = sum w,  p = exp(x' - lse)
    loss = (1 - eps) w_t (lse - x'_t) + eps / C (W lse - sum_c w_c x'_c)
    dx_j = g [(1 - eps) w_t (p_j - [j == t]) + eps / C (W p_j - w_j)]
0 for ignored rows (t < 0 or t >= C); a missing weight is 1, a missing offset 0."""
import math

import torch

LOSS_TOL = dict(rtol=1e-5, atol=1e-5)   # the project's cross-entropy tolerances (tests/test_gpu_kernels.py)
GRAD_TOL = dict(rtol=1e-4, atol=1e-6)


def model(x, y, weight=None, offset=None, eps=0.0, gloss=None):
    """(loss [N], lse [N], dx [N, C] or None) in float64 from the formulas above.  ``gloss``: d objective / d loss, [N]."""
    x = x.detach().double().cpu()
    y = y.detach().cpu().to(torch.int64)
    N, C = x.shape
    w = torch.ones(C, dtype=torch.float64) if weight is None else weight.detach().double().cpu()
    a = torch.zeros(C, dtype=torch.float64) if offset is None else offset.detach().double().cpu()
    xp = x + a
    lse = torch.logsumexp(xp, 1)
    live = (y >= 0) & (y < C)
    t = torch.where(live, y, torch.zeros_like(y))
    W = w.sum()
    xt = xp.gather(1, t[:, None])[:, 0]
    wt = w[t]
    loss = (1 - eps) * wt * (lse - xt) + eps / C * (W * lse - (xp * w).sum(1))
    loss = torch.where(live, loss, torch.zeros_like(loss))
    if gloss is None:
        return loss, lse, None
    p = torch.exp(xp - lse[:, None])
    onehot = torch.zeros_like(p).scatter_(1, t[:, None], 1.0)
    d = (1 - eps) * wt[:, None] * (p - onehot) + eps / C * (W * p - w[None, :])
    d = d * gloss.detach().double().cpu()[:, None]
    d = torch.where(live[:, None], d, torch.zeros_like(d))
    return loss, lse, d


def torch_reference(x, y, weight=None, offset=None, eps=0.0, gloss=None):
    """The same from F.cross_entropy(x + a, y, weight=w, ignore_index=-1, reduction='none', label_smoothing=eps) in float64."""
    import torch.nn.functional as F
    z = x.detach().double().cpu().clone().requires_grad_(True)
    a = 0 if offset is None else offset.detach().double().cpu()
    w = None if weight is None else weight.detach().double().cpu()
    loss = F.cross_entropy(z + a, y.detach().cpu(), weight=w, ignore_index=-1, reduction="none", label_smoothing=eps)
    if gloss is None:
        return loss.detach(), None
    (loss * gloss.detach().double().cpu()).sum().backward()
    return loss.detach(), z.grad


def zipf_counts(C, scale=5000.0, s=1.2):
    """floor(scale / k ** s), k = 1 .. C: a long tail whose far end has classes without a label."""
    return torch.tensor([math.floor(scale / (k ** s)) for k in range(1, C + 1)], dtype=torch.int64)


def zipf_weights(C):
    """f32 effective-number weights (normalised) of the Zipf counts -- the builder's formulas written out here."""
    n = zipf_counts(C).double()
    n1 = n.clamp(min=1.0)
    w = (1 - 0.999) / (1 - 0.999 ** n1)
    w = w * (n.sum() / (n * w).sum())
    return w.float()


def zipf_offsets(C, tau=1.0):
    n1 = zipf_counts(C).double().clamp(min=1.0)
    return (tau * torch.log(n1 / n1.sum())).float()


# ---- known answers of the builders on counts [5000, 10, 1, 0] (beta 0.999, power 1, tau 1), worked out with python floats ---------
COUNTS = [5000, 10, 1, 0]


def known_effective_number(beta=0.999):
    return [(1 - beta) / (1 - beta ** max(n, 1)) for n in COUNTS]


def known_inverse_frequency(power=1.0):
    return [float(max(n, 1)) ** -power for n in COUNTS]


def known_logit_adjust(tau=1.0):
    tot = float(sum(max(n, 1) for n in COUNTS))
    return [tau * math.log(max(n, 1) / tot) for n in COUNTS]
