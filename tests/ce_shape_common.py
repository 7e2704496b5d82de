"""The shaped cross entropy (the tail of egk_ce_task, include/egopack_hip.h) for the tests: the float64 reference,
the numpy f32 restatement of the kernel's arithmetic, the test inputs and the tolerances.  Shared by tests/test_ce_shape_cpu.py,
tests/test_gpu_ce_shape.py and tests/test_gpu_bounds_ce_shape.py.

    z_c  = x_c + a_c - [c == t] m_t,  p = softmax(z),  q = p_t
    S    = F.cross_entropy(z, t, weight=w, label_smoothing=eps, reduction='none')
    loss = (1 - q)^gamma S
    dz_j = g [(1 - q)^gamma dS_j + S gamma q (1 - q)^(gamma - 1) (p_j - [j == t])]

Tolerances.  gamma = 0: the project's cross-entropy tolerances (tests/class_balance_common.py).  gamma > 0: the f32 restatement
below does NOT stay inside them against float64 on the inputs of ``problem`` -- on the row whose target logit dominates, lse - z_t
rounds to 0 in f32 (sum exp = 1 + 1e-11 is 1), so the kernel's 1 - q is 0 where float64 has 1 - q ~ 1e-11, and with smoothing
(S ~ 30 on that row) (1 - q)^0.5 S is ~1e-4, not 0.  The bound is therefore 4 x the restatement's largest absolute error over every
gamma > 0 case of ``cases()`` on ``problem(heads)`` (tests/test_ce_shape_cpu.py measures it and pins the constants to it): loss
4 x 1.84e-4 = 7.36e-4, gradient 4 x 2.02e-5 = 8.08e-5 for seeds |g| <= 1, absolute, no relative term.  Both come from that one
row; every other row of the restatement is inside the project's tolerances."""
import numpy as np
import torch

from tests import class_balance_common as CB

LOSS_TOL, GRAD_TOL = CB.LOSS_TOL, CB.GRAD_TOL               # gamma = 0
SHAPED_LOSS_ERR, SHAPED_GRAD_ERR = 1.84e-4, 2.02e-5         # the restatement's largest |error| against float64, gamma > 0 (measured on the CPU)
SHAPED_LOSS_TOL = dict(rtol=0.0, atol=4 * SHAPED_LOSS_ERR)
SHAPED_GRAD_TOL = dict(rtol=0.0, atol=4 * SHAPED_GRAD_ERR)

HEADS = [(115, 478), (2,), (65,)]   # 65 crosses the 64-lane stride
HEAD_IDS = ["115x478", "2", "65"]
EPS = [0.0, 0.1]
GAMMAS = [0.0, 0.5, 2.0]
ROWS = 9
PRESENCE = [(m, w, a) for m in (False, True) for w in (False, True) for a in (False, True)]   # margin, weight, offset


def tols(gamma):
    return (LOSS_TOL, GRAD_TOL) if gamma == 0 else (SHAPED_LOSS_TOL, SHAPED_GRAD_TOL)


def ldam(C, max_margin=0.5, power=0.25):
    """f32 LDAM margins of the Zipf counts of tests/class_balance_common.py -- the builder's formula written out here."""
    r = CB.zipf_counts(C).double().clamp(min=1.0) ** -power
    return (max_margin * r / r.max()).float()


def problem(heads, seed=None):
    """(``seed`` None: the inputs the tolerances were measured on.)  (logits [9, C] per head, y [9, heads], gloss [9] in (-1, 1)).  Row 0: ignored (-1); 1: label 0; 2: label C - 1; 3: the
    target (class 0) 25 above every other logit -- q rounds to 1 in f32, not in float64; 4: a -inf logit beside the target;
    5: ignored (label == C); 6 .. 8: random."""
    g = torch.Generator().manual_seed(1000 + sum(heads) if seed is None else seed)
    logits = [3 * torch.randn(ROWS, c, generator=g) for c in heads]
    y = torch.stack([torch.randint(0, c, (ROWS,), generator=g) for c in heads], 1)
    for h, c in enumerate(heads):
        y[0, h], y[1, h], y[2, h], y[3, h], y[5, h] = -1, 0, c - 1, 0, c
        logits[h][3, 0] = logits[h][3, 1:].max() + 25.0
        logits[h][4, (int(y[4, h]) + 1) % c] = float("-inf")
    gloss = 2 * torch.rand(ROWS, generator=g) - 1
    return logits, y, gloss


def vectors(heads, presence):
    """(margins, weights, offsets): per head a host f32 vector or None, by the (margin, weight, offset) flags of ``presence``."""
    m, w, a = presence
    return (tuple(ldam(c) if m else None for c in heads), tuple(CB.zipf_weights(c) if w else None for c in heads),
            tuple(CB.zipf_offsets(c) if a else None for c in heads))


def cases():
    """Every (heads, eps, gamma, presence) of the parity tests."""
    return [(hd, eps, gm, pr) for hd in HEADS for eps in EPS for gm in GAMMAS for pr in PRESENCE]


def reference(x, y, w=None, a=None, m=None, eps=0.0, gamma=0.0, gloss=None):
    """(loss [N], dx [N, C], q [N]) in float64: F.cross_entropy on z, times (1 - softmax(z)[t])^gamma, gradient by autograd.
    Labels outside [0, C) are ignored rows.  Where float64 itself has no finite answer (q == 1 exactly with 0 < gamma < 1, or a
    -inf logit under smoothing: S = inf) the entries are inf / nan as autograd leaves them."""
    import torch.nn.functional as F
    x = x.detach().double().cpu().clone().requires_grad_(True)
    N, C = x.shape
    y = y.detach().cpu().to(torch.int64)
    live = (y >= 0) & (y < C)
    yy = torch.where(live, y, torch.full_like(y, -1))
    t = yy.clamp(min=0)
    z = x if a is None else x + a.detach().double().cpu()
    if m is not None:
        md = m.detach().double().cpu()
        z = z - F.one_hot(t, C).double() * md[t][:, None]
    S = F.cross_entropy(z, yy, weight=None if w is None else w.detach().double().cpu(), ignore_index=-1, reduction="none",
                        label_smoothing=eps)
    q = torch.softmax(z, 1).gather(1, t[:, None])[:, 0]
    loss = S if gamma == 0 else (1 - q) ** gamma * S
    loss = torch.where(live, loss, torch.zeros_like(loss))
    gl = torch.ones(N, dtype=torch.float64) if gloss is None else gloss.detach().double().cpu()
    (loss * gl).sum().backward()
    return loss.detach(), x.grad, q.detach()


def restate_f32(x, y, w=None, a=None, m=None, eps=0.0, gamma=0.0, gloss=None):
    """The arithmetic of ce_row_weighted<SHAPED> (csrc/loss.hip) in numpy float32, operation by operation, one row at a time (the sums
    in numpy's order, not the wave's).  Returns (loss [N] f32, dx [N, C] f32)."""
    f = np.float32
    x = x.detach().cpu().numpy().astype(f)
    y = y.detach().cpu().numpy().astype(np.int64)
    N, C = x.shape
    wv = None if w is None else w.detach().cpu().numpy().astype(f)
    av = None if a is None else a.detach().cpu().numpy().astype(f)
    mv = None if m is None else m.detach().cpu().numpy().astype(f)
    gl = np.ones(N, f) if gloss is None else gloss.detach().cpu().numpy().astype(f)
    eps, gamma = f(eps), f(gamma)
    sm = f(eps / f(C)) if eps > 0 else f(0)
    loss, dx = np.zeros(N, f), np.zeros((N, C), f)
    with np.errstate(all="ignore"):
        for n in range(N):
            t = int(y[n])
            if not 0 <= t < C:
                continue
            z = x[n].copy() if av is None else (x[n] + av).astype(f)
            if mv is not None:
                z[t] = f(z[t] - mv[t])
            mx = z.max()
            v = (z - mx).astype(f)
            wc = np.ones(C, f) if wv is None else wv
            se, W, swx = np.exp(v).astype(f).sum(dtype=f), wc.sum(dtype=f), (wc * v).astype(f).sum(dtype=f)
            lg = f(np.log(se))
            l = f(mx + lg)
            wt, zt = wc[t], z[t]
            S = f(f(f(f(1) - eps) * wt) * f(l - zt))
            if eps > 0:
                S = f(S + f(sm * f(f(W * lg) - swx)))
            fS, cf = f(1), f(0)
            loss[n] = S
            if gamma > 0:
                d = max(f(l - zt), f(0))
                q, u = f(np.exp(f(-d))), f(-np.expm1(f(-d)))
                fS = f(np.power(u, gamma)) if u > 0 else f(0)
                cf = f(f(f(S * gamma) * q) * f(np.power(u, f(gamma - f(1))))) if u > 0 else f(0)
                loss[n] = f(fS * S)
            p = np.exp((z - l).astype(f)).astype(f)
            e = p.copy()
            e[t] = f(p[t] - f(1))
            d = (f(f(1) - eps) * wt * e).astype(f)
            if eps > 0:
                d = (d + (sm * ((W * p).astype(f) - wc).astype(f)).astype(f)).astype(f)
            if gamma > 0:
                d = ((fS * d).astype(f) + (cf * e).astype(f)).astype(f)
            dx[n] = (d * gl[n]).astype(f)
    return loss, dx


def check(got_loss, got_grad, x, y, w, a, m, eps, gamma, gloss, what="", measure=False):
    """Assert a head's loss vector and gradient against ``reference`` within ``tols(gamma)``.  Where the reference is finite
    the values are compared.  Where it is not, what the definition says is asserted instead:
      * a row with q == 1 exactly in float64 and gamma > 0 has gradient exactly 0 ("with q = 1 and gamma > 0 both terms are 0";
        autograd has 0 * inf there);
      * elsewhere a non-finite reference entry (S = inf: a -inf logit under smoothing) must be non-finite in the result too;
      * the loss vector must agree with the reference also in its inf / nan entries.
    Returns the largest absolute errors (loss, gradient) over the compared entries; ``measure``: without asserting on them."""
    ref_loss, ref_grad, q = reference(x, y, w, a, m, eps, gamma, gloss)
    ltol, gtol = tols(gamma)
    got_loss, got_grad = got_loss.detach().cpu().double(), got_grad.detach().cpu().double()
    C = x.shape[1]
    live = (y >= 0) & (y < C)
    one = live & (q == 1) if gamma > 0 else torch.zeros_like(live)
    fin = torch.isfinite(ref_loss)
    if not measure:
        torch.testing.assert_close(got_loss[fin], ref_loss[fin], msg=lambda s: f"{what} loss: {s}", **ltol)
    rest = ~fin
    assert torch.equal(torch.isnan(got_loss[rest]), torch.isnan(ref_loss[rest])) and \
        torch.equal(got_loss[rest][~torch.isnan(got_loss[rest])], ref_loss[rest][~torch.isnan(ref_loss[rest])]), f"{what}: inf / nan losses"
    assert not got_grad[one].ne(0).any(), f"{what}: a row with q == 1 has a gradient"
    assert not got_grad[~live].ne(0).any() and not got_loss[~live].ne(0).any(), f"{what}: ignored rows"
    gfin = torch.isfinite(ref_grad) & ~one[:, None]
    if not measure:
        torch.testing.assert_close(got_grad[gfin], ref_grad[gfin], msg=lambda s: f"{what} gradient: {s}", **gtol)
    bad = ~torch.isfinite(ref_grad) & ~one[:, None]
    assert not torch.isfinite(got_grad[bad]).any(), f"{what}: finite where float64 has no finite gradient"
    err = lambda g_, r_: float((g_ - r_).abs().max()) if g_.numel() else 0.0
    return err(got_loss[fin], ref_loss[fin]), err(got_grad[gfin], ref_grad[gfin])
