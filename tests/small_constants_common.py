"""Shared by tests/test_small_constants_cpu.py and tests/test_gpu_small_constants.py: the regimes in which the SMALL CONSTANTS of
the kernels carry weight -- the eps of the two LayerNorms, the eps and the betas of the Adam family, the 1e-6 of the gradient clip
-- with fp64 references, MUTANT references (the same formula with the constant in another place, selected by a keyword), seeded
input builders, the case tables and the tolerances.  Plain torch on the CPU; imports without a GPU.

Every input is drawn in fp64 and rounded to the type the kernel reads (f32 or bf16) BEFORE a reference sees it.  LayerNorm data is
x = (randn + 0.3) * s: |mean| <= std, so E[x^2] - mean^2 stays well conditioned (cancellation is not the subject), the cotangent is
randn + 2 * xhat * w (a plain random cotangent leaves S2 = sum dxhat * xhat at O(sqrt n) and the third term of the graph LayerNorm's
backward invisible).  Adam gradients are sign * 10^U[-12, -1] with every 17th element exactly 0 in every step; every intermediate
stays a normal f32 number (g^2 >= 1e-24)."""
import math

import torch
import torch.nn.functional as F

F64 = torch.float64
BF = torch.bfloat16
BF16_STEP = 2.0 ** -8  # one bf16 rounding step per element (tests/test_gpu_round_once.py)


def gen(seed):
    return torch.Generator().manual_seed(seed)


def rounded(t, dt):
    """fp64 values representable in ``dt``: what the kernel will read."""
    return t.to(dt).to(F64)


# ---- tolerances ----------------------------------------------------------------------------------------------------------------------
# Per tensor: max |got - ref| <= tol * max |ref|.  tol = 4 x the worst error of the kernels against the fp64 reference over the
# whole family, measured on an MI355X (the table in tests/test_gpu_small_constants.py), under two caps that are conditions:
# (a) not looser than the older test of the same kernel, (b) at most 1 / 100 of the smallest mutant gap (test_small_constants_cpu).
# (rounded up to one digit.)
TOL_ROWLN = dict(y=5e-7, dx=6e-7, dw=9e-7, db=7e-7)
TOL_GRAPHLN = dict(y=5e-7, dx=5e-7, dw=1e-6, db=6e-7)
TOL_ADAM_P = 1e-6
# exp_avg / exp_avg_sq span 20 decades: per ELEMENT, relative, atol = 0.  EGK_OPT_ADAM keeps egk_adam_step's f32 ``1.f - beta``
# (include/egopack_optim.h): fl32(1 - fl32(0.999)) is 1.3e-5 away from 0.001, and exp_avg_sq carries that; EGK_OPT_ADAMW rounds
# 1 - beta once from double.
TOL_ADAM_STATE = dict(adam=dict(m=2e-6, v=6e-5), adamw=dict(m=2e-6, v=2e-6))
TOL_EMA = 5e-7
TOL_CLIP_COEF = 2e-7
# what the older tests allow, read relative to max |ref| (cap (a), and what the control regime is held against)
OLD_TOL_LN = dict(y=1e-4, dx=1e-3, dw=1e-3, db=1e-3)  # test_rowln_fwd_bwd, test_graphln_lrelu_fwd_bwd
OLD_TOL_ADAM_P = dict(rtol=1e-5, atol=1e-6)          # test_gpu_optim_rules.TOL


def rel_err(got, ref):
    """max |got - ref| / max |ref|."""
    return float((got.to(F64) - ref.to(F64)).abs().max() / ref.to(F64).abs().max())


def bound_ratio(got, ref, tol, step=0.0):
    """Largest |got - ref| / (tol * max |ref| + step * |ref|) over the tensor: <= 1 passes.  ``step``: BF16_STEP for a tensor the
    kernel stores in bf16."""
    ref = ref.to(F64)
    bound = tol * ref.abs().max() + step * ref.abs()
    return float(((got.to(F64) - ref).abs() / bound).max())


def older_bound_ratio(got, ref):
    """Largest |got - ref| / (atol + rtol * |ref|) with the older Adam test's tolerances: the uniform tol * max |ref| is looser than
    its atol for the small elements of p, so p is held to both."""
    ref = ref.to(F64)
    return float(((got.to(F64) - ref).abs() / (OLD_TOL_ADAM_P["atol"] + OLD_TOL_ADAM_P["rtol"] * ref.abs())).max())


def elementwise_ratio(got, ref, tol):
    """Largest |got - ref| / (tol * |ref|) over the elements whose reference is not 0 (those must be 0: inf otherwise)."""
    got, ref = got.to(F64), ref.to(F64)
    zero = ref == 0
    if bool((got[zero] != 0).any()):
        return math.inf
    if bool(zero.all()):
        return 0.0
    return float(((got[~zero] - ref[~zero]).abs() / (tol * ref[~zero].abs())).max())


# ---- LayerNorm inputs ----------------------------------------------------------------------------------------------------------------
LN_REGIMES = {"eps0.5": (1.0, 0.5), "std1e-4": (1e-4, 1e-5), "std3e-6": (3e-6, 1e-5)}  # name -> (s, eps)
LN_CONTROL = (1.0, 1e-5)  # the regime of every older test: here the mutants are NOT separable
SEGMENT_SCALES = (1.0, 1e-4, 3e-6)


def ln_data(seed, rows, cols, scales, dt):
    """x [rows, cols] = (randn + 0.3) * s with s a number or one value per row; w, b ~ N(0, 1) (f32 parameters); noise ~ N(0, 1)."""
    g = gen(seed)
    s = torch.as_tensor(scales, dtype=F64)
    s = s.reshape(-1, 1) if s.dim() else s
    x = rounded((torch.randn(rows, cols, generator=g, dtype=F64) + 0.3) * s, dt)
    w, b = (rounded(torch.randn(cols, generator=g, dtype=F64), torch.float32) for _ in range(2))
    noise = torch.randn(rows, cols, generator=g, dtype=F64)
    return x, w, b, noise


def row_scales(segs, scales):
    """One scale per row: segment k of ``segs`` takes scales[k % len(scales)]."""
    out = torch.empty(segs[-1], dtype=F64)
    for k, (a, e) in enumerate(zip(segs[:-1], segs[1:])):
        out[a:e] = scales[k % len(scales)]
    return out


def cotangent(noise, xhat, w, dt):
    """randn + 2 * xhat * w, rounded to the activation type."""
    return rounded(noise + 2.0 * xhat * w, dt)


def _inv_std(var, eps, eps_on):
    if eps_on == "var":
        return 1.0 / torch.sqrt(var + eps)
    if eps_on == "std":
        return 1.0 / (torch.sqrt(var) + eps)
    assert eps_on == "none"
    return 1.0 / torch.sqrt(var)


# ---- row LayerNorm (+ReLU, +dropout): nn.LayerNorm -> ReLU -> Dropout -----------------------------------------------------------------
def rowln_ref(x, w, b, eps, relu=False, mask=None, p=0.0, *, noise=None, cot=None, cot_dtype=torch.float32, eps_on="var", dtype=F64):
    """(x - mean) / sqrt(var_biased + eps) * w + b, ReLU, mask / (1 - p); gradients by autograd.  ``cot``: the cotangent, or None:
    randn + 2 * xhat * w from ``noise`` and this call's xhat.  ``eps_on``: "var" (the definition) | "std" | "none" (mutants).
    ``dtype``: the arithmetic (fp64: the reference; f32: what f32 arithmetic can reach)."""
    xl, wl, bl = (t.to(dtype).clone().requires_grad_(True) for t in (x, w, b))
    mean = xl.mean(-1, keepdim=True)
    var = ((xl - mean) ** 2).mean(-1, keepdim=True)
    xhat = (xl - mean) * _inv_std(var, eps, eps_on)
    y = xhat * wl + bl
    if relu:
        y = torch.relu(y)
    if mask is not None:
        y = y * mask.to(dtype) / (1.0 - p)
    if cot is None:
        cot = cotangent(noise, xhat.detach().to(F64), w, cot_dtype)
    y.backward(cot.to(dtype))
    return dict(y=y.detach(), dx=xl.grad, dw=wl.grad, db=bl.grad, xhat=xhat.detach(), cot=cot)


# ---- graph LayerNorm + LeakyReLU: gnn.LayerNorm(mode="graph") per row segment ---------------------------------------------------------
def graphln_ref(x, w, b, segs, eps, slope, *, noise=None, cot=None, cot_dtype=torch.float32, eps_on="std", third_term=None, dtype=F64):
    """Per segment oracle.pyg_ops.graph_layer_norm (statistics over all rows * cols elements of the segment, eps on the STD), then
    LeakyReLU.  ``third_term`` None: gradients by autograd.  Otherwise dx in closed form,
        dx = r * dxhat - r * S1 / n - xhat * S2 / (n * D),   r = 1 / (sigma + eps), S1 = sum dxhat, S2 = sum dxhat * xhat,
    with D = sigma ("sigma": the definition; a segment with sigma = 0 has no third term -- the library's definition, autograd gives
    NaN there), sigma + eps ("sigma_plus_eps") or without the term ("dropped").  Also returned: xhat, dxhat (what a second rank
    contributes to the exchanged sums) and the cotangent."""
    xl, wl, bl = (t.to(dtype).clone().requires_grad_(True) for t in (x, w, b))
    parts, sig = [], []
    for a, e in zip(segs[:-1], segs[1:]):
        blk = xl[a:e]
        mean = blk.mean()
        var = ((blk - mean) ** 2).mean()
        sig.append(torch.sqrt(var).detach())
        parts.append((blk - mean) * _inv_std(var, eps, eps_on))
    xhat = torch.cat(parts)
    pre = xhat * wl + bl
    y = F.leaky_relu(pre, slope)
    if cot is None:
        cot = cotangent(noise, xhat.detach().to(F64), w, cot_dtype)
    c = cot.to(dtype)
    one = torch.ones((), dtype=dtype)
    gg = c * torch.where(pre.detach() > 0, one, one * slope)
    dxhat = gg * wl.detach()
    out = dict(y=y.detach(), xhat=xhat.detach(), dxhat=dxhat, gg=gg, cot=cot)
    if third_term is None:
        y.backward(c)
        out.update(dx=xl.grad, dw=wl.grad, db=bl.grad)
        return out
    xh, dx = xhat.detach(), torch.empty_like(dxhat)
    for k, (a, e) in enumerate(zip(segs[:-1], segs[1:])):
        n = (e - a) * x.shape[1]
        r = _inv_std(sig[k] ** 2, eps, eps_on)
        s1, s2 = dxhat[a:e].sum(), (dxhat[a:e] * xh[a:e]).sum()
        dx[a:e] = r * dxhat[a:e] - r * s1 / n
        den = {"sigma": sig[k], "sigma_plus_eps": sig[k] + eps, "dropped": None}[third_term]
        if den is not None and float(sig[k]) > 0:
            dx[a:e] -= xh[a:e] * s2 / (n * den)
    out.update(dx=dx, dw=(gg * xh).sum(0), db=gg.sum(0))
    return out


# ---- Adam / AdamW --------------------------------------------------------------------------------------------------------------------
ADAM_N = 4099  # n % 4 != 0, more than one workgroup
ADAM_STEPS = 5
ADAM_CHECK = (1, 2, 5)
ADAM_LR = 1e-2
ADAM_HYPERS = {"b0.9-0.999-eps1e-8": (0.9, 0.999, 1e-8), "b0.8-0.95-eps1e-3": (0.8, 0.95, 1e-3)}
ADAM_WD = {"adam": 0.0, "adamw": 1e-2}  # (coupled decay would swamp the tiny gradients with wd * p)
GROUP_CUT = 2048  # two groups: the elements in front of it and behind it
GROUP_ROWS = {"adam": [(1e-2, 0.0), (3e-3, 0.0)], "adamw": [(1e-2, 1e-2), (3e-3, 0.0)]}  # (lr, weight_decay) per group
EMA_DECAY = 0.9


def tiny_gradients(seed, n, steps, dt, zeros=True):
    """``steps`` gradients sign * 10^U[-12, -1], every 17th element exactly 0 in every step, rounded to ``dt``.  The magnitude is
    drawn per step, the sign once per element: with a sign per step exp_avg = b1 * m + (1 - b1) * g cancels in some of the 4099
    elements and f32 arithmetic itself is then 1.6e-5 away from fp64 in exp_avg -- an input property, not a kernel's."""
    g = gen(seed)
    out = []
    sign = torch.where(torch.rand(n, generator=g, dtype=F64) < 0.5, -1.0, 1.0).to(F64)
    for _ in range(steps):
        mag = 10.0 ** (torch.rand(n, generator=g, dtype=F64) * 11.0 - 12.0)
        gr = mag * sign
        if zeros:
            gr[::17] = 0.0
        out.append(rounded(gr, dt))
    return out


def adam_params(seed, n):
    return rounded(torch.randn(n, generator=gen(seed), dtype=F64), torch.float32)


def adam_ref(p, grads, lr, betas, eps, weight_decay=0.0, grad_scale=1.0, *, decoupled=False, eps_at="torch", betas_used=None,
             ema_decay=None, check=ADAM_CHECK, dtype=F64):
    """torch.optim.Adam's single-tensor formulas step by step (``decoupled``: AdamW's); {step: dict(p, m, v[, ema])} for the steps in
    ``check``.  lr / weight_decay: numbers or one value per element (parameter groups).  grad_scale multiplies the gradient first.
    ``eps_at``: "torch" (sqrt(v) / bc2s + eps) | "before_bc" | "inside_sqrt" | "none"; ``betas_used``: betas the update uses whatever
    ``betas`` says (mutants).  ``ema_decay``: ema += (1 - decay) * (p_new - ema), started at p."""
    b1, b2 = betas_used if betas_used is not None else betas
    as_t = lambda a: a.to(dtype) if torch.is_tensor(a) else a
    lr, wd = as_t(lr), as_t(weight_decay)
    p = p.to(dtype).clone()
    m, v, ema = torch.zeros_like(p), torch.zeros_like(p), p.clone()
    out = {}
    for t, g in enumerate(grads, 1):
        g = g.to(dtype) * grad_scale
        if decoupled:
            p = p * (1.0 - lr * wd)
        else:
            g = g + wd * p
        m = m + (g - m) * (1.0 - b1)
        v = v * b2 + (1.0 - b2) * g * g
        bc1, bc2s = 1.0 - b1 ** t, math.sqrt(1.0 - b2 ** t)
        if eps_at == "torch":
            denom = v.sqrt() / bc2s + eps
        elif eps_at == "before_bc":
            denom = (v.sqrt() + eps) / bc2s
        elif eps_at == "inside_sqrt":
            denom = (v + eps).sqrt() / bc2s
        else:
            assert eps_at == "none"
            denom = v.sqrt() / bc2s
            denom = torch.where(v == 0, torch.ones_like(v), denom)  # (m is 0 there)
        p = p - (lr / bc1) * (m / denom)
        if ema_decay is not None:
            ema = ema + (1.0 - ema_decay) * (p - ema)
        if t in check:
            out[t] = dict(p=p.clone(), m=m.clone(), v=v.clone())
            if ema_decay is not None:
                out[t]["ema"] = ema.clone()
    return out


def adamw_ref(p, grads, lr, betas, eps, weight_decay=1e-2, grad_scale=1.0, **kw):
    return adam_ref(p, grads, lr, betas, eps, weight_decay, grad_scale, decoupled=True, **kw)


def group_vectors(rule, n):
    """(lr, weight_decay) per element of the two-group launches."""
    rows = GROUP_ROWS[rule]
    lr, wd = torch.empty(n, dtype=F64), torch.empty(n, dtype=F64)
    lr[:GROUP_CUT], lr[GROUP_CUT:] = rows[0][0], rows[1][0]
    wd[:GROUP_CUT], wd[GROUP_CUT:] = rows[0][1], rows[1][1]
    return lr, wd


def adam_cases():
    """(id, dict): rule x (betas, eps) x grad_scale x gradient type x plain | two groups."""
    out = []
    for rule in ("adam", "adamw"):
        for hyper in ADAM_HYPERS:
            for gs in (1.0, 0.5):
                for gdt in (torch.float32, BF):
                    for grouped in (False, True):
                        name = f"{rule}-{hyper}-gs{gs:g}-{'bf16' if gdt == BF else 'f32'}{'-groups' if grouped else ''}"
                        out.append((name, dict(rule=rule, hyper=hyper, gs=gs, gdt=gdt, grouped=grouped)))
    return out


_ADAM = {}


def adam_problem(case):
    """The inputs of one case and its fp64 reference (with the moving average, which changes nothing else), computed once."""
    key = (case["rule"], case["hyper"], case["gs"], case["gdt"], case["grouped"])
    if key not in _ADAM:
        p = adam_params(7, ADAM_N)
        grads = tiny_gradients(11 + (case["gdt"] == BF), ADAM_N, ADAM_STEPS, case["gdt"])
        _ADAM[key] = dict(p=p, grads=grads, ref=adam_eval(case, p, grads, ema_decay=EMA_DECAY))
    return _ADAM[key]


def adam_eval(case, p, grads, **kw):
    b1, b2, eps = ADAM_HYPERS[case["hyper"]]
    lr, wd = group_vectors(case["rule"], p.numel()) if case["grouped"] else (ADAM_LR, ADAM_WD[case["rule"]])
    return adam_ref(p, grads, lr, (b1, b2), eps, wd, case["gs"], decoupled=case["rule"] == "adamw", **kw)


ADAM_EPS_MUTANTS = ("before_bc", "inside_sqrt", "none")
DEFAULT_BETAS = (0.9, 0.999)


# ---- gradient clip -------------------------------------------------------------------------------------------------------------------
CLIP_MAX_NORM = 1e-6
# with the constant: ~0.5, ~0.999 (NOT clamped: 1e-6 / (1e-9 + 1e-6)), ~1e-3, and exactly 1 for a zero gradient -- the only norm at
# which this bound clamps; without the constant: 1, 1 (clamped), 1e-3 * (1 + 1e-3), 1
CLIP_NORMS = {"norm1e-6": 1e-6, "norm1e-9": 1e-9, "norm1e-3": 1e-3, "norm0": 0.0}


def clip_ref(norm, max_norm, constant=1e-6):
    """torch.nn.utils.clip_grad_norm_: min(1, max_norm / (norm + 1e-6)).  ``constant`` = 0: the mutant."""
    return 1.0 if norm + constant == 0 else min(1.0, max_norm / (norm + constant))


def clip_gradient(seed, n, norm):
    """A gradient of L2 norm ~ ``norm`` with elements of one magnitude (sign * (0.5 + U[0, 1))): nothing near the denormals."""
    g = gen(seed)
    u = (0.5 + torch.rand(n, generator=g, dtype=F64)) * torch.where(torch.rand(n, generator=g, dtype=F64) < 0.5, -1.0, 1.0).to(F64)
    return rounded(u * (norm / float(u.norm())), torch.float32)  # (norm = 0: exact zeros)


# ---- LayerNorm case tables -------------------------------------------------------------------------------------------------------------
# the smallest shapes that reach each kernel family of the row LayerNorm: the one-wave kernels (40; 250 = the scalar path, cols % 4
# != 0; 1024 = the exact-width path; 1280) and the wide-row kernels (2048, 3072, 4096)
ROWLN_SHAPES = [(37, 40), (5, 250), (9, 1024), (3, 1280), (6, 2048), (5, 3072), (5, 4096)]
ROWLN_GROUP = dict(cols=256, rows=[64, 192, 5])
GRAPHLN_SHAPES = [(40, 32, [0, 40]), (64, 1024, [0, 10, 64]), (300, 256, [0, 100, 101, 300])]  # (the last: a one-row segment)
GRAPHLN_SLOPES = (0.2, 0.01)


def rowln_cases():
    """(id, dict): shapes x regimes x ReLU x activation type, and one case with dropout p = 0.25."""
    out = []
    for rows, cols in ROWLN_SHAPES:
        for regime in LN_REGIMES:
            for relu in (False, True):
                for dt in (torch.float32, BF):
                    name = f"{rows}x{cols}-{regime}-{'relu' if relu else 'plain'}-{'bf16' if dt == BF else 'f32'}"
                    out.append((name, dict(rows=rows, cols=cols, regime=regime, relu=relu, dt=dt, p=0.0)))
    out.append(("64x1024-std1e-4-relu-f32-dropout0.25", dict(rows=64, cols=1024, regime="std1e-4", relu=True, dt=torch.float32, p=0.25)))
    return out


def rowln_inputs(case, regime=None):
    s, eps = LN_REGIMES[case["regime"]] if regime is None else regime
    x, w, b, noise = ln_data(case["rows"] * 10000 + case["cols"], case["rows"], case["cols"], s, case["dt"])
    return x, w, b, noise, eps


def graphln_cases():
    """(id, dict): shapes x activation type x slope x regimes.  Several segments: "mixed" gives each segment its own scale (1, 1e-4,
    3e-6) inside one launch with eps = 1e-5 -- statistics mixed between segments would show -- beside the uniform eps = 0.5 regime."""
    out = []
    for rows, cols, segs in GRAPHLN_SHAPES:
        regimes = list(LN_REGIMES) if len(segs) == 2 else ["eps0.5", "mixed"]
        for regime in regimes:
            for dt in (torch.float32, BF):
                for slope in GRAPHLN_SLOPES:
                    name = f"{rows}x{cols}-{len(segs) - 1}seg-{regime}-slope{slope:g}-{'bf16' if dt == BF else 'f32'}"
                    out.append((name, dict(rows=rows, cols=cols, segs=segs, regime=regime, dt=dt, slope=slope)))
    return out


def graphln_inputs(case, regime=None):
    segs = case["segs"]
    if regime is not None:
        s, eps = regime
    elif case["regime"] == "mixed":
        s, eps = row_scales(segs, SEGMENT_SCALES), 1e-5
    else:
        s, eps = LN_REGIMES[case["regime"]]
    x, w, b, noise = ln_data(case["rows"] * 10000 + case["cols"], case["rows"], case["cols"], s, case["dt"])
    return x, w, b, noise, eps


def out_steps(dt):
    """The bf16 rounding step of each LayerNorm output: y and dx are stored in the activation type, dw and db in f32."""
    step = BF16_STEP if dt == BF else 0.0
    return dict(y=step, dx=step, dw=0.0, db=0.0)
