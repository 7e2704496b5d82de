"""The update rules of the flat-buffer optimizer (optim.FlatAdamW, optim.FlatSGD, egk_optim_step) on the GPU: each rule against the
torch class on the CPU, and the bit-for-bit properties the engine relies on (rule 0 = the shipped Adam kernel, slices = one launch,
the bf16 copies = egk_cast / egk_split_bf16 of the stored parameters, a closed gate changes nothing but the offset word)."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
TOL = dict(rtol=1e-5, atol=1e-6)  # tests/test_gpu_kernels.py::test_flat_adam_matches_torch_adam
SHAPES = [(33, 7), (5,), (64, 64), (3,), (130, 9)]
BF = torch.bfloat16


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


def gen(seed):
    return torch.Generator().manual_seed(seed)


def _flat(kind, params, **kw):
    from egopack_amd.optim import FlatAdam, FlatAdamW, FlatSGD
    return {"adam": FlatAdam, "adamw": FlatAdamW, "sgd": FlatSGD}[kind](params, **kw)


def _set_grads(params, grads):
    for p, gr in zip(params, grads):
        if p.grad is None:
            p.grad = gr.clone().to(p.device)
        else:
            p.grad.copy_(gr)


# ---- 1. each rule against the torch class on the CPU ---------------------------------------------------------------------------------
VARIANTS = {
    "adamw-wd1e-2": ("adamw", torch.optim.AdamW, dict(weight_decay=1e-2), False),
    "adam-decoupled": ("adam", torch.optim.Adam, dict(weight_decay=1e-2, decoupled_weight_decay=True), False),
    "sgd-plain": ("sgd", torch.optim.SGD, dict(), False),
    "sgd-wd": ("sgd", torch.optim.SGD, dict(weight_decay=1e-2), False),
    "sgd-momentum": ("sgd", torch.optim.SGD, dict(momentum=0.9), False),
    "sgd-momentum-dampening": ("sgd", torch.optim.SGD, dict(momentum=0.9, dampening=0.1), False),
    "sgd-nesterov": ("sgd", torch.optim.SGD, dict(momentum=0.9, nesterov=True), False),
    "adamw-bf16-gradient": ("adamw", torch.optim.AdamW, dict(weight_decay=1e-2), True),
    "sgd-momentum-wd-bf16-gradient": ("sgd", torch.optim.SGD, dict(momentum=0.9, weight_decay=1e-2), True),
}


@pytest.mark.parametrize("name", list(VARIANTS))
def test_rule_matches_the_torch_class(name):
    """Parameters and gradients N(0, 1), lr = 1e-2, 20 steps, compared after steps 1, 2, 5 and 20: parameters and every state
    buffer.  One parameter never gets a gradient.  The bf16 variants hand the launch a bf16 gradient buffer that holds gradients
    rounded to bf16 beforehand (what a compressed exchange leaves), the torch class steps on the same rounded values."""
    kind, torch_cls, kw, bf16_grad = VARIANTS[name]
    g = gen(61)
    ps = [torch.randn(s, generator=g) for s in SHAPES]
    grads = [[torch.randn(s, generator=g) for s in SHAPES] for _ in range(20)]
    if bf16_grad:
        grads = [[x.to(BF).float() for x in gs] for gs in grads]
    cpu = [p.clone().requires_grad_(True) for p in ps]
    unused_cpu = torch.randn(4, generator=g).requires_grad_(True)
    ref = torch_cls(cpu + [unused_cpu], lr=1e-2, **kw)
    dev = [p.clone().to(DEV).requires_grad_(True) for p in ps]
    unused = unused_cpu.detach().clone().to(DEV).requires_grad_(True)
    opt = _flat(kind, dev + [unused], lr=1e-2, **kw)
    keys = opt._state_keys
    for it in range(20):
        _set_grads(cpu, grads[it])
        _set_grads(dev, grads[it])
        ref.step()
        if bf16_grad:
            if not opt.materialised:
                opt._materialise()
            opt.step(grads=opt.flat_g.to(BF))
        else:
            opt.step()
        if it + 1 not in (1, 2, 5, 20):
            continue
        sd = opt.state_dict()["state"]
        assert sorted(sd) == list(range(len(ps)))  # (nothing for the parameter without a gradient)
        worst = 0.0
        for i, (c, d) in enumerate(zip(cpu, dev)):
            pairs = [(d.detach().cpu(), c.detach())] + [(sd[i][k].cpu(), ref.state[c][k]) for k in keys]
            for got, want in pairs:
                worst = max(worst, float(((got - want).abs() / (TOL["atol"] + TOL["rtol"] * want.abs())).max()))
        print(f"{name}: step {it + 1}, largest |got - want| / (atol + rtol |want|) over parameters and state = {worst:.3f}")
        for i, (c, d) in enumerate(zip(cpu, dev)):
            torch.testing.assert_close(d.detach().cpu(), c.detach(), **TOL, msg=lambda s, i=i: f"step {it + 1}, parameter {i}: {s}")
            for k in keys:
                torch.testing.assert_close(sd[i][k].cpu(), ref.state[c][k], **TOL, msg=lambda s, i=i, k=k: f"step {it + 1}, {k} of {i}: {s}")
            assert float(sd[i]["step"]) == it + 1
    assert torch.equal(unused.detach().cpu(), unused_cpu.detach())  # grad None -> skipped, as torch does
    assert len(opt.state_buffers()) == len(keys) and all(b.numel() == opt.flat_p.numel() for b in opt.state_buffers())


# ---- 2. bit for bit ------------------------------------------------------------------------------------------------------------------
def _p(t, off=0):
    return None if t is None else ctypes.c_void_p(t.data_ptr() + off)


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


@pytest.mark.parametrize("gdt", [torch.float32, BF])
@pytest.mark.parametrize("gate", [None, 1])
def test_rule_zero_is_the_shipped_adam_kernel_bit_for_bit(gdt, gate):
    """EGK_OPT_ADAM through egk_optim_step against egk_adam_step_gated on the same inputs: n % 4 != 0 and a size with several
    workgroups, with both bf16 copies and the offset word.
    Both entry points run ONE body (csrc/optim_rules.hip: optim_body; adam_kernel is a shell over it), so this compares two doors
    to it -- the descriptor filled by the caller against the one egk_adam_step_gated fills, the two kernel names -- and no longer
    pins Adam's bits independently.  What pins them: test_rule_matches_the_torch_class (this file; Adam itself:
    tests/test_gpu_kernels.py::test_flat_adam_matches_torch_adam), tests/test_gpu_small_constants.py against the fp64 formulas, and
    the comparison of every optimizer output against the build before the bodies were unified (profiles/optim_unified_cost.txt)."""
    from egopack_amd import _lib
    lib = _lib.load()
    for n in (1003, 300007):
        g = torch.Generator(device=DEV).manual_seed(n)
        p0, gr = torch.randn(n, device=DEV, generator=g), torch.randn(n, device=DEV, generator=g).to(gdt)
        m0, v0 = torch.randn(n, device=DEV, generator=g) * 0.1, torch.rand(n, device=DEV, generator=g) * 0.01
        hyper = torch.tensor([1e-2, 1 - 0.9 ** 3, (1 - 0.999 ** 3) ** 0.5, 0.5], device=DEV)
        gt = torch.tensor([gate], dtype=torch.int32, device=DEV) if gate is not None else None
        outs = []
        for new in (False, True):
            p, m, v = p0.clone(), m0.clone(), v0.clone()
            hi, lo = torch.zeros(n, dtype=BF, device=DEV), torch.zeros(n, dtype=BF, device=DEV)
            word = torch.tensor([100], dtype=torch.int64, device=DEV)
            if new:
                d = _lib.OptimDesc()
                d.rule, d.g_dtype, d.n = _lib.OPT_ADAM, 1 if gdt == BF else 0, n
                d.p, d.g, d.state0, d.state1, d.hyper = p.data_ptr(), gr.data_ptr(), m.data_ptr(), v.data_ptr(), hyper.data_ptr()
                d.beta1, d.beta2, d.eps, d.weight_decay = 0.9, 0.999, 1e-8, 1e-3
                d.bf16_shadow, d.bf16_lo_shadow, d.bump_word, d.bump = hi.data_ptr(), lo.data_ptr(), word.data_ptr(), 7
                d.gate = gt.data_ptr() if gt is not None else None
                assert lib.egk_optim_step(_stream(), ctypes.byref(d)) == 0, _lib.last_error()
            else:
                assert lib.egk_adam_step_gated(_stream(), _p(p), _p(gr), 1 if gdt == BF else 0, _p(m), _p(v), n, _p(hyper), 0.9, 0.999, 1e-8,
                                               1e-3, _p(hi), _p(lo), _p(word), 7, _p(gt)) == 0, _lib.last_error()
            torch.cuda.synchronize()
            outs.append((p, m, v, hi.view(torch.int16), lo.view(torch.int16), word))
        assert not torch.equal(outs[0][0], p0)
        for a, b, what in zip(outs[0], outs[1], ("p", "m", "v", "bf16 copy", "low half", "offset word")):
            assert torch.equal(a, b), (n, what)


def _pair(kind, seed=5, **kw):
    """Two optimizers of one rule over equal parameters, flat buffers built, low halves allocated."""
    g = gen(seed)
    ps = [torch.randn(s, generator=g) for s in SHAPES]
    grads = [[torch.randn(s, generator=g) for s in SHAPES] for _ in range(3)]
    out = []
    for _ in range(2):
        dev = [p.clone().to(DEV).requires_grad_(True) for p in ps]
        opt = _flat(kind, dev, lr=1e-2, **kw)
        _set_grads(dev, grads[0])
        opt._materialise()
        opt.ensure_lo_shadows()
        opt.refresh_lo_shadows()
        out.append((opt, dev))
    return out, grads


def _bits(opt):
    torch.cuda.synchronize()
    bufs = [opt.flat_p, *opt.state_buffers(), opt.flat_w16.view(torch.int16), opt.flat_w16lo.view(torch.int16), opt._t_dev]
    return [b.clone() for b in bufs]


def test_decoupled_flag_is_flat_adamw_bit_for_bit():
    from egopack_amd.optim import FlatAdam, FlatAdamW
    g = gen(3)
    ps = [torch.randn(s, generator=g) for s in SHAPES]
    grads = [[torch.randn(s, generator=g) for s in SHAPES] for _ in range(3)]
    a = [p.clone().to(DEV).requires_grad_(True) for p in ps]
    b = [p.clone().to(DEV).requires_grad_(True) for p in ps]
    opt_a, opt_b = FlatAdam(a, lr=1e-2, weight_decay=1e-2, decoupled_weight_decay=True), FlatAdamW(b, lr=1e-2, weight_decay=1e-2)
    plain = [p.clone().to(DEV).requires_grad_(True) for p in ps]
    opt_c = FlatAdam(plain, lr=1e-2, weight_decay=1e-2)
    for it in range(3):
        for o, params in ((opt_a, a), (opt_b, b), (opt_c, plain)):
            _set_grads(params, grads[it])
            o.step()
    for x, y in zip(opt_a.state_buffers() + [opt_a.flat_p, opt_a.flat_w16.view(torch.int16)],
                    opt_b.state_buffers() + [opt_b.flat_p, opt_b.flat_w16.view(torch.int16)]):
        assert torch.equal(x, y)
    assert not torch.equal(opt_a.flat_p, opt_c.flat_p)  # (and it is not the L2 rule)


RULES = [("adam", dict(weight_decay=1e-3)), ("adamw", dict(weight_decay=1e-2)), ("sgd", dict(weight_decay=1e-3)),
         ("sgd", dict(momentum=0.9, dampening=0.1)), ("sgd", dict(momentum=0.9, nesterov=True))]
RULE_IDS = ["adam", "adamw", "sgd", "sgd-momentum", "sgd-nesterov"]


@pytest.mark.parametrize("kind,kw", RULES, ids=RULE_IDS)
def test_three_slices_equal_one_launch_and_the_copies_are_cast_and_split_of_the_stored_parameters(kind, kw):
    """Two steps (SGD's first, which stores the gradient as the buffer, and one that uses it): one launch over the whole buffer
    against three [lo, hi) launches, bit for bit in the parameters, the state and both bf16 copies; the copies equal what egk_cast
    and egk_split_bf16 make of the stored parameters."""
    from egopack_amd import _lib
    lib = _lib.load()
    (one, dev1), (three, dev3) = _pair(kind, **kw)[0]
    grads = _pair(kind, **kw)[1]
    n = one.flat_p.numel()
    cuts = [0, n // 3 // 8 * 8, n // 2 // 8 * 8 + 8, n]
    for it in range(2):
        _set_grads(dev1, grads[it])
        _set_grads(dev3, grads[it])
        one.prepare_hyper()
        one.launch()
        one.step_count += 1
        three.prepare_hyper()
        for lo, hi in zip(cuts[:-1], cuts[1:]):
            three.launch(None, lo, hi)
        three.step_count += 1
        for x, y in zip(_bits(one), _bits(three)):
            assert torch.equal(x, y), it
        hi16, lo16 = torch.zeros(n, dtype=BF, device=DEV), torch.zeros(n, dtype=BF, device=DEV)
        assert lib.egk_cast(_stream(), _p(one.flat_p), 0, _p(hi16), 1, n) == 0
        assert lib.egk_split_bf16(_stream(), _p(one.flat_p), n, None, _p(lo16), n, 1, n) == 0
        torch.cuda.synchronize()
        assert torch.equal(one.flat_w16.view(torch.int16), hi16.view(torch.int16)), "bf16 copy"
        assert torch.equal(one.flat_w16lo.view(torch.int16), lo16.view(torch.int16)), "low half"
        assert one._lo_is_fresh(0, n)
    assert int(one._t_dev.item()) == 2


@pytest.mark.parametrize("kind,kw", RULES, ids=RULE_IDS)
def test_closed_gate_changes_nothing_but_the_offset_word(kind, kw):
    """A gradient whose norm is not finite: the launch leaves the parameters, the state and both copies as they were and the
    step is taken back out of the counter, the offset word still moves on.  The next step happens -- for SGD with momentum as the
    FIRST one: its buffer is the gradient itself."""
    (opt, dev), _ = _pair(kind, max_grad_norm=1.0, **kw)[0]
    grads = _pair(kind, **kw)[1]
    word = torch.tensor([100], dtype=torch.int64, device=DEV)
    _set_grads(dev, grads[0])
    opt.flat_g[17] = float("inf")
    before = _bits(opt)
    opt.prepare_hyper()
    opt.norm_partials()
    opt.norm_finalize()
    opt.launch(bump=(word, 7))
    opt.step_count += 1
    after = _bits(opt)
    for x, y in zip(before, after):
        assert torch.equal(x, y)
    assert word.tolist() == [107] and int(opt._t_dev.item()) == 0 and opt.grad_norm_stats()["skipped"] == 1
    _set_grads(dev, grads[1])
    opt.flat_g.mul_(1e-3)  # (a norm below the bound: the coefficient clamps to 1)
    g1 = opt.flat_g.clone()
    p0 = opt.flat_p.clone()
    opt.step()
    torch.cuda.synchronize()
    assert int(opt._t_dev.item()) == 1 and not torch.equal(opt.flat_p, p0)
    if kw.get("momentum") and not kw.get("weight_decay"):
        assert torch.equal(opt.state_buffers()[0], g1)  # buf = g' on the first step that happens


# ---- 3. the capped grid: a workgroup that takes a second stride ----------------------------------------------------------------------
GRID_CAP = 32768                    # workgroups (csrc/optim_rules.hip: optim_grid), 1024 elements each per stride
N_CAPPED = GRID_CAP * 1024 + 1027   # the smallest size at which a workgroup takes a second stride, with a scalar tail (n % 4 == 3)
CUT = 1024 * 1000                   # [CUT, N_CAPPED) alone is 31769 workgroups: under the cap


@pytest.mark.parametrize("rule", ["adam", "sgd"])
def test_second_stride_of_the_capped_grid_equals_two_launches_under_the_cap(rule):
    """n = 32768 * 1024 + 1027, f32 gradient: Adam through egk_adam_step_gated, SGD without momentum through egk_optim_step.  One
    launch over [0, n) -- workgroups 0 and 1 walk on to the blocks 32768 and 32769, the last one ends in a scalar tail -- equals
    the launches over [0, CUT) and [CUT, n), neither of which reaches the cap, bit for bit in p, the state and both bf16 copies.
    4096 elements around 32768 * 1024 are held to the fp64 formula at this file's tolerance, so the equal bits are the right ones."""
    from egopack_amd import _lib
    lib = _lib.load()
    n = N_CAPPED
    lr, b1, b2, eps, wd = 1e-2, 0.9, 0.999, 1e-8, 1e-3
    g = torch.Generator(device=DEV).manual_seed(7)
    p0, gr = torch.randn(n, device=DEV, generator=g), torch.randn(n, device=DEV, generator=g)
    state0 = [torch.randn(n, device=DEV, generator=g) * 0.1, torch.rand(n, device=DEV, generator=g) * 0.01] if rule == "adam" else []
    hyper = torch.tensor([lr, 1 - b1 ** 3, (1 - b2 ** 3) ** 0.5, 0.5], device=DEV)

    def launch(bufs, lo, hi):
        p, state, hi16, lo16 = bufs
        if rule == "adam":
            rc = lib.egk_adam_step_gated(_stream(), _p(p, 4 * lo), _p(gr, 4 * lo), 0, _p(state[0], 4 * lo), _p(state[1], 4 * lo), hi - lo,
                                         _p(hyper), b1, b2, eps, wd, _p(hi16, 2 * lo), _p(lo16, 2 * lo), None, 0, None)
        else:
            d = _lib.OptimDesc()
            d.rule, d.g_dtype, d.n = _lib.OPT_SGD, 0, hi - lo
            d.p, d.g, d.hyper, d.weight_decay = p.data_ptr() + 4 * lo, gr.data_ptr() + 4 * lo, hyper.data_ptr(), wd
            d.bf16_shadow, d.bf16_lo_shadow = hi16.data_ptr() + 2 * lo, lo16.data_ptr() + 2 * lo
            rc = lib.egk_optim_step(_stream(), ctypes.byref(d))
        assert rc == 0, _lib.last_error()

    outs = []
    for pieces in ([(0, n)], [(0, CUT), (CUT, n)]):
        bufs = (p0.clone(), [s.clone() for s in state0], torch.zeros(n, dtype=BF, device=DEV), torch.zeros(n, dtype=BF, device=DEV))
        for lo, hi in pieces:
            launch(bufs, lo, hi)
        torch.cuda.synchronize()
        outs.append([bufs[0], *bufs[1], bufs[2].view(torch.int16), bufs[3].view(torch.int16)])
    names = ["p", *(("exp_avg", "exp_avg_sq") if rule == "adam" else ()), "bf16 copy", "low half"]
    assert not torch.equal(outs[0][0][-1027:], p0[-1027:])  # (the second stride and its tail were stepped)
    for a, b, what in zip(outs[0], outs[1], names):
        assert torch.equal(a, b), what

    w = slice(GRID_CAP * 1024 - 2048, GRID_CAP * 1024 + 2048)
    h = [float(x) for x in hyper.double().cpu()]
    p, gg = p0[w].double().cpu(), gr[w].double().cpu() * h[3]
    gg = gg + wd * p
    if rule == "adam":
        m, v = state0[0][w].double().cpu(), state0[1][w].double().cpu()
        m = m + (gg - m) * (1 - b1)
        v = v * b2 + (1 - b2) * gg * gg
        want = [p - (h[0] / h[1]) * (m / (v.sqrt() / h[2] + eps)), m, v]
    else:
        want = [p - h[0] * gg]
    for got, ref, what in zip(outs[0], want, names):
        err = float(((got[w].double().cpu() - ref).abs() / (TOL["atol"] + TOL["rtol"] * ref.abs())).max())
        print(f"{rule}: {what} around the second stride, largest |got - want| / (atol + rtol |want|) = {err:.4f}")
        torch.testing.assert_close(got[w].cpu(), ref.float(), **TOL, msg=lambda s, what=what: f"{what}: {s}")
