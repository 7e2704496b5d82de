"""``ops.mix_rows`` and the two-target path of ``ops.cross_entropy`` / ``ops.cross_entropy_multi`` / ``MetricSelectorWrapper``
against the float64 models of tests/mixup_common.py.

The fused path needs logits that are column blocks of a classifier bank's buffer whose gradient operand the loss writes itself
(``ops.bank_grad_handoff`` under ``ops.loss_seed``); a test builds that by hand: it gives each logits tensor the hand-off record
``classifier_bank`` gives it.  The plain launch through the same record is the reference for the bitwise statements."""
import pytest
import torch

from tests import mixup_common as MC
from tests import round_once_common as RO

pytestmark = pytest.mark.gpu

DEV = "cuda"
BF, F32T = torch.bfloat16, torch.float32


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from egopack_amd import ops as _ops
    return _ops


def bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == F32T else torch.int16).cpu()


@pytest.mark.parametrize("dt", [F32T, BF])
def test_mix_rows_segments_of_a_merged_buffer(ops, dt):
    """Three task batches as row ranges of ONE [N, S, F] input (viewed [N, S * F]); the second is not mixed."""
    g = MC.gen(11)
    rows, cols = (20, 12, 9), 3 * 40
    x = RO.r16(torch.randn(sum(rows), cols, generator=g)).to(DEV).to(dt)
    out = torch.full_like(x, 7.0)
    srcs = [torch.randperm(r, generator=g).to(torch.int32) for r in rows]
    lams = [torch.rand(r, generator=g) for r in rows]
    lams[0][:5] = 1.0
    lams[2][:3] = 0.0
    offs = [0, rows[0], rows[0] + rows[1], sum(rows)]
    seg = lambda t, i: t[offs[i]:offs[i + 1]]
    ops.mix_rows([seg(x, i) for i in range(3)], [seg(out, i) for i in range(3)],
                 [srcs[0].to(DEV), None, srcs[2].to(DEV)], [lams[0].to(DEV), None, lams[2].to(DEV)])
    torch.cuda.synchronize()
    for i in range(3):
        xi = seg(x, i).float().cpu()
        src, lam = (None, None) if i == 1 else (srcs[i], lams[i])
        exact, bound = MC.mix_model(xi, src, lam), MC.mix_bound(xi, src, lam)
        got = seg(out, i).double().cpu()
        slack = bound if dt == F32T else bound + 2.0 ** -8 * (exact.abs() + bound)  # (and the one rounding of a bf16 store)
        assert bool(((got - exact).abs() <= slack).all()), f"segment {i}"
        if i == 1:
            assert torch.equal(bits(seg(out, i)), bits(seg(x, i))), "an unmixed segment is copied"
    assert torch.equal(bits(seg(out, 0)[:5]), bits(seg(x, 0)[:5])), "lam == 1 rows are copied"
    with pytest.raises(RuntimeError, match="out of place"):
        ops.mix_rows([x], [x], [None], [None])
    with pytest.raises(ValueError, match="both given or both None"):
        ops.mix_rows([x], [out], [None], [torch.ones(sum(rows), device=DEV)])


def case(rows, Cs, g, lam_kind="random"):
    logits = [RO.r16(torch.randn(rows, c, generator=g) * 3) for c in Cs]
    y, yb = MC.mix_labels(rows, Cs, g)
    y, yb = y[:, :len(Cs)].contiguous(), yb[:, :len(Cs)].contiguous()
    lam = MC.lam_vector(lam_kind, rows, g)
    return logits, y, yb, lam


@pytest.mark.parametrize("sm", [0.0, 0.1])
def test_cross_entropy_mix_outside_a_step_against_autograd(ops, sm):
    g = MC.gen(5)
    logits, y, yb, lam = case(67, (115, 478), g)
    wt = torch.randn(67, generator=g)
    ref_loss, _ = MC.ce_mix_model(logits, y, yb, lam, sm, 1.0)
    zs = [l.double().clone().requires_grad_(True) for l in logits]
    # the reference gradient under per-row weights: autograd through the float64 model's expression
    import torch.nn.functional as F
    total = sum(lam.double() * F.cross_entropy(z, y[:, h], ignore_index=-1, reduction="none", label_smoothing=sm)
                + (1 - lam.double()) * F.cross_entropy(z, torch.where(yb[:, h] < z.shape[1], yb[:, h], torch.full_like(yb[:, h], -1)),
                                                       ignore_index=-1, reduction="none", label_smoothing=sm) for h, z in enumerate(zs))
    (total * wt.double()).sum().backward()
    ds = [l.clone().to(DEV).requires_grad_(True) for l in logits]
    out = ops.cross_entropy(tuple(ds), y.to(DEV), sm, mix=(yb.to(DEV), lam.to(DEV)))
    (out * wt.to(DEV)).sum().backward()
    # tests/test_gpu_kernels.py::test_cross_entropy_heads_ignore_index
    torch.testing.assert_close(out.detach().cpu().double(), ref_loss, rtol=1e-5, atol=1e-5)
    for d, z in zip(ds, zs):
        torch.testing.assert_close(d.grad.cpu().double(), z.grad, rtol=1e-4, atol=1e-6)


def banked(ops, logits, dt, pad=3):
    """The heads' logits as a classifier bank hands them over under ``bank_grad_handoff``: blocks of one gradient operand."""
    rows = logits[0].shape[0]
    widths = [l.shape[1] + pad for l in logits]
    gbuf = torch.full((rows, sum(widths)), 7.0, dtype=dt, device=DEV)
    state = {"filled": set(), "pads": False}
    outs, col = [], 0
    for l, w in zip(logits, widths):
        d = l.clone().to(DEV).requires_grad_(True)
        d._egk_grad_dst = (gbuf, col, state)
        outs.append(d)
        col += w
    return outs, gbuf


@pytest.mark.parametrize("dt", [F32T, BF])
@pytest.mark.parametrize("scaled", [False, True])
def test_cross_entropy_multi_with_mixes_is_one_launch_and_keeps_the_plain_bits(ops, dt, scaled):
    g = MC.gen(9)
    A, B = case(67, (115, 478), g), case(40, (20, 9), g)
    coefs, sm = [0.5 / 67, 1.0 / 40], 0.1
    sc = torch.tensor([0.7, 1.3], device=DEV) if scaled else None
    scales = None if sc is None else [sc[0:1], sc[1:2]]
    geff = [c * (float(sc[i]) if scaled else 1.0) for i, c in enumerate(coefs)]

    def run(mixes):
        with ops.bank_grad_handoff():
            la, ga = banked(ops, A[0], dt)
            lb, gb = banked(ops, B[0], dt)
            vs = ops.cross_entropy_multi([(tuple(la), A[1].to(DEV)), (tuple(lb), B[1].to(DEV))], coefs, sm, scales=scales, mixes=mixes)
        torch.cuda.synchronize()
        return [v.detach().cpu() for v in vs], [ga.cpu(), gb.cpu()]

    dev = lambda c: (c[2].to(DEV), c[3].to(DEV))
    plain_v, plain_g = run(None)
    ops.prof_enable(True)  # the launches of one call, counted by the library's own per-kernel profile
    ops.prof_reset()
    try:
        run([dev(A), dev(B)])
        counts = {name: line["launches"] for name, line in ops.prof_report().items() if line["launches"]}
    finally:
        ops.prof_enable(False)
    assert counts == {"ce_mix": 1}, counts
    # task A mixed, task B rides with lam == 1: B has the plain launch's bits, A is the float64 model's
    v, gr = run([dev(A), None])
    assert torch.equal(bits(v[1]), bits(plain_v[1])) and torch.equal(bits(gr[1]), bits(plain_g[1])), "the unmixed task keeps its bits"
    ref_loss, ref_grad = MC.ce_mix_model(A[0], A[1], A[2], A[3], sm, geff[0])
    torch.testing.assert_close(v[0].double(), ref_loss, rtol=1e-5, atol=1e-5)
    col = 0
    for h, l in enumerate(A[0]):
        got = gr[0][:, col:col + l.shape[1]]
        if dt == F32T:
            torch.testing.assert_close(got.double(), ref_grad[h], rtol=1e-4, atol=1e-6)
        else:
            torch.testing.assert_close(got.double(), ref_grad[h], rtol=8e-3, atol=8e-3)  # tests/test_gpu_kernels.py: the rounding of a bf16 output
        assert not bool(gr[0][:, col + l.shape[1]:col + l.shape[1] + 3].ne(0).any()), "pad columns are zero"
        col += l.shape[1] + 3
    # both mixed with lam == 1 and arbitrary partners: the plain launch, bit for bit
    ones = lambda c: (c[2].to(DEV), torch.ones(c[3].shape[0], device=DEV))
    v1, g1 = run([ones(A), ones(B)])
    for i in range(2):
        assert torch.equal(bits(v1[i]), bits(plain_v[i])) and torch.equal(bits(g1[i]), bits(plain_g[i])), f"task {i}: lam == 1 is the plain launch"
    # a mixed task beside class-balance vectors: no two-target form, the caller takes the tasks one by one
    with ops.bank_grad_handoff():
        la, _ = banked(ops, A[0], dt)
        lb, _ = banked(ops, B[0], dt)
        w = [None, (torch.ones(20, device=DEV), torch.ones(9, device=DEV))]
        assert ops.cross_entropy_multi([(tuple(la), A[1].to(DEV)), (tuple(lb), B[1].to(DEV))], coefs, sm, weights=w, mixes=[dev(A), None]) is None


def test_cross_entropy_mix_under_an_announced_seed_writes_the_bank_operand(ops):
    g = MC.gen(13)
    logits, y, yb, lam = case(33, (115, 478), g)
    sc = torch.tensor([0.6], device=DEV)
    with ops.bank_grad_handoff(), ops.loss_seed(0.25, scale=sc):
        ls, gbuf = banked(ops, logits, F32T)
        v = ops.cross_entropy(tuple(ls), y.to(DEV), 0.1, mix=(yb.to(DEV), lam.to(DEV)))
        assert ops.seed_consumed(v), "the launch wrote the gradient itself"
    torch.cuda.synchronize()
    ref_loss, ref_grad = MC.ce_mix_model(logits, y, yb, lam, 0.1, 0.25 * 0.6)
    torch.testing.assert_close(v.detach().cpu().double(), ref_loss, rtol=1e-5, atol=1e-5)
    torch.testing.assert_close(gbuf[:, :115].cpu().double(), ref_grad[0], rtol=1e-4, atol=1e-6)
    torch.testing.assert_close(gbuf[:, 118:118 + 478].cpu().double(), ref_grad[1], rtol=1e-4, atol=1e-6)


class _Labels:
    has_joint_label, num_labels = False, 2


def test_the_wrapper_passes_the_mix_through_in_training_mode_only(ops):
    from egopack_amd.criterion import CrossEntropyNone, MetricSelectorWrapper
    g = MC.gen(21)
    logits, y, yb, lam = case(40, (20, 9), g)
    crit = MetricSelectorWrapper(CrossEntropyNone(label_smoothing=0.1), _Labels())
    dl = tuple(l.to(DEV) for l in logits)
    mix = (yb.to(DEV), lam.to(DEV))
    crit.train()
    ref_loss, _ = MC.ce_mix_model(logits, y, yb, lam, 0.1, 1.0)
    torch.testing.assert_close(crit(dl, y.to(DEV), mix=mix).cpu().double(), ref_loss, rtol=1e-5, atol=1e-5)
    plain = crit(dl, y.to(DEV))
    crit.eval()
    assert torch.equal(bits(crit(dl, y.to(DEV), mix=mix)), bits(plain)), "eval(): the plain cross entropy"
