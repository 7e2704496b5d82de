"""egk_topk_softmax on the GPU against the host model of tests/topk_common.py and against the library's own kernels.

Inputs come from tests/class_report_common.py (the 2^-10 grid, and the integer -2 .. 2 tie rows).  The grid of shapes: C in
{1, 2, 7, 63, 64, 65, 115, 478, 513, 1025} (63 / 64 / 65 straddle the lane edge, 513 and 1025 the register-resident edge), k in
{1, 2, 5, 16, 64} (several cases have k > C), rows in {0, 1, 4, 5, 9, 77} (4 and 5 straddle the four-waves-per-workgroup edge).
One test case per (C, element type); the k and row counts are walked inside it (every launch is a few microseconds).

  * ``idx`` equals the host model bit for bit, for f32 and bf16 inputs (the bf16 model orders the widened values), on grid rows, tie
    rows and the special rows (a NaN planted, -inf entries, all equal, -0 and +0, ...);
  * ``egk_label_rank(logits, idx[:, j]) == j`` for every j < min(k, C): the launch against the existing kernel, no host model.  (An
    entry whose logit is a NaN is left out: the rank kernel compares the LABEL's score with ``>`` and ``==``, which a NaN label fails
    against everything, so it reports rank 0 for it wherever it stands -- the order of the other entries of such a row is checked.);
  * ``idx[:, 0]`` and ``idx[:, 1]`` reproduce egk_class_report's confusion and top-2 counts on the same rows;
  * fl32(lse - x[y]) equals ops.cross_entropy(logits, y, 0.0) bit for bit on every row with a valid label;
  * ``prob`` against the float64 softmax at rtol 1e-5, atol 1e-6 (the tolerance of the f32 cross entropy in tests/test_gpu_kernels.py:
    the error in p is p * (|delta lse| + one expf error)); -inf entries give exactly 0, NaN rows NaN, j >= C gives (-1, 0);
  * two launches give identical bits; eight tasks in one launch equal eight single-task launches bit for bit."""
import numpy as np
import pytest
import torch

from tests import class_report_common as CR
from tests import topk_common as TK

pytestmark = pytest.mark.gpu
DTYPES = [torch.float32, torch.bfloat16]
_ID = lambda v: str(v).replace("torch.", "")


def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from egopack_amd import ops
    return ops


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32 if t.dtype == torch.float32 else t.dtype)


def _check(ops, x, k, what):
    """One launch on ``x`` (a host tensor of the launch's element type) against the host model; returns the device outputs."""
    xd = x.cuda()
    (idx, prob, lse), = ops.topk_softmax([xd], k, want_prob=True, want_lse=True)
    xw = TK.widen(x)
    N, C = xw.shape
    ref_idx, ref_p, ref_lse = TK.model(xw, k)
    got_idx, got_p, got_lse = idx.cpu().numpy(), prob.cpu().numpy(), lse.cpu().numpy()
    assert got_idx.dtype == np.int64 and got_idx.shape == (N, k) and got_p.shape == (N, k) and got_lse.shape == (N,), what
    assert np.array_equal(got_idx, ref_idx), f"{what}: idx differs from the host model at {np.argwhere(got_idx != ref_idx)[:4].tolist()}"
    assert (got_idx[:, C:] == -1).all() and (got_p[:, C:] == 0).all(), f"{what}: entries beyond C"
    if N == 0:
        return xd, idx, prob, lse
    print(f"{what}: max |p - p64| = {np.nanmax(np.abs(got_p - ref_p), initial=0.0):.3e}")
    np.testing.assert_allclose(got_p, ref_p, equal_nan=True, err_msg=what, **TK.PROB_TOL)
    np.testing.assert_allclose(got_lse, ref_lse, equal_nan=True, err_msg=what, **TK.PROB_TOL)
    nan_row = np.isnan(xw).any(axis=1)
    assert np.isnan(got_lse[nan_row]).all() and np.isnan(got_p[nan_row][:, :min(k, C)]).all(), f"{what}: a NaN row gives NaN"
    ok = ~nan_row & np.isfinite(xw.max(axis=1))
    val = xw[np.arange(N)[:, None], np.maximum(got_idx, 0)]
    assert (got_p[ok][(val[ok] == -np.inf) & (got_idx[ok] >= 0)] == 0).all(), f"{what}: a -inf logit gives exactly 0"
    return xd, idx, prob, lse


@pytest.mark.parametrize("dt", DTYPES, ids=_ID)
@pytest.mark.parametrize("C", TK.CS)
def test_topk_softmax_equals_the_host_model_on_the_grid(C, dt):
    ops = _gpu()
    g = CR.gen(1000 + C)
    for rows in TK.ROWS:
        for ties in (False, True):
            x = CR.logits(rows, C, g, ties=ties).to(dt)
            for k in TK.KS:
                _check(ops, x, k, f"C={C} rows={rows} k={k} ties={ties} {dt}")
    for k in TK.KS:
        _check(ops, TK.special_rows(C, g).to(dt), k, f"C={C} special rows k={k} {dt}")


@pytest.mark.parametrize("dt", DTYPES, ids=_ID)
@pytest.mark.parametrize("C", TK.CS)
def test_label_rank_of_entry_j_is_j(C, dt):
    ops = _gpu()
    from egopack_amd.meters import label_rank
    g = CR.gen(2000 + C)
    x = torch.cat([CR.logits(5, C, g), CR.logits(5, C, g, ties=True), TK.special_rows(C, g)]).to(dt)
    xd = x.cuda()
    xf = xd.float()  # (the rank kernel reads f32: the widened values, what the launch orders)
    for k in (5, 64):
        (idx, _, _), = ops.topk_softmax([xd], k, want_prob=False)
        for j in range(min(k, C)):
            rank = label_rank(xf, idx[:, j]).cpu()
            entry_is_nan = torch.isnan(x.float()[torch.arange(x.shape[0]), idx[:, j].cpu()])
            assert bool((rank[~entry_is_nan] == j).all()), f"C={C} k={k}: egk_label_rank of entry {j} is {rank.tolist()}"


@pytest.mark.parametrize("C", TK.CS)
def test_first_two_entries_reproduce_the_class_report_and_lse_is_the_loss_kernels(C):
    ops = _gpu()
    from egopack_amd import meters as M
    g = CR.gen(3000 + C)
    for dt in DTYPES:
        x = torch.cat([CR.logits(40, C, g), CR.logits(28, C, g, ties=True), TK.special_rows(C, g)]).to(dt)
        rows = x.shape[0]
        y = CR.labels(rows, C, g)[:, 0].contiguous()
        xf = x.float().cuda()  # (egk_class_report and the loss kernels read f32: the widened values)
        (idx, _, lse), = ops.topk_softmax([x.cuda()], 2, want_prob=False, want_lse=True)
        # ---- the report's confusion and top-2 counts from entries 0 and 1
        state = M._ClassReport(C, "cuda")
        M.class_report([(xf, y.cuda(), state)])
        i0, i1, yn = idx[:, 0].cpu().numpy(), idx[:, 1].cpu().numpy(), y.numpy()
        valid = (yn >= 0) & (yn < C)
        conf, top2 = np.zeros((C, C), np.int64), np.zeros((C, C), np.int64)
        np.add.at(conf, (yn[valid], i0[valid]), 1)
        m = valid & (i0 != yn) & (i1 == yn)
        np.add.at(top2, (yn[m], i0[m]), 1)
        assert np.array_equal(state.confusion.cpu().numpy(), conf) and np.array_equal(state.top2.cpu().numpy(), top2), f"C={C} {dt}"
        # ---- lse is the loss kernels' own: fl32(lse - x[y]) is the cross entropy's row loss, bit for bit
        with torch.no_grad():
            loss = ops.cross_entropy(xf, y.cuda(), 0.0).cpu().numpy()
        mine = lse.cpu().numpy() - x.float().numpy()[np.arange(rows), np.where(valid, yn, 0)]  # (one f32 subtraction)
        assert mine.dtype == np.float32 and valid.sum() >= rows // 2
        assert np.array_equal(mine[valid].view(np.int32)[~np.isnan(mine[valid])], loss[valid].view(np.int32)[~np.isnan(loss[valid])])
        assert np.array_equal(np.isnan(mine[valid]), np.isnan(loss[valid])), f"C={C} {dt}: NaN losses"


def test_two_launches_and_eight_tasks_give_the_same_bits():
    ops = _gpu()
    g = CR.gen(77)
    Cs = (1, 2, 7, 65, 115, 478, 513, 1025)
    for dt in DTYPES:
        xs = [torch.cat([CR.logits(9, C, g, ties=(i % 2 == 1)), TK.special_rows(C, g)]).to(dt).cuda() for i, C in enumerate(Cs)]
        for k in (5, 64):
            a = ops.topk_softmax(xs, k, want_prob=True, want_lse=True)
            b = ops.topk_softmax(xs, k, want_prob=True, want_lse=True)
            singles = [ops.topk_softmax([x], k, want_prob=True, want_lse=True)[0] for x in xs]
            for h, (ta, tb, ts) in enumerate(zip(a, b, singles)):
                for name, u, v, w in zip(("idx", "prob", "lse"), ta, tb, ts):
                    assert torch.equal(_bits(u), _bits(v)), f"head {h} {name}: two launches differ ({dt}, k={k})"
                    assert torch.equal(_bits(u), _bits(w)), f"head {h} {name}: eight tasks differ from one ({dt}, k={k})"


def test_binding_views_mixed_types_optional_outputs_and_no_rows():
    ops = _gpu()
    g = CR.gen(5)
    x = CR.logits(13, 115, g)
    ref = TK.topk_order(x.numpy(), 5)
    # a view with a unit class stride is read in place through its row stride (NaN in the padding)
    view = CR.padded(x.cuda())
    assert view.stride(0) == 119
    (idx, prob, lse), = ops.topk_softmax([view], 5)
    assert np.array_equal(idx.cpu().numpy(), ref) and prob is not None and lse is None
    assert bool(torch.isfinite(prob).all())
    # mixed element types are widened to f32: the bf16 head gives what its widening gives
    xb = CR.logits(13, 478, g).to(torch.bfloat16)
    (i0, p0, l0), (i1, p1, l1) = ops.topk_softmax([x.cuda(), xb.cuda()], 5, want_prob=True, want_lse=True)
    (j1, q1, m1), = ops.topk_softmax([xb.cuda()], 5, want_prob=True, want_lse=True)
    assert np.array_equal(i0.cpu().numpy(), ref) and torch.equal(i1, j1) and torch.equal(_bits(p1), _bits(q1)) and torch.equal(_bits(l1), _bits(m1))
    (i2, p2, l2), = ops.topk_softmax([x.cuda()], 3, want_prob=False, want_lse=False)
    assert p2 is None and l2 is None and np.array_equal(i2.cpu().numpy(), ref[:, :3])
    # no rows: empty tensors, no launch
    out = ops.topk_softmax([torch.empty((0, 115), device="cuda"), torch.empty((0, 478), device="cuda")], 5, want_lse=True)
    assert [tuple(t.shape) for t in out[1]] == [(0, 5), (0, 5), (0,)] and out[0][0].dtype == torch.int64
    with pytest.raises(RuntimeError, match="k in 1 .. 64"):
        ops.topk_softmax([x.cuda()], 65)
    with pytest.raises(ValueError, match="1 .. 8 heads"):
        ops.topk_softmax([x.cuda()] * 9, 5)
