"""``egk_action_topk`` and ``egk_edit_distance_pairs`` on the GPU against the host model of tests/action_common.py.

Pairs, ``logp`` and ``rank`` are compared BIT FOR BIT with the model run on the launch's own ``lse``; ``lse`` is compared apart --
bit for bit with ``egk_topk_softmax``'s (without beta and at beta = 1) and with float64 at ``topk_common.PROB_TOL`` --, ``prob``
with the float64 exp at the same tolerance.  The shapes are the smallest that take each path: one class, fewer pairs than k, the
lane and slot edges, the workload's widths, the 16-slot instance at its limits, and one row past the grid's capacity."""
import numpy as np
import pytest
import torch

from tests import action_common as AC
from tests import topk_common as TK

pytestmark = pytest.mark.gpu

DTYPES = (torch.float32, torch.bfloat16)
SHAPES = [(1, 1, 1, 3), (3, 5, 4, 5), (3, 5, 32, 5), (3, 5, 15, 5), (65, 130, 5, 7), (115, 478, 5, 7), (600, 1024, 32, 3)]  # (Cv, Cn, k, rows)
GRID_ROWS = 2048 * 4  # the launch's row capacity: 2048 workgroups of four waves


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from egopack_amd import ops as O
    return O


def inputs(Cv, Cn, rows, dt, kind, seed=0):
    """(zv, zn of ``dt`` on the host, labels int64 [rows, 3]).  ``kind``: grid -- multiples of 0.25, ties dominate; smooth -- few
    ties; special -- a grid with duplicated columns, a -inf column in both heads and a NaN in the last row."""
    g = AC.gen(seed + 7 * Cv + Cn)
    make = AC.smooth if kind == "smooth" else AC.grid
    zv, zn = make(rows, Cv, g), make(rows, Cn, g)
    if kind == "special":
        if Cv > 1:
            zv[:, Cv - 1] = zv[:, 0]        # a duplicated column: every row ties there
            zv[:, Cv // 2] = -float("inf")  # (Cv = 2: the duplicate itself)
        if Cn > 2:
            zn[:, 1] = zn[:, Cn - 1]
            zn[:, 2] = -float("inf")
        zn[rows - 1, Cn // 2] = float("nan")  # the last row has a NaN noun: NaN lse, logp and prob; the order stands
    return zv.to(dt), zn.to(dt), AC.pair_labels(rows, Cv, Cn, g)


def check(ops, zv, zn, y, k, beta=None, padded=True):
    """One launch on (padded) device views, held to the model.  Returns the launch's outputs on the host."""
    dev = lambda t: (TK_pad(t.cuda()) if padded else t.cuda())
    dv, dn, dy = dev(zv), dev(zn), y.cuda()
    bw = None if beta is None else torch.tensor(beta, dtype=torch.float32, device="cuda")
    out = ops.action_topk(dv, dn, k, labels=(dy[:, 0], dy[:, 2]), beta=bw, want_prob=True, want_lse=True)  # (label columns: views)
    again = ops.action_topk(dv, dn, k, labels=(dy[:, 0], dy[:, 2]), beta=bw, want_prob=True, want_lse=True)
    torch.cuda.synchronize()
    for key in out:
        a, b = out[key], again[key]
        assert torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a, b.view(torch.int32) if b.dtype == torch.float32 else b), \
            f"{key}: two launches differ in bits"
    got = {key: v.cpu() for key, v in out.items()}
    xv, xn = TK.widen(zv), TK.widen(zn)
    lse = got["lse"].numpy()
    pair, logp, rank, orders = AC.model(xv, xn, lse, k, labels=(y[:, 0].numpy(), y[:, 2].numpy()), beta=beta)
    assert np.array_equal(got["pair"].numpy(), pair), ("pair", np.argwhere(got["pair"].numpy() != pair)[:4])
    glp = got["logp"].numpy()
    assert np.array_equal(np.isnan(glp), np.isnan(logp)), "logp: the NaN entries"
    assert np.array_equal(np.where(np.isnan(glp), 0, glp.view(np.int32)), np.where(np.isnan(logp), 0, logp.view(np.int32))), \
        "logp (bit for bit; a NaN's payload is not part of the definition)"
    assert np.array_equal(got["rank"].numpy(), rank), ("rank", got["rank"].numpy(), rank)
    # lse against float64; prob against the float64 exp (NaN rows: NaN in both)
    lse64 = np.stack([TK.logsumexp64(AC.scaled(xv, beta and beta[0])), TK.logsumexp64(AC.scaled(xn, beta and beta[1]))], 1)
    torch.testing.assert_close(got["lse"].double(), torch.from_numpy(lse64), equal_nan=True, **TK.PROB_TOL)
    torch.testing.assert_close(got["prob"].double(), torch.from_numpy(AC.prob64(xv, xn, pair, beta)), equal_nan=True, **TK.PROB_TOL)
    # rank < k  <=>  the labelled pair is among the exported ones
    for r in range(y.shape[0]):
        listed = any(int(p[0]) >= 0 and int(p[0]) == int(y[r, 0]) and int(p[1]) == int(y[r, 2]) for p in pair[r])  # ((-1, -1): no pair)
        assert (0 <= int(got["rank"][r]) < k) == listed, (r, int(got["rank"][r]), y[r].tolist())
    return got, dv, dn


def TK_pad(x, pad=4):
    from tests.class_report_common import padded
    return padded(x, pad)


@pytest.mark.parametrize("dt", DTYPES, ids=["f32", "bf16"])
@pytest.mark.parametrize("kind", ["grid", "smooth", "special"])
@pytest.mark.parametrize("Cv,Cn,k,rows", SHAPES, ids=[f"{a}x{b}-k{c}" for a, b, c, _ in SHAPES])
def test_pairs_logp_and_rank_are_the_models_bit_for_bit(ops, Cv, Cn, k, rows, kind, dt):
    zv, zn, y = inputs(Cv, Cn, rows, dt, kind)
    got, dv, dn = check(ops, zv, zn, y, k)
    # without beta: the log-sum-exps are egk_topk_softmax's bits, and pair 0 is (its entry 0 of each head)
    (vi, _, vl), (ni, _, nl) = ops.topk_softmax([dv, dn], 1, want_prob=False, want_lse=True)
    assert torch.equal(got["lse"].view(torch.int32), torch.stack([vl, nl], 1).cpu().view(torch.int32)), "lse: egk_topk_softmax's bits"
    assert torch.equal(got["pair"][:, 0, 0], vi[:, 0].cpu()) and torch.equal(got["pair"][:, 0, 1], ni[:, 0].cpu())
    m = min(k, Cv * Cn)
    assert bool((got["pair"][:, m:] == -1).all()) and bool((got["prob"][:, m:] == 0).all()) and bool(torch.isneginf(got["logp"][:, m:]).all())
    assert bool((got["pair"][:, :m] >= 0).all())
    if kind == "special":
        assert bool(torch.isnan(got["lse"][rows - 1, 1])) and bool(torch.isnan(got["logp"][rows - 1, :m]).all())
        assert bool(torch.isnan(got["prob"][rows - 1, :m]).all()) and int(got["rank"][rows - 1]) >= -1
    if (Cv, Cn, k) == (3, 5, 15) and kind != "special":  # all pairs exported: a distribution
        torch.testing.assert_close(got["prob"].double().sum(1), torch.ones(rows, dtype=torch.float64), **TK.PROB_TOL)


@pytest.mark.parametrize("dt", DTYPES, ids=["f32", "bf16"])
@pytest.mark.parametrize("Cv,Cn,k,rows", [(3, 5, 4, 5), (115, 478, 5, 7), (600, 1024, 32, 3)], ids=["3x5", "115x478", "600x1024"])
def test_beta_scales_both_heads_and_one_is_none(ops, Cv, Cn, k, rows, dt):
    zv, zn, y = inputs(Cv, Cn, rows, dt, "grid", seed=3)
    none, _, _ = check(ops, zv, zn, y, k)
    ones, _, _ = check(ops, zv, zn, y, k, beta=(1.0, 1.0))
    for key in none:  # beta = [1, 1]: fl(1 * z) = z, the same bits as without beta
        a, b = none[key], ones[key]
        assert torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a, b.view(torch.int32) if b.dtype == torch.float32 else b), key
    check(ops, zv, zn, y, k, beta=(0.5, 2.0))
    zs, ns, _ = inputs(Cv, Cn, rows, dt, "smooth", seed=4)
    check(ops, zs, ns, y, k, beta=(0.5, 2.0))
    check(ops, zs, ns, y, k, beta=(0.7, 1.3), padded=False)  # (products that round: x = fl(beta z))


def test_one_row_past_the_grids_capacity_takes_the_strided_loop(ops):
    rows, Cv, Cn, k = GRID_ROWS + 1, 3, 5, 2
    zv, zn, y = inputs(Cv, Cn, rows, torch.float32, "grid", seed=9)
    got, _, _ = check(ops, zv, zn, y, k)
    assert int((got["rank"] >= 0).sum()) == rows - 3  # (pair_labels: three rows with a label outside its head)


def test_the_optional_outputs_may_be_absent_and_no_rows_launch_nothing(ops):
    zv, zn, y = inputs(7, 9, 6, torch.float32, "grid", seed=2)
    full = ops.action_topk(zv.cuda(), zn.cuda(), 3, labels=(y[:, 0].cuda(), y[:, 2].cuda()), want_lse=True)
    bare = ops.action_topk(zv.cuda(), zn.cuda(), 3, want_prob=False, want_logp=False)
    assert bare["logp"] is None and bare["prob"] is None and bare["lse"] is None and bare["rank"] is None
    assert torch.equal(bare["pair"], full["pair"])
    mixed = ops.action_topk(zv.cuda().bfloat16(), zn.cuda(), 3)  # (mixed element types: widened)
    assert torch.equal(mixed["pair"], full["pair"])
    empty = ops.action_topk(zv[:0].cuda(), zn[:0].cuda(), 3, labels=(y[:0, 0].cuda(), y[:0, 2].cuda()), want_lse=True)
    assert tuple(empty["pair"].shape) == (0, 3, 2) and tuple(empty["rank"].shape) == (0,) and tuple(empty["lse"].shape) == (0, 2)
    with pytest.raises(RuntimeError, match="k in 1 .. 32"):
        ops.action_topk(zv.cuda(), zn.cuda(), 33)
    with pytest.raises(ValueError, match="want_rank needs the labels"):
        ops.action_topk(zv.cuda(), zn.cuda(), 3, want_rank=True)


# ---- egk_edit_distance_pairs ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,Z,K", [(5, 20, 5), (4, 1, 3), (3, 64, 2), (0, 20, 5)], ids=["5x20x5", "Z1", "Z64", "N0"])
def test_edit_distance_pairs_columns(ops, N, Z, K):
    from egopack_amd import meters as M
    pv, pn, lv, ln = AC.futures(N, Z, K, AC.gen(N + Z + K))
    got = M.action_edit_distances(pv.cuda(), pn.cuda(), lv.cuda(), ln.cuda())
    assert got.dtype == torch.int32 and tuple(got.shape) == (N, K, 3)
    # columns 0 and 1 are egk_edit_distance's integers, column 2 is the Python model's
    assert torch.equal(got[..., 0], M.edit_distances(pv.cuda(), lv.cuda())) and torch.equal(got[..., 1], M.edit_distances(pn.cuda(), ln.cuda()))
    want = AC.edit_model(pv.numpy(), pn.numpy(), lv.numpy(), ln.numpy())
    assert np.array_equal(got.cpu().numpy(), want)
    if N:
        assert int(got[0, 0].abs().sum()) == 0 and bool((got[..., 2] >= got[..., :2].max(-1).values).all())
        if Z > 1:  # (one position: the action distance IS the larger of the two)
            assert bool((got[..., 2] > got[..., :2].max(-1).values).any()), "the inputs must hold partial matches"


def test_edit_distance_pairs_reads_views_through_their_strides(ops):
    """The meter's views: futures as [N, T, K] slices of per-node predictions with the observed nodes dropped, labels as columns of
    one [N * T, 2] label matrix."""
    from egopack_amd import meters as M
    N, T, K, skip = 4, 9, 5, 2
    g = AC.gen(11)
    pred = [torch.randint(0, 3, (N * T, K), generator=g).cuda(), torch.randint(0, 2, (N * T, K), generator=g).cuda()]
    y = torch.stack([torch.randint(0, 3, (N * T,), generator=g), torch.randint(0, 2, (N * T,), generator=g)], 1).cuda()
    pv, pn = (p.reshape(-1, T, K)[:, skip:] for p in pred)
    lv, ln = (y[:, i].reshape(-1, T)[:, skip:] for i in (0, 1))
    got = M.action_edit_distances(pv, pn, lv, ln)
    want = AC.edit_model(pv.cpu().numpy(), pn.cpu().numpy(), lv.cpu().numpy(), ln.cpu().numpy())
    assert np.array_equal(got.cpu().numpy(), want)
