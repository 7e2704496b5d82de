"""DropEdge without a GPU: the host model of the keep decision (tests/edge_drop_common.py), the ``edge_drop:`` block and its
refusals, and the model attribute.  The host model is what the GPU tests hold the device's keep bits to, so its own properties are
pinned here: symmetry, keep_self, p = 0 / 1, one edge set in both CSR orders, disjoint counter reservations, the kept share."""
import math

import numpy as np
import pytest

from tests import edge_drop_common as EC
from tests import philox_ref as PR

SEED, OFF = 0x5EED_0123_4567_89AB, 1000


def _csr(name):
    from egopack_amd import data
    ei, n = EC.GRAPHS[name]()
    return ei, data.build_csr(ei, n)


def test_the_keep_word_is_word_zero_of_the_documented_counter_and_key():
    """One edge transcribed by hand with the scalar generator: (a, b) -> counter offset + word + a, key seed ^ (b << 32)."""
    word = (1 << 40) + 5
    for i, j, sym in ((3, 9, True), (9, 3, True), (3, 9, False), (9, 3, False)):
        a, b = (min(i, j), max(i, j)) if sym else (i, j)
        r = PR.philox_u64_scalar(OFF + word + a, SEED ^ (b << 32))[0]
        want = int(np.float32(r >> 8) * np.float32(2.0 ** -24) >= np.float32(0.3))
        assert int(EC.keep_edges([i], [j], SEED, OFF, 0.3, sym, False, word)[0]) == want
    # 64-bit counter arithmetic wraps
    r = PR.philox_u64_scalar((PR.MASK64 + 1 + 2) & PR.MASK64, SEED)[0]
    assert int(EC.keep_edges([2], [0], SEED, PR.MASK64, 0.5, False, False, 1)[0]) == int(PR.keep_from_words(np.uint32(r), 0.5))


def test_symmetric_mode_gives_both_directions_one_bit():
    i, j = np.meshgrid(np.arange(60), np.arange(60), indexing="ij")
    i, j = i.ravel(), j.ravel()
    fwd = EC.keep_edges(i, j, SEED, OFF, 0.5, True, False)
    rev = EC.keep_edges(j, i, SEED, OFF, 0.5, True, False)
    assert np.array_equal(fwd, rev) and 0 < fwd.sum() < fwd.size


def test_directed_mode_does_not_share_the_bit():
    """Directed mode, offset 0, p = 0.5: seed 2 is the first seed at which 3 -> 4 and 4 -> 3 differ (pinned); symmetric mode gives
    the pair one bit at that seed too."""
    differ = lambda s: EC.keep_edges([4], [3], s, 0, 0.5, False, False)[0] != EC.keep_edges([3], [4], s, 0, 0.5, False, False)[0]  # noqa: E731
    assert not differ(0) and not differ(1) and differ(2)
    assert EC.keep_edges([4], [3], 2, 0, 0.5, True, False)[0] == EC.keep_edges([3], [4], 2, 0, 0.5, True, False)[0]


def test_keep_self_p_zero_and_p_one():
    ei, g = _csr("wrap")
    dst, src = EC.rows_of(g.rowptr.numpy()), g.col.numpy()
    loops = dst == src
    assert loops.any() and not loops.all()
    for sym in (True, False):
        assert EC.keep_fwd(g, SEED, OFF, 0.0, sym, False).all() and EC.keep_fwd(g, SEED, OFF, 0.0, sym, True).all(), "p = 0 keeps all edges"
        assert np.array_equal(EC.keep_fwd(g, SEED, OFF, 1.0, sym, True).astype(bool), loops), "p = 1 keeps only self loops"
        assert not EC.keep_fwd(g, SEED, OFF, 1.0, sym, False).any()
        k = EC.keep_fwd(g, SEED, OFF, 0.9, sym, True)
        assert k[loops].all() and not k[~loops].all(), "keep_self holds while other edges are dropped"
        plain = EC.keep_fwd(g, SEED, OFF, 0.9, sym, False)
        assert np.array_equal(k[~loops], plain[~loops]), "keep_self changes the self loops only"


@pytest.mark.parametrize("name", list(EC.GRAPHS))
@pytest.mark.parametrize("sym", [True, False])
def test_forward_and_transposed_order_describe_one_edge_set(name, sym):
    from egopack_amd import data
    ei, g = _csr(name)
    kf, kb = EC.keep_fwd(g, SEED, OFF, 0.4, sym, True), EC.keep_bwd(g, SEED, OFF, 0.4, sym, True)
    a = EC.edge_set(EC.rows_of(g.rowptr.numpy()), g.col.numpy(), kf)
    b = EC.edge_set(g.t_col.numpy(), EC.rows_of(g.t_rowptr.numpy()), kb)
    assert a == b and int(kf.sum()) == int(kb.sum())
    # the thinned graph lists exactly the kept edges, every row in the full graph's order, in both orientations
    tg = data.build_csr(EC.thin(ei, SEED, OFF, 0.4, sym, True), g.num_nodes)
    assert np.array_equal(tg.col.numpy(), g.col.numpy()[kf.astype(bool)])
    assert np.array_equal(tg.t_col.numpy(), g.t_col.numpy()[kb.astype(bool)])
    cnt = np.bincount(EC.rows_of(g.rowptr.numpy())[kf.astype(bool)], minlength=g.num_nodes)
    assert np.array_equal((tg.rowptr[1:] - tg.rowptr[:-1]).numpy(), cnt)


def test_two_launches_with_disjoint_reservations_share_no_counter():
    rows, word = 6144, 3 << 40
    off0 = 12345
    off1 = off0 + EC.reserved(rows)  # what ops._next_rng(4 * rows) advances by
    assert EC.reserved(rows) == (4 * rows + 3) // 4 + 64
    assert PR.disjoint(EC.intervals(off0, rows, word) + EC.intervals(off1, rows, word))
    assert not PR.disjoint(EC.intervals(off0, rows, word) + EC.intervals(off0 + rows - 1, rows, word))
    # ... and none with the LayerNorm + dropout launch that follows in the stream
    assert PR.disjoint(EC.intervals(off0, rows, word) + [(a + word, b + word) for a, b in PR.row_intervals(off1, 8, 1024)])
    # a replayed step: the device word moves every launch by 2^40, far beyond a step's reservations
    assert PR.disjoint(EC.intervals(off0, rows, 0) + EC.intervals(off0, rows, 1 << 40))


def test_the_kept_share_is_binomial():
    """p = 0.3 over E >= 20 000 distinct edges: within 4 standard deviations, 4 * sqrt(0.3 * 0.7 / E), of 0.7."""
    n = 150
    i, j = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
    off_diag = i != j
    i, j = i[off_diag], j[off_diag]
    E = i.size
    assert E >= 20000
    bound = 4 * math.sqrt(0.21 / E)
    directed = EC.keep_edges(i, j, SEED, OFF, 0.3, False, True).mean()
    assert abs(directed - 0.7) <= bound, (directed, bound)
    # symmetric mode: the independent decisions are the unordered pairs
    n2 = 210
    i2, j2 = np.triu_indices(n2, 1)
    assert i2.size >= 20000
    sym2 = EC.keep_edges(i2, j2, SEED, OFF, 0.3, True, True).mean()
    assert abs(sym2 - 0.7) <= 4 * math.sqrt(0.21 / i2.size), sym2


# ---- configuration -----------------------------------------------------------------------------------------------------------------
def test_defaults():
    from egopack_amd import train as T
    want = {"p": 0.0, "symmetric": True, "keep_self": True, "per_layer": True}
    assert T.edge_drop_config({}) == want and T.check_edge_drop({}) == want
    assert T.edge_drop_config(T.load_config([])) == want, "configs/defaults.yaml"
    got = T.edge_drop_config(T.load_config(["edge_drop.p=0.2", "edge_drop.per_layer=false"]))
    assert got == {**want, "p": 0.2, "per_layer": False}
    T.check_edge_drop({"enable_graphone": True}, enable_graphone=True)  # (p 0: off, nothing to refuse)
    T.check_edge_drop({"edge_drop": {"p": 0.2}, "mixup": {"alpha": 0.4}, "task_weighting": {"mode": "uncertainty"}})


@pytest.mark.parametrize("over, keys", [
    ({"edge_drop": {"p": 1.0}}, ("edge_drop.p",)),
    ({"edge_drop": {"p": -0.1}}, ("edge_drop.p",)),
    ({"edge_drop": {"p": float("nan")}}, ("edge_drop.p",)),
    ({"edge_drop": {"rate": 0.2}}, ("edge_drop", "rate")),
    ({"edge_drop": {"p": 0.2}, "enable_graphone": True}, ("edge_drop.p", "enable_graphone")),
])
def test_every_refusal_names_its_key(over, keys):
    from egopack_amd import train as T
    with pytest.raises(ValueError) as e:
        T.check_edge_drop(dict(over), enable_graphone=bool(over.get("enable_graphone", False)))
    assert all(k in str(e.value) for k in keys), str(e.value)


def test_main_egopack_is_named_in_its_refusal():
    from egopack_amd import train as T
    with pytest.raises(ValueError, match="main_egopack.py"):
        T.check_edge_drop({"edge_drop": {"p": 0.2}}, enable_graphone=True, entry="main_egopack.py")


# ---- the model attribute -------------------------------------------------------------------------------------------------------------
def test_graph_edge_drop_is_a_plain_attribute_outside_the_state_dict():
    from egopack_amd import ops
    from egopack_amd import train as T
    from egopack_amd.models.graph import Graph
    model = Graph(16, hidden_size=16, depth=2)
    assert model.edge_drop is None and model.edge_drop_per_layer is True
    keys = set(model.state_dict())
    T.apply_edge_drop(model, T.edge_drop_config({"edge_drop": {"p": 0.2, "symmetric": False, "per_layer": False}}))
    assert isinstance(model.edge_drop, ops.EdgeDrop) and (model.edge_drop.p, model.edge_drop.symmetric, model.edge_drop.keep_self) == (0.2, False, True)
    assert model.edge_drop_per_layer is False
    assert set(model.state_dict()) == keys and not any("edge_drop" in k for k in keys)
    assert "edge_drop" not in dict(model.named_parameters()) and "edge_drop" not in dict(model.named_buffers())
    T.apply_edge_drop(model, T.edge_drop_config({}))
    assert model.edge_drop is None, "p = 0 leaves the attribute None"


def test_edge_drop_value_type():
    from egopack_amd import ops
    d = ops.EdgeDrop(0.25)
    assert (d.p, d.symmetric, d.keep_self, d.rng, d.flags) == (0.25, True, True, None, 3) and bool(d)
    assert not ops.EdgeDrop(0.0) and ops.EdgeDrop(0.5, symmetric=False, keep_self=False).flags == 0
    assert d.with_rng((7, 9)).rng == (7, 9) and d.rng is None
    for bad in (-0.1, 1.1, float("nan")):
        with pytest.raises(ValueError, match="p must lie in"):
            ops.EdgeDrop(bad)
    before = ops.rng_snapshot()
    seed, off = ops.edge_drop_rng(100)
    assert off == before and ops.rng_snapshot() == before + EC.reserved(100)
