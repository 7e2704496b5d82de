"""The shaped BCE of the PNR head without a GPU: what include/egopack_bce_balanced.h pins beyond the one ledger (tests/test_cabi.py),
the host-side refusals of its three entry points, the host model of tests/pnr_balance_common.py against
F.binary_cross_entropy_with_logits(pos_weight=) and the written-out focal formula in float64, the known answers of
``train.build_pnr_balance``, the configuration keys, and the state-dict keys of a task and a criterion that carry scalars."""
import ctypes
import logging

import pytest
import torch

from tests import pnr_balance_common as PB

# ---- 1. include/egopack_bce_balanced.h beyond the common ledger ------------------------------------------------------------------
# (names, exports, bound types, the bounds ledger and the struct fields of this header: the one ledger, tests/test_cabi.py)


def test_the_bce_balanced_coverage_check_fails_for_an_entry_point_without_a_case():
    from tests import cabi_common as CC
    assert CC.uncovered("bce_balanced") == set() and CC.uncovered("bce_balanced", {"egk_bce_w_not_there"}) == {"egk_bce_w_not_there"}


def test_bce_balanced_has_a_profile_id_of_its_own():
    from egopack_amd import _lib
    lib = _lib.load()
    name = ctypes.create_string_buffer(64)
    n, ms, fl, by = ctypes.c_int64(), ctypes.c_double(), ctypes.c_double(), ctypes.c_double()
    names = []
    for i in range(lib.egk_prof_count()):
        assert lib.egk_prof_get(i, name, 64, ctypes.byref(n), ctypes.byref(ms), ctypes.byref(fl), ctypes.byref(by)) == 0
        names.append(name.value.decode())
    assert {"bce_balanced", "ce_balanced", "bce_fwd", "bce_bwd"} <= set(names) and len(set(names)) == len(names)


# ---- 2. host-side refusals (small fake non-null pointers: every check precedes the first dereference and the first launch) ----------
P = 0x1000
BAD_SCALARS = [dict(pos=-1.0), dict(neg=-0.5), dict(gamma=-2.0), dict(pos=float("nan")), dict(neg=float("inf")),
               dict(gamma=float("inf")), dict(gamma=float("nan")), dict(pos=float("-inf"))]


def _refused(rc, entry, needle):
    from egopack_amd import _lib
    assert rc == -1 and needle in _lib.last_error() and entry in _lib.last_error(), (rc, _lib.last_error())


def test_bce_w_fwd_refuses_bad_arguments_before_any_launch():
    from egopack_amd import _lib
    lib = _lib.load()

    def call(logits=P, y=P, loss=P, n=8, pos=31.0, neg=1.0, gamma=0.0):
        return lib.egk_bce_w_fwd(None, logits, y, loss, n, pos, neg, gamma)

    for k in ("logits", "y", "loss"):
        _refused(call(**{k: None}), "egk_bce_w_fwd", "null pointer")
    _refused(call(n=-1), "egk_bce_w_fwd", "n must be >= 0")
    for kw in BAD_SCALARS:
        _refused(call(**kw), "egk_bce_w_fwd", "must be finite and >= 0")
        _refused(call(n=0, **kw), "egk_bce_w_fwd", "must be finite and >= 0")
    for kw in (dict(), dict(pos=0.0, neg=0.0), dict(gamma=2.0)):  # n == 0 launches nothing; a factor of 0 is allowed
        assert call(n=0, **kw) == 0


def test_bce_w_bwd_refuses_bad_arguments_before_any_launch():
    from egopack_amd import _lib
    lib = _lib.load()

    def call(logits=P, y=P, gloss=P, d=P, n=8, pos=0.25, neg=0.75, gamma=2.0, dtype=0):
        return lib.egk_bce_w_bwd(None, logits, y, gloss, d, n, pos, neg, gamma, dtype)

    for k in ("logits", "y", "gloss", "d"):
        _refused(call(**{k: None}), "egk_bce_w_bwd", "null pointer")
    _refused(call(n=-1), "egk_bce_w_bwd", "n must be >= 0")
    _refused(call(dtype=2), "egk_bce_w_bwd", "unknown activation dtype")
    for kw in BAD_SCALARS:
        _refused(call(**kw), "egk_bce_w_bwd", "must be finite and >= 0")
    for kw in (dict(), dict(dtype=1)):
        assert call(n=0, **kw) == 0


def test_rowdot_bce_w_refuses_bad_arguments_before_any_launch():
    """What egk_rowdot_bce refuses (null pointers, df without ws, unaligned rows of a multiple of 4 columns, rows wider than 4096)
    and what this header adds (rows < 0, the scalars)."""
    from egopack_amd import _lib
    lib = _lib.load()

    def call(f=P, w=P, bias=P, y=P, logits=P, loss=P, df=P, ws=P, rows=8, cols=64, pos=31.0, neg=1.0, gamma=0.0, dtype=1):
        return lib.egk_rowdot_bce_w(None, f, w, bias, y, logits, loss, df, ws, rows, cols, 0.5, pos, neg, gamma, dtype)

    for k in ("f", "w", "y", "logits", "loss"):
        _refused(call(**{k: None}), "egk_rowdot_bce_w", "null pointer")
    _refused(call(ws=None), "egk_rowdot_bce_w", "gradients need the partial-row workspace")
    _refused(call(rows=-1), "egk_rowdot_bce_w", "rows must be >= 0")
    _refused(call(cols=0), "egk_rowdot_bce_w", "cols must be >= 1")
    for kw in BAD_SCALARS:
        _refused(call(**kw), "egk_rowdot_bce_w", "must be finite and >= 0")
    for kw in (dict(f=P + 2), dict(w=P + 4), dict(df=P + 6), dict(f=P + 8, dtype=0)):  # bf16 rows: 8-byte aligned, f32: 16
        _refused(call(**kw), "egk_rowdot_bce_w", "unaligned pointer")
    # rows == 0 launches nothing: the bias and, forward only, df and ws are optional; an odd width has no alignment rule
    for kw in (dict(), dict(bias=None), dict(df=None, ws=None), dict(cols=63, f=P + 2), dict(dtype=0)):
        assert call(rows=0, **kw) == 0
    from egopack_amd._lib import last_error
    assert call(rows=4, cols=4100) != 0 and "4096" in last_error()  # (refused by the width dispatch, before the launch)
    assert call(rows=4, dtype=2) != 0 and "unknown activation dtype" in last_error()


# ---- 3. the host model against torch, float64 ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pos,neg", [(31.0, 1.0), (1.0, 1.0), (15.5, 0.5), (0.25, 0.75)])
def test_host_model_is_torch_bce_with_pos_weight(pos, neg):
    x, y, gl = PB.problem(333, 5)
    assert 0 < int(y.sum()) < y.numel() and float(x.abs().max()) == 100.0
    loss, d = PB.model(x, y, pos, neg, 0.0, gl)
    ref, dref = PB.torch_pos_weight(x, y, pos, neg, gl)
    torch.testing.assert_close(loss, ref, rtol=1e-13, atol=1e-14)
    torch.testing.assert_close(d, dref, rtol=1e-13, atol=1e-14)
    assert bool(torch.isfinite(loss).all()) and bool(torch.isfinite(d).all())
    # (1, 1, 0) is the plain BCE
    import torch.nn.functional as F
    plain, _ = PB.model(x, y)
    torch.testing.assert_close(plain, F.binary_cross_entropy_with_logits(x.double(), y.double(), reduction="none"), rtol=1e-13, atol=1e-14)


@pytest.mark.parametrize("gamma", [2.0, 0.5, 1.0, 5.0])
@pytest.mark.parametrize("pos,neg", [(0.25, 0.75), (1.0, 1.0), (31.0, 1.0)])
def test_host_model_is_the_sigmoid_focal_loss(pos, neg, gamma):
    """torchvision's sigmoid_focal_loss(z, t, alpha, gamma, 'none') written out (pos = alpha, neg = 1 - alpha; alpha < 0: 1, 1),
    gradients by autograd.  The written-out form itself breaks down where the model does not: (1 - p_t) ** gamma with gamma < 1 has
    an infinite derivative at p_t == 1, which sigmoid reaches in float64 beyond |z| ~ 37 -- for gamma < 1 the comparison runs over
    |z| <= 30, and the model's values at the larger logits are checked to be finite."""
    x, y, gl = PB.problem(333, 6)
    loss, d = PB.model(x, y, pos, neg, gamma, gl)
    assert bool(torch.isfinite(loss).all()) and bool(torch.isfinite(d).all())
    keep = x.abs() <= (30.0 if gamma < 1 else 1e9)
    assert int(keep.sum()) >= 320
    ref, dref = PB.torch_focal(x[keep], y[keep], pos, neg, gamma, gl[keep])
    torch.testing.assert_close(loss[keep], ref, rtol=1e-12, atol=1e-14)
    torch.testing.assert_close(d[keep], dref, rtol=1e-11, atol=1e-14)


def test_f32_evaluation_of_the_formulas_stays_inside_the_tolerances():
    """The f32 arithmetic of the header's formulas, in torch on the host, against the float64 model: the reasoning behind
    ``PB.grad_tol`` (no device value enters the bar)."""
    x, y, gl = PB.problem(4096, 7)
    t, z = y.float(), x
    sp = lambda v: v.clamp(min=0) + torch.log1p(torch.exp(-v.abs()))
    for pos, neg, gamma in PB.TRIPLES + [(1.0, 1.0, 0.0), (1.0, 1.0, 5.0)]:
        c = torch.where(y != 0, torch.tensor(pos), torch.tensor(neg))
        if gamma == 0:
            loss = c * ((1 - t) * z + (-z).clamp(min=0) + torch.log1p(torch.exp(-z.abs())))
            d = (c * (1 / (1 + torch.exp(-z)) - t)) * gl
        else:
            s = 2 * t - 1
            u = s * z
            ce, mod, pt = sp(-u), torch.exp(-gamma * sp(u)), 1 / (1 + torch.exp(-u))
            loss, d = c * mod * ce, (s * c * mod * (gamma * pt * (-ce) - (1 - pt))) * gl
        want, dwant = PB.model(x, y, pos, neg, gamma, gl)
        assert loss.dtype == torch.float32 and d.dtype == torch.float32
        torch.testing.assert_close(loss, want.float(), **PB.LOSS_TOL)
        torch.testing.assert_close(d, dwant.float(), **PB.grad_tol(pos, neg))


# ---- 4. the scalars from the counts -------------------------------------------------------------------------------------------------------
class _Cfg(dict):
    pass


def _cfg(*extra, **pb):
    from egopack_amd import train as T
    return T.load_config([f"pnr_balance.{k}={v}" for k, v in pb.items()] + ["synthetic_samples=6", *extra])


def _f32(v):
    return float(torch.tensor(v, dtype=torch.float64).float())


def test_build_pnr_balance_known_answers():
    from egopack_amd import train as T
    cfg = lambda **pb: T.pnr_balance_config(_Cfg(pnr_balance=pb))  # noqa: E731
    # counts (1, 31), auto, normalize: pw = 31, k = 32 / 62
    assert T.pnr_scalars(cfg(mode="pos_weight"), 1, 31) == (_f32(31 * 32 / 62), _f32(32 / 62), 0.0)
    assert T.pnr_scalars(cfg(mode="pos_weight"), 1, 31) == (16.0, _f32(16 / 31), 0.0)
    assert T.pnr_scalars(cfg(mode="pos_weight", normalize=False), 1, 31) == (31.0, 1.0, 0.0)
    assert T.pnr_scalars(cfg(mode="pos_weight", power=0.5, normalize=False), 4, 1020) == (_f32(255 ** 0.5), 1.0, 0.0)
    assert T.pnr_scalars(cfg(mode="pos_weight", pos_weight=3.0, normalize=False), 7, 9) == (3.0, 1.0, 0.0)
    pos, neg, gamma = T.pnr_scalars(cfg(mode="pos_weight", pos_weight=3.0), 10, 90)
    assert (pos, neg, gamma) == (_f32(3 * 100 / 120), _f32(100 / 120), 0.0)
    assert abs((pos * 10 + neg * 90) / 100 - 1) < 1e-6  # the mean factor over the training labels is 1
    assert T.pnr_scalars(cfg(mode="pos_weight"), 0, 64) == (_f32(64.0 * 64 / 64), 1.0, 0.0)  # no positive: n_pos counts as 1 in pw only
    assert T.pnr_scalars(cfg(mode="focal"), 1, 31) == (0.25, 0.75, 2.0)
    assert T.pnr_scalars(cfg(mode="focal", alpha=-1, gamma=1.5), 1, 31) == (1.0, 1.0, 1.5)
    assert T.pnr_scalars(cfg(mode="focal", alpha=0.1, gamma=0.0), 1, 31) == (_f32(0.1), _f32(0.9), 0.0)
    with pytest.raises(ValueError, match="none"):
        T.pnr_scalars(cfg(), 1, 31)


@pytest.mark.parametrize("resident", [False, True])
def test_build_pnr_balance_counts_the_whole_split(resident):
    """One positive node per sequence of T: counts (L, L (T - 1)) from the label table of a resident dataset and from one pass over
    a plain one; the scalars are the formulas of those counts rounded once to f32; PNR not trained or mode none: nothing."""
    from egopack_amd import train as T
    extra = [f"{g}=synthetic_resident" for g in T.DSET_GROUP.values()] if resident else []
    cfg = _cfg("dataset_pnr.T=8", *extra, mode="pos_weight")
    dsets = T.build_datasets(cfg, "train")
    ds = dsets["pnr"]
    assert hasattr(ds, "_tables") == resident
    ys = torch.cat([torch.as_tensor((ds._labels(i) if resident else ds[i]).y).reshape(-1) for i in range(len(ds))])
    n_pos, n_neg = int((ys != 0).sum()), int((ys == 0).sum())
    assert (n_pos, n_neg) == (6, 6 * 7)
    pb = T.build_pnr_balance(cfg, dsets)
    assert (pb["n_pos"], pb["n_neg"]) == (n_pos, n_neg)
    assert (pb["pos"], pb["neg"], pb["gamma"]) == (_f32(7 * 48 / 84), _f32(48 / 84), 0.0)
    assert T.build_pnr_balance(cfg, dsets, tasks=["ar", "lta"]) is None
    assert T.build_pnr_balance(cfg, dsets, tasks=["pnr"]) == pb
    st = T.pnr_balance_state(cfg, pb)
    assert st["config"]["mode"] == "pos_weight" and st["counts"] == {"n_pos": 6, "n_neg": 42}
    assert st["scalars"].dtype == torch.float32 and st["scalars"].tolist() == [pb["pos"], pb["neg"], pb["gamma"]]
    fc = T.build_pnr_balance(_cfg(mode="focal", alpha=0.3, gamma=1.0), dsets)
    assert (fc["pos"], fc["neg"], fc["gamma"], fc["n_pos"]) == (_f32(0.3), _f32(0.7), 1.0, 6)


def test_config_keys_and_refusals():
    from egopack_amd import train as T
    pb = T.pnr_balance_config(_cfg())
    assert pb == {"mode": "none", "pos_weight": "auto", "power": 1.0, "normalize": True, "alpha": 0.25, "gamma": 2.0}
    assert T.pnr_balance_config(_Cfg()) == pb  # a config without the block: the defaults
    assert T.pnr_balance_config(_cfg(mode="focal", gamma=0.5))["gamma"] == 0.5
    assert T.pnr_balance_config(_cfg(mode="pos_weight", pos_weight=31))["pos_weight"] == 31.0
    with pytest.raises(ValueError, match="logit_adjust"):
        T.pnr_balance_config(_cfg(mode="logit_adjust"))
    with pytest.raises(ValueError, match="beta"):
        T.pnr_balance_config(_Cfg(pnr_balance={"beta": 0.999}))
    with pytest.raises(ValueError, match="pos_weight"):
        T.pnr_balance_config(_Cfg(pnr_balance={"mode": "pos_weight", "pos_weight": 0.0}))
    with pytest.raises(ValueError, match="pos_weight"):
        T.pnr_balance_config(_Cfg(pnr_balance={"mode": "pos_weight", "pos_weight": "balanced"}))
    with pytest.raises(ValueError, match="gamma"):
        T.pnr_balance_config(_Cfg(pnr_balance={"mode": "focal", "gamma": -1.0}))
    with pytest.raises(ValueError, match="alpha"):
        T.pnr_balance_config(_Cfg(pnr_balance={"mode": "focal", "alpha": 1.5}))
    # the older block keeps refusing what belongs here
    with pytest.raises(ValueError, match="focal"):
        T.class_balance_config(_Cfg(class_balance={"mode": "focal"}))


def test_mode_none_builds_nothing_and_the_criterion_is_todays():
    from egopack_amd import train as T
    from egopack_amd.criterion import BCEWithLogitsNone
    cfg = _cfg()
    dsets = T.build_datasets(cfg, "train")

    class Untouchable:  # mode none does not even count labels
        def __getitem__(self, k):
            raise AssertionError("mode none looked at the datasets")

        def __contains__(self, k):
            raise AssertionError("mode none looked at the datasets")

    assert T.build_pnr_balance(cfg, Untouchable()) is None
    assert T.pnr_balance_state(cfg, None) is None
    for crit in (T.build_criteria(dsets), T.build_criteria(dsets, None, None), T.build_criteria(dsets, {}, None)):
        assert type(crit["pnr"]) is BCEWithLogitsNone and crit["pnr"].balance() is None and crit["pnr"].train().balance() is None
    on = T.build_criteria(dsets, None, {"pos": 16.0, "neg": 0.5, "gamma": 0.0, "n_pos": 1, "n_neg": 31})["pnr"]
    assert type(on) is BCEWithLogitsNone and on.balance() == (16.0, 0.5, 0.0) and on.eval().balance() is None


def test_checkpoint_comparison_is_bit_for_bit_and_warns_once(caplog):
    from egopack_amd import train as T
    cfg = _cfg("dataset_pnr.T=8", mode="pos_weight")
    pb = T.build_pnr_balance(cfg, T.build_datasets(cfg, "train"))
    st = T.pnr_balance_state(cfg, pb)
    log = logging.getLogger("pnr_balance_test")
    with caplog.at_level(logging.INFO, logger="pnr_balance_test"):
        T.log_pnr_balance(log, cfg, pb)
        T.log_pnr_balance(log, _cfg(), None)
        assert len(caplog.records) == 1
        line = caplog.records[0].getMessage()
        assert line == f"pnr balance: mode pos_weight, 6 positive / 42 negative nodes, pos 4, neg {pb['neg']:.9g}, gamma 0"
        caplog.clear()
        assert T.check_pnr_balance(log, {"pnr_balance": st}, cfg, pb)
        assert T.check_pnr_balance(log, {}, _cfg(), None)
        assert not caplog.records
        st["scalars"][1] = torch.nextafter(st["scalars"][1], torch.tensor(9.0))
        assert not T.check_pnr_balance(log, {"pnr_balance": st}, cfg, pb)
        assert len(caplog.records) == 1 and caplog.records[0].levelno == logging.WARNING
        assert not T.check_pnr_balance(log, {}, cfg, pb)
        assert len(caplog.records) == 2


# ---- 5. state-dict keys, plain attributes ---------------------------------------------------------------------------------------------------
def test_state_dict_keys_do_not_change_with_scalars():
    from egopack_amd.criterion import BCEWithLogitsNone
    from egopack_amd.models.tasks.pnr import PNRTask
    plain, bal = PNRTask(16, 16), PNRTask(16, 16)
    assert plain.loss_balance() is None
    bal.set_loss_balance(31.0, 1.0, 0.0)
    assert list(plain.state_dict()) == list(bal.state_dict())
    plain.load_state_dict(bal.state_dict())  # strict
    bal.load_state_dict(plain.state_dict())
    assert bal.loss_balance() == (31.0, 1.0, 0.0) and not list(bal.buffers())
    bal.set_loss_balance(gamma=2.0)
    assert bal.loss_balance() == (1.0, 1.0, 2.0)  # a missing one defaults to 1, 1, 0
    bal.set_loss_balance(None, None, None)
    assert bal.loss_balance() is None
    for bad in ((-1.0, 1.0, 0.0), (1.0, float("nan"), 0.0), (1.0, 1.0, float("inf"))):
        with pytest.raises(ValueError, match="finite and >= 0"):
            bal.set_loss_balance(*bad)
        with pytest.raises(ValueError, match="finite and >= 0"):
            BCEWithLogitsNone(*bad)
    crit = BCEWithLogitsNone(pos=0.25, neg=0.75, gamma=2.0)
    assert list(crit.state_dict()) == list(BCEWithLogitsNone().state_dict()) == []
    assert not list(crit.buffers()) and not list(crit.parameters())
    assert crit.balance() == (0.25, 0.75, 2.0) and crit.eval().balance() is None and crit.train().balance() == (0.25, 0.75, 2.0)
    assert BCEWithLogitsNone().balance() is None and BCEWithLogitsNone(None, None, None).balance() is None
    assert BCEWithLogitsNone(pos=2.0).balance() == (2.0, 1.0, 0.0)
