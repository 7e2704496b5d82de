"""The shaped cross entropy (LDAM margin, focal term) without a GPU: the tail of egk_ce_task and its zero state,
the host-side refusals of the launches that take the struct, the ``ce_shape:`` configuration, the LDAM margins of known counts, the
side deferred re-weighting picks for an epoch, the wrapper / task plumbing, and the numpy f32 restatement of the kernel's
arithmetic against float64 autograd (tests/ce_shape_common.py) -- which also measures the tolerance of the gamma > 0 GPU tests."""
import ctypes
import logging

import pytest
import torch

from tests import ce_shape_common as S

TAIL = ["margin", "gloss", "focal_gamma", "loss_only", "reserved"]


# ---- 1. the struct ------------------------------------------------------------------------------------------------------------------
def test_the_tail_of_ce_task_and_its_zero_state():
    """(Fails without the feature: the struct ends with ``gscale``.)"""
    from egopack_amd import _lib
    from tests import cabi_common as CC
    names = [n for n, _ in CC.struct_fields("hip", "egk_ce_task")]
    assert names[-len(TAIL):] == TAIL and names[-len(TAIL) - 1] == "gscale"
    assert [f[0] for f in _lib.CETask._fields_] == names
    assert _lib.CETask.margin.offset == _lib.CETask.gscale.offset + 4 and _lib.CETask.margin.size == 32
    assert ctypes.sizeof(_lib.CETask) % 8 == 0 and ctypes.sizeof(_lib.CEWTask) == ctypes.sizeof(_lib.CETask) + 64
    t = _lib.CETask()
    assert all(not t.margin[h] for h in range(4)) and not t.gloss and t.focal_gamma == 0.0 and t.loss_only == 0 and t.reserved == 0
    assert [f[0] for f in _lib.CEWTask._fields_] == ["base", "weight", "offset"]  # egk_ce_w_task keeps its own fields


# ---- 2. host-side refusals (small fake non-null pointers: every check precedes the first dereference and the first launch) --------------
P = 0x1000


def _refused(rc, entry, needle):
    from egopack_amd import _lib
    assert rc == -1 and needle in _lib.last_error() and entry in _lib.last_error(), (rc, _lib.last_error())


def _fill(b, n_heads=2, rows=0, **kw):
    for h in range(n_heads):
        b.logits[h], b.ld[h], b.C[h], b.pad[h], b.dcol[h] = P, 8, 5, 8, 8 * h
    b.n_heads, b.y, b.y_stride, b.loss, b.dlogits, b.ldd, b.rows, b.gscale = n_heads, P, n_heads, P, P, 32, rows, 0.5
    for k, v in kw.items():
        if isinstance(v, tuple):
            getattr(b, k)[v[0]] = v[1]
        else:
            setattr(b, k, v)


ENTRIES = ["egk_ce_fused_multi", "egk_ce_w_fused_multi", "egk_ce_fused_multi_s", "egk_ce_w_fused_multi_s"]


def _call(entry, tasks_kw, dtype=0):
    """``entry`` on one zero-row task per dict of ``tasks_kw`` (fields of egk_ce_task by name)."""
    from egopack_amd import _lib
    lib = _lib.load()
    weighted, scaled = "_w_" in entry, entry.endswith("_s")
    arr = ((_lib.CEWTask if weighted else _lib.CETask) * len(tasks_kw))()
    for a, kw in zip(arr, tasks_kw):
        _fill(a.base if weighted else a, **kw)
    args = [None, arr] + ([(ctypes.c_void_p * len(tasks_kw))(*[0x4000] * len(tasks_kw))] if scaled else []) + [len(tasks_kw), 0.1, dtype]
    return getattr(lib, entry)(*args)


@pytest.mark.parametrize("entry", ENTRIES)
def test_the_tail_is_refused_before_any_launch_each_with_its_own_message(entry):
    for off in (1, 2, 3):
        _refused(_call(entry, [dict(margin=(1, 0x2000 + off))]), entry, "misaligned margin pointer")
        _refused(_call(entry, [dict(), dict(gloss=0x3000 + off)]), entry, "gloss) of task 1 are not 4-byte aligned")
    for bad in (-0.5, float("nan"), float("inf"), -float("inf")):
        _refused(_call(entry, [dict(focal_gamma=bad)]), entry, "focal_gamma must be finite and >= 0")
    for bad in (2, -1):
        _refused(_call(entry, [dict(loss_only=bad)]), entry, "loss_only must be 0 or 1")
    _refused(_call(entry, [dict(loss_only=1, gloss=0x3000)]), entry, "loss_only and gloss are both set")
    _refused(_call(entry, [dict(n_heads=1, margin=(1, 0x2000))]), entry, "margin[1] is set but task 0 has 1 heads")
    _refused(_call(entry, [dict(reserved=1)]), entry, "reserved")
    _refused(_call(entry, [dict(dlogits=None)]), entry, "null pointer")           # a NULL dlogits stays refused with loss_only 0 ...
    assert _call(entry, [dict(dlogits=None, loss_only=1)]) == 0                    # ... and is what a forward-only pass may pass
    # the limits are accepted (no row: nothing is launched)
    assert _call(entry, [dict(margin=(0, 0x2000), focal_gamma=2.0, gloss=0x3000)] * 4, dtype=1) == 0
    assert _call(entry, [dict(n_heads=4, margin=(3, 0x2004))]) == 0
    assert _call(entry, [dict()]) == 0


# ---- 3. configuration ------------------------------------------------------------------------------------------------------------------
class _Cfg(dict):
    pass


def _cfg(*extra, **sh):
    from egopack_amd import train as T
    return T.load_config([f"ce_shape.{k}={v}" for k, v in sh.items()] + ["synthetic_samples=6", *extra])


def test_config_defaults_and_refusals():
    from egopack_amd import train as T
    sh = T.ce_shape_config(_cfg())
    assert sh == {"margin": "none", "max_margin": 0.5, "power": 0.25, "gamma": 0.0, "tasks": ["ar", "lta"], "reweight_after": 0}
    assert T.ce_shape_config(_Cfg()) == sh  # a config without the block: the defaults
    assert T.ce_shape_config(_cfg(margin="ldam", gamma=2, reweight_after=3)) == {**sh, "margin": "ldam", "gamma": 2.0, "reweight_after": 3}
    with pytest.raises(ValueError, match="cosine"):
        T.ce_shape_config(_cfg(margin="cosine"))
    with pytest.raises(ValueError, match="alpha"):
        T.ce_shape_config(_Cfg(ce_shape={"alpha": 0.25}))
    with pytest.raises(ValueError, match="pnr"):
        T.ce_shape_config(_Cfg(ce_shape={"tasks": ["ar", "pnr"]}))
    for k in ("gamma", "max_margin", "power"):
        with pytest.raises(ValueError, match=k):
            T.ce_shape_config(_Cfg(ce_shape={k: -1.0}))
    with pytest.raises(ValueError, match="gamma"):
        T.ce_shape_config(_Cfg(ce_shape={"gamma": float("nan")}))
    with pytest.raises(ValueError, match="reweight_after"):
        T.ce_shape_config(_Cfg(ce_shape={"reweight_after": -1}))
    # the class_balance block keeps its keys and its refusals
    with pytest.raises(ValueError, match="focal"):
        T.class_balance_config(_Cfg(class_balance={"mode": "focal"}))
    with pytest.raises(ValueError, match="gamma"):
        T.class_balance_config(_Cfg(class_balance={"gamma": 2.0}))


def test_off_builds_nothing_and_the_criteria_are_todays():
    from egopack_amd import train as T
    cfg = _cfg()

    class Untouchable:  # off does not even count labels
        def __getitem__(self, k):
            raise AssertionError("ce_shape off looked at the datasets")

        def __contains__(self, k):
            raise AssertionError("ce_shape off looked at the datasets")

    assert T.build_ce_shape(cfg, Untouchable()) == {}
    dsets = T.build_datasets(cfg, "train")
    for crit in (T.build_criteria(dsets), T.build_criteria(dsets, {}, None, {}), T.build_criteria(dsets, ce_shape=None)):
        for t in ("ar", "lta"):
            assert crit[t].n_margin == 0 and crit[t].focal_gamma == 0.0 and crit[t].select_shape((None, None)) == (None, 0.0)
            assert not list(crit[t].buffers())
    with pytest.raises(ValueError, match="class_balance.mode=weight"):
        T.build_ce_shape(_cfg(reweight_after=2), Untouchable())


def test_ldam_margins_of_known_counts():
    from egopack_amd import train as T
    n = torch.tensor([5000, 10, 1, 0])
    m = T.ldam_margins(n, max_margin=0.5, power=0.25)
    assert m.dtype == torch.float64
    want = [0.5 * 5000 ** -0.25, 0.5 * 10 ** -0.25, 0.5, 0.5]   # n' = max(n, 1): a class without a label has the margin of one with one
    torch.testing.assert_close(m, torch.tensor(want, dtype=torch.float64), rtol=1e-14, atol=0)
    assert float(m.max()) == 0.5 and float(m[3]) == float(m[2]) == 0.5
    m = T.ldam_margins(torch.tensor([40, 7, 300]), max_margin=0.3, power=0.5)
    assert float(m.max()) == float(m[1]) == 0.3                  # the largest margin IS max_margin, also without a count of 1
    torch.testing.assert_close(m, torch.tensor([0.3 * (7 / 40) ** 0.5, 0.3, 0.3 * (7 / 300) ** 0.5], dtype=torch.float64), rtol=1e-14, atol=0)
    assert bool((T.ldam_margins(n, 0.0) == 0).all())


@pytest.mark.parametrize("with_balance", [False, True])
def test_build_ce_shape_counts_the_whole_split_like_class_balance(with_balance):
    from egopack_amd import train as T
    cfg = _cfg(*(["class_balance.mode=weight"] if with_balance else []), margin="ldam", gamma=0.5, tasks="[lta]", max_margin=0.4)
    dsets = T.build_datasets(cfg, "train")
    cb = T.build_class_balance(cfg, dsets) if with_balance else None
    sh = T.build_ce_shape(cfg, dsets, class_balance=cb)
    assert list(sh) == ["lta"] and sh["lta"]["gamma"] == 0.5
    counts = T.label_counts(dsets["lta"])
    for h, c in enumerate(counts):
        assert torch.equal(sh["lta"]["counts"][h], c)
        assert sh["lta"]["margins"][h].dtype == torch.float32 and torch.equal(sh["lta"]["margins"][h], T.ldam_margins(c, 0.4, 0.25).float())
        assert float(sh["lta"]["margins"][h].max()) == float(torch.tensor(0.4, dtype=torch.float32))
    crit = T.build_criteria(dsets, cb, None, sh)
    assert crit["ar"].n_margin == 0 and crit["lta"].n_margin == 2 and crit["lta"].focal_gamma == 0.5
    margins, gamma = crit["lta"].select_shape((None, None))
    assert gamma == 0.5 and all(torch.equal(a, b) for a, b in zip(margins, sh["lta"]["margins"]))
    assert crit["lta"].eval().select_shape((None, None)) == (None, 0.0)     # validation: the plain cross entropy
    only_gamma = T.build_ce_shape(_cfg(gamma=2.0), dsets)                    # the focal term alone: nothing is counted
    assert set(only_gamma) == {"ar", "lta"} and only_gamma["ar"] == {"margins": None, "gamma": 2.0, "counts": None}


def test_reweight_after_picks_the_side_from_the_epoch_and_rewrites_in_place():
    from egopack_amd import train as T
    cfg = _cfg("class_balance.mode=weight", reweight_after=3)
    assert [T.reweight_side(cfg, e) for e in (1, 2, 3, 4)] == ["ones", "ones", "weights", "weights"]
    assert [T.reweight_side(_cfg("class_balance.mode=weight"), e) for e in (1, 5)] == ["weights", "weights"]  # 0: never deferred
    dsets = T.build_datasets(cfg, "train")
    cb = T.build_class_balance(cfg, dsets)
    crit = T.build_criteria(dsets, cb)
    log = logging.getLogger("ce_shape_test")
    bufs = {t: [getattr(crit[t], f"class_weight_{h}") for h in range(2)] for t in ("ar", "lta")}
    ptrs = {t: [b.data_ptr() for b in bs] for t, bs in bufs.items()}
    # a run resumed from a checkpoint of epoch 1 starts at epoch 2 (ones); one of epoch 2 starts at epoch 3 (the weights)
    for epoch, side in ((2, "ones"), (3, "weights"), (1, "ones"), (4, "weights")):
        assert T.apply_reweight(log, cfg, cb, crit, epoch) == side
        for t in ("ar", "lta"):
            for h in range(2):
                want = torch.ones_like(cb[t]["weights"][h]) if side == "ones" else cb[t]["weights"][h]
                assert torch.equal(bufs[t][h], want) and bufs[t][h].data_ptr() == ptrs[t][h]   # in place: the pointers stand
    assert not torch.equal(cb["lta"]["weights"][1], torch.ones_like(cb["lta"]["weights"][1]))  # (the stored vectors stay the weights)
    assert T.apply_reweight(log, _cfg("class_balance.mode=weight"), cb, crit, 1) is None       # off: nothing is touched


# ---- 4. wrapper and tasks ----------------------------------------------------------------------------------------------------------------
def test_wrapper_and_tasks_carry_the_terms_outside_the_state_dict():
    from egopack_amd.criterion import CrossEntropyNone, MetricSelectorWrapper
    from egopack_amd.models.tasks.lta import LTATask
    from egopack_amd.models.tasks.recognition import RecognitionTask

    class Joint:
        has_joint_label, num_labels = True, 3

    m = [torch.rand(4), torch.rand(6), torch.rand(24)]
    sep = MetricSelectorWrapper(CrossEntropyNone(), Joint(), class_margins=m, focal_gamma=2.0)
    logits = (torch.zeros(2, 4), torch.zeros(2, 6), torch.zeros(2, 24))
    margins, gamma = sep.select_shape(logits)
    assert gamma == 2.0 and len(margins) == 2 and margins[0] is sep.class_margin_0 and margins[1] is sep.class_margin_1
    joint = MetricSelectorWrapper(CrossEntropyNone(), Joint(), True, class_margins=[None, None, m[2]])
    margins, gamma = joint.select_shape(logits)
    assert gamma == 0.0 and len(margins) == 1 and margins[0] is joint.class_margin_2
    assert list(sep.state_dict()) == [] and sep.eval().select_shape(logits) == (None, 0.0)
    assert MetricSelectorWrapper(CrossEntropyNone(), Joint(), focal_gamma=0.5).select_shape(logits) == (None, 0.5)
    for bad in (-1.0, float("inf"), float("nan")):
        with pytest.raises(ValueError, match="focal exponent"):
            MetricSelectorWrapper(CrossEntropyNone(), Joint(), focal_gamma=bad)
    ce = CrossEntropyNone(margin=m[0], gamma=0.5)
    assert list(ce.state_dict()) == [] and torch.equal(ce.margin, m[0]) and ce.gamma == 0.5
    for cls in (RecognitionTask, LTATask):
        plain, shaped = cls(16, 16, heads=(5, 7)), cls(16, 16, heads=(5, 7))
        assert plain.ce_shape() == (None, 0.0)
        shaped.set_ce_shape([torch.rand(5), None], 2.0)
        assert list(plain.state_dict()) == list(shaped.state_dict())
        got, gamma = shaped.ce_shape()
        assert gamma == 2.0 and got[0] is shaped.class_margin_0 and got[1] is None
        shaped.set_ce_shape(None, 0.0)
        assert shaped.ce_shape() == (None, 0.0)
        with pytest.raises(ValueError, match="head 1"):
            shaped.set_ce_shape([torch.ones(5), torch.ones(6)])
        with pytest.raises(ValueError, match="2 heads"):
            shaped.set_ce_shape([torch.ones(5)])


def test_ops_validate_margin_and_gamma_like_the_vectors():
    from egopack_amd import ops
    logits = (torch.zeros(3, 5), torch.zeros(3, 7))
    assert ops._ce_shape(None, 0.0, logits) is None and ops._ce_shape((None, None), 0, logits) is None
    m, g = ops._ce_shape((torch.ones(5), None), 0.5, logits)
    assert g == 0.5 and m[1] is None and torch.equal(m[0], torch.ones(5))
    assert ops._ce_shape(None, 2.0, logits) == ((None, None), 2.0)
    with pytest.raises(ValueError, match="head 1"):
        ops._ce_shape((None, torch.ones(6)), 0.0, logits)
    with pytest.raises(ValueError, match="head 0"):
        ops._ce_shape((torch.ones(5, dtype=torch.float64), None), 0.0, logits)
    with pytest.raises(ValueError, match="2 heads"):
        ops._ce_shape(torch.ones(5), 0.0, logits)
    for bad in (-1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="gamma"):
            ops._ce_shape(None, bad, logits)


# ---- 5. the f32 restatement against float64 autograd ------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def restated():
    """(loss error, gradient error) of the restatement per case of ``S.cases()``, each the largest over the heads; the checks of
    ``S.check`` that do not depend on a tolerance (ignored rows, q == 1 rows, inf / nan entries) are asserted on the way."""
    out = {}
    for heads, eps, gamma, presence in S.cases():
        logits, y, gloss = S.problem(heads)
        ms, ws, offs = S.vectors(heads, presence)
        errs = []
        for h, x in enumerate(logits):
            loss, dx = S.restate_f32(x, y[:, h], ws[h], offs[h], ms[h], eps, gamma, gloss)
            errs.append(S.check(torch.from_numpy(loss), torch.from_numpy(dx), x, y[:, h], ws[h], offs[h], ms[h], eps, gamma, gloss,
                                what=f"{heads} head {h} eps {eps} gamma {gamma} {presence}", measure=gamma > 0))
        out[(heads, eps, gamma, presence)] = (max(e[0] for e in errs), max(e[1] for e in errs))
    return out


def test_restatement_with_gamma_0_is_inside_the_projects_tolerances(restated):
    """(``S.check`` asserted them case by case; here: the cases exist and the row with q -> 1 is what ``problem`` says it is.)"""
    assert sum(1 for k in restated if k[2] == 0) == len(S.HEADS) * len(S.EPS) * len(S.PRESENCE)
    for heads in S.HEADS:
        logits, y, _ = S.problem(heads)
        for h, x in enumerate(logits):
            q64 = torch.softmax(x.double(), 1)[3, 0]
            assert float(q64) < 1.0 and float(q64.float()) == 1.0, "row 3: q rounds to 1 in f32 and not in float64"
            assert bool(torch.isinf(x[4]).any()) and int(y[0, h]) == -1 and int(y[5, h]) == x.shape[1]


def test_restatement_with_gamma_above_0_measures_the_bound_of_the_gpu_tests(restated):
    """The largest absolute error of the f32 restatement over every gamma > 0 case: outside the project's tolerances (the row
    with q -> 1, tests/ce_shape_common.py), so the GPU tests' bound is 4 x this error -- the constants are pinned to the measurement
    here (within 3 %: exp / pow of another numpy may round differently), never to a kernel's output."""
    shaped = {k: v for k, v in restated.items() if k[2] > 0}
    loss_err, grad_err = max(v[0] for v in shaped.values()), max(v[1] for v in shaped.values())
    print(f"restatement, gamma > 0: max |loss error| {loss_err:.4e}, max |gradient error| {grad_err:.4e}")
    assert loss_err > S.LOSS_TOL["atol"] and grad_err > S.GRAD_TOL["atol"], "inside the project's tolerances after all: use them"
    assert 0.97 * S.SHAPED_LOSS_ERR <= loss_err <= S.SHAPED_LOSS_ERR
    assert 0.97 * S.SHAPED_GRAD_ERR <= grad_err <= S.SHAPED_GRAD_ERR
    assert S.SHAPED_LOSS_TOL == dict(rtol=0.0, atol=4 * S.SHAPED_LOSS_ERR) and S.SHAPED_GRAD_TOL == dict(rtol=0.0, atol=4 * S.SHAPED_GRAD_ERR)
    # without the row whose q rounds to 1 the restatement IS inside the project's tolerances: the bound is that row's
    for (heads, eps, gamma, presence) in shaped:
        logits, y, gloss = S.problem(heads)
        ms, ws, offs = S.vectors(heads, presence)
        keep = torch.arange(S.ROWS) != 3
        for h, x in enumerate(logits):
            loss, dx = S.restate_f32(x[keep], y[keep, h], ws[h], offs[h], ms[h], eps, gamma, gloss[keep])
            ref_loss, ref_grad, q = S.reference(x[keep], y[keep, h], ws[h], offs[h], ms[h], eps, gamma, gloss[keep])
            fin, gfin = torch.isfinite(ref_loss), torch.isfinite(ref_grad)
            torch.testing.assert_close(torch.from_numpy(loss).double()[fin], ref_loss[fin], **S.LOSS_TOL)
            torch.testing.assert_close(torch.from_numpy(dx).double()[gfin], ref_grad[gfin], **S.GRAD_TOL)
