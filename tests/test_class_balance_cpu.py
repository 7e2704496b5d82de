"""The class-balanced cross entropy without a GPU: what include/egopack_ce_balanced.h pins beyond the one ledger (tests/test_cabi.py),
the host-side refusals of its three entry points, the host model of tests/class_balance_common.py against F.cross_entropy in
float64, the vector builders' known answers, the configuration keys, and the state-dict keys of a task and a wrapper that carry
vectors."""
import ctypes

import pytest
import torch

from tests import class_balance_common as CB

# ---- 1. include/egopack_ce_balanced.h beyond the common ledger -------------------------------------------------------------------
# (names, exports, bound types, the bounds ledger and the struct fields of this header: the one ledger, tests/test_cabi.py)


def test_ce_w_task_layout_matches_header():
    from egopack_amd import _lib
    from tests import cabi_common as CC
    names = [n for n, _ in CC.struct_fields("ce_balanced", "egk_ce_w_task")]
    assert names == [f[0] for f in _lib.CEWTask._fields_] == ["base", "weight", "offset"]
    assert _lib.CEWTask.base.offset == 0 and _lib.CEWTask.weight.offset == ctypes.sizeof(_lib.CETask)
    assert ctypes.sizeof(_lib.CETask) % 8 == 0 and ctypes.sizeof(_lib.CEWTask) == ctypes.sizeof(_lib.CETask) + 64


def test_the_ce_balanced_coverage_check_fails_for_an_entry_point_without_a_case():
    from tests import cabi_common as CC
    assert CC.uncovered("ce_balanced") == set() and CC.uncovered("ce_balanced", {"egk_ce_w_not_there"}) == {"egk_ce_w_not_there"}


def test_ce_balanced_has_a_profile_id_of_its_own():
    from egopack_amd import _lib
    lib = _lib.load()
    name = ctypes.create_string_buffer(64)
    n, ms, fl, by = ctypes.c_int64(), ctypes.c_double(), ctypes.c_double(), ctypes.c_double()
    names = []
    for i in range(lib.egk_prof_count()):
        assert lib.egk_prof_get(i, name, 64, ctypes.byref(n), ctypes.byref(ms), ctypes.byref(fl), ctypes.byref(by)) == 0
        names.append(name.value.decode())
    assert {"ce_balanced", "ce_fwd", "ce_bwd"} <= set(names) and len(set(names)) == len(names)


# ---- 2. host-side refusals (small fake non-null pointers: every check precedes the first dereference and the first launch) ----------
P = 0x1000


def _refused(rc, entry, needle):
    from egopack_amd import _lib
    assert rc == -1 and needle in _lib.last_error() and entry in _lib.last_error(), (rc, _lib.last_error())


def test_ce_w_fwd_refuses_bad_arguments_before_any_launch():
    from egopack_amd import _lib
    lib = _lib.load()

    def call(logits=P, y=P, w=0x2000, a=0x3000, loss=P, lse=P, rows=8, C=5):
        return lib.egk_ce_w_fwd(None, logits, 8, y, 1, w, a, loss, lse, rows, C, 0.1, 0)

    for k in ("logits", "y", "loss", "lse"):
        _refused(call(**{k: None}), "egk_ce_w_fwd", "null pointer")
    for C in (0, -3):
        _refused(call(C=C), "egk_ce_w_fwd", "C must be >= 1")
    _refused(call(rows=-1), "egk_ce_w_fwd", "rows must be >= 0")
    for off in (1, 2, 3):
        _refused(call(w=0x2000 + off), "egk_ce_w_fwd", "misaligned vector pointer")
        _refused(call(a=0x3000 + off), "egk_ce_w_fwd", "misaligned vector pointer")
    for kw in (dict(), dict(w=None), dict(a=None), dict(w=None, a=None)):  # rows == 0 launches nothing; both vectors are optional
        assert call(rows=0, **kw) == 0


def test_ce_w_bwd_refuses_bad_arguments_before_any_launch():
    from egopack_amd import _lib
    lib = _lib.load()

    def call(logits=P, y=P, w=0x2000, a=0x3000, lse=P, gloss=P, d=P, rows=8, C=5, dtype=0):
        return lib.egk_ce_w_bwd(None, logits, 8, y, 1, w, a, lse, gloss, d, 8, rows, C, 0.1, dtype)

    for k in ("logits", "y", "lse", "gloss", "d"):
        _refused(call(**{k: None}), "egk_ce_w_bwd", "null pointer")
    _refused(call(C=0), "egk_ce_w_bwd", "C must be >= 1")
    _refused(call(rows=-1), "egk_ce_w_bwd", "rows must be >= 0")
    _refused(call(dtype=2), "egk_ce_w_bwd", "unknown activation dtype")
    for off in (1, 2, 3):
        _refused(call(w=0x2000 + off), "egk_ce_w_bwd", "misaligned vector pointer")
        _refused(call(a=0x3000 + off), "egk_ce_w_bwd", "misaligned vector pointer")
    for kw in (dict(), dict(w=None, a=None), dict(dtype=1)):
        assert call(rows=0, **kw) == 0


def _task(n_heads=2, rows=0, **kw):
    from egopack_amd import _lib
    t = _lib.CEWTask()
    b = t.base
    for h in range(n_heads):
        b.logits[h], b.ld[h], b.C[h], b.pad[h], b.dcol[h] = P, 8, 5, 8, 8 * h
        t.weight[h], t.offset[h] = 0x2000, 0x3000
    b.n_heads, b.y, b.y_stride, b.loss, b.dlogits, b.ldd, b.rows, b.gscale = n_heads, P, n_heads, P, P, 32, rows, 0.5
    for k, v in kw.items():
        if k in ("weight", "offset"):
            getattr(t, k)[v[0]] = v[1]
        elif isinstance(v, tuple):
            getattr(b, k)[v[0]] = v[1]
        else:
            setattr(b, k, v)
    return t


def test_ce_w_fused_multi_refuses_bad_arguments_before_any_launch():
    from egopack_amd import _lib
    lib = _lib.load()

    def call(tasks, count=None, dtype=0):
        arr = (_lib.CEWTask * max(len(tasks), 1))(*tasks)
        return lib.egk_ce_w_fused_multi(None, arr, len(tasks) if count is None else count, 0.1, dtype)

    _refused(lib.egk_ce_w_fused_multi(None, None, 1, 0.0, 0), "egk_ce_w_fused_multi", "null pointer")
    for count in (0, -1, 5):
        _refused(call([_task()], count=count), "egk_ce_w_fused_multi", "1 .. 4 tasks")
    for n_heads in (0, 5, -2):
        bad = _task()
        bad.base.n_heads = n_heads
        _refused(call([_task(), bad]), "egk_ce_w_fused_multi", "1 .. 4 heads")
    for k in ("y", "loss", "dlogits"):
        _refused(call([_task(**{k: None})]), "egk_ce_w_fused_multi", "null pointer")
    _refused(call([_task(), _task(logits=(1, None))]), "egk_ce_w_fused_multi", "null pointer")
    _refused(call([_task(C=(1, 0))]), "egk_ce_w_fused_multi", "C must be >= 1")
    _refused(call([_task(pad=(0, 4))]), "egk_ce_w_fused_multi", "pad must be >= C")
    _refused(call([_task(rows=-1)]), "egk_ce_w_fused_multi", "rows must be >= 0")
    _refused(call([_task()], dtype=2), "egk_ce_w_fused_multi", "unknown activation dtype")
    for off in (1, 2, 3):
        _refused(call([_task(weight=(1, 0x2000 + off))]), "egk_ce_w_fused_multi", "misaligned vector pointer")
        _refused(call([_task(), _task(offset=(0, 0x3000 + off))]), "egk_ce_w_fused_multi", "misaligned vector pointer")
    # the limits are accepted; no row in any task launches nothing; every vector is optional
    assert call([_task(n_heads=4)] * 4) == 0
    assert call([_task(n_heads=1, weight=(0, None), offset=(0, None))], dtype=1) == 0


# ---- 3. the host model is F.cross_entropy(x + a, y, weight=w, ...) ------------------------------------------------------------------------
@pytest.mark.parametrize("C", [2, 115, 478])
@pytest.mark.parametrize("eps", [0.0, 0.1])
@pytest.mark.parametrize("vectors", ["weight", "offset", "both", "none"])
def test_host_model_is_torch_cross_entropy(C, eps, vectors):
    g = torch.Generator().manual_seed(C * 13 + int(eps * 10))
    rows = 41
    x = 3 * torch.randn(rows, C, generator=g, dtype=torch.float64)
    y = torch.randint(0, C, (rows,), generator=g)
    y[::3] = -1
    gl = torch.randn(rows, generator=g, dtype=torch.float64)
    w = CB.zipf_weights(C).double() if vectors in ("weight", "both") else None
    if w is not None:
        w[C // 2] = 0.0                                   # a class of weight exactly 0 ...
        y[1] = C // 2                                     # ... that a live row is labelled with
    a = CB.zipf_offsets(C).double() if vectors in ("offset", "both") else None
    loss, lse, d = CB.model(x, y, w, a, eps, gl)
    ref, dref = CB.torch_reference(x, y, w, a, eps, gl)
    torch.testing.assert_close(loss, ref, rtol=1e-12, atol=1e-12)
    torch.testing.assert_close(d, dref, rtol=1e-11, atol=1e-13)
    torch.testing.assert_close(lse, torch.logsumexp(x + (0 if a is None else a), 1), rtol=0, atol=0)
    assert bool((loss[::3] == 0).all()) and bool((d[::3] == 0).all())
    if w is not None and eps == 0:
        assert float(loss[1]) == 0.0 and bool((d[1] == 0).all())  # weight 0: the row counts for nothing
    # an all-ignored batch
    loss, _, d = CB.model(x, torch.full((rows,), -1), w, a, eps, gl)
    ref, dref = CB.torch_reference(x, torch.full((rows,), -1), w, a, eps, gl)
    assert not loss.any() and not d.any() and not ref.any() and not dref.any()


# ---- 4. the builders ------------------------------------------------------------------------------------------------------------------
def test_builders_known_answers():
    from egopack_amd import train as T
    n = torch.tensor(CB.COUNTS)
    w = T.class_weights(n, "effective_number", beta=0.999, normalize=False)
    assert w.dtype == torch.float64
    torch.testing.assert_close(w, torch.tensor(CB.known_effective_number(), dtype=torch.float64), rtol=1e-12, atol=0)
    torch.testing.assert_close(w, torch.tensor([0.0010067665909753987, 0.10045082541138471, 1.0, 1.0], dtype=torch.float64),
                               rtol=1e-12, atol=0)
    w = T.class_weights(n, "inverse_frequency", power=1.0, normalize=False)
    torch.testing.assert_close(w, torch.tensor([1 / 5000, 1 / 10, 1.0, 1.0], dtype=torch.float64), rtol=1e-15, atol=0)
    assert w.tolist() == CB.known_inverse_frequency()
    w = T.class_weights(n, "inverse_frequency", power=0.5, normalize=False)
    torch.testing.assert_close(w, torch.tensor([5000 ** -0.5, 10 ** -0.5, 1.0, 1.0], dtype=torch.float64), rtol=1e-15, atol=0)
    a = T.logit_offsets(n, tau=1.0)
    torch.testing.assert_close(a, torch.tensor(CB.known_logit_adjust(), dtype=torch.float64), rtol=1e-12, atol=0)
    torch.testing.assert_close(a, torch.tensor([-0.0023971245997215147, -6.217005223021913, -8.51959031601596, -8.51959031601596],
                                               dtype=torch.float64), rtol=1e-12, atol=0)
    torch.testing.assert_close(T.logit_offsets(n, tau=0.5), 0.5 * a, rtol=1e-15, atol=0)
    for scheme in ("effective_number", "inverse_frequency"):
        w = T.class_weights(n, scheme, normalize=True)
        assert abs(float((n.double() * w).sum()) - float(n.sum())) <= 1e-12 * float(n.sum())  # mean weight over the labels is 1
        raw = T.class_weights(n, scheme, normalize=False)
        torch.testing.assert_close(w / w[0], raw / raw[0], rtol=1e-14, atol=0)              # one common factor
        assert float(w[3]) == float(w[2])                                                       # zero count == count 1
    assert float(a[3]) == float(a[2])
    with pytest.raises(ValueError, match="harmonic"):
        T.class_weights(n, "harmonic")


class _Cfg(dict):
    pass


def _cfg(**cb):
    from egopack_amd import train as T
    return T.load_config([f"class_balance.{k}={v}" for k, v in cb.items()] + ["synthetic_samples=6"])


def test_config_keys_and_refusals():
    from egopack_amd import train as T
    cb = T.class_balance_config(_cfg())
    assert cb == {"mode": "none", "scheme": "effective_number", "beta": 0.999, "power": 1.0, "tau": 1.0, "normalize": True,
                  "tasks": ["ar", "lta"]}
    assert T.class_balance_config(_Cfg()) == cb  # a config without the block: the defaults
    assert T.class_balance_config(_cfg(mode="logit_adjust", tau=0.5))["tau"] == 0.5
    with pytest.raises(ValueError, match="focal"):
        T.class_balance_config(_cfg(mode="focal"))
    with pytest.raises(ValueError, match="harmonic"):
        T.class_balance_config(_cfg(mode="weight", scheme="harmonic"))
    with pytest.raises(ValueError, match="gamma"):
        T.class_balance_config(_Cfg(class_balance={"gamma": 2.0}))
    with pytest.raises(ValueError, match="pnr"):
        T.class_balance_config(_Cfg(class_balance={"mode": "weight", "tasks": ["ar", "pnr"]}))
    with pytest.raises(ValueError, match="beta"):
        T.class_balance_config(_cfg(mode="weight", beta=1.0))


def test_mode_none_builds_nothing_and_the_criteria_are_todays():
    from egopack_amd import train as T
    from egopack_amd.criterion import BCEWithLogitsNone, CrossEntropyNone, MetricSelectorWrapper
    cfg = _cfg()
    dsets = T.build_datasets(cfg, "train")

    class Untouchable:  # mode none does not even count labels
        def __getitem__(self, k):
            raise AssertionError("mode none looked at the datasets")

        def __contains__(self, k):
            raise AssertionError("mode none looked at the datasets")

    assert T.build_class_balance(cfg, Untouchable()) == {}
    assert T.class_balance_state(cfg, {}) is None
    for crit in (T.build_criteria(dsets), T.build_criteria(dsets, {}), T.build_criteria(dsets, None)):
        assert [type(crit[t]) for t in ("ar", "lta", "oscc", "pnr")] == [MetricSelectorWrapper, MetricSelectorWrapper,
                                                                          CrossEntropyNone, BCEWithLogitsNone]
        for t in ("ar", "lta"):
            assert crit[t].n_balance == 0 and crit[t].select_balance((None, None)) == (None, None)
            assert not list(crit[t].buffers()) and type(crit[t].criterion) is CrossEntropyNone
            assert crit[t].criterion.weight is None and crit[t].criterion.offset is None


@pytest.mark.parametrize("mode", ["weight", "logit_adjust"])
def test_build_class_balance_counts_the_whole_split(mode):
    """Counts from the label table of a resident dataset and from one pass over a plain dataset agree with a direct count; the
    vectors are the formulas of those counts, rounded once to f32."""
    from egopack_amd import train as T
    cfg = _cfg(mode=mode, tasks="[lta]")
    dsets = T.build_datasets(cfg, "train")
    cb = T.build_class_balance(cfg, dsets)
    assert list(cb) == ["lta"]
    ds = dsets["lta"]
    ys = torch.cat([torch.as_tensor(ds[i].y).reshape(-1, 2) for i in range(len(ds))])
    for h, Cn in enumerate(ds.num_class_labels):
        col = ys[:, h]
        want = torch.bincount(col[col >= 0], minlength=Cn)
        assert torch.equal(cb["lta"]["counts"][h], want) and cb["lta"]["counts"][h].dtype == torch.int64
        if mode == "weight":
            assert cb["lta"]["offsets"] is None
            assert torch.equal(cb["lta"]["weights"][h], T.class_weights(want).float())
        else:
            assert cb["lta"]["weights"] is None
            assert torch.equal(cb["lta"]["offsets"][h], T.logit_offsets(want).float())
    rcfg = T.load_config([f"class_balance.mode={mode}", "synthetic_samples=6"] +
                         [f"{g}=synthetic_resident" for g in T.DSET_GROUP.values()])
    rsets = T.build_datasets(rcfg, "train")
    rb = T.build_class_balance(rcfg, rsets)
    for t in ("ar", "lta"):
        direct = T.label_counts(type("Plain", (), {"num_class_labels": rsets[t].num_class_labels, "__len__": lambda s: len(rsets[t]),
                                                   "__getitem__": lambda s, i: rsets[t]._labels(i)})())
        assert all(torch.equal(a, b) for a, b in zip(rb[t]["counts"], direct))
    st = T.class_balance_state(rcfg, rb)
    assert st["config"]["mode"] == mode and set(st["vectors"]) == {"ar", "lta"}


def test_checkpoint_comparison_is_bit_for_bit_and_warns_once(caplog):
    import logging
    from egopack_amd import train as T
    cfg = _cfg(mode="weight")
    cb = T.build_class_balance(cfg, T.build_datasets(cfg, "train"))
    st = T.class_balance_state(cfg, cb)
    log = logging.getLogger("class_balance_test")
    with caplog.at_level(logging.WARNING, logger="class_balance_test"):
        assert T.check_class_balance(log, {"class_balance": st}, cfg, cb)
        assert T.check_class_balance(log, {}, _cfg(), {})
        assert not caplog.records
        st["vectors"]["lta"]["weights"][1][7] = torch.nextafter(st["vectors"]["lta"]["weights"][1][7], torch.tensor(9.0))
        assert not T.check_class_balance(log, {"class_balance": st}, cfg, cb)
        assert len(caplog.records) == 1
        assert not T.check_class_balance(log, {}, cfg, cb)
        assert len(caplog.records) == 2


# ---- 5. state-dict keys ----------------------------------------------------------------------------------------------------------------
def test_state_dict_keys_do_not_change_with_vectors():
    from egopack_amd.criterion import CrossEntropyNone, MetricSelectorWrapper
    from egopack_amd.models.tasks.lta import LTATask
    from egopack_amd.models.tasks.recognition import RecognitionTask

    class DS:
        has_joint_label, num_labels = False, 2

    w, a = [torch.rand(5) + 0.5, torch.rand(7) + 0.5], [torch.randn(5), None]
    for cls in (RecognitionTask, LTATask):
        plain, bal = cls(16, 16, heads=(5, 7)), cls(16, 16, heads=(5, 7))
        bal.set_class_balance(w, a)
        assert list(plain.state_dict()) == list(bal.state_dict())
        plain.load_state_dict(bal.state_dict())  # strict
        bal.load_state_dict(plain.state_dict())
        assert torch.equal(bal.class_weight_1, w[1]) and bal.class_offset_1 is None
        assert bal.class_balance()[0][0] is bal.class_weight_0 and bal.class_balance()[1] == (bal.class_offset_0, None)
        bal.set_class_balance(None, None)
        assert bal.class_balance() == (None, None)
        with pytest.raises(ValueError, match="head 1"):
            bal.set_class_balance([torch.ones(5), torch.ones(6)], None)
        with pytest.raises(ValueError, match="2 heads"):
            bal.set_class_balance([torch.ones(5)], None)
    wr = MetricSelectorWrapper(CrossEntropyNone(), DS(), class_weights=w, class_offsets=a)
    assert list(wr.state_dict()) == list(MetricSelectorWrapper(CrossEntropyNone(), DS()).state_dict()) == []
    assert len(list(wr.buffers())) == 3
    ws, offs = wr.select_balance((None, None))
    assert ws[0] is wr.class_weight_0 and ws[1] is wr.class_weight_1 and offs == (wr.class_offset_0, None)
    assert wr.eval().select_balance((None, None)) == (None, None)   # eval(): the plain cross entropy
    ce = CrossEntropyNone(weight=w[0], offset=a[0])
    assert list(ce.state_dict()) == [] and torch.equal(ce.weight, w[0]) and ce.weight.dtype == torch.float32


def test_wrapper_picks_the_vectors_of_the_selected_heads():
    from egopack_amd.criterion import CrossEntropyNone, MetricSelectorWrapper

    class Joint:
        has_joint_label, num_labels = True, 3

    w = [torch.ones(4), 2 * torch.ones(6), 3 * torch.ones(24)]
    logits = (torch.zeros(2, 4), torch.zeros(2, 6), torch.zeros(2, 24))
    sep = MetricSelectorWrapper(CrossEntropyNone(), Joint(), class_weights=w)
    ws, offs = sep.select_balance(logits)
    assert offs is None and len(ws) == 2 and ws[0] is sep.class_weight_0 and ws[1] is sep.class_weight_1
    joint = MetricSelectorWrapper(CrossEntropyNone(), Joint(), joint_label_training=True, class_weights=w)
    ws, offs = joint.select_balance(logits)
    assert offs is None and len(ws) == 1 and ws[0] is joint.class_weight_2
    assert len(joint.select(logits, torch.zeros(2, 3, dtype=torch.int64))) == 3  # select() keeps its three-tuple
