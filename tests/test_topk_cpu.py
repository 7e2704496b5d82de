"""The top-k softmax launch and the prediction entry point without a GPU: what include/egopack_topk.h pins beyond the one ledger
(tests/test_cabi.py), the host-side refusals of its entry point, the ``predict:`` config block, the refusals of ``predict.main`` and
the host model's order on tie and NaN rows."""
import ctypes

import numpy as np
import pytest

from tests import class_report_common as CR
from tests import topk_common as TK

# ---- 1. include/egopack_topk.h beyond the common ledger --------------------------------------------------------------------------
# (names, exports, bound types, the bounds ledger and the struct fields of this header: the one ledger, tests/test_cabi.py)


def test_topk_task_struct_layout_matches_header():
    from egopack_amd import _lib
    from tests import cabi_common as CC
    text = _lib.HEADERS["topk"].read_text()
    names = [n for n, _ in CC.struct_fields("topk", "egk_topk_task")]
    assert names == ["logits", "ld", "C", "reserved", "idx", "idx_row_stride", "prob", "prob_row_stride", "lse"]
    T = _lib.TopkTask
    assert ctypes.sizeof(T) == 64 and T.C.offset == 16 and T.reserved.offset == 20 and T.idx.offset == 24 and T.lse.offset == 56
    assert f"#define EGK_TOPK_MAX_TASKS {_lib.TOPK_MAX_TASKS}" in text and _lib.TOPK_MAX_TASKS == 8
    assert f"#define EGK_TOPK_MAX_K {_lib.TOPK_MAX_K}" in text and _lib.TOPK_MAX_K == 64


def test_topk_softmax_has_a_profile_id_of_its_own():
    from egopack_amd import _lib
    lib = _lib.load()
    name = ctypes.create_string_buffer(64)
    n, ms, fl, by = ctypes.c_int64(), ctypes.c_double(), ctypes.c_double(), ctypes.c_double()
    names = []
    for i in range(lib.egk_prof_count()):
        assert lib.egk_prof_get(i, name, 64, ctypes.byref(n), ctypes.byref(ms), ctypes.byref(fl), ctypes.byref(by)) == 0
        names.append(name.value.decode())
    assert {"topk_softmax", "class_report", "categorical_sample"} <= set(names) and len(set(names)) == len(names)


# ---- 2. host-side refusals (small fake non-null pointers: every check precedes the first dereference and the first launch) ---------
def _tasks(n=1, **kw):
    from egopack_amd import _lib
    arr = (_lib.TopkTask * n)()
    for t in arr:
        t.logits, t.ld, t.C, t.reserved = 0x1000, 8, 7, 0
        t.idx, t.idx_row_stride, t.prob, t.prob_row_stride, t.lse = 0x2000, 5, 0x3000, 6, 0x4000
        for k, v in kw.items():
            setattr(t, k, v)
    return arr


def test_topk_softmax_refuses_bad_arguments_before_any_launch():
    from egopack_amd import _lib
    lib = _lib.load()
    F32, BF16 = 0, 1

    def call(tasks, count=1, rows=4, k=5, dtype=F32):
        return lib.egk_topk_softmax(None, tasks, count, rows, k, dtype)

    def refused(rc, needle):
        assert rc == -1 and needle in _lib.last_error() and "egk_topk_softmax" in _lib.last_error(), (rc, _lib.last_error())

    refused(call(None), "null task list")
    for count in (0, -1, 9):
        refused(call(_tasks(8), count=count), "1 .. 8 tasks")
    refused(call(_tasks(), rows=-1), "rows >= 0")
    for k in (0, -1, 65):
        refused(call(_tasks(idx_row_stride=100, prob_row_stride=100), k=k), "k in 1 .. 64")
    for dtype in (2, -1, 7):
        refused(call(_tasks(), dtype=dtype), "unknown logits dtype")
    for name in ("logits", "idx"):
        refused(call(_tasks(**{name: None})), "null pointer")
    refused(call(_tasks(C=0)), "class count")
    refused(call(_tasks(C=-3)), "class count")
    refused(call(_tasks(ld=6)), "leading dimension")
    refused(call(_tasks(idx_row_stride=4)), "idx row stride")
    refused(call(_tasks(idx_row_stride=-5)), "idx row stride")
    refused(call(_tasks(prob_row_stride=4)), "prob row stride")
    refused(call(_tasks(prob_row_stride=-6)), "prob row stride")
    refused(call(_tasks(logits=0x1002)), "misaligned pointer")
    refused(call(_tasks(logits=0x1001), dtype=BF16), "misaligned pointer")
    refused(call(_tasks(idx=0x2004)), "misaligned pointer")
    refused(call(_tasks(prob=0x3002)), "misaligned pointer")
    refused(call(_tasks(lse=0x4002)), "misaligned pointer")
    refused(call(_tasks(reserved=1)), "reserved")
    bad_second = _tasks(2)
    bad_second[1].C = 0
    refused(call(bad_second, count=2), "task 1")
    # without rows nothing is launched (and no pointer is followed); the optional pointers may be null; the limits pass
    assert call(_tasks(8), count=8, rows=0) == 0
    assert call(_tasks(prob=None, lse=None, prob_row_stride=0, ld=7, idx_row_stride=64), rows=0, k=64) == 0
    assert call(_tasks(logits=0x1002), rows=0, dtype=BF16) == 0  # (bf16 logits: aligned to two bytes)
    # ... and the refusals hold without rows too
    refused(call(_tasks(C=0), rows=0), "class count")
    refused(call(_tasks(idx=0x2004), rows=0), "misaligned pointer")
    refused(call(_tasks(idx=None), rows=0), "null pointer")
    refused(call(_tasks(idx_row_stride=4), rows=0), "idx row stride")


# ---- 3. the configuration and the entry point's refusals -------------------------------------------------------------------------------
def test_predict_config_block_parses_with_its_defaults():
    from egopack_amd import predict as P
    from egopack_amd import train as T
    cfg = T.load_config([])
    assert dict(cfg.predict) == {"split": "validation", "topk": 5, "out": None, "json": True}
    assert P.predict_config(cfg) == {"split": "validation", "topk": 5, "out": None, "json": True}
    assert P.predict_config(T.load_config(["validation_split=test"]))["split"] == "test"  # (split: ${validation_split})
    cfg = T.load_config(["predict.split=train", "predict.topk=64", "predict.out=/tmp/x", "predict.json=false"])
    assert P.predict_config(cfg) == {"split": "train", "topk": 64, "out": "/tmp/x", "json": False}
    assert P.predict_config({}) == {"split": "validation", "topk": 5, "out": None, "json": True}  # (a config without the block)
    for bad in ("0", "65", "-1", "2.5", "true"):
        with pytest.raises(ValueError, match="predict.topk"):
            P.predict_config(T.load_config([f"predict.topk={bad}"]))
    with pytest.raises(ValueError) as e:
        P.predict_config(T.load_config(["+predict.format=csv"]))
    assert "format" in str(e.value) and "topk" in str(e.value)


def test_predict_main_refuses_what_it_cannot_export(monkeypatch):
    import predict  # (the entry point at the repository's root)
    from egopack_amd import predict as P
    assert predict.main is P.main
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    with pytest.raises(ValueError, match="resume_from"):
        P.main([])
    with pytest.raises(ValueError, match="enable_graphone"):
        P.main(["resume_from=/nowhere/checkpoint.pth", "enable_graphone=True"])
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(ValueError, match="one process"):
        P.main(["resume_from=/nowhere/checkpoint.pth"])


# ---- 4. the host model's order ---------------------------------------------------------------------------------------------------------
def test_host_model_agrees_with_the_report_order_on_tie_and_nan_rows():
    nan, inf = float("nan"), float("inf")
    x = np.array([[1.0, 3.0, 3.0, 2.0],      # a tie for the first place: the lower index wins, the other is second
                  [nan, nan, nan, nan],      # all NaN: by index
                  [nan, -inf, 0.5, nan],     # NaN below -inf
                  [0.0, -0.0, -1.0, -2.0],   # the two zeros tie
                  [-inf, inf, nan, 7.0]], dtype=np.float32)
    for k in (1, 2, 3, 4, 6):
        idx, p, lse = TK.model(x, k)
        assert idx.shape == (5, k) and np.array_equal(idx[:, :min(k, 2)], CR.order(x)[:, :min(k, 2)])
        assert np.array_equal(idx[:, :min(k, 4)], CR.order(x)[:, :k]) and (idx[:, 4:] == -1).all() and (p[:, 4:] == 0).all()
    idx, p, lse = TK.model(x, 4)
    assert idx.tolist() == [[1, 2, 3, 0], [0, 1, 2, 3], [2, 1, 0, 3], [0, 1, 2, 3], [1, 3, 0, 2]]
    assert np.isnan(p[[1, 2, 4]]).all() and np.isnan(lse[[1, 2, 4]]).all()
    assert p[0].sum() == pytest.approx(1.0, abs=1e-15) and p[0, 0] == p[0, 1] and lse[0] == pytest.approx(np.log(np.exp(x[0].astype(np.float64)).sum()))
    g = CR.gen(3)
    for C in (1, 2, 7, 65):
        s = TK.special_rows(C, g).numpy()
        idx, p, _ = TK.model(s, 5)
        assert np.array_equal(idx[:, :min(C, 2)], CR.order(s)[:, :min(C, 2)]) and (idx[:, C:] == -1).all()
        finite = ~np.isnan(s).any(axis=1)
        assert (p[finite][s[finite][np.arange(finite.sum())[:, None], np.maximum(idx[finite], 0)] == -inf] == 0).all()
    assert TK.model(np.zeros((0, 7), np.float32), 3)[0].shape == (0, 3)
