"""The per-class validation report without a GPU: what include/egopack_class_report.h pins beyond the one ledger (tests/test_cabi.py),
the host-side refusals of its entry point, the host model's ranking, the derived metrics on hand-made matrices, the
``class_report:`` config block, and the keys of every meter with the report off."""
import ctypes

import numpy as np
import pytest
import torch

from tests import class_report_common as CR

# ---- 1. include/egopack_class_report.h beyond the common ledger ------------------------------------------------------------------
# (names, exports, bound types, the bounds ledger and the struct fields of this header: the one ledger, tests/test_cabi.py)


def test_class_report_task_struct_layout_matches_header():
    from egopack_amd import _lib
    from tests import cabi_common as CC
    text = _lib.HEADERS["class_report"].read_text()
    names = [n for n, _ in CC.struct_fields("class_report", "egk_class_report_task")]
    assert names == ["logits", "ld", "labels", "label_stride", "rows", "C", "confusion", "top2", "loss_q24", "counts"]
    T = _lib.ClassReportTask
    assert ctypes.sizeof(T) == 72 and T.rows.offset == 32 and T.C.offset == 36 and T.confusion.offset == 40 and T.counts.offset == 64
    assert f"#define EGK_CLASS_REPORT_MAX_TASKS {_lib.CLASS_REPORT_MAX_TASKS}" in text and _lib.CLASS_REPORT_MAX_TASKS == 8


def test_class_report_has_a_profile_id_of_its_own():
    from egopack_amd import _lib
    lib = _lib.load()
    name = ctypes.create_string_buffer(64)
    n, ms, fl, by = ctypes.c_int64(), ctypes.c_double(), ctypes.c_double(), ctypes.c_double()
    names = []
    for i in range(lib.egk_prof_count()):
        assert lib.egk_prof_get(i, name, 64, ctypes.byref(n), ctypes.byref(ms), ctypes.byref(fl), ctypes.byref(by)) == 0
        names.append(name.value.decode())
    assert {"class_report", "categorical_sample"} <= set(names) and len(set(names)) == len(names)


# ---- 2. host-side refusals (small fake non-null pointers: every check precedes the first dereference and the first launch) ---------
def _tasks(n=1, **kw):
    from egopack_amd import _lib
    arr = (_lib.ClassReportTask * n)()
    for t in arr:
        t.logits, t.ld, t.labels, t.label_stride, t.rows, t.C = 0x1000, 8, 0x2000, 2, 4, 7
        t.confusion, t.top2, t.loss_q24, t.counts = 0x3000, 0x4000, 0x5000, 0x6000
        for k, v in kw.items():
            setattr(t, k, v)
    return arr


def test_class_report_refuses_bad_arguments_before_any_launch():
    from egopack_amd import _lib
    lib = _lib.load()

    def call(tasks, count=1):
        return lib.egk_class_report(None, tasks, count)

    def refused(rc, needle):
        assert rc == -1 and needle in _lib.last_error() and "egk_class_report" in _lib.last_error(), (rc, _lib.last_error())

    refused(call(None), "null task list")
    for name in ("logits", "labels", "confusion", "counts"):
        refused(call(_tasks(**{name: None})), "null pointer")
    for count in (0, -1, 9):
        refused(call(_tasks(8), count=count), "1 .. 8 tasks")
    refused(call(_tasks(C=0)), "class count")
    refused(call(_tasks(C=-3)), "class count")
    refused(call(_tasks(ld=6)), "leading dimension")
    refused(call(_tasks(rows=-1)), "rows >= 0")
    for name in ("confusion", "top2", "loss_q24", "counts", "labels"):
        refused(call(_tasks(**{name: 0x7004})), "misaligned pointer")
    refused(call(_tasks(logits=0x1002)), "misaligned pointer")
    bad_second = _tasks(2)
    bad_second[1].C = 0
    refused(call(bad_second, count=2), "task 1")
    # without rows nothing is launched (and no pointer is followed); the optional pointers may be null; the limits pass
    assert call(_tasks(8, rows=0), count=8) == 0
    assert call(_tasks(rows=0, top2=None, loss_q24=None, ld=7, C=7)) == 0
    # ... and the refusals hold without rows too
    refused(call(_tasks(rows=0, C=0)), "class count")
    refused(call(_tasks(rows=0, confusion=0x3004)), "misaligned pointer")
    refused(call(_tasks(rows=0, counts=None)), "null pointer")


# ---- 3. the host model's ranking -----------------------------------------------------------------------------------------------------
def test_host_model_ranking_and_fixed_point():
    nan, inf = float("nan"), float("inf")
    x = np.array([[1.0, 3.0, 3.0, 2.0],      # a tie for the first place: the lower index wins, the other is second
                  [nan, nan, nan, nan],      # all NaN: classes 0 and 1
                  [nan, -inf, 0.5, nan],     # NaN below -inf
                  [0.0, -0.0, -1.0, -2.0],   # the two zeros tie
                  [-inf, inf, nan, 7.0]], dtype=np.float32)
    o = CR.order(x)
    assert o[:, :2].tolist() == [[1, 2], [0, 1], [2, 1], [0, 1], [1, 3]]
    assert o[2].tolist() == [2, 1, 0, 3]
    y = np.array([2, 1, 1, 1, -1])
    loss = np.array([0.5, nan, inf, 1.0 / 3.0, 0.0], dtype=np.float32)
    conf, top2, q24, counts = CR.model(x, y, loss)
    assert counts.tolist() == [4, 1, 2, 0]
    assert conf[2, 1] == 1 and conf[1, 0] == 2 and conf[1, 2] == 1 and conf.sum() == 4
    assert top2[2, 1] == 1 and top2[1, 0] == 2 and top2[1, 2] == 1 and top2.sum() == 4
    assert q24.tolist() == [0, int(np.rint(np.float64(np.float32(1.0 / 3.0)) * 2 ** 24)), 1 << 23, 0]
    q, ok = CR.loss_q(np.array([2.0 ** 38, 2.0 ** 39, -2.0 ** 39, -1.5], dtype=np.float32))
    assert ok.tolist() == [True, False, False, True] and q[0] == 1 << 62 and q[3] == -(3 << 23)
    c1 = CR.model(np.zeros((3, 1), np.float32), np.array([0, 0, 1]), np.zeros(3, np.float32))
    assert c1[0].tolist() == [[2]] and c1[1].tolist() == [[0]] and c1[3].tolist() == [2, 1, 0, 0]


# ---- 4. the derived metrics on hand-made matrices ------------------------------------------------------------------------------------
def test_derived_metrics_of_a_hand_made_matrix():
    from egopack_amd.meters import report_metrics
    #                 predicted: a  b  c  d
    conf = torch.tensor([[3, 1, 0, 0],    # a: support 4, 3 right
                         [0, 0, 0, 0],    # b: support 0 (predicted once)
                         [2, 0, 2, 0],    # c: support 4, 2 right
                         [1, 0, 1, 0]])   # d: support 2, never predicted
    top2 = torch.tensor([[0, 1, 0, 0], [0, 0, 0, 0], [2, 0, 0, 0], [1, 0, 1, 0]])
    q24 = torch.tensor([1 << 24, 0, 3 << 24, 5 << 23])
    m = report_metrics(conf, top2, q24, names=list("abcd"), train_counts=torch.tensor([101, 100, 20, 19]), shots=(20, 100),
                       top_confusions=3)
    assert m["class_recall"].tolist() == [0.75, 0.0, 0.5, 0.0]
    assert m["class_precision"].tolist() == [0.5, 0.0, 2 / 3, 0.0]  # (d is never predicted: precision 0)
    f1a, f1c = 2 * 0.5 * 0.75 / 1.25, 2 * (2 / 3) * 0.5 / (2 / 3 + 0.5)
    assert m["class_f1"].tolist() == pytest.approx([f1a, 0.0, f1c, 0.0], abs=1e-15)
    # the macro figures: over a, c, d (support > 0), not b
    assert m["macro_recall"] == pytest.approx((0.75 + 0.5 + 0.0) / 3, abs=1e-15)
    assert m["macro_precision"] == pytest.approx((0.5 + 2 / 3 + 0.0) / 3, abs=1e-15)
    assert m["macro_f1"] == pytest.approx((f1a + f1c) / 3, abs=1e-15)
    cl = m["class_loss"]
    assert cl.dtype == torch.float64 and cl[[0, 2, 3]].tolist() == [0.25, 0.75, 1.25] and bool(torch.isnan(cl[1]))
    # buckets: 101 > hi -> many; exactly hi = 100 and exactly lo = 20 -> medium; 19 < lo -> few
    assert (m["classes_many"], m["classes_medium"], m["classes_few"]) == (1, 2, 1)
    assert (m["samples_many"], m["samples_medium"], m["samples_few"]) == (4, 4, 2)
    assert (m["acc_many"], m["acc_medium"], m["acc_few"]) == (0.75, 0.5, 0.0)
    # the largest cells of the top-2 matrix, ties by the lower flat index: (c, a) 2, then (a, b), (d, a) -- (d, c) is cut off
    assert m["top_confusions"] == [("c", "a", 2), ("a", "b", 1), ("d", "a", 1)]
    assert report_metrics(conf, top2, q24, names=list("abcd"), top_confusions=20)["top_confusions"][3:] == [("d", "c", 1)]
    assert torch.equal(m["confusion"], conf) and torch.equal(m["top2_confusion"], top2)
    # without training counts: no bucket key
    m0 = report_metrics(conf, top2, q24)
    assert not [k for k in m0 if k.startswith(("acc_", "classes_", "samples_"))] and m0["top_confusions"][0] == ("2", "0", 2)
    # nothing seen: zeros, no division by zero
    z = report_metrics(torch.zeros(3, 3, dtype=torch.int64), torch.zeros(3, 3, dtype=torch.int64), torch.zeros(3, dtype=torch.int64),
                       train_counts=torch.tensor([0, 50, 500]))
    assert (z["macro_f1"], z["macro_recall"], z["acc_many"], z["acc_few"], z["top_confusions"]) == (0.0, 0.0, 0.0, 0.0, [])


# ---- 5. the configuration ------------------------------------------------------------------------------------------------------------
def test_class_report_config_accepts_and_rejects_as_documented():
    from egopack_amd import train as T
    cfg = T.load_config([])
    assert dict(cfg.class_report) == {"shots": [20, 100], "top_confusions": 20, "save": True} and cfg.log_confusion_matrices is False
    assert T.class_report_config(cfg) == {"shots": (20, 100), "top_confusions": 20, "save": True, "enabled": False}
    assert T.class_report_meter_args(cfg, None, "ar") == {} and T.class_report_train_counts(cfg, {}) == {}
    cfg = T.load_config(["log_confusion_matrices=true", "class_report.shots=[5,50]", "class_report.top_confusions=3",
                         "class_report.save=false"])
    assert T.class_report_config(cfg) == {"shots": (5, 50), "top_confusions": 3, "save": False, "enabled": True}
    assert T.class_report_meter_args(cfg, {"ar": ["v", "n"]}, "ar") == dict(class_report=True, train_counts=["v", "n"], shots=(5, 50),
                                                                             top_confusions=3)
    assert T.class_report_meter_args(cfg, {}, "pnr") == {}  # (PNR takes no report)
    assert T.class_report_config({})["shots"] == (20, 100)  # (a config without the block: the defaults)
    with pytest.raises(ValueError) as e:
        T.class_report_config(T.load_config(["+class_report.plot=true"]))
    assert "plot" in str(e.value) and "shots" in str(e.value) and "top_confusions" in str(e.value)
    for bad in ("[100,20]", "[20,20]", "[20]", "[1,2,3]", "[-1,5]", "[1.5,9]"):
        with pytest.raises(ValueError, match="class_report.shots"):
            T.class_report_config(T.load_config([f"class_report.shots={bad}"]))
    with pytest.raises(ValueError, match="class_report.top_confusions"):
        T.class_report_config(T.load_config(["class_report.top_confusions=-1"]))


# ---- 6. with the report off every meter has the keys it had --------------------------------------------------------------------------
class _DS:
    label_names = ["verbs", "nouns"]
    class_labels = [[f"verb_{i}" for i in range(5)], [f"noun_{i}" for i in range(7)]]


_VN = ("verbs", "nouns")
KEYS = {
    "RecognitionMeter": {f"{h}_{k}" for h in _VN for k in ("top1", "top2", "top3", "top5", "mc", "class_acc", "calibration_erorr",
                                                           "brier_score")} | {"loss"},
    "AnticipationMeter": {f"{h}_{m}_top{k}" for h in _VN for m in ("accuracy", "recall") for k in (1, 2, 3, 5)} | {"loss"},
    "LTAMeter": {"verbs_ed", "nouns_ed", "verbs_top1", "nouns_top1", "loss"},
    "OSCCMeter": {"accuracy", "loss"},
    "PNRMeter": {"accuracy", "recall", "auroc", "localization_error", "loss"},
}
REPORT = ("macro_precision", "macro_recall", "macro_f1", "confusion", "top2_confusion", "class_loss", "class_precision", "class_recall",
          "class_f1", "top_confusions")
BUCKETS = tuple(f"{k}_{b}" for k in ("acc", "classes", "samples") for b in ("many", "medium", "few"))


@pytest.mark.parametrize("name", sorted(KEYS))
def test_meter_keys_with_the_report_off_and_on(name):
    from egopack_amd import meters as M
    cls = getattr(M, name)
    off = cls(_DS(), device="cpu")
    assert set(off.get_logs()) == KEYS[name] and off.reports == {} and len(off.print_logs()) >= 1
    if name == "PNRMeter":
        return
    assert set(cls(_DS(), device="cpu", class_report=False).get_logs()) == KEYS[name]
    assert len(off._sums()) + (4 if name == "OSCCMeter" else 8) == len(cls(_DS(), device="cpu", class_report=True)._sums())
    prefixes = ("",) if name == "OSCCMeter" else ("verbs_", "nouns_")
    on = cls(_DS(), device="cpu", class_report=True)
    assert set(on.get_logs()) == KEYS[name] | {p + k for p in prefixes for k in REPORT}
    tc = [torch.tensor([0, 50])] if name == "OSCCMeter" else [torch.arange(5) * 40, torch.arange(7) * 30]
    on = cls(_DS(), device="cpu", class_report=True, train_counts=tc)
    logs = on.get_logs()
    assert set(logs) == KEYS[name] | {p + k for p in prefixes for k in REPORT + BUCKETS}
    state = [t for st, _, _ in on.reports.values() for t in st.tensors()]
    assert len(state) == 4 * len(prefixes) and all(t.dtype == torch.int64 for t in state)
    assert all(any(t is s for s in on._sums()) for t in state)  # (merge and all_reduce see them: no new code there)
    assert len(on.print_logs()) == len(off.print_logs()) + len(prefixes)
    tables = on.report_tables()
    assert all(not isinstance(v, (int, float)) for v in tables.values()) and {p + "class_names" for p in prefixes} <= set(tables)


def test_build_meter_for_dataset_passes_the_report_through():
    from egopack_amd import meters as M

    class DS(_DS):
        task = "ar"
    m = M.build_meter_for_dataset(DS(), device="cpu")
    assert not m.class_report and m.reports == {}
    m = M.build_meter_for_dataset(DS(), device="cpu", class_report=True, train_counts=[torch.zeros(5), torch.zeros(7)], shots=(3, 9),
                                  top_confusions=4)
    assert m.class_report and set(m.reports) == {"verbs_", "nouns_"} and m.shots == (3, 9) and m.top_confusions == 4
    DS.task = "pnr"
    assert M.build_meter_for_dataset(DS(), device="cpu", class_report=True).reports == {}
