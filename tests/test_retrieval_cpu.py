"""The retrieval report and the EgoPack prediction entry point without a GPU: what include/egopack_retrieval.h pins beyond the one
ledger (tests/test_cabi.py), the host-side refusals of its entry point, known answers of the host model (tests/retrieval_common.py),
``graphone.bank_labels`` against the reference's recipe, the ``predict_egopack:`` config block and the refusals of
``predict_egopack.main``."""
import ctypes

import numpy as np
import pytest
import torch

from tests import retrieval_common as RC

# ---- 1. include/egopack_retrieval.h beyond the common ledger ---------------------------------------------------------------------
# (names, exports, bound types, the bounds ledger and the struct fields of this header: the one ledger, tests/test_cabi.py)


def test_retrieval_task_struct_layout_matches_header():
    from egopack_amd import _lib
    from tests import cabi_common as CC
    text = _lib.HEADERS["retrieval"].read_text()
    names = [n for n, _ in CC.struct_fields("retrieval", "egk_retrieval_task")]
    assert names == ["f", "f_ld", "f_act", "f_act_ld", "bank", "bank_ld", "K", "reserved", "nn", "nn_row_stride", "dist",
                     "dist_row_stride", "wins", "wins_row_stride"]
    T = _lib.RetrievalTask
    assert ctypes.sizeof(T) == 104 and T.K.offset == 48 and T.reserved.offset == 52 and T.nn.offset == 56 and T.wins.offset == 88
    assert f"#define EGK_RETRIEVAL_MAX_TASKS {_lib.RETRIEVAL_MAX_TASKS}" in text and _lib.RETRIEVAL_MAX_TASKS == 8
    assert f"#define EGK_RETRIEVAL_MAX_K {_lib.RETRIEVAL_MAX_K}" in text and _lib.RETRIEVAL_MAX_K == 32


def test_retrieval_report_has_a_profile_id_of_its_own():
    from egopack_amd import _lib
    lib = _lib.load()
    name = ctypes.create_string_buffer(64)
    n, ms, fl, by = ctypes.c_int64(), ctypes.c_double(), ctypes.c_double(), ctypes.c_double()
    names = []
    for i in range(lib.egk_prof_count()):
        assert lib.egk_prof_get(i, name, 64, ctypes.byref(n), ctypes.byref(ms), ctypes.byref(fl), ctypes.byref(by)) == 0
        names.append(name.value.decode())
    assert {"retrieval_report", "topk_softmax", "gather_max_fwd"} <= set(names) and len(set(names)) == len(names)


# ---- 2. host-side refusals (small fake non-null pointers: every check precedes the first dereference and the first launch) ---------
H, K_NN = 64, 4


def _tasks(n=1, **kw):
    from egopack_amd import _lib
    arr = (_lib.RetrievalTask * n)()
    for t in arr:
        t.f, t.f_ld, t.f_act, t.f_act_ld, t.bank, t.bank_ld, t.K, t.reserved = 0x1000, H, 0x2000, H, 0x3000, H, 37, 0
        t.nn, t.nn_row_stride, t.dist, t.dist_row_stride, t.wins, t.wins_row_stride = 0x4000, K_NN, 0x5000, K_NN, 0x6000, K_NN + 1
        for k, v in kw.items():
            setattr(t, k, v)
    return arr


def test_retrieval_report_refuses_bad_arguments_before_any_launch():
    from egopack_amd import _lib
    lib = _lib.load()
    F32, BF16 = 0, 1

    def call(tasks, count=1, rows=4, Hn=H, k=K_NN, distance=0, dtype=F32):
        return lib.egk_retrieval_report(None, tasks, count, rows, Hn, k, distance, dtype)

    def refused(rc, needle):
        assert rc == -1 and needle in _lib.last_error() and "egk_retrieval_report" in _lib.last_error(), (rc, _lib.last_error())

    refused(call(None), "null task list")
    for count in (0, -1, 9):
        refused(call(_tasks(8), count=count), "1 .. 8 tasks")
    refused(call(_tasks(), rows=-1), "rows >= 0")
    for Hn in (0, -4):
        refused(call(_tasks(), Hn=Hn), "H >= 1")
    for k in (0, -1, 33):
        refused(call(_tasks(nn_row_stride=100, dist_row_stride=100, wins_row_stride=100), k=k), "k in 1 .. 32")
    for distance in (2, -1):
        refused(call(_tasks(), distance=distance), "unknown distance")
    for dtype in (2, -1, 7):
        refused(call(_tasks(), dtype=dtype), "unknown f_act dtype")
    for name in ("f", "f_act", "bank", "nn"):
        refused(call(_tasks(**{name: None})), "null pointer")
    for Kb in (0, -3):
        refused(call(_tasks(K=Kb)), "bank rows")
    refused(call(_tasks(reserved=1)), "reserved")
    for name in ("f_ld", "f_act_ld", "bank_ld"):
        refused(call(_tasks(**{name: H - 1})), "leading dimension")
        refused(call(_tasks(**{name: -H})), "leading dimension")
    refused(call(_tasks(nn_row_stride=K_NN - 1)), "nn row stride")
    refused(call(_tasks(nn_row_stride=-K_NN)), "nn row stride")
    refused(call(_tasks(dist_row_stride=K_NN - 1)), "dist row stride")
    refused(call(_tasks(dist_row_stride=-K_NN)), "dist row stride")
    refused(call(_tasks(wins_row_stride=K_NN)), "wins row stride")
    refused(call(_tasks(wins_row_stride=-K_NN - 1)), "wins row stride")
    refused(call(_tasks(dist=None, wins=None)), "both null")
    refused(call(_tasks(f=0x1002)), "misaligned pointer")
    refused(call(_tasks(bank=0x3002)), "misaligned pointer")
    refused(call(_tasks(f_act=0x2002)), "misaligned pointer")
    refused(call(_tasks(f_act=0x2001), dtype=BF16), "misaligned pointer")
    refused(call(_tasks(nn=0x4004)), "misaligned pointer")
    refused(call(_tasks(dist=0x5002)), "misaligned pointer")
    refused(call(_tasks(wins=0x6002)), "misaligned pointer")
    bad_second = _tasks(2)
    bad_second[1].K = 0
    refused(call(bad_second, count=2), "task 1")
    # without rows nothing is launched (and no pointer is followed); either output may be absent; the limits pass
    assert call(_tasks(8), count=8, rows=0) == 0
    assert call(_tasks(dist=None, dist_row_stride=0, nn_row_stride=32, wins_row_stride=33), rows=0, k=32) == 0
    assert call(_tasks(wins=None, wins_row_stride=0), rows=0, distance=1) == 0
    assert call(_tasks(f_act=0x2002, f=0x1004, bank=0x3004), rows=0, dtype=BF16) == 0  # (to the element, not to a vector)
    assert call(_tasks(f_ld=1, f_act_ld=1, bank_ld=1, K=1, nn_row_stride=1, dist_row_stride=1, wins_row_stride=2), rows=0, Hn=1, k=1) == 0
    # ... and the refusals hold without rows too
    refused(call(_tasks(K=0), rows=0), "bank rows")
    refused(call(_tasks(nn=None), rows=0), "null pointer")
    refused(call(_tasks(wins_row_stride=K_NN), rows=0), "wins row stride")
    refused(call(_tasks(dist=None, wins=None), rows=0), "both null")


def test_the_wrapper_refuses_what_the_launch_cannot_take():
    from egopack_amd import ops
    f, bank = torch.zeros(3, 8), torch.zeros(40, 8)
    with pytest.raises(ValueError, match="k in 1 .. 32"):
        ops.retrieval_report([f], [f], [bank], [torch.zeros(3, 33, dtype=torch.int64)])
    with pytest.raises(ValueError, match="1 .. 8 tasks"):
        ops.retrieval_report([f] * 9, [f] * 9, [bank] * 9, [torch.zeros(3, 4, dtype=torch.int64)] * 9)
    with pytest.raises(ValueError, match="1 .. 8 tasks"):
        ops.retrieval_report([], [], [], [])
    with pytest.raises(ValueError, match="Unknown distance"):
        ops.retrieval_report([f], [f], [bank], [torch.zeros(3, 4, dtype=torch.int64)], distance_func="l1")
    with pytest.raises(ValueError, match="nothing to report"):
        ops.retrieval_report([f], [f], [bank], [torch.zeros(3, 4, dtype=torch.int64)], want_dist=False, want_wins=False)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.retrieval_report([f], [f], [bank], [torch.zeros(3, 4, dtype=torch.int64)])


# ---- 3. known answers of the host model ----------------------------------------------------------------------------------------------
def test_host_model_known_answers():
    nan, inf = float("nan"), float("inf")
    bank = np.array([[1.0, 5.0, nan, 0.0, -inf, 2.0],
                     [1.0, 7.0, nan, 0.0, -inf, 2.0],
                     [3.0, 7.0, nan, -1.0, -inf, 2.0]], dtype=np.float32)
    f = np.array([[3.0, 7.5, nan, 0.0, -inf, 1.0],     # ties with a prototype: the prototype keeps the channel
                  [9.0, 9.0, nan, 9.0, 9.0, 9.0]], dtype=np.float32)
    nn = np.array([[0, 1, 2], [2, 1, 0]])
    w = RC.wins_model(f, bank, nn)
    # row 0, sources (p0, p1, p2, self): ch0 1,1,3,3 -> p2 (self ties: not strictly larger); ch1 5,7,7,7.5 -> self; ch2 all NaN ->
    # source 0; ch3 0,0,-1,0 -> p0 (the tie between two prototypes goes to the earlier one); ch4 all -inf -> source 0; ch5 2,2,2,1 -> p0
    assert w[0].tolist() == [4, 0, 1, 1]
    # row 1, sources (p2, p1, p0, self): the node is strictly larger everywhere but in the NaN channel
    assert w[1].tolist() == [1, 0, 0, 5]
    assert w.dtype == np.int32 and (w.sum(1) == 6).all()
    # k = 1
    w1 = RC.wins_model(f, bank, nn[:, :1])
    assert w1.shape == (2, 2) and w1[0].tolist() == [4, 2] and w1[1].tolist() == [1, 5]
    # the rows sum to H on random inputs with ties, whatever k is
    g = torch.Generator().manual_seed(2)
    for k in (1, 4, 32):
        fa, b = RC.grid(9, 50, g).numpy(), RC.grid(40, 50, g).numpy()
        w = RC.wins_model(fa, b, RC.lists(9, 40, k, g).numpy())
        assert w.shape == (9, k + 1) and (w.sum(1) == 50).all() and (w >= 0).all()
    # distances: the formulas
    f = np.array([[3.0, 4.0], [0.0, 0.0]], dtype=np.float32)
    bank = np.array([[3.0, 4.0], [4.0, -3.0], [-6.0, -8.0]], dtype=np.float32)
    nn = np.array([[0, 1, 2], [0, 1, 2]])
    with np.errstate(all="ignore"):
        c, l = RC.dist_model(f, bank, nn, "cosine"), RC.dist_model(f, bank, nn, "l2")
    assert c[0].tolist() == pytest.approx([0.0, 1.0, 2.0], abs=1e-15) and np.isnan(c[1]).all()  # a zero row: the reference's 0 / 0
    assert l[0].tolist() == pytest.approx([0.0, 50 ** 0.5 / 4096, 15 / 4096]) and l[1].tolist() == pytest.approx([5 / 4096, 5 / 4096, 10 / 4096])
    assert RC.dist_bound(1024) == 32 * 2.0 ** -24 and RC.dist_bound(8) == 16.125 * 2.0 ** -24


# ---- 4. bank_labels -----------------------------------------------------------------------------------------------------------------
def test_bank_labels_are_the_rows_finalise_banks_keeps():
    """The reference's recipe (graphone.py: ``bincount(all_labels) > 0`` over ``verb * |N| + noun`` of the rows with
    ``y[:, 0] != -1``) over the batches the loader yields: 10 samples in batches of 4 with drop_last leave the last two samples out."""
    import graphone as root
    from egopack_amd import train as T
    from egopack_amd.data import build_dataloader
    from egopack_amd.graphone import bank_labels
    assert root.bank_labels is bank_labels
    ds = T.build_datasets(T.load_config(["synthetic_samples=10", "k=1"]), "train")["ar"]
    V, N = ds.num_class_labels
    dl = build_dataloader(ds, 4, False, 0, True, 1, rank=0, world_size=1, shard="batches")
    got = bank_labels(dl, (V, N))
    ys = torch.cat([ds[i].y for i in range(8)])          # (the two batches that survive drop_last)
    everything = torch.cat([ds[i].y for i in range(10)])
    assert int((ys[:, 0] == -1).sum()) > 0, "the split has ignored rows"
    keep = ys[ys[:, 0] != -1]
    want = torch.nonzero(torch.bincount(keep[:, 0] * N + keep[:, 1], minlength=V * N) > 0).reshape(-1)
    assert got.dtype == torch.int64 and got.dim() == 1 and torch.equal(got, want)
    assert bool((got[1:] > got[:-1]).all()) and got.numel() < V * N  # ascending, with gaps
    kept_all = everything[everything[:, 0] != -1]
    assert got.numel() < torch.unique(kept_all[:, 0] * N + kept_all[:, 1]).numel(), "the dropped batch must hold labels of its own"
    # hand-made batches: a label twice, an ignored row whose noun is set, the last class
    from types import SimpleNamespace as NS
    batches = [NS(y=torch.tensor([[1, 2], [-1, 5], [0, 0]])), NS(y=torch.tensor([[1, 2], [2, 3]], dtype=torch.int32)), NS(y=torch.zeros(0, 2, dtype=torch.int64))]
    assert bank_labels(batches, (3, 4)).tolist() == [0, 6, 11]
    assert bank_labels([], (3, 4)).tolist() == []


# ---- 5. the configuration and the entry point's refusals -------------------------------------------------------------------------------
def test_predict_egopack_config_block_parses_with_its_defaults():
    from egopack_amd import predict as P
    from egopack_amd import predict_egopack as PE
    from egopack_amd import train as T
    cfg = T.load_config([])
    assert dict(cfg.predict_egopack) == {"retrieval": True, "labels": True}
    assert PE.predict_egopack_config(cfg) == {"retrieval": True, "labels": True} == PE.PREDICT_EGOPACK_DEFAULTS
    assert PE.predict_egopack_config({}) == {"retrieval": True, "labels": True}  # (a config without the block)
    cfg = T.load_config(["predict_egopack.retrieval=false", "predict_egopack.labels=false"])
    assert PE.predict_egopack_config(cfg) == {"retrieval": False, "labels": False}
    with pytest.raises(ValueError) as e:
        PE.predict_egopack_config(T.load_config(["+predict_egopack.format=csv"]))
    assert "format" in str(e.value) and "retrieval" in str(e.value) and "labels" in str(e.value)
    # the predict: block keeps exactly its four keys
    assert dict(T.load_config([]).predict) == {"split": "validation", "topk": 5, "out": None, "json": True} == P.PREDICT_DEFAULTS
    import main_egopack
    assert PE.AUX_ORDER == main_egopack.AUX_ORDER


def test_predict_egopack_main_refuses_what_it_cannot_export(monkeypatch, tmp_path):
    import predict_egopack  # (the entry point at the repository's root)
    from egopack_amd import predict as P
    from egopack_amd import predict_egopack as PE
    assert predict_egopack.main is PE.main
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    plain = tmp_path / "mtl.pth"
    torch.save({"temporal_graph": {}, "epoch": 1}, plain)
    empty = tmp_path / "empty.pth"
    torch.save({"temporal_graph": {}, "epoch": 1, "graphone": {"conv_stages.ar.0.module_1.weight": torch.zeros(2)}}, empty)
    with pytest.raises(ValueError, match="resume_from"):
        PE.main(["enable_graphone=True"])
    with pytest.raises(ValueError, match="enable_graphone"):
        PE.main([f"resume_from={plain}"])
    with pytest.raises(ValueError, match="enable_graphone"):
        PE.main([f"resume_from={plain}", "enable_graphone=False"])
    with pytest.raises(ValueError, match="'graphone' entry"):   # (read on the host, before any dataset or device is touched)
        PE.main([f"resume_from={plain}", "enable_graphone=True"])
    with pytest.raises(ValueError, match="no prototype bank"):
        PE.main([f"resume_from={empty}", "enable_graphone=True"])
    with pytest.raises(ValueError, match="format"):
        PE.main([f"resume_from={plain}", "enable_graphone=True", "+predict_egopack.format=csv"])
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(ValueError, match="one process"):
        PE.main([f"resume_from={plain}", "enable_graphone=True"])
    monkeypatch.delenv("WORLD_SIZE")
    # predict.py still refuses the GraphONE, and now says where to go
    with pytest.raises(ValueError, match="enable_graphone") as e:
        P.main([f"resume_from={plain}", "enable_graphone=True"])
    assert "predict_egopack.py" in str(e.value)
    assert PE.inspect_checkpoint.__doc__ and PE.main.__doc__


def test_to_json_carries_the_retrieval_only_where_a_file_has_it():
    from egopack_amd import predict as P
    pred = {"sample": torch.tensor([0, 1]), "pred": torch.tensor([1, 0]), "prob_change": torch.tensor([0.75, 0.25])}
    assert P.to_json("oscc", pred, None) == {"0": {"state_change": True, "prob": 0.75}, "1": {"state_change": False, "prob": 0.25}}
    pred.update(retrieval_sample=torch.tensor([0, 0, 1]), retrieval_pos=torch.tensor([4, 5, 9]),
                retrieval_ar_index=torch.tensor([[3, 1], [2, 0], [1, 3]]), retrieval_ar_dist=torch.tensor([[0.25, 0.5], [0.0, 1.0], [0.5, 0.75]]),
                retrieval_ar_wins=torch.tensor([[1, 2, 5], [8, 0, 0], [0, 0, 8]], dtype=torch.int32))
    doc = P.to_json("oscc", pred, None)
    assert doc["0"]["state_change"] is True and doc["0"]["retrieval"] == {
        "pos": [4, 5], "ar": {"index": [[3, 1], [2, 0]], "dist": [[0.25, 0.5], [0.0, 1.0]], "wins": [[1, 2, 5], [8, 0, 0]]}}
    assert doc["1"]["retrieval"] == {"pos": [9], "ar": {"index": [[1, 3]], "dist": [[0.5, 0.75]], "wins": [[0, 0, 8]]}}
    pred["retrieval_ar_label"] = torch.tensor([[[0, 3], [0, 1]], [[0, 2], [0, 0]], [[0, 1], [0, 3]]])
    assert P.to_json("oscc", pred, None)["1"]["retrieval"]["ar"]["label"] == [[[0, 1], [0, 3]]]
