"""Action-level scores without a GPU: the host model (tests/action_common.py) against a float64 brute force, the candidate
statement of include/egopack_action.h on tie-heavy grids, every host-side refusal of the two entry points, their profile ids, the
``action_scores:`` config block, the integer arithmetic of ``meters._ActionCounts`` and the meters' keys with the block off."""
import ctypes

import numpy as np
import pytest
import torch

from egopack_amd import _lib
from tests import action_common as AC
from tests.class_report_common import order

vp = ctypes.c_void_p


# ---- 1. the model -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Cv,Cn,k", [(1, 1, 1), (3, 5, 4), (5, 7, 35), (8, 11, 32)])
def test_the_model_is_the_float64_order_on_tie_free_inputs(Cv, Cn, k):
    """Inputs whose float64 pair scores are at least 1e-3 apart: f32 rounding (errors of a few 1e-7) cannot reorder them, so the
    model's pairs and ranks are those of the float64 sort and its logp is the float64 score to f32 accuracy."""
    g = AC.gen(17 * Cv + Cn)
    rows = []
    while len(rows) < 6:  # (rejection: keep the rows whose scores are well separated)
        zv, zn = torch.randn(1, Cv, generator=g).numpy() * 2, torch.randn(1, Cn, generator=g).numpy() * 2
        s = (zv[0][:, None].astype(np.float64) + zn[0][None, :].astype(np.float64)).reshape(-1)
        if Cv * Cn == 1 or np.diff(np.sort(s)).min() >= 1e-3:
            rows.append((zv, zn))
    zv, zn = np.concatenate([r[0] for r in rows]), np.concatenate([r[1] for r in rows])
    y = AC.pair_labels(len(rows), Cv, Cn, g)
    pair, logp, rank, _ = AC.model(zv, zn, AC.lse32(zv, zn), k, labels=(y[:, 0].numpy(), y[:, 2].numpy()))
    lv = zv.astype(np.float64) - np.log(np.exp(zv.astype(np.float64)).sum(1, keepdims=True))
    ln = zn.astype(np.float64) - np.log(np.exp(zn.astype(np.float64)).sum(1, keepdims=True))
    for r in range(len(rows)):
        s64 = (lv[r][:, None] + ln[r][None, :]).reshape(-1)
        o = np.argsort(-s64, kind="stable")
        m = min(k, Cv * Cn)
        assert pair[r, :m, 0].tolist() == (o[:m] // Cn).tolist() and pair[r, :m, 1].tolist() == (o[:m] % Cn).tolist()
        assert (pair[r, m:] == -1).all() and np.isneginf(logp[r, m:]).all()
        np.testing.assert_allclose(logp[r, :m], s64[o[:m]], rtol=1e-5, atol=1e-6)
        yv, yn = int(y[r, 0]), int(y[r, 2])
        want = int(np.nonzero(o == yv * Cn + yn)[0][0]) if 0 <= yv < Cv and 0 <= yn < Cn else -1
        assert rank[r] == want
    assert abs(np.exp(AC.model(zv, zn, AC.lse32(zv, zn), Cv * Cn)[1].astype(np.float64)).sum(1) - 1).max() < 1e-5  # (a distribution)


@pytest.mark.parametrize("beta", [None, (0.5, 2.0), (1.0, 1.0), (0.3, 1.7)])
def test_every_best_pair_lies_in_the_best_verbs_times_the_best_nouns(beta):
    """The candidate statement on tie-heavy grids (multiples of 0.25 in [-1.5, 1.5], Cv <= 8, Cn <= 11), for every k at once: the
    pair at place j of the FULL order has a verb among its head's best j + 1 and a noun among its head's best j + 1.  Also with
    -inf columns, a NaN row and rows of equal values."""
    g = AC.gen(5)
    checked = 0
    for trial in range(400):
        Cv, Cn = int(torch.randint(1, 9, (1,), generator=g)), int(torch.randint(1, 12, (1,), generator=g))
        zv, zn = AC.grid(4, Cv, g).numpy(), AC.grid(4, Cn, g).numpy()
        if trial % 7 == 0:
            zv[1, Cv - 1] = -np.inf
            zn[2, 0] = -np.inf
        if trial % 11 == 0:
            zv[3, 0] = np.nan
        if trial % 13 == 0:
            zv[0], zn[0] = 0.25, -0.5
        s, pv, pn = AC.table(zv, zn, AC.lse32(zv, zn, beta), beta)
        for r in range(4):
            o = AC.pair_order(s[r], pv[r], pn[r])
            place = np.arange(o.size)
            assert (pv[r][o // Cn] <= place).all() and (pn[r][o % Cn] <= place).all(), (trial, r, zv[r], zn[r])
            checked += 1
    assert checked == 1600


def test_levenshtein_known_answers():
    assert AC.levenshtein([], []) == 0 and AC.levenshtein([1, 2, 3], []) == 3 and AC.levenshtein("kitten", "sitting") == 3
    assert AC.levenshtein([(1, 1), (2, 2)], [(1, 1), (2, 3)]) == 1  # (verb right, noun wrong: the action token differs)
    pv, pn, lv, ln = (t.numpy() for t in AC.futures(4, 9, 3, AC.gen(2)))
    d = AC.edit_model(pv, pn, lv, ln)
    assert (d[0, 0] == 0).all() and (d[..., 2] >= d[..., :2].max(-1)).all() and (d[..., 2] <= 9).all()


# ---- 2. the host-side refusals ---------------------------------------------------------------------------------------------------------
def test_every_argument_error_is_refused_on_the_host_naming_the_entry_point():
    """Small fake non-null pointers are safe: every check precedes the first dereference and the first launch."""
    lib = _lib.load()
    A, U4, U2 = vp(0x1000), vp(0x1004), vp(0x1002)
    F32, BF16 = 0, 1

    def refused(rc, *needles):
        err = _lib.last_error()
        assert rc == -1 and all(n in err for n in needles), (rc, err)

    def topk(verb=A, ld_v=8, Cv=8, noun=A, ld_n=16, Cn=16, beta=None, yv=A, yn=A, rows=4, k=5, pair=A, pstride=10, logp=A, prob=A,
             ostride=5, lse=A, rank=A, dt=F32):
        return lib.egk_action_topk(None, verb, ld_v, Cv, noun, ld_n, Cn, beta, yv, 1, yn, 1, rows, k, pair, pstride, logp, prob, ostride,
                                   lse, rank, dt)
    for kw, arg in ((dict(verb=None), "verb_logits"), (dict(noun=None), "noun_logits"), (dict(pair=None), "pair")):
        refused(topk(**kw), "egk_action_topk", "null pointer", arg)
    refused(topk(yv=None), "egk_action_topk", "both NULL or both given")
    refused(topk(yn=None), "egk_action_topk", "both NULL or both given")
    refused(topk(yv=None, yn=None), "egk_action_topk", "rank requires the labels")
    refused(topk(rank=None), "egk_action_topk", "labels are given for rank")
    refused(topk(rows=-1), "egk_action_topk", "rows")
    refused(topk(k=0), "egk_action_topk", "k in 1 .. 32")
    refused(topk(k=33, pstride=66, ostride=33), "egk_action_topk", "k in 1 .. 32")
    refused(topk(Cv=0), "egk_action_topk", "Cv in 1 .. 1024")
    refused(topk(Cv=1025, ld_v=1025), "egk_action_topk", "Cv in 1 .. 1024")
    refused(topk(Cn=0), "egk_action_topk", "Cn in 1 .. 1024")
    refused(topk(Cn=1025, ld_n=1025), "egk_action_topk", "Cn in 1 .. 1024")
    refused(topk(ld_v=7), "egk_action_topk", "ld_v >= Cv")
    refused(topk(ld_n=15), "egk_action_topk", "ld_n >= Cn")
    refused(topk(pstride=9), "egk_action_topk", "pair row stride")
    refused(topk(ostride=4), "egk_action_topk", "logp / prob row stride")
    refused(topk(dt=2), "egk_action_topk", "dtype")
    refused(topk(verb=U2), "egk_action_topk", "misaligned logits")
    refused(topk(pair=U4), "egk_action_topk", "misaligned pair")
    refused(topk(yn=U4), "egk_action_topk", "misaligned labels")
    for arg in ("beta", "logp", "prob", "lse", "rank"):
        refused(topk(**{arg: U2}), "egk_action_topk", "misaligned", arg)
    assert topk(rows=0) == 0 and topk(verb=U2, noun=U2, dt=BF16, rows=0) == 0  # (no rows: nothing is launched)
    assert topk(rows=0, logp=None, prob=None, ostride=0, lse=None, yv=None, yn=None, rank=None) == 0  # (every optional argument absent)

    def ed(pv=A, pn=A, lv=A, ln=A, out=A, N=3, Z=20, K=5):
        return lib.egk_edit_distance_pairs(None, pv, pn, 100, 5, 1, lv, ln, 20, 1, out, N, Z, K)
    for arg, name in (("pv", "pred_v"), ("pn", "pred_n"), ("lv", "label_v"), ("ln", "label_n"), ("out", "out")):
        refused(ed(**{arg: None}), "egk_edit_distance_pairs", "null pointer", name)
    refused(ed(N=-1), "egk_edit_distance_pairs", "N >= 0")
    refused(ed(K=-1), "egk_edit_distance_pairs", "K >= 0")
    refused(ed(Z=65), "egk_edit_distance_pairs", "sequence length 65")
    refused(ed(Z=-1), "egk_edit_distance_pairs", "sequence length -1")
    refused(ed(N=1 << 30, K=4), "egk_edit_distance_pairs", "N * K")
    refused(ed(pv=U4), "egk_edit_distance_pairs", "misaligned pred or label")
    refused(ed(ln=U4), "egk_edit_distance_pairs", "misaligned pred or label")
    refused(ed(out=U2), "egk_edit_distance_pairs", "misaligned out")
    assert ed(N=0) == 0 and ed(K=0) == 0  # (nothing is launched)


def test_the_launches_have_their_profile_ids():
    lib = _lib.load()
    names = []
    for i in range(lib.egk_prof_count()):
        name = ctypes.create_string_buffer(64)
        n, ms, fl, by = ctypes.c_int64(), ctypes.c_double(), ctypes.c_double(), ctypes.c_double()
        assert lib.egk_prof_get(i, name, 64, ctypes.byref(n), ctypes.byref(ms), ctypes.byref(fl), ctypes.byref(by)) == 0
        names.append(name.value.decode())
    assert "action_topk" in names and "edit_distance_pairs" in names and len(set(names)) == len(names)
    assert _lib.ACTION_MAX_K == 32 and _lib.ACTION_MAX_C == 1024
    text = _lib.ADDON_HEADERS["action"].read_text()
    assert "#define EGK_ACTION_MAX_K 32" in text and "#define EGK_ACTION_MAX_C 1024" in text


# ---- 3. the configuration ---------------------------------------------------------------------------------------------------------------
def test_action_scores_config_accepts_and_rejects_as_documented():
    from egopack_amd import train as T
    cfg = T.load_config([])
    assert dict(cfg.action_scores) == {"enabled": False, "tasks": ["ar", "lta"], "topk": 5, "calibrated": "auto",
                                       "seen_split": False} == T.ACTION_SCORES_DEFAULTS
    assert T.action_scores_config({}) == T.ACTION_SCORES_DEFAULTS  # (a config without the block: the defaults, off)
    assert T.action_scores_meter_args(cfg, "ar") == {} and T.action_scores_meter_args({}, "lta") == {}
    assert T.action_scores_seen(cfg, {}) == {} and T.action_scores_betas(cfg, ".", "ar") == (None, None)
    cfg = T.load_config(["action_scores.enabled=true", "action_scores.tasks=[ar]", "action_scores.topk=32", "action_scores.calibrated=True"])
    ac = T.action_scores_config(cfg)
    assert ac["enabled"] and ac["tasks"] == ["ar"] and ac["topk"] == 32 and ac["calibrated"] == "true"
    assert T.action_scores_meter_args(cfg, "ar") == {"action_scores": {"topk": 32}}
    assert T.action_scores_meter_args(cfg, "lta") == {} and T.action_scores_meter_args(cfg, "oscc") == {}
    seen = {"ar": torch.tensor([3, 9])}
    on = T.load_config(["action_scores.enabled=true", "action_scores.seen_split=true"])
    assert T.action_scores_meter_args(on, "ar", seen)["action_scores"]["seen"] is seen["ar"]
    assert "seen" not in T.action_scores_meter_args(on, "lta", seen)["action_scores"]
    for bad, needle in ((["+action_scores.k=5"], "k"), (["action_scores.topk=0"], "topk"), (["action_scores.topk=33"], "topk"),
                        (["action_scores.topk=2.5"], "topk"), (["action_scores.topk=true"], "topk"), (["action_scores.calibrated=maybe"], "maybe"),
                        (["action_scores.tasks=[ar,oscc]"], "oscc")):
        with pytest.raises(ValueError) as e:
            T.action_scores_config(T.load_config(bad))
        assert needle in str(e.value), (bad, str(e.value))
    # the predict block is as it was: the export's k lives in action_scores
    from egopack_amd import predict as P
    assert set(P.PREDICT_DEFAULTS) == {"split", "topk", "out", "json"}


def test_calibrated_decides_the_betas(tmp_path):
    from egopack_amd import predict as P
    from egopack_amd import train as T
    blob = {"task": "ar", "heads": {"verbs_": {"temperature": 2.0}, "nouns_": {"temperature": 0.5}}}
    auto = T.load_config(["action_scores.enabled=true"])
    assert T.action_scores_betas(auto, tmp_path, "ar") == (None, None)  # (auto: no file is loaded -> the raw logits)
    assert T.action_scores_betas(auto, tmp_path, "ar", calibration=blob) == (blob, [0.5, 2.0])
    assert T.action_scores_betas(T.load_config(["action_scores.enabled=true", "action_scores.calibrated=false"]), tmp_path, "ar",
                                 calibration=blob) == (None, None)
    must = T.load_config(["action_scores.enabled=true", "action_scores.calibrated=true"])
    with pytest.raises(FileNotFoundError, match="action_scores.calibrated=true"):
        T.action_scores_betas(must, tmp_path, "ar")
    torch.save(blob, T.calibration_path(tmp_path, "ar"))
    assert T.action_scores_betas(must, tmp_path, "ar")[1] == [0.5, 2.0]
    action, doc = P.action_export(must, tmp_path, "ar")
    assert action == {"topk": 5, "betas": [0.5, 2.0]} and doc == {"action_topk_k": 5, "action_betas": {"verb": 0.5, "noun": 2.0}}
    assert P.action_export(must, tmp_path, "oscc") == (None, {}) and P.action_export(T.load_config([]), tmp_path, "ar") == (None, {})
    assert P.action_export(auto, tmp_path, "lta") == ({"topk": 5, "betas": None}, {"action_topk_k": 5, "action_betas": None})


def test_the_training_split_pairs_are_sorted_distinct_codes():
    from egopack_amd import train as T

    class Sample:
        def __init__(self, y):
            self.y = torch.tensor(y)

    class DS:
        label_names, num_class_labels = ["verbs", "nouns"], (3, 4)
        samples = [Sample([[2, 3], [0, 1]]), Sample([[0, 1], [-1, 2], [1, 4]]), Sample([[1, 0]])]

        def __len__(self):
            return len(self.samples)

        def __getitem__(self, i):
            return self.samples[i]

    assert T.action_pair_codes(DS()).tolist() == [1, 4, 11]  # (0, 1) twice, (1, 0), (2, 3); (-1, 2) and (1, 4) are no pairs
    on = T.load_config(["action_scores.enabled=true", "action_scores.seen_split=true", "action_scores.tasks=[ar]"])
    assert {t: v.tolist() for t, v in T.action_scores_seen(on, {"ar": DS(), "lta": DS()}).items()} == {"ar": [1, 4, 11]}


# ---- 4. the meters ------------------------------------------------------------------------------------------------------------------------
def test_action_counts_arithmetic_and_merge_on_hand_made_ranks():
    from egopack_amd import meters as M
    rank = torch.tensor([0, 4, -1, 2, 5, 1, 0, -1], dtype=torch.int32)
    yv = torch.tensor([0, 1, -1, 2, 0, 1, 2, 5])
    yn = torch.tensor([1, 0, 3, 3, 0, 1, 2, 0])
    seen = torch.tensor([1, 4, 11])  # codes v * 4 + n: (0, 1), (1, 0), (2, 3)
    whole = M._ActionCounts(3, 4, "cpu", seen=seen)
    whole.count(rank, yv, yn)
    assert whole.hits.tolist() == [2, 3, 4, 5] and int(whole.valid) == 6  # ranks 0 0 | 1 | 2 | 4 of six rows; rank 5 misses top-5
    assert [whole.accuracy(k) for k in M.KS] == [2 / 6, 3 / 6, 4 / 6, 5 / 6]
    # seen rows: (0,1) r0 hit, (1,0) r4, (2,3) r2 -> 1 of 3; unseen rows: (0,0) r5, (1,1) r1, (2,2) r0 hit -> 1 of 3
    assert whole.split.tolist() == [1, 3, 1, 3]
    assert whole.split_logs() == {"actions_seen_top1": 1 / 3, "actions_seen_support": 3, "actions_unseen_top1": 1 / 3, "actions_unseen_support": 3}
    a, b = M._ActionCounts(3, 4, "cpu", seen=seen), M._ActionCounts(3, 4, "cpu", seen=seen)
    a.count(rank[:3], yv[:3], yn[:3])
    b.count(rank[3:], yv[3:], yn[3:])
    for x, y in zip(a.tensors(), b.tensors()):
        x += y
    assert all(torch.equal(x, y) and x.dtype == torch.int64 for x, y in zip(a.tensors(), whole.tensors()))  # (integers: bit for bit)
    off = M._ActionCounts(3, 4, "cpu")
    off.count(rank, yv, yn)
    assert off.split_logs() == {} and off.split.tolist() == [0, 0, 0, 0] and off.hits.tolist() == whole.hits.tolist()
    empty = M._ActionCounts(3, 4, "cpu", seen=torch.zeros(0, dtype=torch.int64))
    empty.count(rank, yv, yn)
    assert empty.split.tolist() == [0, 0, 2, 6] and empty.accuracy(1) == 2 / 6
    assert M._ActionCounts(3, 4, "cpu").accuracy(1) == 0.0  # (no rows)


TODAY = {  # the scalar and table keys of get_logs() before this feature (class report and calibration off)
    "ar": {"loss"} | {f"{h}_{s}" for h in ("verbs", "nouns") for s in ("top1", "top2", "top3", "top5", "mc", "class_acc", "calibration_erorr", "brier_score")},
    "anticipation": {"loss"} | {f"{h}_{m}_top{k}" for h in ("verbs", "nouns") for m in ("accuracy", "recall") for k in (1, 2, 3, 5)},
    "lta": {"loss", "verbs_ed", "nouns_ed", "verbs_top1", "nouns_top1"},
    "oscc": {"loss", "accuracy"},
}


def test_the_logs_have_todays_keys_with_the_block_off_and_the_new_ones_with_it_on():
    from egopack_amd import meters as M

    class DS:
        label_names = ["verbs", "nouns"]
        class_labels = [[f"v{i}" for i in range(5)], [f"n{i}" for i in range(7)]]

    for task, keys in TODAY.items():
        DS.task = task
        m = M.build_meter_for_dataset(DS(), device="cpu")
        assert set(m.get_logs()) == keys, (task, sorted(set(m.get_logs()) ^ keys))
        assert getattr(m, "actions", None) is None and m.action_cfg is None
        assert not any("ction" in line for line in m.print_logs())
        before = len(m._sums())
        if task == "oscc":
            continue
        on = M.build_meter_for_dataset(DS(), device="cpu", action_scores={"topk": 5})
        new = {"actions_top1", "actions_ed"} if task == "lta" else {f"actions_top{k}" for k in (1, 2, 3, 5)}
        assert set(on.get_logs()) == keys | new, (task, sorted(set(on.get_logs()) ^ (keys | new)))
        assert len(on._sums()) == before + (4 if task == "lta" else 3) and any(line.startswith("Actions") for line in on.print_logs())
        split = M.build_meter_for_dataset(DS(), device="cpu", action_scores={"topk": 5, "seen": torch.tensor([0, 8])})
        assert set(split.get_logs()) == keys | new | {"actions_seen_top1", "actions_seen_support", "actions_unseen_top1", "actions_unseen_support"}
    DS.task = "pnr"
    assert not hasattr(M.build_meter_for_dataset(DS(), device="cpu", action_scores={"topk": 5}), "actions")  # (PNR has no pair)
