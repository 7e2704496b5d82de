"""The cluster bootstrap without a GPU: the threshold table, the statistics of the host model of
tests/bootstrap_common.py (the weights are Poisson(1); the standard error is the one of the CLUSTERS, not of the rows), the interval
rule, the config block, the C-side refusals of include/egopack_bootstrap.h with fake pointers (every check precedes the first
dereference and the first launch) and ``compare_runs`` on model files."""
import ctypes
import math

import numpy as np
import pytest
import torch

from egopack_amd import _lib, compare, meters, ops, train
from tests import bootstrap_common as BC


# ---- the table and the weights --------------------------------------------------------------------------------------------------------
def test_the_threshold_table_is_the_poisson_distribution_function_in_60_digit_decimals():
    assert BC.table(12, 60) == BC.T and len(BC.T) == 12
    assert BC.table(13, 60)[12] == (1 << 32) - 1  # (T[12] would be 2^32 - 1: left out, the weight stops at 12)
    header = _lib.ADDON_HEADERS["bootstrap"].read_text()
    flat = " ".join(header.replace("*", " ").split())
    assert ", ".join(str(t) for t in BC.T) in flat, "the header quotes the table"
    for name, value in (("EGK_BOOT_MAX_R", _lib.BOOT_MAX_R), ("EGK_BOOT_MAX_M", _lib.BOOT_MAX_M), ("EGK_BOOT_MAX_C", _lib.BOOT_MAX_C)):
        assert f"#define {name} {value}" in header
    assert (_lib.BOOT_MAX_R, _lib.BOOT_MAX_M, _lib.BOOT_MAX_C) == (BC.MAX_R, BC.MAX_M, BC.MAX_C)


def test_the_key_is_the_seed_under_a_salt_of_its_own():
    assert ops.BOOTSTRAP_KEY_SALT == BC.KEY_SALT and ops.BOOTSTRAP_KEY_SALT.to_bytes(8, "big") == b"BOOT_CLU"
    assert len({ops.BOOTSTRAP_KEY_SALT, ops.SAMPLER_KEY_SALT, ops.OPTIM_STATE_KEY_SALT, 0}) == 4
    for seed in (0, 1, 12345, (1 << 64) - 1):
        assert ops.bootstrap_key(seed) == BC.key(seed) == (seed ^ BC.KEY_SALT) & ((1 << 64) - 1)
    assert ops.BOOTSTRAP_MAX_CLUSTER == BC.MAX_CLUSTER


def test_model_weights_are_poisson_1():
    """2^20 draws (clusters 0 .. 2^18 - 1, replicates 0 .. 3, key of seed 0): every frequency of w = 0 .. 4 within 5 binomial standard
    deviations of e^-1 / w!, the mean within 5 / sqrt(2^20) of 1 (the variance of Poisson(1) is 1).  Deterministic."""
    w = BC.weights(np.arange(1 << 18), 4, ops.bootstrap_key(0))
    n = w.size
    assert n == 1 << 20 and int(w.max()) <= 12
    for k in range(5):
        p = math.exp(-1) / math.factorial(k)
        f = float((w == k).mean())
        assert abs(f - p) <= 5 * math.sqrt(p * (1 - p) / n), (k, f, p)
    assert abs(float(w.mean()) - 1.0) <= 5 / math.sqrt(n)


def test_a_weight_is_a_function_of_key_cluster_and_replicate_alone():
    k = BC.key(3)
    c = np.array([0, 5, 5, -1, BC.MAX_CLUSTER, 17, -9])
    w = BC.weights(c, 9, k)
    assert np.array_equal(w[1], w[2]) and not w[3].any() and not w[6].any()
    assert np.array_equal(BC.weights(c[::-1].copy(), 9, k), w[::-1])  # (not of the row)
    assert np.array_equal(BC.weights(c, 5, k), w[:, :5])  # (not of R)
    assert not np.array_equal(BC.weights(c, 9, BC.key(4)), w)
    for row, r in ((0, 0), (4, 7), (5, 8)):  # the scalar transcription of the header's rule
        ctr = (int(c[row]) << 14) | (r >> 2)
        word = BC.PR.philox_u64_scalar(ctr, k)[r & 3]
        assert int(w[row, r]) == sum(word >= t for t in BC.T)


# ---- the standard error is the clusters' ----------------------------------------------------------------------------------------------
def _se(cluster, hit, R=2000):
    acc = BC.accumulate(BC.empty(R, 1), cluster, hit[:, None], np.ones((len(hit), 1), dtype=np.int64), BC.key(0))
    return BC.interval(BC.ratio_values(acc["acc_num"][:, 0], acc["acc_den"][:, 0]), 0.95, R)


def test_independent_rows_give_the_binomial_standard_error():
    hit = (np.random.default_rng(11).random(400) < 0.3).astype(np.int64)
    p = hit.mean()
    ci = _se(np.arange(400), hit)
    want = math.sqrt(p * (1 - p) / 400)
    assert abs(ci["se"] - want) <= 0.10 * want, (ci["se"], want)  # (the bootstrap's own error of an se at R = 2000: 1 / sqrt(2 R) = 1.6 %)
    assert ci["lo"] <= p <= ci["hi"]


def test_clustered_rows_give_the_standard_error_of_the_clusters_not_of_the_rows():
    hit = (np.random.default_rng(11).random(400) < 0.3).astype(np.int64)
    p = hit.mean()
    ci = _se(np.repeat(np.arange(400), 8), np.repeat(hit, 8))  # 3200 rows, 8 per cluster
    want = math.sqrt(p * (1 - p) / 400)
    assert abs(ci["se"] - want) <= 0.10 * want, (ci["se"], want, math.sqrt(p * (1 - p) / 3200))
    assert ci == _se(np.arange(400), hit)  # (8 w n / 8 w d: the very same quotients)


# ---- the interval rule ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fn", [BC.interval, lambda v, level, R: meters.bootstrap_interval(torch.as_tensor(v), level, R)], ids=["model", "meters"])
def test_interval_rule(fn):
    v = np.random.default_rng(5).permutation(1000).astype(np.float64)
    ci = fn(v, 0.95, 1000)
    assert (ci["lo"], ci["hi"], ci["valid"], ci["dropped"]) == (25.0, 974.0, 1000, 0)
    assert ci["se"] == float(np.std(np.arange(1000.0), ddof=1))
    ci = fn(np.concatenate([v[:600], np.full(400, np.nan)]), 0.9, 1000)  # zero-denominator replicates are dropped and counted
    s = np.sort(v[:600])
    assert (ci["lo"], ci["hi"], ci["valid"], ci["dropped"]) == (s[30], s[569], 600, 400)
    assert fn(np.concatenate([v[:499], np.full(501, np.nan)]), 0.95, 1000) is None  # fewer than R / 2 valid: no interval
    assert fn(np.concatenate([v[:500], np.full(500, np.nan)]), 0.95, 1000) is not None
    assert fn(np.full(10, np.nan), 0.95, 10) is None
    one = fn(np.array([3.0]), 0.95, 1)
    assert (one["lo"], one["hi"], one["se"]) == (3.0, 3.0, 0.0)


def test_replicate_values_of_the_meters_are_the_models():
    g = np.random.default_rng(2)
    num, den = g.integers(0, 50, (64, 3)), g.integers(0, 3, (64, 3)) * g.integers(1, 50, (64, 3))
    for m in range(3):
        got = meters.bootstrap_ratio(torch.from_numpy(num[:, m]), torch.from_numpy(den[:, m])).numpy()
        assert np.array_equal(got, BC.ratio_values(num[:, m], den[:, m]), equal_nan=True) and np.isnan(got).sum() == (den[:, m] == 0).sum()
    cd = g.integers(0, 4, (64, 9)) * g.integers(0, 2, (64, 1))
    cn = np.minimum(g.integers(0, 4, (64, 9)), cd)
    got, want = meters.bootstrap_mean_class(torch.from_numpy(cn), torch.from_numpy(cd)).numpy(), BC.mean_class_values(cn, cd)
    assert np.array_equal(np.isnan(got), np.isnan(want)) and np.isnan(want).any()
    np.testing.assert_allclose(got[~np.isnan(got)], want[~np.isnan(want)], rtol=1e-12, atol=0)


# ---- the config block and the meters ------------------------------------------------------------------------------------------------------
def test_the_config_block_refuses_what_it_does_not_know_by_name():
    cfg = train.load_config([])
    assert train.bootstrap_config(cfg) == {"replicates": 0, "level": 0.95, "seed": 0, "save": True} == train.BOOTSTRAP_DEFAULTS
    assert train.bootstrap_meter_args(cfg, "ar") == {}
    on = train.load_config(["bootstrap.replicates=1000", "bootstrap.seed=7", "bootstrap.level=0.9"])
    assert train.bootstrap_meter_args(on, "pnr") == {"bootstrap": {"replicates": 1000, "level": 0.9, "seed": 7}}
    for args, needle in ((["+bootstrap.replicas=5"], "bootstrap: unknown key(s) ['replicas']"), (["bootstrap.replicates=-1"], "bootstrap.replicates"),
                         (["bootstrap.replicates=65537"], "bootstrap.replicates"), (["bootstrap.replicates=1.5"], "bootstrap.replicates"),
                         (["bootstrap.level=1.0"], "bootstrap.level"), (["bootstrap.level=0"], "bootstrap.level"),
                         (["bootstrap.seed=abc"], "bootstrap.seed")):
        with pytest.raises(ValueError) as e:
            train.bootstrap_config(train.load_config(args))
        assert needle in str(e.value), (args, str(e.value))


class _DS:
    task = "ar"
    label_names = ["verbs", "nouns"]
    class_labels = [[f"v{i}" for i in range(7)], [f"n{i}" for i in range(11)]]


def test_replicates_0_builds_the_meters_without_the_helper():
    for kind in ("ar", "anticipation", "lta", "oscc", "pnr"):
        ds = type("DS", (_DS,), {"task": kind})()
        plain = meters.build_meter_for_dataset(ds, device="cpu")
        off = meters.build_meter_for_dataset(ds, device="cpu", bootstrap={"replicates": 0, "level": 0.95, "seed": 3})
        assert plain.boot is None and off.boot is None
        assert [tuple(t.shape) for t in off._sums()] == [tuple(t.shape) for t in plain._sums()]
        assert off.get_logs().keys() == plain.get_logs().keys() and off.bootstrap_tables() == {}
        on = meters.build_meter_for_dataset(ds, device="cpu", bootstrap={"replicates": 12, "level": 0.95, "seed": 3})
        assert on.boot is not None and on.boot.R == 12 and on.boot.key == BC.key(3)
        assert len(on._sums()) > len(plain._sums()) and all(t.dtype == torch.int64 for t in on.boot.tensors())
    ar = meters.build_meter_for_dataset(_DS(), device="cpu", bootstrap={"replicates": 12}, action_scores={"topk": 5})
    assert {n: (g.keys, g.class_key) for n, g in ar.boot.groups.items()} == {
        "verbs": ([None, "verbs_top1", "verbs_top2", "verbs_top3", "verbs_top5"], "verbs_mc"),
        "nouns": ([None, "nouns_top1", "nouns_top2", "nouns_top3", "nouns_top5"], "nouns_mc"),
        "actions": ([None, "actions_top1", "actions_top2", "actions_top3", "actions_top5"], None)}
    assert ar.boot.groups["nouns"].cls_den.shape == (12, 11) and ar.boot.groups["actions"].cls_den is None
    with pytest.raises(ValueError, match="bootstrap.replicates"):
        meters.build_meter_for_dataset(_DS(), device="cpu", bootstrap={"replicates": 65537})


def test_ops_refuse_a_cluster_bound_beyond_40_bits_on_the_host():
    c = torch.zeros(4, dtype=torch.int64)
    with pytest.raises(ValueError, match="40 bits"):
        ops.bootstrap_weights(c, 4, 0, max_cluster=1 << 40)
    with pytest.raises(ValueError, match="40 bits"):
        ops.bootstrap_accumulate(c, c[:, None], c[:, None], torch.zeros(4, 1, dtype=torch.int64), torch.zeros(4, 1, dtype=torch.int64), 0,
                                 max_cluster=1 << 40)


# ---- the C side refuses what it can see -------------------------------------------------------------------------------------------------
def test_the_entry_points_refuse_bad_arguments_before_any_launch():
    lib = _lib.load()
    vp = ctypes.c_void_p
    A, U4 = 0x1000, 0x1004
    base = dict(cluster=A, num=A, den=A, label=A, acc_num=A, acc_den=A, cls_num=A, cls_den=A, w=A)

    def acc(ld=5, rows=16, M=5, stride=1, class_col=1, C=478, R=1000, **over):
        q = {**base, **over}
        return lib.egk_bootstrap_accumulate(None, vp(q["cluster"]), vp(q["num"]), vp(q["den"]), ld, rows, M, vp(q["label"]), stride, class_col, C,
                                            vp(q["acc_num"]), vp(q["acc_den"]), vp(q["cls_num"]), vp(q["cls_den"]), R, 1)

    def wts(rows=16, R=1000, **over):
        q = {**base, **over}
        return lib.egk_bootstrap_weights(None, vp(q["cluster"]), rows, R, 1, vp(q["w"]))

    def refused(rc, needle, name="egk_bootstrap_accumulate"):
        assert rc == -1 and needle in _lib.last_error() and _lib.last_error().startswith(name + ":"), (rc, _lib.last_error())

    refused(acc(cluster=None), "null cluster")
    for name in ("num", "den"):
        refused(acc(**{name: None}), "null num / den")
    for name in ("acc_num", "acc_den"):
        refused(acc(**{name: None}), "null acc_num / acc_den")
    refused(acc(rows=-1), "rows must be >= 0")
    refused(acc(rows=(1 << 24) + 1), "2^24 rows")
    for M in (0, 9):
        refused(acc(M=M, ld=16, class_col=-1), "M must lie in 1..8")
    for R in (0, 65537):
        refused(acc(R=R), "R must lie in 1..65536")
    refused(acc(ld=4), "ld must be >= M")
    for cc in (-2, 5):
        refused(acc(class_col=cc), "class_col must lie in [-1, M)")
    for name in ("label", "cls_num", "cls_den"):
        refused(acc(**{name: None}), "class_col >= 0 with a null label / cls_num / cls_den")
    for C in (0, 1025):
        refused(acc(C=C), "C must lie in 1..1024")
    for name in ("cluster", "num", "den", "label", "acc_num", "acc_den", "cls_num", "cls_den"):
        refused(acc(**{name: U4}), "8-byte aligned")
    # rows == 0 passes the same checks and launches nothing; the class part off takes NULL class pointers and any C
    assert acc(rows=0) == 0 and acc(rows=0, R=5, M=8, ld=8, class_col=7) == 0
    assert acc(rows=0, class_col=-1, label=None, cls_num=None, cls_den=None, C=0) == 0
    refused(acc(rows=0, ld=4), "ld must be >= M")
    name = "egk_bootstrap_weights"
    refused(wts(cluster=None), "null cluster", name)
    refused(wts(w=None), "null w", name)
    refused(wts(rows=-1), "rows must be >= 0", name)
    refused(wts(rows=(1 << 24) + 1), "2^24 rows", name)
    for R in (0, 65537):
        refused(wts(R=R), "R must lie in 1..65536", name)
    refused(wts(cluster=U4), "8-byte aligned", name)
    assert wts(rows=0) == 0 and wts(rows=0, R=5, w=U4 + 1) == 0
    names, buf = [], ctypes.create_string_buffer(64)
    n, ms, fl, by = ctypes.c_int64(), ctypes.c_double(), ctypes.c_double(), ctypes.c_double()
    for i in range(lib.egk_prof_count()):
        lib.egk_prof_get(i, buf, 64, ctypes.byref(n), ctypes.byref(ms), ctypes.byref(fl), ctypes.byref(by))
        names.append(buf.value.decode())
    assert "bootstrap" in names and len(set(names)) == len(names)


# ---- compare_runs ------------------------------------------------------------------------------------------------------------------------
def _file(seed=0, R=64, split="val", p=0.3, data_seed=1, drop_last=False):
    g = np.random.default_rng(data_seed)
    n = 120
    cluster = np.repeat(np.arange(n // 4), 4)
    if drop_last:
        cluster = cluster[:-4]
    rows = len(cluster)
    ok = (np.arange(rows) % 7 != 0).astype(np.int64)
    hit = (np.random.default_rng(data_seed + 100).random(rows) < p).astype(np.int64) * ok
    label = g.integers(0, 5, rows)
    num, den = np.stack([np.ones(rows, dtype=np.int64), hit], 1), np.stack([np.ones(rows, dtype=np.int64), ok], 1)
    acc = BC.accumulate(BC.empty(R, 2, 5), cluster, num, den, BC.key(seed), label=label, class_col=1)
    return BC.tables({"verbs": ([None, "verbs_top1"], "verbs_mc", acc)}, seed, R, split=split, clusters=rows // 4,
                     point={"verbs_top1": hit.sum() / ok.sum(), "verbs_mc": 0.5})


def test_compare_runs_pairs_two_files_and_refuses_unpaired_ones_by_name(tmp_path, capsys):
    a, b = _file(p=0.3), _file(p=0.6)
    res = compare.compare(a, b)
    assert set(res) == {"verbs_top1", "verbs_mc"}
    r = res["verbs_top1"]
    d = b["values"]["verbs_top1"].numpy() - a["values"]["verbs_top1"].numpy()
    want = BC.interval(d, 0.95, 64)
    assert r["diff"] == b["point"]["verbs_top1"] - a["point"]["verbs_top1"] and (r["lo"], r["hi"], r["se"]) == (want["lo"], want["hi"], want["se"])
    assert r["p"] == (1 + int((d <= 0).sum())) / 65 and r["lo"] > 0 and r["p"] == 1 / 65  # (0.3 against 0.6 on the same rows)
    same = compare.compare(a, _file(p=0.3))
    for k, r in same.items():  # a run against itself: exactly 0, [0, 0]
        assert (r["diff"], r["lo"], r["hi"], r["se"], r["p"]) == (0.0, 0.0, 0.0, 0.0, 1.0), (k, r)
    for other, needle in ((_file(seed=1), "differ in seed"), (_file(R=60), "differ in replicates"), (_file(split="test"), "differ in split"),
                          (_file(drop_last=True), "valid counts of group 'verbs'")):
        with pytest.raises(ValueError) as e:
            compare.compare(a, other)
        assert needle in str(e.value), (needle, str(e.value))
    one = _file(p=0.6)
    one["groups"]["verbs"]["acc_den"][17, 0] += 1  # one changed valid count
    with pytest.raises(ValueError, match="valid counts of group 'verbs' differ in 1 of 64"):
        compare.compare(a, one)
    torch.save(a, tmp_path / "a.pt")
    torch.save(b, tmp_path / "b.pt")
    import compare_runs
    out = compare_runs.main([f"a={tmp_path / 'a.pt'}", f"b={tmp_path / 'b.pt'}"])
    text = capsys.readouterr().out
    assert out == res and "verbs_top1: b - a = +" in text and "seed 0, 64 replicates, split val, 30 clusters" in text
    with pytest.raises(SystemExit):
        compare_runs.main([f"a={tmp_path / 'a.pt'}"])
