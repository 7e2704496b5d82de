"""The cluster bootstrap on the GPU (include/egopack_bootstrap.h) against the host model of tests/bootstrap_common.py.

Every comparison of integers is ``torch.equal``: the weights, the accumulators of one launch, of split and reordered launches and of
launches over non-zero accumulators; the meters' accumulators against the model fed with what the meters fed the launch (their own
ranks, distances and cluster ids), merged shards against the single pass.  The replicate values of a single ratio, ``lo`` / ``hi`` /
``se`` are float64 quotients and order statistics of those integers and must be EQUAL to the model's; mean-class is a float64 sum over
classes and is held to 1e-12 relative.  Then two ``main_temporal.py`` runs with one seed, and ``compare_runs.py`` on their files."""
import numpy as np
import pytest
import torch

from tests import bootstrap_common as BC

pytestmark = pytest.mark.gpu
DEV = "cuda"
KEY = BC.key(2024)


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from egopack_amd import ops
    return ops


def _clusters(g, rows, mode):
    """mode 0: every row in one cluster; 1: every row in its own (0, 2^40 - 1 and negative ids among them); 2: repeated ids."""
    if mode == 0:
        return np.full(rows, 77, dtype=np.int64)
    if mode == 1:
        c = np.arange(rows, dtype=np.int64) * 1000003
    else:
        c = g.integers(0, max(rows // 4, 1), rows)
    if rows > 1:
        c[-1] = BC.MAX_CLUSTER
    if rows > 4:
        c[g.integers(1, rows - 1, max(rows // 10, 1))] = -1 - g.integers(0, 3)
        c[0] = 0
    return c


# ---- egk_bootstrap_weights ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R", [1, 4, 5, 1000])
@pytest.mark.parametrize("rows", [1, 63, 257])
def test_weights_equal_the_host_model(ops, rows, R):
    c = _clusters(np.random.default_rng(rows + R), rows, 2)
    got = ops.bootstrap_weights(torch.from_numpy(c).to(DEV), R, KEY, max_cluster=BC.MAX_CLUSTER)
    want = BC.weights(c, R, KEY)
    assert got.dtype == torch.uint8 and torch.equal(got.cpu(), torch.from_numpy(want))
    assert not want[c < 0].any() and (rows < 5 or want.any())  # negative ids: weight 0 written


# ---- egk_bootstrap_accumulate --------------------------------------------------------------------------------------------------------------
def _inputs(rows, M, C, mode, seed):
    g = np.random.default_rng(seed)
    c = _clusters(g, rows, mode)
    den = g.integers(0, 3, (rows, M))
    num = g.integers(0, 5, (rows, M)) * (den != 0)
    if rows:
        num[g.integers(0, rows), g.integers(0, M)] = 1 << 40  # the int64 path
        den[g.integers(0, rows), g.integers(0, M)] = (1 << 40) - 3
    label = g.integers(-1, C + 2, rows)  # -1 and >= C among them
    return c, num, den, label


def _launch(ops, c, num, den, label, R, C, cc, start=None, order=None):
    M = num.shape[1]
    acc = {k: torch.zeros((R, M), dtype=torch.int64, device=DEV) for k in ("acc_num", "acc_den")}
    if cc >= 0:
        acc.update({k: torch.zeros((R, C), dtype=torch.int64, device=DEV) for k in ("cls_num", "cls_den")})
    for k, v in (start or {}).items():
        acc[k].copy_(torch.from_numpy(v))
    for rows in order if order is not None else [slice(None)]:
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a[rows])).to(DEV)  # noqa: E731
        ops.bootstrap_accumulate(t(c), t(num), t(den), acc["acc_num"], acc["acc_den"], KEY, max_cluster=BC.MAX_CLUSTER,
                                 label=t(label) if cc >= 0 else None, class_col=cc, cls_num=acc.get("cls_num"), cls_den=acc.get("cls_den"))
    return {k: v.cpu() for k, v in acc.items()}


def _model(c, num, den, label, R, C, cc, start=None):
    acc = BC.empty(R, num.shape[1], C if cc >= 0 else 0)
    for k, v in (start or {}).items():
        acc[k] += v
    return BC.accumulate(acc, c, num, den, KEY, label=label, class_col=cc)


def _same(got, want, what=""):
    assert set(got) == set(want)
    for k in want:
        assert torch.equal(got[k], torch.from_numpy(want[k])), (what, k, int((got[k] != torch.from_numpy(want[k])).sum()))


# every value of rows, R, M, C and class_col the kernel treats differently, each of them with several of the others: rows around the
# workgroup's 256, R around the four replicates of a workgroup, one / five / eight columns, one class / the nouns' 478 / the largest
ROWS, RS, MS, CS = (0, 1, 255, 256, 257, 1000), (1, 3, 4, 5, 1000), (1, 5, 8), (1, 3, 478, 1024)
GRID = [(rows, R, MS[(i + j) % 3], CS[(i + 2 * j) % 4], (i + 2 * j) % 3, (2 * i + j + 1) % 3) for i, rows in enumerate(ROWS) for j, R in enumerate(RS)]


@pytest.mark.parametrize("rows,R,M,C,cc_kind,mode", GRID, ids=[f"rows{a}-R{b}-M{c}-C{d}-cc{e}-mode{f}" for a, b, c, d, e, f in GRID])
def test_accumulate_equals_the_host_model(ops, rows, R, M, C, cc_kind, mode):
    cc = (-1, 0, M - 1)[cc_kind]
    c, num, den, label = _inputs(rows, M, C, mode, rows * 31 + R)
    _same(_launch(ops, c, num, den, label, R, C, cc), _model(c, num, den, label, R, C, cc), "one launch")


def test_the_grid_covers_every_value():
    assert {g[0] for g in GRID} == set(ROWS) and {g[1] for g in GRID} == set(RS) and {g[2] for g in GRID} == set(MS)
    assert {g[3] for g in GRID} == set(CS) and {g[4] for g in GRID} == {0, 1, 2} and {g[5] for g in GRID} == {0, 1, 2}
    assert {(g[2], g[4]) for g in GRID} >= {(m, k) for m in MS for k in (0, 1, 2)}  # class_col in {-1, 0, M - 1} for every M


@pytest.mark.parametrize("R,M,C,cc", [(1000, 5, 478, 1), (5, 8, 1024, 7), (3, 1, 3, 0), (4, 5, 1, -1)])
def test_split_reordered_and_repeated_launches_have_the_bits_of_one(ops, R, M, C, cc):
    rows = 1000
    c, num, den, label = _inputs(rows, M, C, 2, R + M)
    one = _launch(ops, c, num, den, label, R, C, cc)
    _same(one, _model(c, num, den, label, R, C, cc))
    two = _launch(ops, c, num, den, label, R, C, cc, order=[slice(0, 100), slice(100, None)])
    rev = _launch(ops, c, num, den, label, R, C, cc, order=[slice(None, None, -1)])
    for k in one:
        assert torch.equal(one[k], two[k]) and torch.equal(one[k], rev[k]), k
    g = np.random.default_rng(9)
    start = {k: g.integers(-(1 << 45), 1 << 45, tuple(v.shape)) for k, v in one.items()}  # a launch ADDS to what is there
    _same(_launch(ops, c, num, den, label, R, C, cc, start=start), _model(c, num, den, label, R, C, cc, start=start), "non-zero start")


def test_ops_read_views_and_narrow_dtypes_where_they_lie(ops):
    c, num, den, label = _inputs(300, 5, 11, 2, 4)
    wide_n, wide_d = (torch.from_numpy(np.concatenate([a, a + 1], 1)).to(DEV) for a in (num, den))
    lab = torch.from_numpy(np.stack([label, label + 1, label], 1)).to(DEV)
    acc = {k: torch.zeros((9, 5), dtype=torch.int64, device=DEV) for k in ("acc_num", "acc_den")}
    cls = {k: torch.zeros((9, 11), dtype=torch.int64, device=DEV) for k in ("cls_num", "cls_den")}
    ops.bootstrap_accumulate(torch.from_numpy(c).to(DEV), wide_n[:, :5], wide_d[:, :5], acc["acc_num"], acc["acc_den"], KEY,
                             max_cluster=BC.MAX_CLUSTER, label=lab[:, 2], class_col=1, **cls)
    _same({k: v.cpu() for k, v in {**acc, **cls}.items()}, _model(c, num, den, label, 9, 11, 1))
    hit = torch.from_numpy(num[:, :2] != 0).to(DEV)  # bool columns and an int32 cluster vector
    acc = {k: torch.zeros((9, 2), dtype=torch.int64, device=DEV) for k in ("acc_num", "acc_den")}
    ops.bootstrap_accumulate(torch.from_numpy(np.abs(c) % 50).to(DEV, torch.int32), hit, torch.ones_like(hit), acc["acc_num"], acc["acc_den"],
                             KEY, max_cluster=49)
    _same({k: v.cpu() for k, v in acc.items()}, _model(np.abs(c) % 50, (num[:, :2] != 0).astype(np.int64), np.ones((300, 2), dtype=np.int64),
                                                        None, 9, 0, -1))
    with pytest.raises(ValueError, match="contiguous int64"):
        ops.bootstrap_accumulate(torch.from_numpy(c).to(DEV), wide_n[:, :5], wide_d[:, :5], acc["acc_num"], acc["acc_den"], KEY, max_cluster=1)


# ---- the meters -----------------------------------------------------------------------------------------------------------------------------
BOOT = dict(replicates=200, level=0.95, seed=7)
DATA_SEED, MODEL_SEED, SAMPLER_SEED = 3, 0, 5  # the synthetic datasets' seed (tests/test_gpu_meters.py), the weights', the LTA futures'
TASKS = ("ar", "lta", "oscc", "pnr")
COVERED = {"ar": {f"{h}_top{k}" for h in ("verbs", "nouns", "actions") for k in (1, 2, 3, 5)} | {"verbs_mc", "nouns_mc"},
           "lta": {"verbs_top1", "nouns_top1", "actions_top1", "verbs_ed", "nouns_ed", "actions_ed"},
           "oscc": {"accuracy"}, "pnr": {"localization_error"}}
TRN_CFG = {"_target_": "egopack_amd.models.temporal_pooling.trn_pooling.TRNPooling", "dropout": 0.0, "hidden_size": 64}


@pytest.fixture(scope="module")
def W(ops):
    """The validation pass of every task on the tiny synthetic datasets of tests/test_gpu_meters.py (12 samples of 8 nodes, batches
    of 4), with the bootstrap off, at 0 replicates and at 200 (traced), and sharded over two ranks; the launches are counted."""
    import egopack_amd.data as data
    import egopack_amd.meters as meters
    import egopack_amd.validate as validate
    from egopack_amd.models import Graph
    from egopack_amd.models.tasks import LTATask, OSCCTask, PNRTask, RecognitionTask
    H = 64
    ds = {t: data.SyntheticTaskDataset(t, 12, 8, 3, 48, (7, 11), k=1, seed=DATA_SEED) for t in TASKS}
    torch.manual_seed(MODEL_SEED)
    model = Graph(48, hidden_size=H, depth=2, temporal_pooling=TRN_CFG, num_segments=3).to(DEV)
    tasks = {"ar": RecognitionTask(H, H, (7, 11)).to(DEV), "lta": LTATask(H, H, (7, 11)).to(DEV), "oscc": OSCCTask(H, H).to(DEV),
             "pnr": PNRTask(H, H).to(DEV)}
    calls = []
    real = ops.bootstrap_accumulate

    def counted(*a, **kw):
        calls.append(1)
        return real(*a, **kw)

    def run(t, boot, rank=0, world=1):
        dl = data.build_dataloader(ds[t], 4, False, 0, False, 1, rank=rank, world_size=world, shard="batches")
        extra = dict(action_scores={"topk": 5}) if t in ("ar", "lta") else {}
        meter = meters.build_meter_for_dataset(ds[t], device=DEV, bootstrap=boot, **extra)
        if meter.boot is not None:
            meter.boot.trace = []
        n0 = len(calls)
        if t == "lta":
            validate.validate_lta(model, dl, meter, tasks[t], device=DEV, sampler=ops.FutureSampler(SAMPLER_SEED))
        elif t == "pnr":
            validate.validate_pnr(model, dl, meter, tasks[t], device=DEV)
        else:
            validate.validate(1, model, dl, meter, tasks[t], device=DEV)
        meter.launches = len(calls) - n0
        return meter

    ops.bootstrap_accumulate = counted
    try:
        out = {"plain": {t: run(t, None) for t in TASKS}, "zero": {t: run(t, {**BOOT, "replicates": 0}) for t in TASKS},
               "on": {t: run(t, BOOT) for t in TASKS}, "even": {t: run(t, BOOT, 0, 2) for t in TASKS},
               "odd": {t: run(t, BOOT, 1, 2) for t in TASKS}}
    finally:
        ops.bootstrap_accumulate = real
    out["validate"], out["model"], out["tasks"], out["ds"], out["data"], out["meters"] = validate, model, tasks, ds, data, meters
    return out


def _scalars(logs):
    return {k: v for k, v in logs.items() if isinstance(v, (int, float))}


@pytest.mark.parametrize("t", TASKS)
def test_replicates_0_has_the_keys_and_bits_of_no_bootstrap_and_launches_nothing(W, t):
    plain, zero = W["plain"][t], W["zero"][t]
    assert zero.boot is None and zero.launches == 0 and plain.launches == 0
    a, b = plain.get_logs(), zero.get_logs()
    assert list(a) == list(b) and _scalars(a) == _scalars(b) and plain.print_logs() == zero.print_logs()
    for x, y in zip(plain._sums(), zero._sums()):
        assert torch.equal(x, y)


@pytest.mark.parametrize("t", TASKS)
def test_meters_with_200_replicates_equal_the_model_fed_with_their_own_rows(W, t):
    plain, on = W["plain"][t], W["on"][t]
    a, b = plain.get_logs(), on.get_logs()
    new = {f"{k}_{s}" for k in COVERED[t] for s in ("ci_lo", "ci_hi", "se")}
    assert set(b) - set(a) == new and set(a) <= set(b)
    assert _scalars(a) == {k: v for k, v in _scalars(b).items() if k in a}  # every pre-existing key keeps its bits
    boot = on.boot
    assert on.launches == len(boot.trace) == 3 * len(boot.groups) and int(boot.clusters) == 12  # one launch per group and batch
    assert boot.key == BC.key(BOOT["seed"]) and boot.R == 200
    for name, g in boot.groups.items():
        rows = [e for e in boot.trace if e[0] == name]
        acc = BC.empty(200, len(g.keys), g.cls_num.shape[1] if g.cls_num is not None else 0)
        for _, cluster, num, den, label in rows:
            assert 0 <= int(cluster.min()) and int(cluster.max()) <= 11 and bool((num[:, 0] == 1).all()) and bool((den[:, 0] == 1).all())
            BC.accumulate(acc, cluster.numpy(), num.numpy(), den.numpy(), boot.key, label=None if label is None else label.numpy(),
                          class_col=g.class_col)
        assert sorted(set(torch.cat([e[1] for e in rows]).tolist())) == list(range(12))  # cluster = ordinal * 4 + the row's sequence
        _same({k: getattr(g, k).cpu() for k in acc}, acc, (t, name))
        for m, key in enumerate(g.keys):
            if key is None:
                continue
            want = BC.interval(BC.ratio_values(acc["acc_num"][:, m], acc["acc_den"][:, m]), 0.95, 200)
            assert (b[f"{key}_ci_lo"], b[f"{key}_ci_hi"], b[f"{key}_se"]) == (want["lo"], want["hi"], want["se"]), (t, key)
            # the point estimate is the same quotient of the unweighted sums of what the launch was fed
            n, d = (sum(int(e[i][:, m].sum()) for e in rows) for i in (2, 3))
            tol = dict(rel=0, abs=2.0 ** -25) if key == "localization_error" else dict(rel=1e-12, abs=1e-15)  # (seconds rounded to 2^-24)
            assert a[key] == pytest.approx(n / max(d, 1), **tol), (t, key)
        if g.class_key is not None:
            want = BC.interval(BC.mean_class_values(acc["cls_num"], acc["cls_den"]), 0.95, 200)
            for s, w in (("ci_lo", want["lo"]), ("ci_hi", want["hi"]), ("se", want["se"])):
                assert b[f"{g.class_key}_{s}"] == pytest.approx(w, rel=1e-12, abs=0), (t, g.class_key, s)
    text = "\n".join(on.print_logs())
    assert text.count("[") >= len(COVERED[t]) and "\n".join(plain.print_logs()).count("[") == 0


@pytest.mark.parametrize("t", TASKS)
def test_the_interval_holds_the_point_estimate(W, t):
    """Datasets of seed 3, weights of torch seed 0, bootstrap seed 7, futures of seed 5."""
    logs = W["on"][t].get_logs()
    for k in COVERED[t]:
        assert logs[f"{k}_ci_lo"] <= logs[k] <= logs[f"{k}_ci_hi"] and logs[f"{k}_se"] >= 0, (t, k, logs[f"{k}_ci_lo"], logs[k], logs[f"{k}_ci_hi"])


@pytest.mark.parametrize("t", TASKS)
def test_merged_shards_have_the_accumulators_of_the_single_pass(W, t):
    whole, merged = W["on"][t], W["even"][t].merge(W["odd"][t])
    assert len(whole.boot.tensors()) == len(merged.boot.tensors()) > 1
    for a, b in zip(whole.boot.tensors(), merged.boot.tensors()):
        assert torch.equal(a, b)
    got, want = merged.get_logs(), whole.get_logs()
    for k in COVERED[t]:
        for s in ("ci_lo", "ci_hi", "se"):
            assert got[f"{k}_{s}"] == want[f"{k}_{s}"], (t, k, s)


def test_a_batch_without_an_ordinal_raises_with_the_message_of_predict(W):
    dl = W["data"].build_dataloader(W["ds"]["oscc"], 4, False, 0, False, 1)
    batches = list(dl)
    for b in batches:
        b.ordinal = None

    class Loader(list):
        batch_size = 4
    meter = W["meters"].build_meter_for_dataset(W["ds"]["oscc"], device=DEV, bootstrap=BOOT)
    with pytest.raises(ValueError, match="predict: the batch carries no ordinal"):
        W["validate"].validate(1, W["model"], Loader(batches), meter, W["tasks"]["oscc"], device=DEV)
    W["validate"].validate(1, W["model"], batches, W["meters"].build_meter_for_dataset(W["ds"]["oscc"], device=DEV), W["tasks"]["oscc"], device=DEV)


# ---- the entry point ------------------------------------------------------------------------------------------------------------------------
def test_two_runs_of_main_temporal_write_the_same_accumulators_and_compare_to_zero(ops, tmp_path, capsys):
    import compare_runs
    import main_temporal
    files = []
    for run in ("a", "b"):
        main_temporal.main(["k=1", "batch_size=4", "num_epochs=2", "synthetic_samples=16", "synthetic_val_samples=10", "model.hidden_size=64",
                            "model.temporal_pooling.hidden_size=64", "oscc_feat_size=64", f"checkpoint_dir={tmp_path / run}", "save_model=True",
                            "compute=f32", "optimizer.lr=1e-3", "enabled_tasks=[ar,lta,oscc,pnr]", "lta_sampling.seed=5",
                            "lta_sampling.mode=philox", "bootstrap.replicates=100", "bootstrap.seed=11"])
        found = {p.stem[len("bootstrap_"):]: p for p in (tmp_path / run).rglob("bootstrap_*.pt")}
        assert set(found) == set(TASKS), found  # one file per enabled task, beside the checkpoint
        assert all((p.parent / "checkpoint.pth").exists() for p in found.values())
        files.append(found)
    for t in TASKS:
        a, b = (torch.load(f[t], map_location="cpu", weights_only=False) for f in files)
        assert (a["seed"], a["replicates"], a["level"], a["clusters"]) == (11, 100, 0.95, 10) and a["split"] == b["split"]
        assert set(a["values"]) >= COVERED[t] - {k for k in COVERED[t] if k.startswith("actions_")} and set(a["point"]) == set(a["values"])
        for g in a["groups"]:
            for k in ("acc_num", "acc_den", "cls_num", "cls_den"):
                if k in a["groups"][g]:
                    assert torch.equal(a["groups"][g][k], b["groups"][g][k]), (t, g, k)  # byte-identical accumulators
        res = compare_runs.main([f"a={files[0][t]}", f"b={files[1][t]}"])
        assert res and all((r["diff"], r["lo"], r["hi"]) == (0.0, 0.0, 0.0) for r in res.values()), (t, res)
    assert "b - a = +0.000000" in capsys.readouterr().out
