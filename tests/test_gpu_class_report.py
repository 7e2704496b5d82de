"""egk_class_report on the GPU against the host model (tests/class_report_common.py): every comparison of the integer state is
exact (``torch.equal`` on int64).

The fixed-point loss sums are checked twice.  Exactly: the report forms a row's loss with the row function of the loss kernels
(csrc/ce_row.h), so ``loss_q24`` must equal the host model fed with the per-row f32 loss of ``ops.cross_entropy`` on the same
tensors.  Independently: against the fp64 cross entropy, per class within the sum over the class's rows of the bound
tests/test_gpu_kernels.py::test_cross_entropy_heads_ignore_index asserts per row (rtol 1e-5, atol 1e-5), plus support * 2^-25 for
the rounding to 24 fractional bits."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import class_report_common as CR

pytestmark = pytest.mark.gpu
DEV = "cuda"
CE_RTOL, CE_ATOL = 1e-5, 1e-5  # tests/test_gpu_kernels.py::test_cross_entropy_heads_ignore_index (the f32 cross entropy, per row)


@pytest.fixture(scope="module")
def M():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from egopack_amd import meters
    return meters


@pytest.fixture(scope="module")
def ops(M):
    from egopack_amd import ops
    return ops


def _batch(rows, C, seed, ties=False):
    """(x cpu [rows, C], y cpu [rows, 2], logits view on the device with ld = C + 4 and NaN padding, label column view)."""
    g = CR.gen(seed)
    x, y = CR.logits(rows, C, g, ties), CR.labels(rows, C, g)
    return x, y, CR.padded(x.to(DEV)), y.to(DEV)[:, 0]


def _row_loss(ops, xd, yd):
    with torch.no_grad():
        return ops.cross_entropy(xd, yd).cpu().numpy()


def _check_fp64(x, y, q24):
    """|loss_q24[c] / 2^24 - sum of the fp64 losses of class c| within the per-row bound of the f32 cross-entropy test, summed over
    the class's rows, plus support * 2^-25."""
    C = x.shape[1]
    valid = (y >= 0) & (y < C)
    ref = F.cross_entropy(x[valid].double(), y[valid], reduction="none")
    want = torch.zeros(C, dtype=torch.float64).index_add_(0, y[valid], ref)
    bound = torch.zeros(C, dtype=torch.float64).index_add_(0, y[valid], CE_ATOL + CE_RTOL * ref.abs())
    support = torch.bincount(y[valid], minlength=C).double()
    err = (q24.cpu().double() / CR.Q24 - want).abs()
    slack = (bound + support * 2.0 ** -25 - err)[support > 0]
    print(f"C={C}: largest |q24 / 2^24 - fp64| {float(err.max()):.3e}, smallest slack of a class with support {float(slack.min()):.3e}")
    assert bool((err <= bound + support * 2.0 ** -25).all()), (err.max(), bound.max())


SHAPES = [((44, 115), (44, 478)), ((5, 513),), ((3, 1),), ((3, 2),), ((7, 63),), ((7, 64),), ((7, 65),), ((3, 1030),), ((1, 64),),
          ((8200, 7),)]


@pytest.mark.parametrize("ties", [False, True], ids=["grid", "ties"])
@pytest.mark.parametrize("shapes", SHAPES, ids=["+".join(f"{r}x{c}" for r, c in s) for s in SHAPES])
def test_state_equals_the_host_model_and_the_existing_counters(M, ops, shapes, ties):
    """Checks 1-3: confusion / top2 / counts against the model, loss_q24 against the model fed with ops.cross_entropy's rows and
    against fp64, and the identities that tie the ranking to egk_label_rank through _HeadCounts."""
    heads = []
    for i, (rows, C) in enumerate(shapes):
        x, y, xd, yd = _batch(rows, C, 100 * rows + C + i, ties)
        assert xd.stride(0) == C + 4 and yd.stride(0) == 2 and bool(torch.isnan(xd.as_strided((rows, 4), (C + 4, 1), C)).all())
        heads.append((x, y[:, 0], xd, yd, CR.State(C, DEV)))
    M.class_report([(xd, yd, st) for _, _, xd, yd, st in heads])  # ONE launch for all heads
    for x, y, xd, yd, st in heads:
        C = x.shape[1]
        CR.assert_state(st, CR.model(x.numpy(), y.numpy(), _row_loss(ops, xd, yd)), f"{tuple(x.shape)}")
        _check_fp64(x, y, st.loss_q24)
        assert int(st.counts[2]) == 0 and int(st.counts[3]) == 0
        hc = M._HeadCounts(C, DEV, ks=(1, 2))
        hc.update(xd, yd)
        assert torch.equal(st.confusion.diagonal(), hc.class_hits[0])
        assert torch.equal(st.confusion.sum(1), hc.support)
        assert torch.equal(st.top2.sum(1), hc.class_hits[1] - hc.class_hits[0])
        assert torch.equal(st.counts[0], hc.valid)


def test_special_rows(M, ops):
    """Check 4: an all-NaN row, a +inf, the label's logit -inf, a NaN at the label's position."""
    nan, inf = float("nan"), float("inf")
    C = 70
    x = CR.logits(5, C, CR.gen(5))
    y = torch.tensor([3, 1, 4, 6, 2])
    x[0, :] = nan                  # top1 = 0, top2 = 1, the loss is not finite
    x[1, 9] = inf                  # top1 = 9; lse = inf: not finite
    x[2, 4] = -inf                 # the label's logit: the loss is +inf
    x[3, 6] = nan                  # a NaN at the label: it ranks last, the loss is NaN
    x[4, 2], x[4, 66] = 9.0, 9.0   # an ordinary row: a tie for the first place, the label (the lower index) wins
    st = CR.State(C, DEV)
    xd, yd = CR.padded(x.to(DEV)), torch.stack([y, y], 1).to(DEV)[:, 0]
    M.class_report([(xd, yd, st)])
    loss = _row_loss(ops, xd, yd)
    assert not np.isfinite(loss[:4]).any() and np.isfinite(loss[4])
    ref = CR.model(x.numpy(), y.numpy(), loss)
    CR.assert_state(st, ref)
    conf, top2 = st.confusion.cpu(), st.top2.cpu()
    assert conf[3, 0] == 1 and top2[3].sum() == 0 and conf[1, 9] == 1 and conf[4].sum() == 1 and conf[4, 4] == 0
    assert conf[6].sum() == 1 and conf[6, 6] == 0 and conf[2, 2] == 1 and top2[2].sum() == 0
    assert st.counts.tolist() == [5, 0, 4, 0]
    q = st.loss_q24.cpu()
    assert int((q != 0).sum()) == 1 and int(q[2]) == int(np.rint(np.float64(loss[4]) * 2 ** 24))
    # the all-NaN row labelled with its runner-up makes a top-2 entry at [1, 0]
    st2 = CR.State(C, DEV)
    M.class_report([(xd[:1], torch.tensor([[1, 0]], device=DEV)[:, 0], st2)])
    assert int(st2.top2[1, 0]) == 1 and int(st2.confusion[1, 0]) == 1 and st2.counts.tolist() == [1, 0, 1, 0] and int(st2.loss_q24.abs().sum()) == 0


def test_contention_on_one_cell(M, ops):
    """Check 5: 8200 rows with the same label and the same arg-max."""
    g = CR.gen(8)
    row = CR.logits(1, 7, g)
    row[0, 3] = 9.0
    x, y = row.repeat(8200, 1), torch.full((8200, 2), 5, dtype=torch.int64)
    st, one = CR.State(7, DEV), CR.State(7, DEV)
    M.class_report([(CR.padded(x.to(DEV)), y.to(DEV)[:, 0], st)])
    M.class_report([(CR.padded(row.to(DEV)), y.to(DEV)[:1, 0], one)])
    assert int(st.confusion[5, 3]) == 8200 and int(st.confusion.sum()) == 8200 and st.counts.tolist() == [8200, 0, 0, 0]
    assert int(one.loss_q24[5]) > 0 and int(st.loss_q24[5]) == 8200 * int(one.loss_q24[5]) and int(st.loss_q24.sum()) == int(st.loss_q24[5])


def test_two_launches_accumulate_like_one(M):
    """Check 6a."""
    x, y, xd, yd = _batch(90, 37, 61, ties=True)
    whole, parts = CR.State(37, DEV), CR.State(37, DEV)
    M.class_report([(xd, yd, whole)])
    M.class_report([(xd[:31], yd[:31], parts)])
    M.class_report([(xd[31:], yd[31:], parts)])
    for a, b in zip(whole.tensors(), parts.tensors()):
        assert torch.equal(a, b)
    assert int(whole.counts[0]) + int(whole.counts[1]) == 90


class _DS:
    label_names = ["verbs", "nouns"]
    class_labels = [[f"verb_{i}" for i in range(23)], [f"noun_{i}" for i in range(41)]]
    lta_nodes = 4


def _vn_batches(n_batches, rows, seed, ties=False):
    g = CR.gen(seed)
    out = []
    for _ in range(n_batches):
        lv, ln = CR.logits(rows, 23, g, ties), CR.logits(rows, 41, g, ties)
        y = torch.stack([torch.randint(0, 23, (rows,), generator=g), torch.randint(0, 41, (rows,), generator=g)], 1)
        y[::5] = -1
        out.append(((lv.to(DEV), ln.to(DEV)), y.to(DEV), torch.rand(rows, generator=g).to(DEV)))
    return out


def test_merged_shards_equal_the_single_pass(M):
    """Check 6b: three meters fed disjoint thirds and merged hold the tensors of one meter fed everything, and derive the same
    Python floats."""
    tc = [torch.arange(23) * 9, torch.arange(41) * 5]
    batches = _vn_batches(6, 40, 7, ties=True)
    one = M.RecognitionMeter(_DS(), device=DEV, class_report=True, train_counts=tc)
    shards = [M.RecognitionMeter(_DS(), device=DEV, class_report=True, train_counts=tc) for _ in range(3)]
    for i, (logits, y, loss) in enumerate(batches):
        one.update(logits, y, loss)
        shards[i % 3].update(logits, y, loss)
    merged = shards[0].merge(shards[1]).merge(shards[2])
    state = lambda m: [t for st, _, _ in m.reports.values() for t in st.tensors()]
    assert len(state(one)) == 8 and all(torch.equal(a, b) for a, b in zip(state(one), state(merged)))
    assert int(one.reports["verbs_"][0].counts[0]) == 6 * 32
    a, b = one.get_logs(), merged.get_logs()
    keys = [k for k in a if k.startswith(("verbs_", "nouns_")) and any(k.endswith(s) for s in ("_precision", "_recall", "_f1", "_many",
                                                                                             "_medium", "_few", "_confusions", "_loss"))]
    assert len(keys) == 2 * (3 + 3 + 9 + 1 + 1)
    for k in keys:
        if torch.is_tensor(a[k]):
            assert torch.equal(a[k].nan_to_num(-1.0), b[k].nan_to_num(-1.0)), k
        else:
            assert a[k] == b[k], k  # (Python floats / ints / lists: identical, not close)


def test_optional_outputs_leave_the_rest_unchanged(M, ops):
    """Check 7: top2 = null and loss_q24 = null."""
    from egopack_amd import _lib
    x, y, xd, yd = _batch(60, 33, 77, ties=True)
    x2 = x.clone()
    x2[4, :] = float("nan")  # (a non-finite loss: counts[2] does not depend on loss_q24)
    xd = CR.padded(x2.to(DEV))
    full, bare = CR.State(33, DEV), CR.State(33, DEV, fill=-9)
    M.class_report([(xd, yd, full)])
    bare.confusion.zero_()
    bare.counts.zero_()
    t = (_lib.ClassReportTask * 1)()
    t[0].logits, t[0].ld, t[0].labels, t[0].label_stride, t[0].rows, t[0].C = xd.data_ptr(), xd.stride(0), yd.data_ptr(), 2, 60, 33
    t[0].confusion, t[0].counts = bare.confusion.data_ptr(), bare.counts.data_ptr()
    assert _lib.load().egk_class_report(ops._stream(), t, 1) == 0, _lib.last_error()
    torch.cuda.synchronize()
    assert torch.equal(bare.confusion, full.confusion) and torch.equal(bare.counts, full.counts) and int(full.counts[2]) == int(y[4, 0] >= 0)
    assert bool((bare.top2 == -9).all()) and bool((bare.loss_q24 == -9).all())  # (buffers the call was not given)


@pytest.mark.parametrize("name", ["RecognitionMeter", "AnticipationMeter", "LTAMeter", "OSCCMeter"])
def test_meters_keep_their_values_with_the_report_on(M, name):
    """Check 8: every pre-existing key has the value it has with the report off; the new keys are there; the bucket keys only with
    training counts."""
    cls = getattr(M, name)
    g = CR.gen(31)
    if name == "OSCCMeter":
        batches = [(CR.logits(50, 2, g).to(DEV), torch.randint(0, 2, (50,), generator=g).to(DEV), torch.rand(50, generator=g).to(DEV))
                   for _ in range(3)]
        tc, prefixes = [torch.tensor([10, 500])], ("",)
    else:
        batches = _vn_batches(3, 24, 32)
        tc, prefixes = [torch.arange(23) * 9, torch.arange(41) * 5], ("verbs_", "nouns_")
    meters = [cls(_DS(), device=DEV), cls(_DS(), device=DEV, class_report=True), cls(_DS(), device=DEV, class_report=True, train_counts=tc)]
    for logits, y, loss in batches:
        for m in meters:
            if name == "LTAMeter":  # (sampled futures [rows, K = 5] per head; 24 rows = 6 sequences of lta_nodes = 4)
                gp = CR.gen(33)
                pred = (torch.randint(0, 23, (24, 5), generator=gp).to(DEV), torch.randint(0, 41, (24, 5), generator=gp).to(DEV))
                m.update(logits, y, pred, loss)
            else:
                m.update(logits, y, loss)
    off, on, on_tc = (m.get_logs() for m in meters)
    for k, v in off.items():
        for other in (on, on_tc):
            w = other[k]
            if isinstance(v, dict):
                assert all(torch.equal(v[s], w[s]) for s in v), k
            else:
                assert v == w, k
    new = {p + k for p in prefixes for k in ("macro_precision", "macro_recall", "macro_f1", "confusion", "top2_confusion", "class_loss",
                                              "class_precision", "class_recall", "class_f1", "top_confusions")}
    buckets = {f"{p}{k}_{b}" for p in prefixes for k in ("acc", "classes", "samples") for b in ("many", "medium", "few")}
    assert set(on) == set(off) | new and set(on_tc) == set(off) | new | buckets
    for p in prefixes:
        conf = on_tc[p + "confusion"]
        valid = int(meters[2].reports[p][0].counts[0])
        assert int(conf.sum()) == valid > 0 and sum(on_tc[f"{p}samples_{b}"] for b in ("many", "medium", "few")) == valid
        top1 = off["accuracy"] if name == "OSCCMeter" else off.get(f"{p}top1", off.get(f"{p}accuracy_top1"))
        assert int(conf.diagonal().sum()) / valid == top1  # (the same integers behind both)
    assert len(meters[2].print_logs()) == len(meters[0].print_logs()) + len(prefixes)


def test_main_temporal_reports_and_saves_with_the_config_key(M, tmp_path):
    """``log_confusion_matrices=true`` through the entry point: the scalar keys reach the returned metrics, the bucket keys come
    from the training split's label counts, rank 0 writes class_report_<task>.pt beside the checkpoint; without the key the
    metrics have no report key and nothing is written."""
    import main_temporal
    args = ["k=1", "batch_size=4", "num_epochs=0", "+validate_untrained=true", "synthetic_samples=16", "model.hidden_size=64",
            "model.temporal_pooling.hidden_size=64", "oscc_feat_size=64", "compute=f32", "enabled_tasks=[ar,oscc]"]
    off = main_temporal.main(args + [f"checkpoint_dir={tmp_path / 'off'}"])["metrics"]
    assert not [k for t in off for k in off[t] if "macro" in k or "_many" in k] and not list(tmp_path.glob("off/*/class_report_*.pt"))
    on = main_temporal.main(args + [f"checkpoint_dir={tmp_path / 'on'}", "log_confusion_matrices=true", "class_report.shots=[1,3]"])["metrics"]
    for t in off:
        assert set(off[t]) <= set(on[t])
        for k, v in off[t].items():  # (the keys of before, with their values: two runs of the same seed)
            assert on[t][k] == pytest.approx(v, rel=1e-6, abs=1e-9), (t, k)
    assert {"verbs_macro_f1", "nouns_macro_recall", "verbs_acc_many", "nouns_acc_few", "verbs_samples_medium"} <= set(on["ar"])
    assert {"macro_f1", "acc_many", "classes_few"} <= set(on["oscc"])
    saved = {p.name: torch.load(p, weights_only=False) for p in tmp_path.glob("on/*/class_report_*.pt")}
    assert set(saved) == {"class_report_ar.pt", "class_report_oscc.pt"}
    ar = saved["class_report_ar.pt"]
    assert {"verbs_confusion", "verbs_top2_confusion", "verbs_class_loss", "nouns_class_f1", "nouns_top_confusions", "verbs_class_names",
            "nouns_counts", "verbs_train_counts"} <= set(ar)
    assert int(ar["verbs_confusion"].sum()) == int(ar["verbs_counts"][0]) > 0 and len(ar["verbs_class_names"]) == ar["verbs_confusion"].shape[0]
    assert sum(on["ar"][f"verbs_samples_{b}"] for b in ("many", "medium", "few")) == int(ar["verbs_counts"][0])
