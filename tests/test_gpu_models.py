"""GPU parity of the model mirror (egopack_amd.models.*, engine steps) against the golden vectors
produced by the REFERENCE's own Python (tests/golden/, oracle/make_golden.py) and the CPU oracle.

Two compute modes are checked:
  * 'f32'  : exact-f32 MFMA.  Tolerance rtol 2e-4 / atol 2e-4 on features, logits and losses
             (summation-order noise through ~12 chained contractions and 5 normalisations).
  * 'bf16' : bf16 MFMA inputs, f32 accumulate -- the benchmark mode.  Tolerance: logits/features
             within 6e-2 absolute at these O(1) magnitudes, loss vectors within 5e-2.
Index outputs (k-NN assignments) are exact.
"""
import contextlib

import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import path as O  # noqa: E402
from oracle import pyg_ops as P  # noqa: E402

DEV = "cuda"
F32_TOL = dict(rtol=2e-4, atol=2e-4)
BF16_TOL = dict(rtol=6e-2, atol=6e-2)
TRN_CFG = {"_target_": "egopack_amd.models.temporal_pooling.trn_pooling.TRNPooling", "dropout": 0.0, "hidden_size": 40}


@pytest.fixture(scope="module")
def A():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    import egopack_amd.data as data
    import egopack_amd.engine as engine
    import egopack_amd.ops as ops
    import egopack_amd.sched as sched
    from egopack_amd.criterion import BCEWithLogitsNone, CrossEntropyNone, MetricSelectorWrapper
    from egopack_amd.graphone import build_graphone
    from egopack_amd.models import Graph
    from egopack_amd.models.graphONE.graphONE import GraphONE
    from egopack_amd.models.tasks import LTATask, OSCCTask, PNRTask, RecognitionTask
    from egopack_amd.optim import FlatAdam

    class NS:
        pass
    ns = NS()
    ns.__dict__.update(locals())
    return ns


def to_data(A, d):
    b = A.data.Data(**{k: v for k, v in d.items()})
    b.graph = A.data.build_csr(b.edge_index, b.x.shape[0])
    b.ptr32 = b.ptr.to(torch.int32)
    return b.to(DEV)


def make_graph(A, sd, depth=3):
    m = A.Graph(48, hidden_size=32, depth=depth, pre_dropout=0, temporal_pooling=TRN_CFG, num_segments=3)
    m.load_state_dict(sd)
    return m.to(DEV)


@pytest.mark.parametrize("mode,tol", [("f32", F32_TOL), ("bf16_f32act", BF16_TOL), ("bf16", BF16_TOL)])
@pytest.mark.parametrize("case", ["ar_T9_k1", "lta_T22_k1", "oscc_T4_k2", "pnr_T16_k2"])
def test_graph_forward_backward_vs_reference(A, golden, mode, tol, case):
    G = golden("graph_forward")
    c = G["cases"][case]
    m = make_graph(A, G["sd"], G["depth"])
    with A.ops.compute_mode(mode):
        out = m(to_data(A, c["data"]))
        (out * c["w"].to(DEV)).sum().backward()
    torch.testing.assert_close(out.detach().float().cpu(), c["out"], **tol)
    named = dict(m.named_parameters())
    for k, g in c["grads"].items():
        if mode == "f32":
            torch.testing.assert_close(named[k].grad.float().cpu(), g, rtol=2e-3, atol=2e-3, msg=lambda s: f"{k}: {s}")
        else:
            # bf16 operands through ~15 chained contractions, 5 normalisations and ReLU / LeakyReLU gates that
            # flip for near-zero pre-activations: per-element errors scale with the tensor, so the gradient check
            # is the relative Frobenius error of the whole tensor.  At these toy widths (H=32, <= 44 nodes) a
            # single flipped gate is a visible fraction of a gradient: bound 20 % here; the moderate-size test
            # below bounds it much tighter where errors average out.
            rel = (named[k].grad.float().cpu() - g).norm() / g.norm().clamp(min=1e-6)
            assert rel < 0.2, f"{k}: relative error {rel:.3f}"


def test_bf16_backbone_vs_oracle_moderate_size(A):
    """Full bf16 mode (bf16 MFMA, bf16 activations and weight operands) against the fp32 CPU oracle at a
    width where rounding noise averages out (F=128, S=3, Hp=H=256, 8 sequences x 16 nodes): features within
    3 % and every parameter gradient within 8 % relative Frobenius error."""
    torch.manual_seed(0)
    trn = {"_target_": "egopack_amd.models.temporal_pooling.trn_pooling.TRNPooling", "dropout": 0.0, "hidden_size": 256}
    m = A.Graph(128, hidden_size=256, depth=3, temporal_pooling=trn, num_segments=3)
    sd = {k: v.clone() for k, v in m.state_dict().items()}
    ds = A.data.SyntheticTaskDataset("pnr", 8, 16, 3, 128, k=1, seed=9)
    host = A.data.collate([ds[i] for i in range(8)])
    w = torch.randn(128, 256)
    leaf = {k: (v.clone().requires_grad_(True) if not k.endswith("frequency") else v) for k, v in sd.items()}
    ref = O.graph_forward(leaf, host.x, host.pos, host.edge_index, 3)
    (ref * w).sum().backward()
    m = m.to(DEV)
    with A.ops.compute_mode("bf16"):
        out = m(host.to(DEV))
        (out * w.to(DEV)).sum().backward()
    rel = (out.detach().float().cpu() - ref.detach()).norm() / ref.detach().norm()
    assert rel < 3e-2, f"features: {rel:.4f}"
    for k, p in m.named_parameters():
        g = leaf[k].grad
        r = (p.grad.float().cpu() - g).norm() / g.norm().clamp(min=1e-6)
        assert r < 8e-2, f"{k}: {r:.4f}"


@pytest.mark.parametrize("mode,ftol,gtol", [("bf16", 2e-2, 5e-2), ("f32", 1e-4, 1e-3)])
def test_recognition_head_real_class_counts(A, mode, ftol, gtol):
    """AR head with the Ego4D class counts (115 verbs, 478 nouns: widths that are NOT multiples of 8) on 2048 nodes,
    so that logits / loss gradients take the padded-stride operand path and the pipelined dX / dW kernels: logits,
    loss and every parameter gradient against the fp32 oracle (relative Frobenius error)."""
    torch.manual_seed(3)
    H, N = 256, 2048
    t = A.RecognitionTask(H, H, (115, 478))
    sd = {k: v.clone() for k, v in t.state_dict().items()}
    feat = torch.randn(N, H)
    y = torch.stack([torch.randint(0, 115, (N,)), torch.randint(0, 478, (N,))], 1)
    y[::5] = -1
    leaf = {k: v.clone().requires_grad_(True) for k, v in sd.items()}
    fo = O.projection_features(leaf, feat)
    lo = O.multihead_logits(leaf, fo, 2)
    loss_o = O.multihead_ce(lo, y)
    loss_o.mean().backward()
    t = t.to(DEV).train()
    with A.ops.compute_mode(mode):
        f = t.forward_features(feat.to(DEV))
        logits = t.forward_logits(f)
        loss = t.compute_loss(logits, y.to(DEV))
        A.ops.weighted_mean_sum([loss], [1.0]).backward()

    def rel(a, b):
        return ((a.float().cpu() - b).norm() / b.norm().clamp(min=1e-12)).item()
    for a, b in zip(logits, lo):
        assert a.shape == b.shape and rel(a.detach(), b.detach()) < ftol
    assert rel(loss.detach(), loss_o.detach()) < ftol
    for k, p in t.named_parameters():
        assert rel(p.grad, leaf[k].grad) < gtol, f"{k}: {rel(p.grad, leaf[k].grad):.4f}"


def test_graph_accepts_plain_batch_without_csr(A, golden):
    """Drop-in contract: a batch that only carries x / pos / edge_index / batch (what PyG's loader gives)."""
    G = golden("graph_forward")
    c = G["cases"]["ar_T9_k1"]
    m = make_graph(A, G["sd"])
    d = A.data.Data(x=c["data"]["x"].to(DEV), pos=c["data"]["pos"].to(DEV), edge_index=c["data"]["edge_index"].to(DEV),
                    batch=c["data"]["batch"].to(DEV))
    with A.ops.compute_mode("f32"):
        out = m(d)
    torch.testing.assert_close(out.detach().float().cpu(), c["out"], **F32_TOL)


def test_fused_multitask_backbone_equals_separate_passes(A, golden):
    """The fused pass over several task batches (per-task graph-LN statistics) reproduces the separate
    per-batch passes of the reference (main_temporal.py:87-90)."""
    G = golden("graph_forward")
    m = make_graph(A, G["sd"])
    names = ["ar_T9_k1", "lta_T22_k1", "pnr_T16_k2"]
    batches = [to_data(A, G["cases"][n]["data"]) for n in names]
    host = [A.data.Data(**G["cases"][n]["data"]) for n in names]
    merged = A.data.merge_batches(host).to(DEV)
    merged.x = [b.x for b in batches]
    with A.ops.compute_mode("f32"):
        fused = m(merged)
        m.zero_grad()
        w = torch.cat([G["cases"][n]["w"] for n in names]).to(DEV)
        (fused * w).sum().backward()
    off = 0
    for n in names:
        ref = G["cases"][n]["out"]
        torch.testing.assert_close(fused[off:off + ref.shape[0]].detach().float().cpu(), ref, **F32_TOL)
        off += ref.shape[0]
    named = dict(m.named_parameters())
    for k in G["cases"][names[0]]["grads"]:
        ref = sum(G["cases"][n]["grads"][k] for n in names)
        torch.testing.assert_close(named[k].grad.float().cpu(), ref, rtol=2e-3, atol=2e-3, msg=lambda s: f"{k}: {s}")


@pytest.mark.parametrize("mode,tol", [("f32", F32_TOL), ("bf16_f32act", BF16_TOL), ("bf16", BF16_TOL)])
@pytest.mark.parametrize("key", ["ar_avg0", "ar_avg1", "lta_avg0", "lta_avg1"])
def test_multihead_tasks_vs_reference(A, golden, mode, tol, key):
    G = golden("heads")
    c = G[key]
    cls = A.RecognitionTask if key.startswith("ar") else A.LTATask
    t = cls(32, 32, (7, 11), aux_tasks=tuple(c["aux"].keys()), average_logits=key.endswith("1"))
    t.load_state_dict(c["sd"])
    t = t.to(DEV).eval()
    with A.ops.compute_mode(mode):
        f = t.forward_features(G["feat"].to(DEV))
        plain = t.forward_logits(f)
        fused = t.forward_logits(f, None, {k: v.to(DEV) for k, v in c["aux"].items()})
        loss = t.compute_loss(fused, G["y2"].to(DEV))
    torch.testing.assert_close(f.detach().float().cpu(), c["features"], **tol)
    for a, b in zip(plain, c["logits"]):
        torch.testing.assert_close(a.detach().float().cpu(), b, **tol)
    for a, b in zip(fused, c["logits_fused"]):
        torch.testing.assert_close(a.detach().float().cpu(), b, rtol=tol["rtol"], atol=tol["atol"] * 3)
    ltol = F32_TOL if mode == "f32" else dict(rtol=5e-2, atol=0.15)
    torch.testing.assert_close(loss.detach().float().cpu(), c["loss"], **ltol)


def test_metric_selector_wrapper(A, golden):
    G = golden("heads")

    class DS:
        has_joint_label = False
        num_labels = 2
    crit = A.MetricSelectorWrapper(A.CrossEntropyNone(), DS())
    logits = tuple(l.to(DEV) for l in G["selector"]["logits"])
    torch.testing.assert_close(crit(logits, G["y2"].to(DEV)).cpu(), G["selector"]["loss"], rtol=1e-5, atol=1e-5)
    with pytest.raises(ValueError):
        crit(logits[:1], G["y2"].to(DEV))


@pytest.mark.parametrize("avg", [0, 1])
def test_oscc_task_vs_reference(A, golden, avg):
    G = golden("heads")
    c = G[f"oscc_ce_avg{avg}"]
    t = A.OSCCTask(32, 32, 0, 0, loss_func="ce", aux_tasks=("ar", "lta", "pnr"), average_logits=bool(avg))
    t.load_state_dict(c["sd"])
    t = t.to(DEV).eval()
    batch = G["batch"].to(DEV)
    with A.ops.compute_mode("f32"):
        f = t.forward_features(G["feat"].to(DEV))
        plain = t.forward_logits(f, batch)
        fused = t.forward_logits(f, batch, {k: v.to(DEV) for k, v in c["aux"].items()})
        loss = t.compute_loss(fused, c["y"].to(DEV))
    torch.testing.assert_close(plain.detach().float().cpu(), c["logits"], **F32_TOL)
    torch.testing.assert_close(fused.detach().float().cpu(), c["logits_fused"], **F32_TOL)
    torch.testing.assert_close(loss.detach().float().cpu(), c["loss"], **F32_TOL)
    with pytest.raises(ValueError):
        A.OSCCTask(32, 32).to(DEV).forward_aux_logits(f, batch, "ar")


@pytest.mark.parametrize("avg", [0, 1])
def test_pnr_task_vs_reference(A, golden, avg):
    G = golden("heads")
    c = G[f"pnr_avg{avg}"]
    t = A.PNRTask(32, 32, 0, 0, aux_tasks=("ar", "oscc", "lta"), average_logits=bool(avg))
    t.load_state_dict(c["sd"])
    t = t.to(DEV).eval()
    with A.ops.compute_mode("f32"):
        f = t.forward_features(G["feat"].to(DEV))
        plain = t.forward_logits(f)
        fused = t.forward_logits(f, {k: v.to(DEV) for k, v in c["aux"].items()})
        loss = t.compute_loss(fused, c["y"].to(DEV))
    assert plain.shape == c["logits"].shape
    torch.testing.assert_close(plain.detach().float().cpu(), c["logits"], **F32_TOL)
    torch.testing.assert_close(fused.detach().float().cpu(), c["logits_fused"], **F32_TOL)
    torch.testing.assert_close(loss.detach().float().cpu(), c["loss"], **F32_TOL)


@pytest.mark.parametrize("mode", ["f32", "bf16_f32act", "bf16"])
@pytest.mark.parametrize("residual", [0, 1])
def test_graphone_vs_reference(A, golden, mode, residual):
    G = golden("graphone")
    c = G[f"residual{residual}"]
    m = A.GraphONE({k: v.clone() for k, v in G["banks"].items()}, features_size=32, hidden_size=32, k=G["k"],
                   depth=c["depth"], residual=bool(residual), dropout=0, output_dropout=0, output_projection=True)
    m.load_state_dict(c["sd"])
    m = m.to(DEV)
    feats = {t: f.clone().to(DEV).requires_grad_(True) for t, f in c["features"].items()}
    with A.ops.compute_mode(mode):
        out, closest = m.interact(feats)
        sum((out[t] * c["w"][t].to(DEV)).sum() for t in feats).backward()
    tol = F32_TOL if mode == "f32" else dict(rtol=6e-2, atol=0.1)
    for t in feats:
        for a, b in zip(closest[t], c["closest"][t]):
            if mode != "bf16":  # same stored feature values -> k-NN (always on the exact path) is index-exact
                assert torch.equal(a.cpu(), b)
            else:  # features are bf16-rounded before the search: near-ties may flip
                assert (a.cpu() == b).float().mean() > 0.8
        torch.testing.assert_close(out[t].detach().float().cpu(), c["out"][t], **tol)
    if mode == "f32":
        for t in feats:
            torch.testing.assert_close(feats[t].grad.float().cpu(), c["grad_features"][t], rtol=2e-3, atol=2e-3)
        named = dict(m.named_parameters())
        for k, g in c["grads"].items():
            torch.testing.assert_close(named[k].grad.float().cpu(), g, rtol=2e-3, atol=2e-3, msg=lambda s: f"{k}: {s}")
    assert all(not p.requires_grad for n, p in m.named_parameters() if n.startswith("embeddings."))


def test_build_graphone_vs_reference(A, golden):
    G = golden("build_graphone")
    model = make_graph(A, G["backbone"])
    ar = A.RecognitionTask(32, 32, G["n_classes"])
    lta = A.LTATask(32, 32, G["n_classes"])
    pnr = A.PNRTask(32, 32)
    for t, k in ((ar, "ar"), (lta, "lta"), (pnr, "pnr")):
        t.load_state_dict(G["tasks"][k])
        t.to(DEV)
    batches = [A.data.Data(**b) for b in G["batches"]]
    with A.ops.compute_mode("f32"):
        banks = A.build_graphone(model, ar, [ar, lta, pnr], batches, device=DEV)
    assert set(banks) == set(G["banks"])
    for k in banks:
        assert banks[k].dtype == torch.float32 and banks[k].shape == G["banks"][k].shape
        torch.testing.assert_close(banks[k].float().cpu(), G["banks"][k], **F32_TOL)


def _load_all(A, G, aux=False):
    model = make_graph(A, G["before"]["temporal_graph"])
    if aux:
        ar = A.RecognitionTask(32, 32, (7, 11), aux_tasks=("oscc", "lta", "pnr"))
        oscc = A.OSCCTask(32, 32, aux_tasks=("ar", "lta", "pnr"), average_logits=True)
        lta = A.LTATask(32, 32, (7, 11), aux_tasks=("ar", "oscc", "pnr"))
        pnr = A.PNRTask(32, 32, aux_tasks=("ar", "oscc", "lta"))
    else:
        ar, oscc, lta, pnr = A.RecognitionTask(32, 32, (7, 11)), A.OSCCTask(32, 32), A.LTATask(32, 32, (7, 11)), A.PNRTask(32, 32)
    tasks = {"ar": ar, "oscc": oscc, "lta": lta, "pnr": pnr}
    names = {"ar": "task/recognition", "oscc": "task/oscc", "lta": "task/lta", "pnr": "task/pnr"}
    for t, n in names.items():
        tasks[t].load_state_dict(G["before"][n])
        tasks[t].to(DEV)
    return model, tasks, names


@pytest.mark.parametrize("fused", [False, True])
def test_mtl_train_two_iterations_vs_reference(A, golden, fused):
    """Two iterations of the multi-task step (AR + LTA + PNR enabled, OSCC weight 0) with FlatAdam reproduce
    the parameters the reference's main_temporal.train + torch.optim.Adam produced (exact-f32 mode)."""
    G = golden("mtl_train")
    model, tasks, names = _load_all(A, G)

    class DS:
        has_joint_label = False
        num_labels = 2
    crit = {"ar": A.MetricSelectorWrapper(A.CrossEntropyNone(), DS()), "lta": A.MetricSelectorWrapper(A.CrossEntropyNone(), DS()),
            "oscc": A.CrossEntropyNone(), "pnr": A.BCEWithLogitsNone()}
    params = [*model.parameters(), *(p for t in ("ar", "oscc", "lta", "pnr") for p in tasks[t].parameters())]
    opt = A.FlatAdam(params, lr=G["lr"], weight_decay=G["weight_decay"])
    step = A.engine.MTLStep(model, tasks, crit, G["weights"], opt, fused_backbone=fused)
    model.train()
    for t in tasks.values():
        t.train()
    with A.ops.compute_mode("f32"):
        for it in range(2):
            batches = {t: to_data(A, G["batches"][t][it]) for t in ("ar", "lta", "oscc", "pnr")}
            total, vectors = step.step(batches)
            for t in ("ar", "lta", "pnr"):
                torch.testing.assert_close(vectors[t].float().cpu(), G["loss_vectors"][t][it], rtol=1e-3, atol=1e-3)
            assert "oscc" not in vectors
    for grp, mod in [("temporal_graph", model)] + [(n, tasks[t]) for t, n in names.items()]:
        sd = mod.state_dict()
        for k, v in G["after"][grp].items():
            # Adam normalises the update: a parameter moves by ~lr per step whatever the gradient scale, so the
            # comparison is absolute, at a small fraction of the 2*lr = 2e-3 total movement
            torch.testing.assert_close(sd[k].cpu(), v, rtol=0, atol=1.5e-4, msg=lambda s: f"{grp}/{k}: {s}")
    for k, v in G["before"]["task/oscc"].items():
        assert torch.equal(tasks["oscc"].state_dict()[k].cpu(), v)  # disabled task untouched


def test_egopack_train_two_iterations_vs_reference(A, golden):
    G = golden("egopack_train")
    model, tasks, names = _load_all(A, G, aux=True)
    sd = G["before"]["graphone"]
    banks = {t: sd[f"embeddings.{t}.weight"].clone() for t in ("ar", "lta", "pnr")}
    gone = A.GraphONE(banks, features_size=32, hidden_size=32, k=G["k"], depth=G["depth"], residual=G["residual"],
                      dropout=0, output_dropout=0, output_projection=True)
    gone.load_state_dict(sd)
    gone = gone.to(DEV)
    params = [*model.parameters(), *(p for t in ("ar", "oscc", "lta", "pnr") for p in tasks[t].parameters()),
              *gone.parameters()]
    opt = A.FlatAdam(params, lr=G["lr"], weight_decay=G["weight_decay"])
    step = A.engine.EgoPackStep(model, tasks, gone, {"oscc": 1.0}, opt, backprop_temporal_graph=True,
                                temporal_graph_train_mode=False)
    with A.ops.compute_mode("f32"):
        for it in range(2):
            total, vectors = step.step({"oscc": to_data(A, G["batches"]["oscc"][it])})
            torch.testing.assert_close(vectors["oscc"].float().cpu(), G["loss_vectors"]["oscc"][it], rtol=1e-3, atol=1e-3)
    mods = [("temporal_graph", model), ("graphone", gone)] + [(n, tasks[t]) for t, n in names.items()]
    for grp, mod in mods:
        cur = mod.state_dict()
        for k, v in G["after"][grp].items():
            torch.testing.assert_close(cur[k].cpu(), v, rtol=0, atol=1.5e-4, msg=lambda s: f"{grp}/{k}: {s}")


def test_captured_egopack_step_equals_eager_step(A, golden):
    """hipGraph replay of the EgoPack novel-task step (GraphONE task chains on their own streams) leaves the parameters
    of the eager step, bit for bit: nothing of the optimizer may start before every chain's gradients are final."""
    G = golden("egopack_train")

    def run(use_graph):
        model, tasks, names = _load_all(A, G, aux=True)
        sd = G["before"]["graphone"]
        banks = {t: sd[f"embeddings.{t}.weight"].clone() for t in ("ar", "lta", "pnr")}
        gone = A.GraphONE(banks, features_size=32, hidden_size=32, k=G["k"], depth=G["depth"], residual=G["residual"],
                          dropout=0, output_dropout=0, output_projection=True)
        gone.load_state_dict(sd)
        gone = gone.to(DEV)
        params = [*model.parameters(), *(p for t in ("ar", "oscc", "lta", "pnr") for p in tasks[t].parameters()), *gone.parameters()]
        opt = A.FlatAdam(params, lr=G["lr"], weight_decay=G["weight_decay"])
        step = A.engine.EgoPackStep(model, tasks, gone, {"oscc": 1.0}, opt, backprop_temporal_graph=True,
                                    temporal_graph_train_mode=False)
        batches = {"oscc": to_data(A, G["batches"]["oscc"][0])}
        with A.ops.compute_mode("f32"):
            if use_graph:
                step.capture(batches, warmup=2)
                for _ in range(3):
                    step.replay()
            else:
                for _ in range(5):
                    step.step(batches)
        torch.cuda.synchronize()
        return opt.flat_p.clone().cpu(), opt.step_count

    p_eager, n_eager = run(False)
    p_graph, n_graph = run(True)
    assert n_eager == n_graph == 5
    assert torch.equal(p_graph, p_eager)


def test_captured_step_equals_eager_step(A, golden):
    """hipGraph replay of forward+backward+Adam gives the same parameters as the eager step."""
    G = golden("mtl_train")

    class DS:
        has_joint_label = False
        num_labels = 2

    def run(use_graph):
        model, tasks, names = _load_all(A, G)
        crit = {"ar": A.MetricSelectorWrapper(A.CrossEntropyNone(), DS()), "lta": A.MetricSelectorWrapper(A.CrossEntropyNone(), DS()),
                "oscc": A.CrossEntropyNone(), "pnr": A.BCEWithLogitsNone()}
        live = [*model.parameters(), *(p for t in ("ar", "lta", "pnr") for p in tasks[t].parameters())]
        opt = A.FlatAdam(live, lr=1e-3, weight_decay=1e-5)
        step = A.engine.MTLStep(model, tasks, crit, G["weights"], opt, fused_backbone=True)
        batches = {t: to_data(A, G["batches"][t][0]) for t in ("ar", "lta", "pnr")}
        with A.ops.compute_mode("f32"):
            if use_graph:
                step.capture(batches, warmup=2)
                for _ in range(3):
                    step.replay()
            else:
                for _ in range(5):
                    step.step(batches)
        torch.cuda.synchronize()
        return opt.flat_p.clone().cpu(), opt.step_count

    p_eager, n_eager = run(False)
    p_graph, n_graph = run(True)
    assert n_eager == n_graph == 5
    torch.testing.assert_close(p_graph, p_eager, rtol=0, atol=1e-6)


@pytest.mark.parametrize("workload", ["mtl", "egopack_oscc"])
def test_single_writer_gradient_slots_are_stored_not_cleared_and_accumulated(workload, monkeypatch):
    """Captured one-rank steps leave the gradient slots that ONE weight-gradient launch writes per step (learnt from an eager step,
    checked in the capture: FlatAdam.learn_begin / store_begin) out of the buffer clear and let that launch STORE
    (optimizer.zero_grad() + the accumulation of .grad, reference main_temporal.py:76-131 / main_egopack.py:45-61): parameters,
    moments, bf16 copies and gradients after three replays equal those of the step that clears everything and accumulates
    (EGK_DISABLE=grad_store), bit for bit."""
    import bench
    from egopack_amd import engine, ops
    from egopack_amd.optim import FlatAdam
    prev = ops.get_compute()

    def run(on):
        if on:
            monkeypatch.delenv("EGK_DISABLE", raising=False)
        else:
            monkeypatch.setenv("EGK_DISABLE", "grad_store")
        a = ["--workload", workload, "--batch", "16", "--T", "16", "--hidden", "128", "--trn-hidden", "256", "--dropout", "0.5"]
        args = bench.parse_args(a + (["--bank", "256"] if workload == "egopack_oscc" else []))
        args.compute = "bf16"
        ops.set_compute("bf16")
        ops.manual_seed(11)
        model, tasks, crit, weights, dev, merged = bench.build_workload(args, 0, torch.device(DEV))
        model.to(DEV).train()
        for t in tasks.values():
            t.to(DEV).train()
        params = [*model.parameters(), *(p for t in tasks.values() for p in t.parameters())]
        if workload == "egopack_oscc":
            from egopack_amd.models.graphONE.graphONE import GraphONE
            g = torch.Generator(device=DEV)
            g.manual_seed(7)
            banks = {t: torch.randn(args.bank, args.hidden, device=DEV, generator=g) for t in ("ar", "lta", "pnr")}
            graphone = GraphONE(banks, features_size=args.hidden, hidden_size=args.hidden, k=4, depth=2, residual=True).to(DEV)
            opt = FlatAdam(params + list(graphone.parameters()), lr=1e-3, weight_decay=1e-5)
            step = engine.EgoPackStep(model, tasks, graphone, weights, opt, backprop_temporal_graph=True, temporal_graph_train_mode=False)
        else:
            opt = FlatAdam(params, lr=1e-3, weight_decay=1e-5)
            step = engine.MTLStep(model, tasks, crit, weights, opt, fused_backbone=True)
        step.capture(dev, merged, warmup=2)
        for _ in range(3):
            step.replay()
        torch.cuda.synchronize()
        return ([t.clone().cpu() for t in (opt.flat_p, opt.flat_m, opt.flat_v, opt.flat_w16.view(torch.int16), opt.flat_g)],
                getattr(step, "_grad_store_slots", 0), opt)

    try:
        got, n_on, opt = run(True)
        ref, n_off, _ = run(False)
    finally:
        ops.set_compute(prev)
    assert n_off == 0 and n_on >= 8, (n_on, n_off)
    stored = sum(opt.store_slots.values())
    assert stored > 0.5 * opt.flat_g.numel(), (stored, opt.flat_g.numel())  # most of the buffer is no longer cleared
    for a, b, name in zip(got, ref, ("p", "m", "v", "bf16 copy", "gradient")):
        assert torch.equal(a, b), name


@pytest.mark.parametrize("mode", ["f32", "bf16"])
def test_classifier_bank_equals_the_separate_classifiers(mode):
    """The verb / noun classifiers of a head as ONE contraction over the zero-padded bank the optimizer lays out
    (forward, dX, dW, bias gradients; the loss writing its gradient straight into the bank's operand buffer or not)
    against the per-classifier path on the same parameters; the padding stays zero under Adam."""
    from egopack_amd import ops
    from egopack_amd.models.tasks import RecognitionTask
    from egopack_amd.optim import FlatAdam
    heads, H, M = (115, 478), 128, 200
    torch.manual_seed(5)
    ref = RecognitionTask(H, H, heads).to(DEV)
    tasks = {k: RecognitionTask(H, H, heads).to(DEV) for k in ("bank", "handoff", "seeded")}
    for t in tasks.values():
        t.load_state_dict(ref.state_dict())
    x = torch.randn(M, H, device=DEV)
    y = torch.stack([torch.randint(-1, heads[0], (M,)), torch.randint(-1, heads[1], (M,))], 1).to(DEV)

    def run(task, bank, handoff, steps=2):
        opt = FlatAdam(task.parameters(), lr=1e-2, weight_decay=1e-3)
        out = []
        for _ in range(steps):
            opt.zero_grad()
            xin = x.clone().requires_grad_(True)
            views = getattr(task.classifiers[0][1].weight, "_egk_bank_views", None)
            assert (views is not None) == (bank and opt.materialised)
            ctx = ops.bank_grad_handoff() if handoff else contextlib.nullcontext()
            # "seeded": the constant gradient of the loss vector is announced up front -> ONE fused launch computes the loss
            # and writes its gradient (and the zero pad columns) into the bank's operand buffer (egk_ce_fused)
            seed = ops.loss_seed(1.0 / M) if handoff == "seeded" else contextlib.nullcontext()
            with ctx, seed:
                logits = task.forward_logits(task.forward_features(xin))
                loss = task.compute_loss(logits, y)
            loss.backward(torch.full_like(loss, 1.0 / M))
            out.append((tuple(l.detach().float().clone() for l in logits), xin.grad.clone(),
                        [p.grad.detach().clone() for p in task.parameters()]))
            opt.step()
        return out, opt
    with ops.compute_mode(mode):
        for p in ref.parameters():  # the reference task: no bank tags -> the per-classifier path on the same layout rules
            if hasattr(p, "_egk_bank"):
                del p._egk_bank
        want, _ = run(ref, False, False)
        tol = dict(rtol=1e-4, atol=1e-5) if mode == "f32" else dict(rtol=3e-2, atol=3e-3)
        for name in ("bank", "handoff", "seeded"):
            got, opt = run(tasks[name], True, {"bank": False, "handoff": True, "seeded": "seeded"}[name])
            for (lg, dxg, pg), (lw, dxw, pw) in zip(got, want):
                for a, b in zip(lg, lw):
                    torch.testing.assert_close(a, b, **tol)
                torch.testing.assert_close(dxg.float(), dxw.float(), **tol)
                for a, b in zip(pg, pw):
                    torch.testing.assert_close(a, b, **tol)
            v = tasks[name].classifiers[0][1].weight._egk_bank_views
            assert v["rows"] == [(0, 115), (128, 478)] and v["n"] == 640
            pad = torch.ones(640, dtype=torch.bool, device=DEV)
            for r0, n in v["rows"]:
                pad[r0:r0 + n] = False
            for buf in (v["wp"], v["w16"], v["wg"]):
                assert float(buf[pad].float().abs().max()) == 0.0
            assert float(v["b"][pad].abs().max()) == 0.0 and float(v["bg"][pad].abs().max()) == 0.0


# ---- variants of the cited functions beside the configured ones (tests/golden/variants.pt, reference-generated) -------
@pytest.mark.parametrize("name", ["l2", "trainable", "l2_trainable"])
def test_graphone_variants_vs_reference(A, golden, name):
    """GraphONE(distance_func='l2') (reference graphONE.py:126-127,144-145) and GraphONE(freeze=False) (:47-49) in exact-f32
    mode: outputs, nearest-prototype indices (exact), feature / stage gradients and the prototype gradients."""
    G = golden("variants")
    c = G[name]
    m = A.GraphONE({k: v.clone() for k, v in G["banks"].items()}, features_size=32, hidden_size=32, k=G["k"], depth=G["depth"],
                   residual=True, dropout=0, output_dropout=0, output_projection=True, **c["kw"])
    m.load_state_dict(c["sd"])
    m = m.to(DEV)
    feats = {t: f.clone().to(DEV).requires_grad_(True) for t, f in c["features"].items()}
    with A.ops.compute_mode("f32"):
        out, closest = m.interact(feats)
        sum((out[t] * c["w"][t].to(DEV)).sum() for t in feats).backward()
    for t in feats:
        for a, b in zip(closest[t], c["closest"][t]):
            assert torch.equal(a.cpu(), b)
        torch.testing.assert_close(out[t].detach().float().cpu(), c["out"][t], **F32_TOL)
        torch.testing.assert_close(feats[t].grad.float().cpu(), c["grad_features"][t], rtol=2e-3, atol=2e-3)
    named = dict(m.named_parameters())
    for k, g in c["grads"].items():
        assert named[k].grad is not None, k
        torch.testing.assert_close(named[k].grad.float().cpu(), g, rtol=2e-3, atol=2e-3, msg=lambda s: f"{k}: {s}")
    trainable_banks = not c["kw"]["freeze"]
    assert all(p.requires_grad == trainable_banks for n, p in m.named_parameters() if n.startswith("embeddings."))


def test_trainable_prototypes_move_under_flat_adam(A, golden):
    """freeze=False end to end: the prototypes are optimizer parameters (main_egopack.py:323 passes graphone.parameters());
    one FlatAdam step equals torch.optim.Adam on the reference-generated gradients."""
    G = golden("variants")
    c = G["trainable"]
    m = A.GraphONE({k: v.clone() for k, v in G["banks"].items()}, features_size=32, hidden_size=32, k=G["k"], depth=G["depth"],
                   residual=True, **c["kw"])
    m.load_state_dict(c["sd"])
    m = m.to(DEV)
    opt = A.FlatAdam(m.parameters(), lr=1e-2, weight_decay=1e-3)
    feats = {t: f.clone().to(DEV) for t, f in c["features"].items()}
    with A.ops.compute_mode("f32"):
        out, _ = m.interact(feats)
        sum((out[t] * c["w"][t].to(DEV)).sum() for t in feats).backward()
        opt.step()
    ref = {k: v.clone().requires_grad_(True) for k, v in c["sd"].items()}
    for k, g in c["grads"].items():
        ref[k].grad = g.clone()
    topt = torch.optim.Adam([ref[k] for k in c["grads"]], lr=1e-2, weight_decay=1e-3)
    topt.step()
    cur = m.state_dict()
    for k in c["grads"]:
        torch.testing.assert_close(cur[k].cpu(), ref[k].detach(), rtol=0, atol=2e-4, msg=lambda s: f"{k}: {s}")
    assert not torch.equal(cur["embeddings.ar.weight"].cpu(), c["sd"]["embeddings.ar.weight"])


def test_oscc_bce_vs_reference_and_focal_vs_oracle(A, golden):
    """OSCCTask.compute_loss 'bce' against the reference's own outputs and gradients (oscc.py:91-93) and 'focal'
    (oscc.py:94-96: torchvision.ops.sigmoid_focal_loss, absent package -> restated in the oracle) against the oracle."""
    c = golden("variants")["oscc_bce"]
    for kind in ("bce", "focal"):
        t = A.OSCCTask(32, 32, 0, 0, loss_func=kind)
        t.load_state_dict(c["sd"])
        t = t.to(DEV).eval()
        with A.ops.compute_mode("f32"):
            logits = t.forward_logits(t.forward_features(c["feat"].to(DEV)), c["batch"].to(DEV))
            loss = t.compute_loss(logits, c["y"].to(DEV))
            (loss * c["w"].to(DEV)).sum().backward()
        if kind == "bce":
            want_loss, want_grads = c["loss"], c["grads"]
        else:
            sd = {k: v.clone().requires_grad_(True) for k, v in c["sd"].items()}
            lo = O.oscc_loss(O.oscc_logits(sd, O.projection_features(sd, c["feat"]), c["batch"]), c["y"], "focal")
            (lo * c["w"]).sum().backward()
            want_loss, want_grads = lo.detach(), {k: v.grad for k, v in sd.items() if v.grad is not None}
        assert loss.shape == want_loss.shape == (3, 2)
        torch.testing.assert_close(loss.detach().cpu(), want_loss, **F32_TOL)
        named = dict(t.named_parameters())
        for k, g in want_grads.items():
            torch.testing.assert_close(named[k].grad.float().cpu(), g, rtol=2e-3, atol=2e-4, msg=lambda s: f"{kind} {k}: {s}")


@pytest.mark.parametrize("gamma,alpha", [(2.0, 0.5), (1.5, 0.25), (2.0, -1.0)])
def test_onehot_sigmoid_focal_kernel_vs_autograd(A, gamma, alpha):
    """The focal kernel pair over a range of logits (saturated ones included) against torch autograd of the published
    formula in fp64."""
    g = torch.Generator().manual_seed(5)
    x = torch.cat([torch.randn(40, 2, generator=g) * 3, torch.tensor([[30., -30.], [-30., 30.], [0., 0.]])])
    y = torch.randint(0, 2, (x.shape[0],), generator=g)
    w = torch.randn(x.shape, generator=g)
    xd = x.to(DEV).requires_grad_(True)
    loss = A.ops.onehot_sigmoid_focal_loss(xd, y.to(DEV), alpha, gamma)
    (loss * w.to(DEV)).sum().backward()
    x64 = x.double().requires_grad_(True)
    t = torch.nn.functional.one_hot(y, 2).double()
    p = torch.sigmoid(x64)
    ce = torch.nn.functional.binary_cross_entropy_with_logits(x64, t, reduction="none")
    ref = ce * (1 - (p * t + (1 - p) * (1 - t))) ** gamma
    if alpha >= 0:
        ref = (alpha * t + (1 - alpha) * (1 - t)) * ref
    (ref * w.double()).sum().backward()
    torch.testing.assert_close(loss.detach().double().cpu(), ref.detach(), rtol=1e-5, atol=1e-6)
    torch.testing.assert_close(xd.grad.double().cpu(), x64.grad, rtol=1e-4, atol=1e-6)


@pytest.mark.parametrize("what", ["grouped_heads", "wgrad_grouping"])
def test_grouped_launches_equal_the_per_problem_launches(A, what):
    """engine.MTLStep with (a) the task heads' projections as ONE chain of grouped launches (ops.grouped_projection) and (b) the
    H x H weight gradients parked and issued four at a time as one grouped launch (sched._wgrad_defer), each against the same
    step without it: objective, loss vectors and every parameter after 3 Adam steps (bf16 mode: the paths run the same
    kernel bodies with other tile variants / no split-K -> fp32 accumulation-order noise, then bf16 rounding)."""
    import argparse
    import bench

    def run(on):
        args = argparse.Namespace(hidden=256, trn_hidden=256, dropout=0.0, compute="bf16", workload="mtl4", batch=8, T=16)
        A.ops.set_compute("bf16")
        A.ops.manual_seed(11)
        model, tasks, crit, weights, dev, merged = bench.build_workload(args, 0, torch.device(DEV))
        model.to(DEV).train()
        for t in tasks.values():
            t.to(DEV).train()
        params = [*model.parameters(), *(p for t in tasks.values() for p in t.parameters())]
        opt = A.FlatAdam(params, lr=1e-3, weight_decay=1e-5)
        step = A.engine.MTLStep(model, tasks, crit, weights, opt, fused_backbone=True)
        step.grouped_heads = on if what == "grouped_heads" else False
        step.wgrad_grouping = on if what == "wgrad_grouping" else False
        used = []
        name = "grouped_projection" if what == "grouped_heads" else "gemm_grouped"
        orig = getattr(A.ops, name)

        def spy(*a, **k):
            used.append(1)
            return orig(*a, **k)
        setattr(A.ops, name, spy)
        try:
            outs = [step.step(dev, merged) for _ in range(3)]
        finally:
            setattr(A.ops, name, orig)
        torch.cuda.synchronize()
        return outs, opt.flat_p.clone(), len(used)

    try:
        (o1, p1, n1), (o0, p0, n0) = run(True), run(False)
    finally:
        A.ops.set_compute("bf16")
    # the first step builds the optimizer's flat buffers on the per-problem paths; the grouped ones run from the second on
    assert n0 == 0 and (n1 == 2 if what == "grouped_heads" else n1 >= 4), (n0, n1)
    for (t1, v1), (t0, v0) in zip(o1, o0):
        torch.testing.assert_close(t1, t0, rtol=2e-3, atol=2e-3)
        for k in v0:
            torch.testing.assert_close(v1[k], v0[k], rtol=2e-2, atol=2e-2)
    rel = float((p1 - p0).norm() / p0.norm())
    assert rel < 2e-3, rel


@pytest.mark.parametrize("residual", [True, False])
def test_graphone_stages_of_all_tasks_as_one_grouped_chain(A, residual, monkeypatch):
    """GraphONE.interact inside engine.EgoPackStep with the stages of the three auxiliary tasks as ONE chain of grouped launches
    (ops.graphone_stages) against the same step with one chain per task (EGK_DISABLE=graphone_grouped): loss vector, logits
    and every parameter after 3 Adam steps (bf16 mode: same kernel bodies with other tile variants -> f32 accumulation-order
    noise, then bf16 rounding).  The per-task interaction is the one the reference-control-flow fixtures pin."""
    import argparse
    import bench
    from egopack_amd.models.graphONE.graphONE import GraphONE

    def run(grouped):
        if grouped:
            monkeypatch.delenv("EGK_DISABLE", raising=False)
        else:
            monkeypatch.setenv("EGK_DISABLE", "graphone_grouped")
        args = argparse.Namespace(hidden=256, trn_hidden=256, dropout=0.0, compute="bf16", workload="egopack_oscc", batch=8, T=16)
        A.ops.set_compute("bf16")
        A.ops.manual_seed(11)
        model, tasks, crit, weights, dev, merged = bench.build_workload(args, 0, torch.device(DEV))
        model.to(DEV).train()
        for t in tasks.values():
            t.to(DEV).train()
        gen = torch.Generator(device=DEV)
        gen.manual_seed(7)
        banks = {t: torch.randn(96, 256, device=DEV, generator=gen) for t in ("ar", "lta", "pnr")}
        torch.manual_seed(5)
        gone = GraphONE(banks, features_size=256, hidden_size=256, k=4, depth=2, residual=residual).to(DEV)
        params = [*model.parameters(), *(p for t in tasks.values() for p in t.parameters()), *gone.parameters()]
        opt = A.FlatAdam(params, lr=1e-3, weight_decay=1e-5)
        step = A.engine.EgoPackStep(model, tasks, gone, weights, opt, backprop_temporal_graph=True, temporal_graph_train_mode=False)
        before = {k: v.clone() for k, v in gone.state_dict().items()}
        used = []
        orig = A.ops.graphone_stages

        def spy(*a, **k):
            used.append(1)
            return orig(*a, **k)
        A.ops.graphone_stages = spy
        try:
            outs = [step.step(dev, merged) for _ in range(3)]
        finally:
            A.ops.graphone_stages = orig
        torch.cuda.synchronize()
        return outs, opt.flat_p.clone(), len(used), before, {k: v.clone() for k, v in gone.state_dict().items()}

    try:
        (o1, p1, n1, b1, g1), (o0, p0, n0, b0, g0) = run(True), run(False)
    finally:
        A.ops.set_compute("bf16")
    # the first step builds the optimizer's flat buffers on the per-task path; the grouped chain runs from the second on
    assert n0 == 0 and n1 == 2, (n0, n1)
    for (t1, v1), (t0, v0) in zip(o1, o0):
        torch.testing.assert_close(t1, t0, rtol=2e-3, atol=2e-3)
        for k in v0:
            torch.testing.assert_close(v1[k], v0[k], rtol=2e-2, atol=2e-2)
    assert float((p1 - p0).norm() / p0.norm()) < 2e-3
    for k in g0:  # GraphONE's own parameters: trained by both paths, by the same amounts (Adam: three steps of ~lr each)
        assert torch.equal(b1[k], b0[k])
        if "embeddings" in k:
            assert torch.equal(g1[k], b1[k]) and torch.equal(g0[k], b0[k])  # (frozen banks)
            continue
        d1, d0 = (g1[k] - b1[k]).float(), (g0[k] - b0[k]).float()
        assert float(d0.norm()) > 0, k
        assert float((d1 - d0).norm() / d0.norm()) < 0.1, (k, float((d1 - d0).norm() / d0.norm()))


def test_parked_weight_gradients_survive_an_aliased_backward_stream(A):
    """Pooled HIP stream handles are reused: the backward stream of a step (a graph-capture stream) can carry a handle that
    an earlier step registered as a task-head stream.  Work parked for the grouped weight-gradient launch must still be
    issued by the step's own end-of-backward join (regression: it was skipped, the norm layers then trained on zero
    gradients).  Here the backward stream itself is registered as excluded; the parameters after 3 steps must equal the
    normal run's."""
    import argparse
    import bench

    def run(alias):
        args = argparse.Namespace(hidden=256, trn_hidden=256, dropout=0.0, compute="bf16", workload="mtl", batch=8, T=16)
        A.ops.set_compute("bf16")
        A.ops.manual_seed(11)
        model, tasks, crit, weights, dev, merged = bench.build_workload(args, 0, torch.device(DEV))
        model.to(DEV).train()
        for t in tasks.values():
            t.to(DEV).train()
        params = [*model.parameters(), *(p for t in tasks.values() for p in t.parameters())]
        opt = A.FlatAdam(params, lr=1e-3, weight_decay=1e-5)
        step = A.engine.MTLStep(model, tasks, crit, weights, opt, fused_backbone=True)
        st = torch.cuda.Stream()
        key = A.sched.stream_key(st)
        if alias:
            A.sched._wgrad.exclude.add(key)
        try:
            st.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(st):
                for _ in range(3):
                    step.step(dev, merged)
            torch.cuda.current_stream().wait_stream(st)
            torch.cuda.synchronize()
        finally:
            A.sched._wgrad.exclude.discard(key)
        return opt.flat_p.clone()

    try:
        p_alias, p_ref = run(True), run(False)
    finally:
        A.ops.set_compute("bf16")
    rel = float((p_alias - p_ref).norm() / p_ref.norm())
    assert rel < 2e-3, rel
    # the norm layers' parameters in particular moved as in the reference run
    assert torch.isfinite(p_alias).all()


def test_backbone_with_epilogue_layernorm_statistics_equals_the_two_pass_layernorm(A):
    """models.Graph forward + backward with the graph LayerNorm's segment sums taken in the producing contractions'
    epilogues (ops._ln_fusion on, the default) against the same pass with every LayerNorm running its own statistics
    launches: features and every parameter gradient (bf16 mode, H = 256, three task segments of unequal length)."""
    torch.manual_seed(0)
    trn = {"_target_": "egopack_amd.models.temporal_pooling.trn_pooling.TRNPooling", "dropout": 0.0, "hidden_size": 256}
    m = A.Graph(128, hidden_size=256, depth=3, temporal_pooling=trn, num_segments=3).to(DEV)
    parts = []
    for t, n, T in (("ar", 8, 16), ("lta", 6, 40), ("pnr", 10, 16)):
        ds = A.data.SyntheticTaskDataset(t, n, T, 3, 128, k=1, seed=9)
        parts.append(A.data.collate([ds[i] for i in range(n)]))
    merged = A.data.merge_batches(parts).to(DEV)
    assert merged.min_seg_rows == 128
    merged.x = [p.x.to(DEV) for p in parts]
    w = torch.randn(merged.pos.shape[0], 256, device=DEV)
    res = {}
    for on in (True, False):
        A.ops._ln_fusion["on"] = on
        try:
            m.zero_grad()
            with A.ops.compute_mode("bf16"):
                out = m(merged)
                (out.float() * w).sum().backward()
            res[on] = (out.detach().float().clone(), {k: p.grad.clone() for k, p in m.named_parameters()})
        finally:
            A.ops._ln_fusion["on"] = True
    rel = lambda a, b: float((a - b).norm() / b.norm().clamp(min=1e-12))
    assert rel(res[True][0], res[False][0]) < 1e-2
    for k in res[False][1]:
        assert rel(res[True][1][k], res[False][1][k]) < 3e-2, k


# ---- RelationModuleMultiScale: pinned by the reference class itself (tests/golden/trn_multiscale.pt) -----------------------
@pytest.mark.parametrize("mode,otol,gtol", [("f32", 2e-5, 1e-4), ("bf16", 2e-2, 6e-2)])
def test_relation_module_multiscale_vs_reference(A, golden, mode, otol, gtol):
    """Forward output, input gradient and every parameter gradient of the multi-scale relation module against the reference's
    own class (models/TRN.py:9-74) on its own seeded parameters: f32 mode to summation order (largest deviation relative to
    the largest magnitude of each tensor), bf16 mode to operand rounding (relative L2 distance).  Also as a step under FlatAdam: the weight gradients land in the
    optimizer's flat buffer."""
    from egopack_amd.models.trn_multiscale import RelationModuleMultiScale
    for c in golden("trn_multiscale")["cases"]:
        m = RelationModuleMultiScale(c["img_feature_dim"], c["num_bottleneck"], c["num_frames"])
        m.load_state_dict(c["state_dict"])
        m.to(DEV)
        x = c["x"].to(DEV).requires_grad_(True)
        with A.ops.compute_mode(mode):
            out = m(x)
            assert out.shape == c["out"].shape
            (out.float() * c["cot"].to(DEV)).sum().backward()
        torch.cuda.synchronize()

        def rel(a, b):
            d = a.float().cpu() - b
            if mode == "bf16":  # (a ReLU whose pre-activation rounds across zero flips one whole gradient row: norm-wise)
                return float(d.norm() / b.norm().clamp(min=1e-12))
            return float(d.abs().max() / b.abs().max().clamp(min=1e-12))
        assert rel(out.detach(), c["out"]) <= otol, (c["num_frames"], rel(out.detach(), c["out"]))
        assert rel(x.grad, c["dx"]) <= gtol, (c["num_frames"], "dx", rel(x.grad, c["dx"]))
        for k, p in m.named_parameters():
            assert rel(p.grad, c["grads"][k]) <= gtol, (c["num_frames"], k, rel(p.grad, c["grads"][k]))
    # under the flat optimizer: gradients accumulate into the flat buffer, one Adam launch moves every scale's layer
    c = golden("trn_multiscale")["cases"][0]
    m = RelationModuleMultiScale(c["img_feature_dim"], c["num_bottleneck"], c["num_frames"])
    m.load_state_dict(c["state_dict"])
    m.to(DEV)
    opt = A.FlatAdam(m.parameters(), lr=1e-2)
    with A.ops.compute_mode("f32"):
        for _ in range(2):
            opt.zero_grad()
            (m(c["x"].to(DEV)).float() * c["cot"].to(DEV)).sum().backward()
            A.ops.join_wgrad(force=True)
            opt.step()
    torch.cuda.synchronize()
    # (Adam's first update is -lr * sign(g): every weight with a gradient moved against the golden gradient's sign)
    w = m.fc_fusion_scales[0][1].weight
    g0 = c["grads"]["fc_fusion_scales.0.1.weight"]
    moved = (c["state_dict"]["fc_fusion_scales.0.1.weight"] - w.detach().cpu())
    assert (torch.sign(moved[g0.abs() > 1e-6]) == torch.sign(g0[g0.abs() > 1e-6])).float().mean() > 0.99


@pytest.mark.parametrize("encoding", ["positional", "temporal", "learnt"])
@pytest.mark.parametrize("level", ["frame", "action"])
def test_temporal_pooling_encodings_follow_the_reference_base_class(A, encoding, level):
    """``TemporalPooling.apply_positional_embedding`` (reference models/temporal_pooling/pooling.py:64-83; not reached by
    TRNPooling, which passes no encoding): the reference's control flow restated on the CPU in f32 -- PyG's two encodings from
    their published definitions, the per-batch-id loop of the 'action' level as written -- against the HIP path."""
    from egopack_amd.models.temporal_pooling.pooling import TemporalPooling
    torch.manual_seed(7)
    S, F, N = 3, 64, 40
    m = TemporalPooling(F, F, S, encoding, level)
    if encoding == "learnt" and level == "action":
        assert m.encoding is None and m.encoding_mlp is None  # (the reference warns and uses no encoding)
        x = torch.randn(N, S, F)
        assert m.apply_positional_embedding(x, None, None) is x
        return
    x = torch.randn(N, S, F)
    batch = torch.arange(0, N // 4).repeat_interleave(4)
    pos = torch.arange(0, 4).repeat(N // 4) - 1
    W, b = m.encoding_mlp.weight.detach().clone(), m.encoding_mlp.bias.detach().clone()

    def enc_rows(p):
        p = p.float().view(-1, 1)
        if encoding == "positional":
            f = torch.logspace(0, 1, F // 2, 1e-4).view(1, -1)
            return torch.cat([torch.sin(p * f), torch.cos(p * f)], -1)
        if encoding == "temporal":
            w = (1.0 / 10 ** torch.linspace(0, 9, F)).view(1, -1)
            return (1.0 / F) ** 0.5 * torch.cos(p * w)
        raise AssertionError
    if level == "frame":
        rows = m.encoding.detach().clone() if encoding == "learnt" else enc_rows(torch.arange(0, S))
        ref = x + (rows @ W.t() + b).unsqueeze(0)
    else:
        ref = torch.zeros_like(x)
        for bid in batch.unique():  # (as the reference writes it)
            sel = batch == bid
            ref[sel] = x[sel] + (enc_rows(pos[sel]) @ W.t() + b).unsqueeze(1)
    m.to(DEV)
    with A.ops.compute_mode("f32"):
        got = m.apply_positional_embedding(x.to(DEV), batch.to(DEV), pos.to(DEV))
    torch.testing.assert_close(got.float().cpu(), ref, rtol=1e-4, atol=1e-4)
