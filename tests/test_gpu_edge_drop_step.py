"""DropEdge inside ``engine.MTLStep``, at the sizes of tests/test_gpu_mixup_step.py (its builders are imported):
hidden 64, B = 4 sequences per task, T = 5 nodes, AR + LTA + PNR.

* captured == eager bit for bit over three steps, f32 and bf16, ONE capture and fresh masks in every replay: replay k draws at the
  host offsets baked into the graph plus the device word k * 2^40, so the eager run issues its step k at that stream state
  (``ops.rng_replay`` at the capture's position, the word set by hand) -- the comparison of tests/test_gpu_dropout_masks.py;
* the same with grad_clip_norm, EMA and mixup on together;
* ``per_layer: false`` gives all layers one recorded (seed, offset), ``true`` gives each its own, rows + 64 counters apart;
* ``model.eval()`` and p = 0 issue exactly the launches of a step without the attribute (the profile ledger), a dropping step swaps
  one gather per layer and direction for a ``csr_mean_drop`` launch;
* main_temporal.py edge_drop.p=0.2 trains, logs one line per epoch, and resumed after an interruption equals the uninterrupted run;
* main_egopack.py edge_drop.p=0.2 is refused."""
import logging

import pytest
import torch

from tests import edge_drop_common as EC
from tests import step_matrix_common as M
from tests.test_gpu_mixup_step import build, same, set_fields, snapshot

pytestmark = pytest.mark.gpu

DEV = "cuda"


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


@pytest.fixture
def compute_restored():
    from egopack_amd import ops
    before = ops.get_compute()
    yield
    ops.set_compute(before)


def with_drop(step, p=0.2, per_layer=True, **kw):
    from egopack_amd import ops
    assert hasattr(step.model, "edge_drop") and step.model.edge_drop is None
    step.model.edge_drop, step.model.edge_drop_per_layer = ops.EdgeDrop(p, **kw), per_layer
    return step


CLIP_EMA = ["grad_clip_norm=0.05", f"ema.decay={M.EMA_DECAY}", "ema.warmup=true"]


@pytest.mark.parametrize("compute,over,mixup", [("f32", (), False), ("bf16", (), False), ("bf16", tuple(CLIP_EMA), True)],
                         ids=["f32", "bf16", "bf16-clip-ema-mixup"])
def test_captured_equals_eager_over_three_steps_with_fresh_masks(compute, over, mixup, compute_restored):
    from egopack_amd import ops
    STRIDE = ops.RNG_DEVICE_STRIDE
    words = {}

    def fields(dev, k):
        if mixup:
            set_fields(dev, k)

    def run(graph):
        step, opt, dev, merged = build(compute, over)
        with_drop(step)
        word = ops.rng_device_offset(torch.device(DEV, torch.cuda.current_device()))  # (the word the step's launches read)
        for k in range(2):  # two eager steps first, in both runs (a capture needs the flat buffers and the learnt slots)
            fields(dev, k)
            step.step(dev, merged)
        snap = ops.rng_snapshot()  # the host position the captured step's launches are baked at
        tap, recs = ops.tap_dropout_masks(), []
        if graph:
            with tap:
                step.capture(dev, merged, warmup=0)
            recs += tap.launches
        for k in range(3):
            fields(dev, 2 + k)
            if graph:
                torch.cuda.synchronize()
                assert int(word.item()) == k * STRIDE, "the word moves one stride per replay"
                step.replay()
            else:
                word.fill_(k * STRIDE)
                with ops.rng_replay(snap), tap:
                    step.step(dev, merged)
                recs += tap.launches
        out = snapshot(step, opt)
        out["loss_sums"] = step.loss_sums()
        if graph:
            assert step.captures == 1, "fresh masks are a device word, not a new capture"
        edges = [r for r in recs if r[0] == "edge"]
        assert len(edges) == (3 if graph else 9) and all(r[2] >= snap for r in edges), edges
        words[graph] = edges[:3]
        assert bool(torch.isfinite(out["flat_p"]).all())
        return out, merged
    (eager, merged), (graph, _) = run(False), run(True)
    assert eager["t"] == graph["t"] == 5
    assert words[True] == words[False], "the captured step's launches are baked at the offsets the eager step draws there"
    same(graph, eager)
    # fresh masks: the host model of one layer's launch at the three words gives three different edge sets
    g = getattr(merged, "graph", None)
    _, seed, off, rows, E = words[True][0]
    if g is not None and g.num_nodes == rows:
        keeps = [EC.keep_edges(EC.rows_of(g.rowptr.cpu().numpy()), g.col.cpu().numpy(), seed, off, 0.2, True, True, k * STRIDE)
                 for k in range(3)]
        assert not (keeps[0] == keeps[1]).all() and not (keeps[1] == keeps[2]).all()


@pytest.mark.parametrize("per_layer", [True, False])
def test_per_layer_false_gives_all_layers_one_seed_and_offset(per_layer, compute_restored):
    from egopack_amd import ops
    step, opt, dev, merged = build("bf16")
    with_drop(step, per_layer=per_layer)
    tap = ops.tap_dropout_masks()
    with tap:
        step.step(dev, merged)
    torch.cuda.synchronize()
    edges = [r for r in tap.launches if r[0] == "edge"]
    depth = step.model.depth
    assert len(edges) == depth == 3 and len({r[3:] for r in edges}) == 1
    if per_layer:
        rows = edges[0][3]
        assert [r[2] - edges[0][2] for r in edges] == [k * EC.reserved(rows) for k in range(depth)], edges
    else:
        assert len({r[1:3] for r in edges}) == 1, edges


def _ledger(setup):
    from egopack_amd import ops
    step, opt, dev, merged = build("bf16", batch=8, t_nodes=8)
    setup(step)
    for _ in range(2):
        step.step(dev, merged)
    torch.cuda.synchronize()
    ops.prof_enable(True)
    ops.prof_reset()
    try:
        step.step(dev, merged)
        torch.cuda.synchronize()
        return {name: line["launches"] for name, line in ops.prof_report().items() if line["launches"]}
    finally:
        ops.prof_enable(False)


def test_eval_and_p_zero_issue_the_launches_of_today(compute_restored):
    from egopack_amd import ops

    def evaluating(step):
        with_drop(step)
        step.model.eval()

    def evaluating_plain(step):
        step.model.eval()
    off = _ledger(lambda step: None)
    assert "csr_mean_drop" not in off and off.get("csr_gather", 0) >= 6, off
    assert _ledger(lambda step: with_drop(step, p=0.0)) == off, "p = 0"
    assert _ledger(evaluating) == _ledger(evaluating_plain), "eval mode never drops"
    on = _ledger(with_drop)
    assert on.get("csr_mean_drop") == 6, (on, "three layers, forward and backward")
    assert on.get("csr_gather", 0) == off["csr_gather"] - 6
    assert {k: v for k, v in on.items() if k not in ("csr_mean_drop", "csr_gather")} == {k: v for k, v in off.items() if k != "csr_gather"}


# ---- the entry points ----------------------------------------------------------------------------------------------------------------
BASE = ["k=1", "batch_size=4", "synthetic_samples=16", "model.hidden_size=64", "model.temporal_pooling.hidden_size=64", "oscc_feat_size=64",
        "save_model=True", "compute=f32", "optimizer.lr=1e-3", "enabled_tasks=[ar,lta,pnr]", "lr_scheduler.T_max=3", "use_graph=false",
        "edge_drop.p=0.2"]


@pytest.mark.timeout(600)
def test_main_temporal_trains_with_edge_drop_and_a_resumed_run_equals_the_uninterrupted_one(tmp_path, caplog):
    import main_temporal
    with caplog.at_level(logging.INFO):
        main_temporal.main(BASE + ["num_epochs=2", "save_every=1", f"checkpoint_dir={tmp_path / 'full'}"])
    lines = [r.getMessage() for r in caplog.records if "edge_drop p" in r.getMessage()]
    assert len(lines) == 2 and all("p 0.2 symmetric True keep_self True per_layer True" in l for l in lines), lines
    main_temporal.main(BASE + ["num_epochs=1", "save_every=1", f"checkpoint_dir={tmp_path / 'part'}"])
    name = "MTL_ar-lta-pnr"
    part = tmp_path / "part" / name / "checkpoint.pth"
    assert torch.load(part, weights_only=False)["epoch"] == 1
    main_temporal.main(BASE + ["num_epochs=2", f"checkpoint_dir={tmp_path / 'resumed'}", f"resume_from={part}"])
    full = torch.load(tmp_path / "full" / name / "checkpoint.pth", weights_only=False)
    res = torch.load(tmp_path / "resumed" / name / "checkpoint.pth", weights_only=False)
    assert res["epoch"] == 2 and not any("edge_drop" in k for k in full["temporal_graph"])
    for key in ("temporal_graph", "task/recognition", "task/lta", "task/pnr"):
        for k, v in full[key].items():
            torch.testing.assert_close(res[key][k], v, rtol=0, atol=0, msg=lambda s: f"{key}.{k}: {s}")


def test_main_egopack_refuses_edge_drop():
    import main_egopack
    with pytest.raises(ValueError, match=r"edge_drop\.p = 0\.2 with enable_graphone=True \(main_egopack\.py\)"):
        main_egopack.main(["edge_drop.p=0.2", "enable_graphone=True", "enabled_tasks=[oscc]", "k=1", "batch_size=4", "synthetic_samples=16"])
