"""CPU tests of the host-side logic: edge builders, CSR construction, collation, the multi-task
loader (vs the reference's own outputs in tests/golden/edges_loader.pt), the Hydra-compatible config
loader, and the loud failure of the product path without a GPU."""
import sys
from pathlib import Path

import pytest
import torch

from egopack_amd import data as D
from oracle import path as O
from oracle import pyg_ops as P

REPO = Path(__file__).resolve().parents[1]


@pytest.mark.parametrize("name", ["lta_T22", "lta_T22_verb0", "lta_T8_verb0_first", "lta_T12_r2.5"])
def test_lta_connectivity_bit_exact_vs_reference(golden, name):
    c = golden("edges_loader")[name]
    assert torch.equal(D.lta_connectivity_edges(c["pos"], c["y"], c["r"]), c["edge_index"])
    d = D.LTATemporalConnectivity(r=c["r"])(D.Data(x=torch.zeros(c["pos"].shape[0], 1), pos=c["pos"], y=c["y"], batch=None))
    assert torch.equal(d.edge_index, c["edge_index"])


def test_lta_transform_rejects_batched_graphs():
    with pytest.raises(ValueError):
        D.LTATemporalConnectivity(r=1.5)(D.Data(pos=torch.arange(3), y=torch.zeros(3, 2), batch=torch.zeros(3)))


@pytest.mark.parametrize("T,k", [(9, 1), (32, 1), (4, 2), (1, 1), (40, 2)])
def test_radius_band_matches_oracle_set(T, k):
    pos = torch.arange(T) - T // 2
    mine = D.radius_band_edges(pos, k)
    ref = O.temporal_radius_edges(pos, k)
    assert torch.equal(mine, ref)
    assert mine.shape[1] == max(0, 2 * k * T - k * (k + 1)) if T > k else True


def test_multiloader_restart_semantics_vs_reference(golden):
    G = golden("edges_loader")["multiloader"]
    seq = [tuple(x) for x in D.multiloader([[1, 2, 3], [10, 20], None, [7]], [1.0, 1.0, 1.0, 1.0])]
    assert seq == G["case1"]
    seq2 = [tuple(x) for x in D.multiloader([[1, 2], [10, 20, 30], [5], [7]], [1.0, 0.0, 1.0, 1.0])]
    assert seq2 == G["case2"]


def test_build_csr_both_orientations():
    ei = torch.tensor([[1, 0, 2, 1, 3, 1], [0, 1, 1, 2, 2, 3]])
    g = D.build_csr(ei, 5)  # node 4 isolated
    assert g.rowptr.tolist() == [0, 1, 3, 5, 6, 6]
    assert g.col.tolist() == [1, 0, 2, 1, 3, 1]
    assert g.t_rowptr.tolist() == [0, 1, 4, 5, 6, 6]
    assert g.t_col.tolist() == [1, 0, 2, 3, 1, 2]
    torch.testing.assert_close(g.t_wgt, torch.tensor([0.5, 1.0, 0.5, 1.0, 0.5, 0.5]))
    assert g.rowptr.dtype == torch.int32 and g.col.dtype == torch.int32
    # CSR mean == oracle scatter mean (host check of the index structure)
    x = torch.randn(5, 3)
    agg = torch.stack([x[g.col[g.rowptr[i]:g.rowptr[i + 1]].long()].mean(0) if g.rowptr[i + 1] > g.rowptr[i] else torch.zeros(3)
                       for i in range(5)])
    torch.testing.assert_close(agg, P.scatter_mean(x[ei[0]], ei[1], 5))


def test_collate_matches_oracle_collate_and_merge_segments():
    ds_ar = D.SyntheticTaskDataset("ar", 3, 9, 3, 8, (7, 11), k=1, seed=5)
    ds_lta = D.SyntheticTaskDataset("lta", 2, 12, 3, 8, (7, 11), k=1, seed=5)
    a = D.collate([ds_ar[i] for i in range(3)])
    ref = P.collate([ds_ar[i] for i in range(3)])
    for k in ("x", "y", "pos", "edge_index", "batch", "ptr"):
        assert torch.equal(getattr(a, k), getattr(ref, k)), k
    assert a.num_graphs == 3 and a.ptr32.dtype == torch.int32
    assert (a.y[:, 0] != -1).sum() == 3  # AR: only the centre node of each sequence is labelled
    b = D.collate([ds_lta[i] for i in range(2)])
    assert (b.y[:2] == -1).all() and (b.y[2:12, 1] >= 0).all()
    m = D.merge_batches([a, b])
    assert m.seg_ptr.tolist() == [0, 27, 51] and isinstance(m.x, list) and len(m.x) == 2
    assert m.graph.num_nodes == 51 and m.pos.shape[0] == 51
    assert int(m.edge_index[:, a.edge_index.shape[1]:].min()) >= 27  # second block offset by the first block's nodes
    oscc = D.collate([D.SyntheticTaskDataset("oscc", 4, 4, 3, 8)[i] for i in range(4)])
    assert oscc.y.shape == (4,) and oscc.y.dtype == torch.int64
    pnr = D.collate([D.SyntheticTaskDataset("pnr", 2, 16, 3, 8)[i] for i in range(2)])
    assert pnr.y.view(2, 16).sum(1).tolist() == [1, 1]


def test_batch_loader_sharding_is_disjoint_and_equal():
    ds = D.SyntheticTaskDataset("ar", 37, 5, 3, 4, (7, 11))
    seen = []
    lens = []
    for r in range(2):
        dl = D.BatchLoader(ds, 4, shuffle=True, drop_last=True, seed=3, rank=r, world_size=2)
        idx = dl._indices()
        seen.append(set(idx))
        lens.append(len(dl))
        assert sum(1 for _ in dl) == len(dl)
    assert seen[0].isdisjoint(seen[1]) and len(seen[0]) == len(seen[1]) == 18
    assert lens[0] == lens[1] == 4  # same number of steps on every rank (all-reduce would deadlock otherwise)


def test_config_compose_overrides_interpolation_and_instantiate():
    from egopack_amd.config import compose, instantiate
    cfg = compose(REPO / "configs", "defaults", ["k=1", "batch_size=16", "num_epochs=40", "model/temporal_pooling=trn",
                                                  "model.temporal_pooling.hidden_size=1024", "model.hidden_size=1024",
                                                  "enabled_tasks=[ar,lta,pnr]"])
    assert cfg.k == 1 and cfg.batch_size == 16 and cfg.enabled_tasks == ["ar", "lta", "pnr"]
    assert cfg.lr_scheduler.T_max == 40  # ${num_epochs}
    assert cfg.model._target_ == "models.graph.Graph" and cfg.model.depth == 3
    assert cfg.model.temporal_pooling._target_ == "models.temporal_pooling.trn_pooling.TRNPooling"
    assert cfg.model.temporal_pooling.hidden_size == 1024 and cfg.model.temporal_pooling.dropout == 0.5
    assert cfg.graphone.k == 8 and cfg.optimizer._target_ == "torch.optim.Adam"
    model = instantiate(cfg.model, input_size=48, num_segments=3, _recursive_=False)
    import models.graph
    assert isinstance(model, models.graph.Graph)
    assert model.temporal_pooling.proj[0].in_features == 3 * 48
    opt = instantiate(cfg.optimizer, [torch.nn.Parameter(torch.zeros(2))])
    assert isinstance(opt, torch.optim.Adam) and opt.defaults["weight_decay"] == 1e-5


def test_reference_module_paths_resolve_to_the_mirror():
    """The YAML _target_ paths and import paths of the reference resolve to this implementation."""
    import criterion.wrapper
    import graphone
    import models.graphONE.graphONE
    import models.tasks
    import models.temporal_pooling.trn_pooling
    import models.transforms.lta_temp_connectivity
    import utils.dataloading
    from egopack_amd.models.graph import Graph
    import models.graph
    assert models.graph.Graph is Graph
    assert hasattr(models.tasks, "RecognitionTask") and hasattr(models.tasks, "PNRTask")
    assert callable(graphone.build_graphone) and callable(utils.dataloading.multiloader)
    assert hasattr(models.TRN, "RelationModuleMultiScale") if hasattr(models, "TRN") else True


def test_state_dict_layout_matches_reference_checkpoints(golden):
    from egopack_amd.models import Graph
    from egopack_amd.models.graphONE.graphONE import GraphONE
    from egopack_amd.models.tasks import LTATask, OSCCTask, PNRTask, RecognitionTask
    trn = {"_target_": "models.temporal_pooling.trn_pooling.TRNPooling", "dropout": 0.0, "hidden_size": 40}
    g = Graph(48, hidden_size=32, depth=3, temporal_pooling=trn, num_segments=3)
    G = golden("egopack_train")["before"]
    assert list(g.state_dict().keys()) == list(G["temporal_graph"].keys())
    g.load_state_dict(G["temporal_graph"])
    ar = RecognitionTask(32, 32, (7, 11), aux_tasks=("oscc", "lta", "pnr"))
    assert list(ar.state_dict().keys()) == list(G["task/recognition"].keys())
    assert list(OSCCTask(32, 32, aux_tasks=("ar", "lta", "pnr"), average_logits=True).state_dict().keys()) == list(G["task/oscc"].keys())
    assert list(LTATask(32, 32, (7, 11), aux_tasks=("ar", "oscc", "pnr")).state_dict().keys()) == list(G["task/lta"].keys())
    assert list(PNRTask(32, 32, aux_tasks=("ar", "oscc", "lta")).state_dict().keys()) == list(G["task/pnr"].keys())
    banks = {t: G["graphone"][f"embeddings.{t}.weight"] for t in ("ar", "lta", "pnr")}
    go = GraphONE(banks, features_size=32, hidden_size=32, k=4, depth=2, residual=True, dropout=0, output_dropout=0,
                  output_projection=True)
    assert list(go.state_dict().keys()) == list(G["graphone"].keys())
    assert go.task_labels == ["ar", "lta", "pnr"]
    # what graphone.build_graphone introspects (reference graphone.py:29-30)
    assert ar.net[-1].out_features == 32 and tuple(c[-1].out_features for c in ar.classifiers) == (7, 11)
    # mismatched checkpoints from the MTL phase load with strict=False (aux classifiers are new): main_egopack.py:292-295
    mtl = golden("mtl_train")["before"]["task/recognition"]
    res = ar.load_state_dict(mtl, strict=False)
    assert all(k.startswith("aux_classifiers.") for k in res.missing_keys) and not res.unexpected_keys


def test_product_path_fails_loudly_without_gpu():
    from egopack_amd import ops
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.row_layernorm(torch.randn(4, 8), torch.ones(8), torch.zeros(8))
    from egopack_amd.models.tasks import PNRTask
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        PNRTask(8, 8).forward_features(torch.randn(2, 8))
    from egopack_amd.optim import FlatAdam
    p = torch.nn.Parameter(torch.zeros(3))
    p.grad = torch.ones(3)
    with pytest.raises(RuntimeError, match="ROCm device"):
        FlatAdam([p]).step()


def test_product_never_imports_oracle():
    """The oracle is test infrastructure: nothing under egopack_amd/ or the top-level mirror imports it."""
    import re
    bad = []
    for root in ("egopack_amd", "models", "criterion", "utils"):
        for f in (REPO / root).rglob("*.py"):
            if re.search(r"^\s*(from|import)\s+oracle\b", f.read_text(), flags=re.M):
                bad.append(str(f))
    for f in ("graphone.py", "main_temporal.py", "main_egopack.py"):
        if (REPO / f).exists() and re.search(r"^\s*(from|import)\s+oracle\b", (REPO / f).read_text(), flags=re.M):
            bad.append(f)
    assert not bad, bad


@pytest.mark.timeout(120)
def test_batch_loader_worker_processes_deliver_the_in_process_batches_in_order():
    """``workers`` > 0: forked processes collate whole batches ahead (bounded in flight) and hand them back in order --
    for a dataset whose samples are a function of their index, exactly the in-process batches, shuffled epochs included."""
    from egopack_amd import data as D
    ds = D.SyntheticTaskDataset("lta", 37, 6, 3, 8, (5, 7), k=1, seed=3)
    ref = D.BatchLoader(ds, 4, shuffle=True, drop_last=False, seed=11)
    par = D.build_dataloader(ds, 4, True, 0, False, seed=11, workers=2)
    try:
        for _ in range(2):  # two epochs: the shuffle generator advances identically, the pool persists
            a, b = list(ref), list(par)
            assert len(a) == len(b) == 10
            for x, y in zip(a, b):
                assert torch.equal(x.x, y.x) and torch.equal(x.y, y.y) and torch.equal(x.edge_index, y.edge_index)
                assert torch.equal(x.graph.rowptr, y.graph.rowptr) and torch.equal(x.graph.t_col, y.graph.t_col)
        it = iter(par)  # a consumer that stops early leaves nothing hanging
        next(it)
        del it
    finally:
        par.close()


# ---- static-shape batches of the captured training step (engine.train_step) -------------------------------------------
def _lta_batch(seed, B=6, T=12):
    ds = D.SyntheticTaskDataset("lta", B, T, 3, 8, (7, 11), k=1, seed=seed)
    return D.collate([ds[i] for i in range(B)])


def test_merged_csr_is_the_concatenation_of_the_task_csrs():
    """merge_batches builds the merged CSR from the tasks' CSR arrays with offsets: identical, entry for entry, to
    build_csr over the merged edge list (stable sorts), heavy rows and modes included."""
    batches = []
    for t, T, seed in (("ar", 9, 1), ("lta", 40, 2), ("pnr", 16, 3), ("lta", 12, 4)):
        ds = D.SyntheticTaskDataset(t, 4, T, 3, 8, (7, 11), k=1, seed=seed)
        batches.append(D.collate([ds[i] for i in range(4)]))
    m = D.merge_batches(batches)
    ref = D.build_csr(m.edge_index, m.pos.shape[0])
    for f in ("rowptr", "col", "t_rowptr", "t_col", "t_wgt", "heavy", "t_heavy", "band"):
        a, b = getattr(m.graph, f), getattr(ref, f)
        assert a.dtype == b.dtype and torch.equal(a, b), f
    assert (m.graph.num_nodes, m.graph.heavy_mode, m.graph.t_heavy_mode) == (ref.num_nodes, ref.heavy_mode, ref.t_heavy_mode)
    assert m.graph.t_heavy.numel() > 0  # the T = 40 LTA fan-out rows are listed


def test_band_codes_name_exactly_the_rows_whose_neighbours_are_adjacent():
    """CSRGraph.band (egk_csr_gather_banded): bit 0 / 1 / 2 = neighbour i - 1 / i / i + 1 for rows whose CSR entries are an
    ascending subset of those, 0xFF for every other row; checked entry by entry against the CSR itself."""
    ds = D.SyntheticTaskDataset("lta", 3, 12, 3, 8, (7, 11), k=1, seed=5)
    b = D.collate([ds[i] for i in range(3)])
    loops = torch.arange(b.pos.shape[0]).repeat(2, 1)[:, ::5]  # a few self loops as well
    far = torch.tensor([[0, 7], [9, 2]])
    for ei in (b.edge_index, torch.cat([b.edge_index, loops], 1), torch.cat([b.edge_index, far], 1), torch.tensor([[1, 0, 2], [1, 1, 1]])):
        n = int(ei.max()) + 1
        g = D.build_csr(ei, n)
        for i in range(n):
            cols = g.col[g.rowptr[i]:g.rowptr[i + 1]].tolist()
            offs = [c - i for c in cols]
            banded = all(abs(o) <= 1 for o in offs) and offs == sorted(set(offs))
            code = int(g.band[i])
            assert (code != 0xFF) == banded, (i, cols, code)
            if banded:
                assert code == sum(1 << (o + 1) for o in offs), (i, cols, code)
    assert (D.build_csr(b.edge_index, b.pos.shape[0]).band == 0xFF).any()  # the LTA forecast nodes are general rows


def test_signature_is_stable_across_lta_batches_with_different_edge_counts():
    """the LTA edge count moves with the labels; the replay signature compares edge CAPACITIES and ignores the
    structure fingerprints, so fresh LTA batches keep replaying the captured step."""
    from egopack_amd import engine as E
    a, b = _lta_batch(11), _lta_batch(12)
    for x, k in ((a, 101), (b, 202)):
        x._struct_key = k
    # force different edge counts (drop one band edge of b) while staying in one capacity bucket
    b.edge_index = b.edge_index[:, 1:]
    b.graph = D.build_csr(b.edge_index, b.pos.shape[0])
    assert a.edge_index.shape != b.edge_index.shape
    assert E.batch_signature({"lta": a}) == E.batch_signature({"lta": b})
    c = _lta_batch(13, B=5)
    assert E.batch_signature({"lta": a}) != E.batch_signature({"lta": c})  # another node count is another signature


def test_copy_batch_values_tracks_the_structure_fingerprint_A_B_A():
    """sequence A, B, A through one set of static buffers -- the third copy must restore A's structure (the
    destination's fingerprint follows every full copy), and the padded edge arrays receive the first E entries."""
    from egopack_amd import engine as E
    A_, B_ = _lta_batch(21), _lta_batch(22)
    B_.edge_index = B_.edge_index[:, 2:]
    B_.graph = D.build_csr(B_.edge_index, B_.pos.shape[0])
    A_._struct_key, B_._struct_key = 7, 9
    static = E._clone_batch(A_, pad_edges=True)
    cap = E._edge_capacity(A_.edge_index.shape[1])
    assert static.edge_index.shape == (2, cap) and static.graph.col.shape == (cap,)
    static._struct_key = A_._struct_key
    for src in (B_, A_, A_, B_):
        E.copy_batch_values({"lta": static}, None, {"lta": src}, None)
        e = src.edge_index.shape[1]
        assert static._struct_key == src._struct_key
        assert torch.equal(static.edge_index[:, :e], src.edge_index)
        assert torch.equal(static.graph.rowptr, src.graph.rowptr) and torch.equal(static.graph.col[:e], src.graph.col)
        assert torch.equal(static.graph.t_wgt[:e], src.graph.t_wgt) and torch.equal(static.y, src.y)
    unknown = _lta_batch(23)  # no fingerprint: everything is copied and the destination forgets its own
    E.copy_batch_values({"lta": static}, None, {"lta": unknown}, None)
    assert static._struct_key == 0 and torch.equal(static.graph.rowptr, unknown.graph.rowptr)


def test_bench_gpus_n_spawns_n_ranks_and_propagates_failure():
    """``python bench.py --gpus N`` without a launcher environment starts N ranks itself (the driver's own command line),
    as child processes of a parent that never touches the GPU.  Without GPUs (this container) every rank must fail loudly
    and the parent must exit non-zero with no result line."""
    import subprocess
    import bench
    plan = bench.spawn_plan(2, ["--gpus", "2", "--steps", "3"], port=29431)
    assert plan[1:4] == ["-m", "torch.distributed.run", "--nnodes=1"] and "--nproc-per-node=2" in plan
    assert plan[plan.index("--master-addr") + 1] == "127.0.0.1" and plan[plan.index("--master-port") + 1] == "29431"
    assert plan[-5].endswith("bench.py") and plan[-4:] == ["--gpus", "2", "--steps", "3"]
    assert bench.parse_args([]).grad_compress == "none" and bench.parse_args([]).gpus == 1  # the entry points' exchange type
    if torch.cuda.is_available():
        pytest.skip("the failure leg needs a box without GPUs")
    r = subprocess.run([sys.executable, str(Path(bench.__file__)), "--gpus", "2", "--steps", "1", "--warmup", "0"],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode != 0
    assert r.stderr.count("bench.py needs a ROCm GPU") >= 2  # both ranks were started and both raised
    assert '"metric"' not in r.stdout


def test_bench_plain_run_takes_only_the_headline_and_full_keeps_the_legs():
    """A plain ``bench.py`` run times exactly --steps steps once and takes no other leg; ``--full`` takes the roofline,
    CPU-baseline and f32 legs and the repeated timed blocks, each still switchable off on its own."""
    import bench
    plain = bench.parse_args(["--steps", "7"])
    assert not plain.full and plain.steps == 7 and plain.min_timed_s == 0.0 and plain.dump_outputs is None
    assert plain.no_roofline and plain.no_cpu_baseline and plain.no_f32_leg
    full = bench.parse_args(["--full"])
    assert full.min_timed_s == 0.5 and not (full.no_roofline or full.no_cpu_baseline or full.no_f32_leg)
    some = bench.parse_args(["--full", "--no-roofline", "--min-timed-s", "0", "--dump-outputs", "out"])
    assert some.no_roofline and not some.no_cpu_baseline and some.min_timed_s == 0.0 and some.dump_outputs == "out"


def test_bench_dump_outputs_writes_f32_f64_and_a_fixed_parameter_sample(tmp_path):
    """``bench.dump_outputs``: the objective as f64, the loss vectors as f32, and the parameters as a fixed, seeded sample when
    they outnumber DUMP_PARAMS (the same indices every run), in full otherwise."""
    import numpy as np
    import bench
    flat = torch.arange(bench.DUMP_PARAMS + 1000, dtype=torch.float32)
    vectors = {"ar": torch.rand(6), "pnr": torch.rand(6, dtype=torch.float64)}
    for d in ("a", "b"):
        bench.dump_outputs(tmp_path / d, torch.tensor(2.5), vectors, flat)
    assert sorted(p.name for p in (tmp_path / "a").iterdir()) == ["loss_ar.npy", "loss_pnr.npy", "loss_total.npy", "params_sample.npy"]
    assert np.load(tmp_path / "a" / "loss_total.npy").dtype == np.float64 and float(np.load(tmp_path / "a" / "loss_total.npy")) == 2.5
    assert np.load(tmp_path / "a" / "loss_pnr.npy").dtype == np.float32
    s = np.load(tmp_path / "a" / "params_sample.npy")
    assert s.dtype == np.float32 and s.shape == (bench.DUMP_PARAMS,) and np.all(np.diff(s) > 0)  # sorted distinct indices
    assert np.array_equal(s, np.load(tmp_path / "b" / "params_sample.npy"))
    bench.dump_outputs(tmp_path / "c", torch.tensor(2.5), {}, flat[:10])
    assert np.array_equal(np.load(tmp_path / "c" / "params_sample.npy"), flat[:10].numpy())


# ---- whole-batch builders of the live loaders --------------------------------------------------------------
def _same_fields(a, b, skip=()):
    from egopack_amd import engine as E
    A, B = dict(E._walk(a)), dict(E._walk(b))
    keys = lambda m: {k for k in m if "._" not in k and k not in skip}
    assert keys(A) == keys(B), keys(A) ^ keys(B)
    for k in keys(A):
        if torch.is_tensor(A[k]):
            assert A[k].dtype == B[k].dtype and torch.equal(A[k], B[k]), k
        else:
            assert A[k] == B[k], k


@pytest.mark.parametrize("task", ["ar", "lta", "pnr", "oscc"])
@pytest.mark.parametrize("T,split", [(4, "train"), (9, "train"), (22, "val"), (32, "train")])
def test_resident_dataset_batch_builder_equals_collating_its_items(task, T, split):
    """``SyntheticResidentDataset.batch(chunk)`` (index matrices, labels, graph templates and CSR assembled for the whole batch
    with array arithmetic) is field for field ``collate([ds[i] for i in chunk])``, and consumes the sampling stream the same way."""
    import numpy as np
    mk = lambda: D.SyntheticResidentDataset(task, 40, T, seed=4, split=split, n_videos=3, frames=900)
    a, b = mk(), mk()
    for chunk in ([0, 1, 2, 3, 4, 5, 6, 7], [39, 3, 17], [12]):
        np.random.seed(21)
        ref = D.collate([a[i] for i in chunk])
        after_ref = np.random.rand()
        np.random.seed(21)
        got = D.collate_chunk(b, chunk)
        assert after_ref == np.random.rand()
        _same_fields(ref, got)


@pytest.mark.parametrize("task", ["ar", "lta", "pnr", "oscc"])
@pytest.mark.parametrize("T,split", [(4, "train"), (9, "train"), (22, "val"), (32, "train")])
def test_native_batch_builder_equals_the_numpy_builder_and_the_collated_items(task, T, split):
    """``SyntheticResidentDataset.batch`` is ONE native call (egk_host_build_batch: window rows on the dataset's
    own MT19937 stream, labels, positions, the batch graph from the samples' templates in both CSR orientations, band codes,
    heavy-row lists, labelled-row lists).  Field for field -- values, dtypes, shapes -- the numpy builder's batch and
    ``collate`` of the items, with the sampling stream left where they leave it; bad indices are refused."""
    import numpy as np
    mk = lambda: D.SyntheticResidentDataset(task, 40, T, seed=4, split=split, n_videos=3, frames=900)
    nat, vec, per = mk(), mk(), mk()
    vec.native_batches = False
    assert nat.native_batches
    for chunk in ([0, 1, 2, 3, 4, 5, 6, 7], [39, 3, 17], [12], [5, 5, 5], list(range(40))):
        a, b = nat.batch(chunk), vec.batch(chunk)
        _same_fields(b, a)
        _same_fields(D.collate([per[i] for i in chunk]), a)
        for k in ("y", "pos", "edge_index", "x_idx", "ptr32"):  # (edge_index: the first E columns of its [2, capacity] region)
            assert getattr(a, k).dtype == getattr(b, k).dtype and (k == "edge_index" or getattr(a, k).is_contiguous())
        for f in ("rowptr", "col", "t_rowptr", "t_col", "t_wgt", "band", "heavy", "t_heavy"):
            assert getattr(a.graph, f).dtype == getattr(b.graph, f).dtype, f
        assert (getattr(a, "live_ap", None), a.graph.heavy_mode, a.graph.t_heavy_mode) == (getattr(b, "live_ap", None), b.graph.heavy_mode, b.graph.t_heavy_mode)
    sa, sb, sp = nat.rng.get_state(), vec.rng.get_state(), per.rng.get_state()
    assert sa[2] == sb[2] == sp[2] and np.array_equal(sa[1], sb[1]) and np.array_equal(sa[1], sp[1])
    with pytest.raises((ValueError, IndexError)):
        nat.batch([0, 40])


def test_arena_batches_merge_and_pack_like_the_tensor_by_tensor_path():
    """The native builder writes a batch into ONE buffer (data.Arena) and hands out a lazy batch; ``merge_batches`` of such batches
    is one host call (egk_host_merge_batches) and ``to_device_packed`` one memcpy per batch.  Against the numpy builder + tensor-by-
    tensor merge + generic packing: the same fields (values, dtypes, shapes; edge-sized arrays at capacity in the static views), one
    layout signature for steps whose edge counts differ inside a capacity bucket, and no tensor view is built by the staging itself."""
    import numpy as np
    from egopack_amd.engine import structure_key
    tasks = ["ar", "lta", "pnr", "oscc"]
    mk = lambda t: D.SyntheticResidentDataset(t, 96, 16, seed=3, split="train", n_videos=4, frames=600)
    nat, vec = {t: mk(t) for t in tasks}, {t: mk(t) for t in tasks}
    rng = np.random.default_rng(0)
    sigs, keys = set(), set()
    for it in range(5):
        chunks = {t: rng.integers(0, 96, 32) for t in tasks}
        xa = [nat[t].batch(chunks[t]) for t in tasks]
        xb = [vec[t].batch_numpy(chunks[t]) for t in tasks]
        assert all(b.__dict__.get("_arena") is not None and "_fill" in b.__dict__ for b in xa)
        assert all(structure_key(b) == b.__dict__["_struct_key"] for b in xa)
        keys.add(structure_key(xa[1]))
        for b in xa + xb:
            b.x = torch.empty(0)
        ma, mb = D.merge_batches(xa), D.merge_batches(xb)
        assert ma.__dict__.get("_arena") is not None and mb.__dict__.get("_arena") is None
        for b in xa + xb + [ma, mb]:
            b.x = None
        fills = D.LazyData.fills
        pa = D.to_device_packed([*xa, ma], "cpu", pack_on_cpu=True)
        assert D.LazyData.fills == fills and all("_fill" in b.__dict__ for b in [*xa, ma, *pa])  # nothing was looked at
        pb = D.to_device_packed([*xb, mb], "cpu", pack_on_cpu=True)
        ref = pa[0]._blob
        assert all(p._blob is ref for p in pa) and ref.gsig is not None
        sigs.add((ref.gsig, ref.dev.shape))
        assert pa[0].num_graphs == 32 and "_fill" in pa[0].__dict__  # plain values are there without building the views
        for u, v in zip(pa, pb):
            _same_fields(v, u)
        for u, v in zip(ref.rebuild(ref.dev.clone(), True), pb[0]._blob.rebuild(pb[0]._blob.dev.clone(), True)):
            _same_fields(v, u)  # static views: capacity shapes
        _same_fields(mb, ma)
    # LTA's edge count moves with the labels of a batch, the capacity bucket does not; the structure fingerprints do differ
    assert len(sigs) == 1 and len(keys) == 5
    # a batch of another size is another layout; an index out of range is refused before anything is written
    assert nat["ar"].batch([1, 2, 3])._arena.layout is not xa[0]._arena.layout
    with pytest.raises(ValueError):
        nat["ar"].batch([0, 96])


def test_pack_data_round_trip_is_one_buffer_per_batch():
    b = _lta_batch(31)
    buf, spec = D.pack_data(b)
    assert buf.dtype == torch.uint8 and buf.dim() == 1
    _same_fields(b, D.unpack_data(buf, spec))


def test_packed_transfer_layout_lazy_views_and_static_rebuild():
    """``to_device_packed`` on its CPU stand-in: the returned (lazy) batches equal the originals, edge-sized arrays occupy their
    CAPACITY in the buffer so that LTA batches with different edge counts share ONE layout signature, attributes assigned before
    the first use survive it, and ``rebuild(buffer, static=True)`` gives capacity-shaped views that take the next batch with one
    buffer copy (what engine.StepBase.train_step does per replayed step)."""
    from egopack_amd import engine as E
    a, b = _lta_batch(41), _lta_batch(42)
    b.edge_index = b.edge_index[:, 3:]
    b.graph = D.build_csr(b.edge_index, b.pos.shape[0])
    oa, ob = (D.to_device_packed([x, _lta_batch(43)], "cpu", pack_on_cpu=True) for x in (a, b))
    ra, rb = oa[0]._blob, ob[0]._blob
    assert ra is oa[1]._blob and ra.gsig is not None and ra.gsig == rb.gsig and ra.dev.shape == rb.dev.shape
    assert "_fill" in oa[0].__dict__  # nothing built yet
    oa[0].marker = torch.arange(3)
    _same_fields(a, oa[0], skip=(".marker",))
    assert "_fill" not in oa[0].__dict__ and torch.equal(oa[0].marker, torch.arange(3))
    with pytest.raises(AttributeError):
        oa[1].no_such_field
    _same_fields(b, ob[0])
    # static buffers: capacity shapes, filled by ONE copy of the next transfer's buffer
    blob = torch.zeros_like(ra.dev)
    static = ra.rebuild(blob, True)[0]
    cap = E._edge_capacity(a.edge_index.shape[1])
    assert static.edge_index.shape == (2, cap) and static.graph.col.shape == (cap,) and static.graph.t_wgt.shape == (cap,)
    for src, ref in ((b, rb), (a, ra)):
        blob.copy_(ref.dev)
        e = src.edge_index.shape[1]
        assert torch.equal(static.edge_index[:, :e], src.edge_index) and not static.edge_index[:, e:].any()
        assert torch.equal(static.graph.rowptr, src.graph.rowptr) and torch.equal(static.graph.col[:e], src.graph.col)
        assert torch.equal(static.y, src.y) and torch.equal(static.pos, src.pos)
    # another node count is another layout
    c = D.to_device_packed([_lta_batch(44, B=5), _lta_batch(43)], "cpu", pack_on_cpu=True)
    assert c[0]._blob.gsig != ra.gsig


def test_relation_module_multiscale_structure_and_init_equal_the_reference_class(golden):
    """``RelationModuleMultiScale`` (reference models/TRN.py:9-74): scales, relation sets, sub-sampling, the relations a forward
    pass selects, state-dict keys and -- under the same seed -- the initial parameters bit for bit, against the reference class
    itself (tests/golden/trn_multiscale.pt); reachable under the reference's import path."""
    from models.TRN import RelationModuleMultiScale
    for c in golden("trn_multiscale")["cases"]:
        torch.manual_seed(c["seed"])
        m = RelationModuleMultiScale(c["img_feature_dim"], c["num_bottleneck"], c["num_frames"])
        assert m.scales == c["scales"] and m.subsample_scales == c["subsample_scales"] and m.subsample_num == 3
        assert [[list(r) for r in rs] for rs in m.relations_scales] == c["relations_scales"]
        assert [[list(r) for r in m.selected_relations(i)] for i in range(len(m.scales))] == c["selected"]
        sd = m.state_dict()
        assert list(sd) == list(c["state_dict"])
        for k, v in c["state_dict"].items():
            assert torch.equal(sd[k], v), k
        with pytest.raises(ValueError):
            m(torch.zeros(2, c["num_frames"] + 1, c["img_feature_dim"]))


# ---- round 4: ADVICE r3 items and the test-suite layout ---------------------------------------------------------------
def test_sharded_moments_refuse_a_state_dict_until_gathered():
    """dist.GradSync(shard_update=True) leaves every rank with its own 1 / world slice of the Adam moments: a checkpoint
    written from that state would restart (world - 1) / world of the parameters with zero moments.
    FlatAdam.state_dict() refuses until GradSync.gather_moments -- a collective the entry points call on every rank -- has run."""
    from egopack_amd.optim import FlatAdam
    p = torch.nn.Parameter(torch.zeros(8))
    opt = FlatAdam([p])
    opt.state_dict()  # (nothing materialised, nothing sharded: fine)
    opt._moments_sharded = True
    with pytest.raises(RuntimeError, match="gather_moments"):
        opt.state_dict()
    from egopack_amd.dist import GradSync
    GradSync(1).gather_moments(opt)  # (no process group: a one-rank "gather" clears the flag)
    assert opt._moments_sharded is False
    opt.state_dict()


def test_packed_transfer_signature_covers_scalar_tuples_and_lazy_batches_expose_scalars():
    """ a captured step bakes host scalars AND tuples of scalars (pos_range) into its kernel arguments: the
    packed transfer's layout signature must tell two batches apart that differ in such a tuple; and reading a plain scalar
    of a lazy batch (``int(b.num_graphs)`` in the training loops) must not build its tensor views."""
    from egopack_amd import data as D
    ds = D.SyntheticTaskDataset("ar", 4, 8, 3, 8, (5, 7), k=1, seed=1)
    a = D.collate([ds[i] for i in range(4)])
    b = D.collate([ds[i] for i in range(4)])
    assert a.pos_range == b.pos_range
    oa = D.to_device_packed([a], "cpu", pack_on_cpu=True)[0]
    ob = D.to_device_packed([b], "cpu", pack_on_cpu=True)[0]
    assert oa._blob.gsig == ob._blob.gsig
    b.pos_range = (a.pos_range[0] - 1, a.pos_range[1])
    oc = D.to_device_packed([b], "cpu", pack_on_cpu=True)[0]
    assert oc._blob.gsig != oa._blob.gsig
    assert "_fill" in oa.__dict__ and int(oa.num_graphs) == 4 and oa.pos_range == a.pos_range and "_fill" in oa.__dict__
    assert oa.pos.shape[0] == 32 and "_fill" not in oa.__dict__ and int(oa.num_graphs) == 4


def test_gpu_suite_runs_parity_files_first_and_process_spawners_last():
    """The driver runs ``pytest tests/ -x``: the files that ARE the parity evidence are collected first, everything that spawns
    processes last, and no test module owns a torch.distributed process group in the pytest process."""
    import conftest

    class Item:
        def __init__(self, stem, gpu=True):
            self.fspath, self._gpu = f"/x/tests/{stem}.py", gpu

        def get_closest_marker(self, name):
            return object() if (name == "gpu" and self._gpu) else None
    names = ["test_gpu_dist", "test_gpu_two_rank", "test_gpu_blockwise", "test_cabi", "test_gpu_models", "test_gpu_kernels",
             "test_gpu_new_thing", "test_gpu_configs", "test_gpu_entrypoints"]
    items = [Item(n, gpu=n != "test_cabi") for n in names]
    conftest.pytest_collection_modifyitems(None, None, items)
    order = [Path(i.fspath).stem for i in items]
    assert order[0] == "test_cabi" and order[1:5] == ["test_gpu_kernels", "test_gpu_models", "test_gpu_configs", "test_gpu_blockwise"]
    assert order[-2:] == ["test_gpu_two_rank", "test_gpu_dist"] and order.index("test_gpu_new_thing") < order.index("test_gpu_two_rank")
    tests_dir = Path(__file__).resolve().parent
    for f in tests_dir.glob("test_gpu_*.py"):
        assert "init_process_group" not in f.read_text(), f"{f.name} creates a process group inside the pytest process"


def test_bench_names_one_pmc_file_per_configuration():
    import bench
    a = bench.parse_args([])
    assert bench.pmc_key(a) == "mtl_B64_T32_H1024_Hp1024_bf16" and bench.pmc_file(a).name in ("pmc_latest.json", f"pmc_{bench.pmc_key(a)}.json")
    c4 = bench.parse_args(["--workload", "egopack_oscc"])
    c5 = bench.parse_args(["--workload", "mtl4", "--T", "256", "--batch", "16"])
    assert bench.pmc_file(c4).name == "pmc_egopack_oscc_B64_T32_H1024_Hp1024_bf16.json"
    assert bench.pmc_file(c5).name == "pmc_mtl4_B16_T256_H1024_Hp1024_bf16.json"


def test_ranges_minus_holes():
    """engine._minus: the optimizer slices that are left when parts of the flat buffers were stepped earlier in the step."""
    from egopack_amd.engine import _minus
    assert _minus([(0, 100), (200, 300)], [(50, 60), (250, 400)]) == [(0, 50), (60, 100), (200, 250)]
    assert _minus([(0, 100)], []) == [(0, 100)] and _minus([(0, 100)], [(0, 100)]) == []
    assert _minus([(0, 8), (8, 8)], [(100, 200)]) == [(0, 8)]
    assert _minus([(0, 100)], [(10, 20), (15, 30), (90, 120)]) == [(0, 10), (30, 90)]


def test_live_label_rows_of_a_multi_head_label_tensor():
    """data.live_label_rows: the nodes with a label in any head, in node order, padded to 64 rows with -1; absent when most nodes
    are labelled (LTA) or the labels are not per node and head (OSCC, PNR); collate attaches the arrays to AR batches."""
    from egopack_amd import data as D
    y = torch.full((40, 2), -1, dtype=torch.long)
    y[5, 0], y[5, 1], y[22, 1] = 3, 9, 4
    idx, inv, yl = D.live_label_rows(y, 40)
    assert idx.tolist() == [5, 22] + [-1] * 62
    assert inv[5] == 0 and inv[22] == 1 and int((inv == -1).sum()) == 38
    assert yl[:2].tolist() == [[3, 9], [-1, 4]] and bool((yl[2:] == -1).all())
    assert D.live_label_rows(torch.zeros(40, 2, dtype=torch.long), 40) is None        # every node labelled
    assert D.live_label_rows(torch.zeros(40, dtype=torch.long), 40) is None           # PNR: one label per node, no heads
    assert D.live_label_rows(torch.zeros(5, dtype=torch.long), 40) is None            # OSCC: one label per sequence
    none = D.live_label_rows(torch.full((40, 2), -1, dtype=torch.long), 40)           # nothing labelled: 64 pad rows
    assert none[0].shape == (64,) and bool((none[0] == -1).all())
    for task, want in (("ar", True), ("lta", False), ("pnr", False), ("oscc", False)):
        ds = D.SyntheticTaskDataset(task, 4, 16, 3, 8, (7, 11), k=1, seed=3)
        b = D.collate([ds[i] for i in range(4)])
        assert (getattr(b, "live_idx", None) is not None) == want, task
        if want:
            assert b.live_idx[:4].tolist() == [8, 24, 40, 56] and b.live_inv.shape == (64,) and torch.equal(b.live_y[:4], b.y[b.live_idx[:4]])


def test_dual_replay_refuses_a_tape_that_was_not_consumed():
    """ops.dual_record / dual_replay (the one-pass EgoPack step): the recording scope restores the previous tape, and a replay
    that leaves taped nodes behind -- the two passes issued different node sequences -- is an error, not a silent mismatch."""
    import pytest
    from egopack_amd import ops
    with ops.dual_record() as tape:
        assert ops._dual["tape"] is tape
        with ops.dual_record() as inner:
            assert ops._dual["tape"] is inner
        assert ops._dual["tape"] is tape
    assert ops._dual["tape"] is None
    with pytest.raises(RuntimeError, match="not consumed"):
        with ops.dual_replay([("linear", {})]):
            pass
    assert ops._dual["replay"] is None
    with pytest.raises(ValueError):  # (an exception inside the scope is not masked by the left-over check)
        with ops.dual_replay([("linear", {})]):
            raise ValueError("x")
    assert ops._dual["replay"] is None


def test_step_schedule_installs_its_settings_and_leaves_nothing_behind():
    """sched.step_schedule (every step of the engine is issued inside one): the five settings hold inside and come back on the way
    out, a nested scope hands the outer one's settings back, and whichever way the scope is left -- normally or by an exception
    in the body -- nothing parked or deferred and no hook survives it."""
    import pytest
    from egopack_amd import sched
    q, side, forks, last = sched._wq, sched._wgrad, sched._deferred, sched._last_wgrad

    def settings():
        return side.enabled, q.on, q.count, forks.on, side.handoff

    def assert_clean():
        assert q.items == [] and q.hold == [] and q.reds == [] and q.riders == [] and q.tiles == 0
        assert forks.items == []
        assert last["param"] is None and last["hook"] is None and last["pre"] is None
        assert last["tail"] is None and sched._g1_hook["fn"] is None

    def litter():  # (what a step leaves when it is abandoned half-way)
        buf = torch.zeros(128 * 128)
        sched._park((128, 128, buf, 128, buf, 128, 64, buf, 128), {}, (buf,))
        q.reds.append(sched.Reduction(buf, buf[:4], buf[4:8], 1, 4, 0))  # (as issue_ln_reduce parks it when the queue is on)
        q.hold.append(buf)
        q.riders.append(lambda: None)
        forks.items.append(sched.Fork((0, 0), None, lambda ev: None))
        sched.set_last_wgrad_hook(torch.zeros(1), lambda: None, pre=lambda: None)
        sched.set_last_wgrad_tail(64, 128)
        sched.set_graphone_backward_hook(lambda: None)

    # every field is in the literal that creates its structure: no .get / getattr fallbacks
    assert set(vars(q)) == {"on", "count", "items", "tiles", "hold", "reds", "riders"}
    assert set(vars(side)) == {"enabled", "streams", "pending", "queued", "exclude", "handoff"}
    assert set(vars(forks)) == {"items", "busy", "on"}
    assert set(last) == {"param", "hook", "pre", "inline", "tail", "leaked"}
    idle = settings()
    # 1. chosen settings inside, the previous ones afterwards
    with sched.step_schedule(True, True, 8, False, True):
        assert settings() == (True, True, 8, False, True)
        assert_clean()
        with sched.step_schedule(False, True, None, True):  # nested: the outer scope's settings come back
            assert settings() == (False, True, None, True, False)
        assert settings() == (True, True, 8, False, True)
    assert settings() == idle
    assert_clean()
    # 2. left through an exception, with work parked / deferred and hooks installed inside
    with pytest.raises(ValueError):
        with sched.step_schedule(True, True, 6, True, False):
            litter()
            assert q.items and q.reds and q.hold and q.riders and q.tiles == 1 and forks.items and last["tail"] == (64, 128)
            raise ValueError("abandoned")
    assert settings() == idle
    assert_clean()
    # ... and the same litter is dropped on a normal exit, and on the way IN (left by whoever issued outside a scope)
    with sched.step_schedule(True, False):
        litter()
    assert settings() == idle
    assert_clean()
    litter()
    with sched.step_schedule(True, True):
        assert q.items == [] and q.reds == [] and q.riders == [] and q.hold == [] and q.tiles == 0 and forks.items == []
    assert_clean()


def _reds(targets):
    """sched.Reduction records over CPU slots: ``targets`` = (dw, db) pairs."""
    from egopack_amd import sched
    return [sched.Reduction(torch.zeros(1), dw, db, 4, 4, 0) for dw, db in targets]


def test_reduction_batches_are_greedy_ordered_and_never_repeat_a_target():
    """sched.reduction_batches: at most 8 reductions per batch, no dw / db address twice in a batch, order kept, and a batch
    ends ONLY when it is full or at a repeated target."""
    from egopack_amd import sched
    buf = torch.zeros(64)
    slot = lambda i: buf[i:i + 1]

    def batches(reds):
        got = sched.reduction_batches(reds)
        flat = [r for b in got for r in b]
        assert len(flat) == len(reds) and all(r is g for r, g in zip(reds, flat))  # (the concatenation of the batches IS the input)
        for b in got:
            ptrs = [t.data_ptr() for r in b for t in (r.dw, r.db)]
            assert 1 <= len(b) <= 8 and len(set(ptrs)) == len(ptrs)
        return [len(b) for b in got]

    assert batches([]) == []
    assert batches(_reds([(slot(2 * i), slot(2 * i + 1)) for i in range(9)])) == [8, 1]  # nine distinct targets
    targets = [(slot(2 * i), slot(2 * i + 1)) for i in range(11)]
    targets[4] = (targets[1][0], targets[4][1])  # the fifth shares its dw with the second
    assert batches(_reds(targets)) == [4, 7]
    targets = [(slot(2 * i), slot(2 * i + 1)) for i in range(5)]
    targets[3] = (targets[3][0], targets[0][0])  # a db that repeats an earlier dw
    assert batches(_reds(targets)) == [3, 2]


@pytest.fixture
def parked_queue(monkeypatch):
    """The parking queue inside a scope, with the streams stubbed out: nothing excluded, launches recorded instead of issued."""
    from egopack_amd import sched
    launched = []
    monkeypatch.setattr(sched, "_on_excluded_stream", lambda: False)
    monkeypatch.setattr(sched, "_wgrad_launch", lambda in_place, tensors, launch, in_backward=True: launched.append((in_place, list(tensors))))
    with sched.step_schedule(True, True):
        yield sched, launched


def _park_at(sched, buf, first, M=128, N=128):
    """Park an M x N problem whose gradient slot starts at element ``first`` of ``buf``."""
    op = torch.zeros(8)
    sched._park((M, N, op, 8, op, 8, 64, buf[first:], N), {"tag": first}, (op,))


def test_take_parked_is_all_or_none(parked_queue):
    sched, _ = parked_queue
    buf = torch.zeros(256)
    for first, (M, N) in zip((0, 64, 128), ((128, 128), (129, 128), (256, 300))):
        _park_at(sched, buf, first, M, N)
    assert [p.tiles for p in sched._wq.items] == [1, 2, 6] and sched._wq.tiles == 9 == sum(sched.tiles(*p.args[:2]) for p in sched._wq.items)
    assert sched._take_parked(2) == [] and len(sched._wq.items) == 3 and sched._wq.tiles == 9
    got = sched._take_parked(3)
    assert [kw["tag"] for _, kw in got] == [0, 64, 128] and sched._wq.items == [] and sched._wq.tiles == 0
    assert sched._take_parked(3) == []


def test_tail_take_splits_what_is_parked_by_slot_address(parked_queue):
    sched, _ = parked_queue
    buf = torch.zeros(256)
    base = buf.data_ptr()

    def park_all():
        for first, (M, N) in zip((0, 64, 96, 128), ((128, 128), (129, 128), (128, 257), (256, 300))):
            _park_at(sched, buf, first, M, N)
        for dw, db in ((64, 100), (64, 128), (0, 100), (127, 65)):  # (only the first and the last lie inside with BOTH targets)
            sched.issue_ln_reduce(torch.zeros(1), buf[dw:], buf[db:], 1, 1, 0)
    park_all()
    assert sched._take_tail_items() == ([], []) and len(sched._wq.items) == 4 and len(sched._wq.reds) == 4  # no tail set
    sched.set_last_wgrad_hook(torch.zeros(1), lambda: None)
    sched.set_last_wgrad_tail(base + 4 * 64, base + 4 * 128)
    items, reds = sched._take_tail_items()
    assert [p.kw["tag"] for p in items] == [64, 96] and all(p.out.data_ptr() == base + 4 * p.kw["tag"] for p in items)
    assert [p.kw["tag"] for p in sched._wq.items] == [0, 128]
    assert sched._wq.tiles == 1 + 6 == sum(p.tiles for p in sched._wq.items)
    assert [(r.dw.data_ptr() - base) // 4 for r in reds] == [64, 127]
    assert [(r.dw.data_ptr() - base) // 4 for r in sched._wq.reds] == [64, 0]
    assert sched.last_wgrad_tail_on_backward_stream()  # (taken, not flushed: nothing of the range left for the side stream)


def test_tail_range_leaks_when_a_flush_issues_one_of_its_gradients(parked_queue):
    sched, launched = parked_queue
    last = sched._last_wgrad
    buf = torch.zeros(256)
    base = buf.data_ptr()

    def arm():
        sched.set_last_wgrad_hook(torch.zeros(1), lambda: None)
        sched.set_last_wgrad_tail(base + 4 * 64, base + 4 * 128)
        assert last["leaked"] is False and sched.last_wgrad_tail_on_backward_stream()
    arm()
    _park_at(sched, buf, 0)
    sched.issue_ln_reduce(torch.zeros(1), buf[0:], buf[128:], 1, 1, 0)
    sched.flush_wgrad()  # (nothing of the range among what went out)
    assert len(launched) == 1 and launched[0][0] is True and len(launched[0][1]) == 2
    assert sched._wq.items == [] and sched._wq.reds == [] and sched._wq.hold == [] and last["leaked"] is False
    _park_at(sched, buf, 96)
    sched.flush_wgrad()  # a problem of the range
    assert last["leaked"] is True and not sched.last_wgrad_tail_on_backward_stream()
    arm()  # (set_last_wgrad_tail clears the flag)
    sched.issue_ln_reduce(torch.zeros(1), buf[0:], buf[100:], 1, 1, 0)
    sched.flush_wgrad()  # a reduction with ONE target in the range
    assert last["leaked"] is True and len(launched) == 3
    sched.flush_wgrad()  # (nothing parked: no launch)
    assert len(launched) == 3
    sched.set_last_wgrad_hook(None, None)
    assert last["tail"] is None and not sched.last_wgrad_tail_on_backward_stream()


def test_the_benchmark_switches_reach_the_scheduler(monkeypatch):
    """bench.py assigns the ``side`` key of ``ops._wgrad_ln`` and the ``inline`` key of ``ops._last_wgrad``: the scheduler's own objects."""
    import types
    from egopack_amd import ops, sched
    assert ops._wgrad_ln is sched._wgrad_ln and ops._last_wgrad is sched._last_wgrad
    assert "side" in sched._wgrad_ln and "inline" in sched._last_wgrad
    own = [n for n, v in vars(sched).items() if getattr(v, "__module__", None) == sched.__name__]  # its functions and record types
    # (ops re-exports nothing else -- but ``join_wgrad``, which whoever calls backward() over these ops needs after it)
    assert "issue_wgrad" in own and "Problem" in own and [n for n in own if hasattr(ops, n)] == ["join_wgrad"]
    assert ops.join_wgrad is sched.join_wgrad
    assert not [n for n in ("_wq", "_wgrad", "_deferred", "_g1_hook") if hasattr(ops, n)]

    def no_stream():
        raise AssertionError("a stream was asked for")
    monkeypatch.setattr(sched, "_on_excluded_stream", no_stream)
    monkeypatch.setattr(sched._wgrad, "enabled", True)
    slot, x = torch.zeros(4), types.SimpleNamespace(is_cuda=True)
    with pytest.raises(AssertionError, match="a stream was asked for"):  # (side streams on, in-place slots: the stream decides)
        sched._ln_reduce_on_side(slot, slot, x)
    monkeypatch.setitem(sched._wgrad_ln, "side", False)
    assert sched._ln_reduce_on_side(slot, slot, x) is False  # ... and with the switch off it is never asked


def test_fast_key_sees_the_labelled_row_set_of_a_compacted_head():
    """two AR batches with the same graph structure, feature shape and label shape but another labelled-row set
    (a sequence whose centre labels are all -1) differ in what a capture bakes in (the strided row view, the padded height of
    the labelled-row arrays): the cheap key must differ wherever the full signature does."""
    from egopack_amd import engine as E
    ds = D.SyntheticTaskDataset("ar", 64, 8, 3, 8, (7, 11), k=1, seed=3)  # 64 labelled rows: the padded list IS a progression
    a, b = D.collate([ds[i] for i in range(64)]), D.collate([ds[i] for i in range(64)])
    row = int(b.live_idx[1])
    b.y[row] = -1  # the second sequence loses its label: three labelled rows, no arithmetic progression over the padded list
    D._attach_live_rows(b)
    if getattr(b, "live_ap", None) is not None and D.live_rows_progression(b.live_idx) is None:
        del b.live_ap
    for x in (a, b):
        x._struct_key = 77
        x.x = torch.zeros(x.pos.shape[0], 3, 8)
    assert getattr(a, "live_ap", None) != getattr(b, "live_ap", None)
    assert E.batch_signature({"ar": a}) != E.batch_signature({"ar": b})
    assert E._fast_key({"ar": a}, None) != E._fast_key({"ar": b}, None)
    assert E._fast_key({"ar": a}, None) == E._fast_key({"ar": a}, None)


def test_switch_registry_covers_every_switch_the_code_reads(monkeypatch):
    """egopack_amd/switches.py is the ONE place a development switch is declared: every name the package asks for is registered,
    nothing else reads EGK_ENABLE / EGK_DISABLE / EGK_DBG, names match exactly (no substrings), an unknown name in the environment
    is reported, and the tri-state override leaves per-class defaults alone when the environment says nothing."""
    import re
    import warnings
    from pathlib import Path
    from egopack_amd import switches
    root = Path(switches.__file__).resolve().parent
    asked, raw = set(), []
    for f in [*root.glob("*.py"), *root.glob("models/**/*.py"), root.parent / "bench.py", root.parent / "main_temporal.py", root.parent / "main_egopack.py"]:
        text = f.read_text()
        if f.name != "switches.py":
            raw += [f"{f.name}: {m}" for m in re.findall(r'environ\S*\("EGK_(?:ENABLE|DISABLE|DBG)"', text)]
        if f.name == "switches.py":
            continue
        asked |= set(re.findall(r'switches\.(?:enabled|override|value)\("([a-z_0-9]+)"\)', text))
        asked |= set(re.findall(r'for name in \(("[a-z_0-9", ]+)\):\n\s+forced = switches\.override\(name\)', text) and ["wgrad_grouping", "deferred_forks"])
        for name in re.findall(r'switches\.debug\("([a-z_0-9]+)"\)', text):
            assert name in switches.DEBUG, name
    assert not raw, raw
    assert asked and asked <= set(switches.REGISTRY), asked - set(switches.REGISTRY)
    assert set(switches.REGISTRY) <= asked, f"registered but never read: {set(switches.REGISTRY) - asked}"
    monkeypatch.delenv("EGK_ENABLE", raising=False)
    monkeypatch.setenv("EGK_DISABLE", "oscc_one_pass")
    assert not switches.enabled("oscc_one_pass") and switches.enabled("one_pass")  # (exact names: the substring bug of rounds 3-5)
    assert switches.override("wgrad_grouping") is None
    monkeypatch.setenv("EGK_ENABLE", "sharded_update,wgrad_grouping")
    assert switches.enabled("sharded_update") and switches.override("wgrad_grouping") is True
    monkeypatch.setenv("EGK_DISABLE", "no_such_switch")
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        switches.enabled("grad_store")
    assert any("no_such_switch" in str(x.message) for x in w)
    import pytest
    with pytest.raises(KeyError):
        switches.enabled("not_registered")
    assert "grad_store" in switches.table()
