"""The EgoPack prediction entry point on the GPU: one epoch of ``main_temporal.main`` on [ar, lta, pnr], one epoch of
``main_egopack.main`` on [oscc] over it (sizes and overrides of tests/test_gpu_entrypoints.py; a validation split of 10 samples, so
that a pass has three batches, the last one short), then ``predict_egopack.main`` on the EgoPack checkpoint.

What the OSCC file says is recomputed: the accuracy must EQUAL what ``main_egopack.validate_metrics`` reports for the same weights
and loaders (quotients of the same integers); the retrieval fields must be what ``GraphONE.interact`` consumed -- the lists of
``ops.nearest_prototypes`` on recomputed features, their first column the ``closest`` the interaction returns --, the distances the
host model's (tests/retrieval_common.py) within its bound, the labels the rows of ``graphone.bank_labels``."""
import json

import numpy as np
import pytest
import torch

from tests import retrieval_common as RC

pytestmark = pytest.mark.gpu
AUX = ("ar", "lta", "pnr")
H, K_NN = 64, 4
OSCC_FIELDS = {"sample", "pred", "prob_change", "lse", "label"}
RETRIEVAL_FIELDS = {"retrieval_sample", "retrieval_pos"} | {f"retrieval_{a}_{f}" for a in AUX for f in ("index", "dist", "wins", "label")}


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    import main_egopack
    import main_temporal
    import predict_egopack
    tmp = tmp_path_factory.mktemp("predict_egopack")
    common = ["k=1", "batch_size=4", "num_epochs=1", "synthetic_samples=16", "synthetic_val_samples=10", "model.hidden_size=64",
              "model.temporal_pooling.hidden_size=64", "oscc_feat_size=64", f"checkpoint_dir={tmp}", "save_model=True", "compute=f32",
              "optimizer.lr=1e-3"]
    main_temporal.main(common + ["enabled_tasks=[ar,lta,pnr]"])
    mtl = tmp / "MTL_ar-lta-pnr" / "checkpoint.pth"
    assert mtl.exists()
    common[3] = "synthetic_samples=256"  # build_graphone reads the AR split with batch 256, drop_last=True
    ego_args = common + ["enabled_tasks=[oscc]", "enable_graphone=True", "graphone.k=4", "graphone.depth=2", "graphone.hidden_size=64",
                         "+graphone.features_size=64", "artifact_prefix=EGO"]
    main_egopack.main(ego_args + [f"resume_from={mtl}"])
    ckpt = tmp / "EGO_egopack_oscc" / "checkpoint.pth"
    assert ckpt.exists()
    out = tmp / "pred"
    args = ego_args + [f"resume_from={ckpt}"]
    r = predict_egopack.main(args + [f"predict.out={out}"])
    f = torch.load(out / "predictions_oscc.pt", weights_only=False)
    return dict(r=r, f=f, out=out, args=args, ckpt=ckpt, tmp=tmp)


def _walk(run):
    """Per batch of the OSCC loader: (the batch on the device, the auxiliary features ``_logits`` hands to ``interact``)."""
    r = run["r"]
    model, tasks = r["model"], r["tasks"]
    model.eval()
    with torch.no_grad():
        for data in r["loaders"]["oscc"]:
            data = data.to("cuda")
            feat = model(data)
            yield data, {a: tasks[a].forward_features(feat, out_f32=True) for a in AUX}


@pytest.mark.timeout(600)
def test_the_file_has_its_fields_and_provenance(run):
    f, ds = run["f"], run["r"]["datasets"]["oscc"]
    assert OSCC_FIELDS | RETRIEVAL_FIELDS | {"topk", "seed", "split", "epoch", "retrieval_tasks", "retrieval_k"} <= set(f), sorted(f)
    assert f["retrieval_tasks"] == list(AUX) and f["retrieval_k"] == K_NN and f["retrieval_distance"] == "cosine" and f["epoch"] == 1
    assert all(not v.is_cuda for v in f.values() if torch.is_tensor(v))
    samples = [ds[i] for i in range(len(ds))]
    assert len(samples) == 10 and torch.equal(f["sample"], torch.arange(10))
    assert torch.equal(f["label"], torch.tensor([int(d.y) for d in samples]))
    assert torch.equal(f["retrieval_sample"], torch.cat([torch.full((d.pos.numel(),), i, dtype=torch.int64) for i, d in enumerate(samples)]))
    assert torch.equal(f["retrieval_pos"], torch.cat([d.pos for d in samples]))
    n = f["retrieval_sample"].numel()
    for a in AUX:
        idx, dist, wins, lab = (f[f"retrieval_{a}_{x}"] for x in ("index", "dist", "wins", "label"))
        assert idx.shape == (n, K_NN) and idx.dtype == torch.int64 and dist.shape == (n, K_NN) and dist.dtype == torch.float32
        assert wins.shape == (n, K_NN + 1) and wins.dtype == torch.int32 and lab.shape == (n, K_NN, 2) and lab.dtype == torch.int64


@pytest.mark.timeout(600)
def test_accuracy_recomputed_from_the_file_equals_the_egopack_validation(run):
    import main_egopack
    from egopack_amd import train as T
    r, f = run["r"], run["f"]
    cfg = T.load_config(run["args"])
    vm = main_egopack.validate_metrics(0, r["model"], r["tasks"], r["graphone"], T.task_weights(cfg), r["datasets"], r["loaders"],
                                       late_fusion=cfg.late_fusion, device="cuda")
    mine = int((f["pred"] == f["label"]).sum()) / 10
    print(f"oscc accuracy: file {mine} meter {vm['oscc']['accuracy']}")
    assert mine == vm["oscc"]["accuracy"]


@pytest.mark.timeout(600)
def test_indices_distances_and_wins_are_what_the_interaction_consumed(run):
    from egopack_amd import ops
    r, f = run["r"], run["f"]
    go = r["graphone"].eval()
    lists = {a: [] for a in AUX}
    feats = {a: [] for a in AUX}
    with torch.no_grad():
        for data, aux in _walk(run):
            _, closest = go.interact(aux)
            for a in AUX:
                nn = ops.nearest_prototypes(aux[a], go.embeddings[a].weight, K_NN, go.distance_func)
                assert torch.equal(nn[:, 0], closest[a][0])
                lists[a].append(nn.cpu()), feats[a].append(aux[a].cpu())
    bound = RC.dist_bound(H)
    for a in AUX:
        idx, dist, wins = (f[f"retrieval_{a}_{x}"] for x in ("index", "dist", "wins"))
        assert torch.equal(idx, torch.cat(lists[a])), a
        bank, x = go.embeddings[a].weight.detach().cpu(), torch.cat(feats[a])
        assert int(idx.min()) >= 0 and int(idx.max()) < bank.shape[0]
        assert bool((wins.sum(1) == H).all()) and bool((wins >= 0).all())
        # compute=f32: the first stage reads the searched features themselves
        assert np.array_equal(wins.numpy(), RC.wins_model(x.numpy(), bank.numpy(), idx.numpy()))
        ref = RC.dist_model(x.numpy(), bank.numpy(), idx.numpy(), "cosine")
        err = float(np.abs(dist.numpy().astype(np.float64) - ref).max())
        print(f"retrieval_{a}_dist: largest error {err:.3e}, bound {bound:.3e}")
        assert err <= bound
        assert bool((dist[:, 1:] - dist[:, :-1] >= -2 * bound).all())  # (the search and the report round differently)


@pytest.mark.timeout(600)
def test_labels_are_the_bank_rows_labels(run):
    import graphone as root
    from egopack_amd import graphone as G
    from egopack_amd import train as T
    from egopack_amd.data import build_dataloader
    r, f = run["r"], run["f"]
    cfg = T.load_config(run["args"])
    ar_train = T.build_datasets(cfg, "train")["ar"]
    n_classes = tuple(c[-1].out_features for c in r["tasks"]["ar"].classifiers)
    loader = lambda: build_dataloader(ar_train, 256, False, 0, True, cfg.seed, rank=0, world_size=1, shard="batches")
    labels = root.bank_labels(loader(), n_classes)
    assert torch.equal(labels, r["bank_labels"])
    go = r["graphone"]
    assert all(go.embeddings[a].weight.shape[0] == labels.numel() for a in AUX)
    _, count = G.accumulate_banks(r["model"], r["tasks"]["ar"], [r["tasks"]["ar"]], loader(), "cuda")
    assert torch.equal(labels, torch.nonzero(count > 0).reshape(-1).cpu())
    for a in AUX:
        lab = labels[f[f"retrieval_{a}_index"]]
        assert torch.equal(f[f"retrieval_{a}_label"], torch.stack([lab // n_classes[1], lab % n_classes[1]], -1))
        assert int(f[f"retrieval_{a}_label"][..., 0].max()) < n_classes[0]


@pytest.mark.timeout(600)
def test_a_second_run_writes_the_same_bits_and_retrieval_can_be_switched_off(run):
    import predict_egopack
    f = run["f"]
    out2, out3 = run["tmp"] / "pred2", run["tmp"] / "pred3"
    predict_egopack.main(run["args"] + [f"predict.out={out2}"])
    g = torch.load(out2 / "predictions_oscc.pt", weights_only=False)
    assert set(g) == set(f)
    for key, v in f.items():
        if torch.is_tensor(v):
            assert v.dtype == g[key].dtype and torch.equal(v.view(torch.int32) if v.dtype == torch.float32 else v,
                                                           g[key].view(torch.int32) if v.dtype == torch.float32 else g[key]), key
        else:
            assert v == g[key], key
    predict_egopack.main(run["args"] + [f"predict.out={out3}", "predict_egopack.retrieval=false"])
    h = torch.load(out3 / "predictions_oscc.pt", weights_only=False)
    assert not [k for k in h if k.startswith("retrieval")]
    assert set(h) == {k for k in f if not k.startswith("retrieval")}
    for key in OSCC_FIELDS:
        assert torch.equal(h[key], f[key]), key
    assert "retrieval" not in json.loads((out3 / "predictions_oscc.json").read_text())["0"]
    # labels off: the indices without the labels
    out4 = run["tmp"] / "pred4"
    predict_egopack.main(run["args"] + [f"predict.out={out4}", "predict_egopack.labels=false", "predict.json=false"])
    q = torch.load(out4 / "predictions_oscc.pt", weights_only=False)
    assert set(q) == {k for k in f if not k.endswith("_label")} and torch.equal(q["retrieval_ar_index"], f["retrieval_ar_index"])
    assert not (out4 / "predictions_oscc.json").exists()


@pytest.mark.timeout(600)
def test_the_json_round_trips_to_the_tensors(run):
    f = run["f"]
    doc = json.loads((run["out"] / "predictions_oscc.json").read_text())
    assert sorted(doc, key=int) == [str(i) for i in range(10)]
    assert doc["3"]["state_change"] == bool(f["pred"][3] == 1) and set(doc["0"]) == {"state_change", "prob", "retrieval"}
    for s in range(10):
        rows = f["retrieval_sample"] == s
        entry = doc[str(s)]["retrieval"]
        assert set(entry) == {"pos", *AUX} and entry["pos"] == f["retrieval_pos"][rows].tolist()
        for a in AUX:
            assert set(entry[a]) == {"index", "dist", "wins", "label"}
            assert torch.equal(torch.tensor(entry[a]["index"]), f[f"retrieval_{a}_index"][rows])
            assert torch.equal(torch.tensor(entry[a]["wins"], dtype=torch.int32), f[f"retrieval_{a}_wins"][rows])
            assert torch.equal(torch.tensor(entry[a]["label"]), f[f"retrieval_{a}_label"][rows])
            assert torch.equal(torch.tensor(entry[a]["dist"], dtype=torch.float32), f[f"retrieval_{a}_dist"][rows])
