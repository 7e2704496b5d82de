"""The ``action_scores:`` block through the entry points on the GPU: one epoch of ``main_temporal.main`` on tiny synthetic AR / LTA
datasets (hidden size 64, a validation split of 10 samples), then validation with the block on and off on the same weights, loaders
and sampler seed, and ``predict.main`` with the block on (raw and at the temperatures of a calibration file) and off.

What the meters log is recomputed on the host: the logits and labels every ``_ActionCounts.update`` saw are recorded, ranked by the
model of tests/action_common.py (on the launch's own log-sum-exps) and counted; the futures every ``action_edit_distances`` call saw
go through the plain-Python Levenshtein.  Accuracies are quotients of the same integers and must be EQUAL."""
import json

import numpy as np
import pytest
import torch

from tests import action_common as AC
from tests import topk_common as TK

pytestmark = pytest.mark.gpu
SEED = 5
TASKS = ("ar", "lta")
ACTION_FIELDS = {"action_topk", "action_logp", "action_prob"}
NEW = {"ar": {f"actions_top{k}" for k in (1, 2, 3, 5)}, "lta": {"actions_top1", "actions_ed"}}
SPLIT = {"actions_seen_top1", "actions_seen_support", "actions_unseen_top1", "actions_unseen_support"}
TEMPS = {"verbs_": 2.0, "nouns_": 0.5}


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    import main_temporal
    import predict
    from egopack_amd import meters as M
    from egopack_amd import ops
    from egopack_amd import train as T
    tmp = tmp_path_factory.mktemp("action")
    common = ["k=1", "batch_size=4", "num_epochs=1", "synthetic_samples=16", "synthetic_val_samples=10", "model.hidden_size=64",
              "model.temporal_pooling.hidden_size=64", "oscc_feat_size=64", f"checkpoint_dir={tmp}", "save_model=True", "compute=f32",
              "optimizer.lr=1e-3", "enabled_tasks=[ar,lta]", f"lta_sampling.seed={SEED}", "lta_sampling.mode=philox"]
    on_args = ["action_scores.enabled=true", "action_scores.seen_split=true"]
    trained = main_temporal.main(common + on_args)  # (the training run validates with the block on: its metrics carry the keys)
    ckpt = tmp / "MTL_ar-lta" / "checkpoint.pth"
    assert ckpt.exists()
    off = predict.main(common + [f"resume_from={ckpt}", f"predict.out={tmp / 'off'}"])
    raw = predict.main(common + on_args + [f"resume_from={ckpt}", f"predict.out={tmp / 'raw'}", "action_scores.topk=7"])

    # validation on the exported weights, block on (the launches' inputs recorded) and off
    cfg_on = T.load_config(common + on_args)
    seen = T.action_scores_seen(cfg_on, T.build_datasets(cfg_on, "train"))
    calls, dists = [], []
    update, pairs = M._ActionCounts.update, M.action_edit_distances

    def rec_update(self, zv, zn, yv, yn):
        calls.append((self, zv.detach().clone(), zn.detach().clone(), yv.clone(), yn.clone()))
        return update(self, zv, zn, yv, yn)

    def rec_pairs(pv, pn, lv, ln):
        d = pairs(pv, pn, lv, ln)
        dists.append(tuple(t.cpu().numpy().copy() for t in (pv, pn, lv, ln, d)))
        return d

    M._ActionCounts.update, M.action_edit_distances = rec_update, rec_pairs
    try:
        on = main_temporal.validate_metrics(0, raw["model"], raw["tasks"], list(TASKS), raw["datasets"], raw["loaders"], "cuda",
                                            sampler=ops.FutureSampler(SEED), report=lambda t: T.action_scores_meter_args(cfg_on, t, seen))
    finally:
        M._ActionCounts.update, M.action_edit_distances = update, pairs
    n_on = (len(calls), len(dists))
    plain = main_temporal.validate_metrics(0, raw["model"], raw["tasks"], list(TASKS), raw["datasets"], raw["loaders"], "cuda",
                                           sampler=ops.FutureSampler(SEED))
    assert (len(calls), len(dists)) == n_on

    # a calibration file by hand beside the checkpoint, then the export at its temperatures
    for t in TASKS:
        torch.save({"task": t, "heads": {p: {"temperature": v} for p, v in TEMPS.items()}, "t_range": [0.05, 20.0], "split": "validation"},
                   T.calibration_path(ckpt.parent, t))
    records = []
    action_topk = ops.action_topk

    def rec_topk(zv, zn, k, **kw):
        out = action_topk(zv, zn, k, **kw)
        records.append((zv.detach().clone(), zn.detach().clone(), k, None if kw.get("beta") is None else kw["beta"].clone(), out))
        return out

    ops.action_topk = rec_topk
    try:
        cal = predict.main(common + on_args + [f"resume_from={ckpt}", f"predict.out={tmp / 'cal'}", "action_scores.calibrated=true"])
    finally:
        ops.action_topk = action_topk
    return dict(tmp=tmp, trained=trained, off=off, raw=raw, cal=cal, on=on, plain=plain, calls=calls, dists=dists, records=records, seen=seen)


@pytest.mark.timeout(600)
def test_validation_logs_the_action_keys_and_they_are_the_host_models(run):
    from egopack_amd import ops
    for t in TASKS:
        on, plain = run["on"][t], run["plain"][t]
        assert set(on) - set(plain) == NEW[t] | SPLIT, (t, sorted(set(on) ^ set(plain)))
        assert set(run["trained"]["metrics"][t]) == set(on), "the training run's validation logs the same keys"
        for k, v in plain.items():  # the block changes no existing value (the LTA distances now come from the pair launch)
            assert on[k] == v, f"{t}: {k} moved with action_scores on ({on[k]} != {v})"
        # verb and noun labels are present on the same rows of the synthetic splits: a pair is right only if both parts are
        head = "verbs_top1", "nouns_top1"
        assert on["actions_top1"] <= min(on[head[0]], on[head[1]]) + 1e-15, (t, on)
        assert 0.0 <= on["actions_seen_top1"] <= 1.0 and on["actions_seen_support"] + on["actions_unseen_support"] > 0
    # the meters' counts from the recorded logits: the model's ranks on the launch's own log-sum-exps
    meters = {}
    for who, zv, zn, yv, yn in run["calls"]:
        lse = ops.action_topk(zv, zn, 1, want_lse=True, want_prob=False, want_logp=False)["lse"].cpu().numpy()
        _, _, rank, _ = AC.model(TK.widen(zv), TK.widen(zn), lse, 1, labels=(yv.cpu().numpy(), yn.cpu().numpy()))
        code = yv.cpu().numpy() * zn.shape[1] + yn.cpu().numpy()
        meters.setdefault(id(who), []).append((rank, code))  # (the recorded meters are alive: their ids are distinct)
    assert len(meters) == 2  # one _ActionCounts per task, in the order of TASKS
    for t, parts in zip(TASKS, meters.values()):
        rank, code = np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])
        valid = rank >= 0
        assert valid.sum() > 0
        for k in ((1, 2, 3, 5) if t == "ar" else (1,)):
            assert run["on"][t][f"actions_top{k}"] == int((valid & (rank < k)).sum()) / int(valid.sum()), (t, k)
        known = valid & np.isin(code, run["seen"][t].numpy())
        assert run["on"][t]["actions_seen_support"] == int(known.sum()) and run["on"][t]["actions_unseen_support"] == int((valid & ~known).sum())
        assert run["on"][t]["actions_seen_top1"] == int((known & (rank < 1)).sum()) / max(int(known.sum()), 1)
        assert run["on"][t]["actions_unseen_top1"] == int((valid & ~known & (rank < 1)).sum()) / max(int((valid & ~known).sum()), 1)


@pytest.mark.timeout(600)
def test_the_lta_distances_come_from_the_pair_launch(run):
    assert run["dists"], "LTAMeter with the block on takes its distances from egk_edit_distance_pairs"
    ed = []
    for pv, pn, lv, ln, d in run["dists"]:
        assert np.array_equal(d, AC.edit_model(pv, pn, lv, ln))
        assert (d[..., 2] >= d[..., :2].max(-1)).all()  # per sample and future, before the minimum over the futures
        ed.append(d.min(axis=1).astype(np.float64) / pv.shape[1])
    ed = np.concatenate(ed)
    on = run["on"]["lta"]
    for key, col in (("verbs_ed", 0), ("nouns_ed", 1), ("actions_ed", 2)):
        assert abs(on[key] - ed[:, col].mean()) <= 1e-12, (key, on[key], ed[:, col].mean())
    assert on["actions_ed"] >= max(on["verbs_ed"], on["nouns_ed"])


@pytest.mark.timeout(600)
def test_predict_writes_the_three_fields_only_with_the_block_on(run):
    for t in TASKS:
        off, raw, cal = (run[name]["predictions"][t] for name in ("off", "raw", "cal"))
        assert not ACTION_FIELDS & set(off) and "action_betas" not in off and "action_topk_k" not in off
        assert set(raw) - set(off) == ACTION_FIELDS | {"action_betas", "action_topk_k"}, sorted(set(raw) ^ set(off))
        for k, v in off.items():  # everything else is today's file
            assert torch.equal(v, raw[k]) if torch.is_tensor(v) else v == raw[k], (t, k)
        n = raw["sample"].numel()
        assert raw["action_topk"].shape == (n, 7, 2) and raw["action_topk"].dtype == torch.int64 and raw["action_topk_k"] == 7
        assert raw["action_logp"].shape == (n, 7) and raw["action_prob"].shape == (n, 7) and raw["action_betas"] is None
        # raw: pair 0 is the heads' own first entries, the scores descend, and the best pair's probability is the product's
        assert torch.equal(raw["action_topk"][:, 0, 0], raw["verb_topk"][:, 0]) and torch.equal(raw["action_topk"][:, 0, 1], raw["noun_topk"][:, 0])
        assert bool((raw["action_logp"][:, :-1] >= raw["action_logp"][:, 1:]).all())
        torch.testing.assert_close(raw["action_prob"][:, 0].double(), raw["verb_prob"][:, 0].double() * raw["noun_prob"][:, 0].double(), **TK.PROB_TOL)
        doc = json.loads((run["tmp"] / "raw" / f"predictions_{t}.json").read_text())
        first = doc[sorted(doc, key=int)[0]]
        assert ACTION_FIELDS <= set(first) and len(first["action_topk"][0]) == 7 and len(first["action_topk"][0][0]) == 2
        assert not ACTION_FIELDS & set(json.loads((run["tmp"] / "off" / f"predictions_{t}.json").read_text())["0"])
        # calibrated=true: the file's temperatures are recorded, and they are the betas the launch read
        assert cal["action_betas"] == {"verb": 1 / TEMPS["verbs_"], "noun": 1 / TEMPS["nouns_"]} and cal["action_topk_k"] == 5
        assert cal["temperature"] == {"verbs": TEMPS["verbs_"], "nouns": TEMPS["nouns_"]}  # (predict.temperatures: the meters' head names)
    # the calibrated export equals ops.action_topk on the exported batches' logits at the file's betas, batch after batch
    from egopack_amd import ops
    recs = run["records"]
    assert recs and all(k == 5 and b is not None and b.tolist() == [0.5, 2.0] for _, _, k, b, _ in recs)
    n_ar = run["cal"]["predictions"]["ar"]["sample"].numel()
    fresh = [ops.action_topk(zv, zn, k, beta=b, want_prob=True) for zv, zn, k, b, _ in recs]
    for f, key in (("action_topk", "pair"), ("action_logp", "logp"), ("action_prob", "prob")):
        whole = torch.cat([o[key] for o in fresh]).cpu()
        got = torch.cat([run["cal"]["predictions"]["ar"][f], run["cal"]["predictions"]["lta"][f]])
        assert whole.shape == got.shape and torch.equal(whole, got), f
        assert torch.equal(torch.cat([r[4][key] for r in recs]).cpu(), got), f
    assert sum(r[0].shape[0] for r in recs) == n_ar + run["cal"]["predictions"]["lta"]["sample"].numel()
    # ... and the model's, on the launch's own log-sum-exps (the first AR batch)
    zv, zn, k, b, out = recs[0]
    lse = ops.action_topk(zv, zn, 1, beta=b, want_lse=True)["lse"].cpu().numpy()
    pair, logp, _, _ = AC.model(TK.widen(zv), TK.widen(zn), lse, k, beta=(0.5, 2.0))
    assert np.array_equal(out["pair"].cpu().numpy(), pair) and np.array_equal(out["logp"].cpu().numpy().view(np.int32), logp.view(np.int32))
