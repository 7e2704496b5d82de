"""Gradient clipping over the N-rank gradient-exchange paths (dist.GradSync): the exchange dry run through the configuration key
(captured staged graphs on one GPU), and two real rank processes.  Every run owns its process group in a child process
(tests/clip_child.py)."""
import json
import os
import subprocess
import sys
from pathlib import Path

import pytest
import torch

pytestmark = pytest.mark.gpu
REPO = Path(__file__).resolve().parents[1]
CHILD = str(REPO / "tests" / "clip_child.py")


def _main_run(tmp_path, name, args, env=None):
    out = tmp_path / f"{name}.pt"
    r = subprocess.run([sys.executable, CHILD, "main", str(out), json.dumps(args + [f"checkpoint_dir={tmp_path / name}"])],
                       capture_output=True, text=True, timeout=600, env=None if env is None else dict(os.environ, **env))
    assert r.returncode == 0 and out.exists(), f"{name}: rc {r.returncode}\n{r.stdout[-1500:]}\n{r.stderr[-4000:]}"
    return torch.load(out, weights_only=False)


@pytest.mark.timeout(900)
@pytest.mark.parametrize("compress", ["none", "bf16"])
def test_exchange_dry_run_with_grad_clip_norm(tmp_path, compress):
    """main_temporal.py ... exchange_dry_run=2 grad_clip_norm=X: the run completes through the captured exchange, and its logged
    norms and final weights equal the same run without exchange_dry_run to the degree the UNCLIPPED pair of runs agrees (that pair
    runs here too, with a bound that clamps -- grad_clip_norm=1e30, bit for bit the unclipped update -- so that it logs its norms;
    its distance times two is the bound).

    A dry run on ONE process steps on 1 / N of its own gradient (the peers' contributions are what is missing), so it reports
    1 / N of the plain run's norm: the dry runs get grad_clip_norm = X / N, and their norms are compared times N."""
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    groups = [f"{g}=synthetic_resident" for g in ("dataset_recognition", "dataset_lta", "dataset_oscc", "dataset_pnr")]
    base = [*groups, "k=1", "batch_size=4", "synthetic_samples=24", "model.hidden_size=64", "model.temporal_pooling.hidden_size=64",
            "oscc_feat_size=64", "num_epochs=2", "enabled_tasks=[ar,lta,pnr]", "compute=bf16", "model.temporal_pooling.dropout=0"]
    dry = ["exchange_dry_run=2", f"grad_compress={compress}"]
    N = 2
    loose = _main_run(tmp_path, "loose", base + ["grad_clip_norm=1e30"])
    loose_dry = _main_run(tmp_path, "loose_dry", base + dry + ["grad_clip_norm=1e30"])
    limit = 0.5 * loose["norms"][0][0]  # (half the first epoch's mean norm: clipping is active)
    clip = _main_run(tmp_path, "clip", base + [f"grad_clip_norm={limit!r}"])
    clip_dry = _main_run(tmp_path, "clip_dry", base + dry + [f"grad_clip_norm={limit / N!r}"])
    assert clip_dry["capture"] == "staged graphs" and loose_dry["capture"] == "staged graphs" and clip["capture"] == "one graph"
    assert clip_dry["replayed"] and not clip_dry["replayed"][-1].startswith("epoch 2: 0 steps"), clip_dry["replayed"]
    assert len(clip["norms"]) == len(clip_dry["norms"]) == 2
    assert clip["norms"][0][2] >= 1 and clip_dry["norms"][0][2] >= 1 and loose["norms"][0][2] == 0  # (clipped steps)
    assert all(e[4] == 0 for e in clip["norms"] + clip_dry["norms"])  # (none skipped)

    def dist_w(a, b):
        return float((a["flat_p"].double() - b["flat_p"].double()).norm() / a["flat_p"].double().norm())

    def dist_n(a, b):
        return max(abs(N * y[k] - x[k]) / x[k] for x, y in zip(a["norms"], b["norms"]) for k in (0, 1))
    w_loose, w_clip, n_loose, n_clip = dist_w(loose, loose_dry), dist_w(clip, clip_dry), dist_n(loose, loose_dry), dist_n(clip, clip_dry)
    print(f"grad_compress={compress}: weights, relative distance dry run vs plain: unclipped {w_loose:.3e}, clipped {w_clip:.3e}; "
          f"norms (mean / largest per epoch), largest relative difference: unclipped {n_loose:.3e}, clipped {n_clip:.3e}")
    assert w_clip <= 2 * w_loose, (w_clip, w_loose)
    assert n_clip <= 2 * n_loose, (n_clip, n_loose)
    if compress == "none":
        # the opt-in capture that holds the collectives and the Adam slices in ONE graph: the same bounds
        one = _main_run(tmp_path, "clip_dry_one", base + dry + [f"grad_clip_norm={limit / N!r}"], env={"EGK_ENABLE": "one_graph_exchange"})
        assert one["capture"] == "one graph incl. the gradient exchange", one["capture"]
        assert one["replayed"] and not one["replayed"][-1].startswith("epoch 2: 0 steps"), one["replayed"]
        w_one, n_one = dist_w(clip, one), dist_n(clip, one)
        print(f"one graph incl. the collectives: weights {w_one:.3e}, norms {n_one:.3e}")
        assert w_one <= 2 * w_loose and n_one <= 2 * n_loose, (w_one, n_one)


@pytest.mark.timeout(900)
def test_two_rank_processes_clip_to_the_same_norm(tmp_path):
    """Two real rank processes (gloo transport, both on the box's one GPU): with clipping active both report the same norm bit for
    bit at every step and end with identical parameters -- eagerly and through the staged graphs, f32 and bf16 exchange; the
    sharded update refuses the combination on both ranks with an error that says so."""
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    out = tmp_path / "ranks.json"
    r = subprocess.run([sys.executable, CHILD, "ranks", str(out)], capture_output=True, text=True, timeout=800)
    assert r.returncode == 0 and out.exists(), f"rc {r.returncode}\n{r.stdout[-1500:]}\n{r.stderr[-4000:]}"
    res = json.loads(out.read_text())
    print(json.dumps(res, indent=1))
    assert res["limit"] > 0
    for name in ("eager", "graph", "graph_bf16"):
        leg = res[name]
        assert leg["norms_bit_identical"] and leg["params_bit_identical"] and leg["finite"], (name, leg)
        assert leg["stats"]["steps"] == 4 and leg["stats"]["clipped"] >= 1 and leg["stats"]["skipped"] == 0, (name, leg)
    assert res["graph"]["kind"] == "staged graphs" and res["graph_bf16"]["kind"] == "staged graphs"
    # (tools/two_rank_check.py: replayed steps = eagerly issued steps, bit for bit, with clipping off -- and with it on)
    assert res["graph_vs_eager_max_abs"] == 0.0 and res["graph"]["norms"] == res["eager"]["norms"][2:]
    assert "sharded update" in res["sharded"] and "clipping" in res["sharded"]
