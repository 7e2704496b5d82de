"""Child-process bodies of tests/test_gpu_grad_clip_ranks.py: everything that owns a process group runs here, never in the
pytest process (the rule of tests/dist_child.py).

    python tests/clip_child.py main <result.pt> <JSON list of main_temporal arguments>
    python tests/clip_child.py ranks <result.json>          # parent of two rank processes
    python tests/clip_child.py rank <r> <port> <result.json>

``main``: one main_temporal run; the result holds its logged gradient-norm figures per epoch and its final weights.
``ranks``: two REAL rank processes on the box's one GPU (gloo transport, the pattern of tools/two_rank_check.py) step the
3-task MTL step with clipping on, eagerly and as staged graphs."""
import json
import logging
import os
import re
import subprocess
import sys
from pathlib import Path

REPO = Path(__file__).resolve().parents[1]
if str(REPO) not in sys.path:
    sys.path.insert(0, str(REPO))


def run_main(out_path, args):
    import torch
    import main_temporal
    lines = []

    class Keep(logging.Handler):
        def emit(self, record):
            lines.append(record.getMessage())
    logging.getLogger().addHandler(Keep())
    logging.getLogger().setLevel(logging.INFO)
    torch.manual_seed(3)
    out = main_temporal.main(args)
    norms = []
    for l in lines:
        m = re.search(r"gradient norm mean (\S+), largest (\S+), clipped (\d+) of (\d+) steps \(max norm \S+\), skipped (\d+)", l)
        if m:
            norms.append([float(m.group(1)), float(m.group(2)), int(m.group(3)), int(m.group(4)), int(m.group(5))])
    opt = out["step"].optimizer
    torch.cuda.synchronize()
    capture = ("staged graphs" if isinstance(out["step"]._graph, list) else
               "one graph incl. the gradient exchange" if getattr(out["step"], "_graph_has_exchange", False) else "one graph")
    torch.save({"norms": norms, "flat_p": opt.flat_p.detach().cpu(), "capture": capture,
                "replayed": [l for l in lines if "replayed the captured step" in l]}, out_path)


def run_rank(rank, port, out_path):
    import argparse
    import torch
    import torch.distributed as dist
    from egopack_amd import dist as edist
    from egopack_amd import ops
    from tools import two_rank_check as TR
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=2)
    device = torch.device("cuda:0")
    args = argparse.Namespace(hidden=128, batch=4, T=8)
    B = args.batch
    ops.set_compute("bf16")

    def run(limit, graph, shard=False, compress="none"):
        ops.manual_seed(5)
        step, opt, dev, merged = TR.build(args, device, rank * B, (rank + 1) * B, edist.GradSync(2, shard_update=shard, compress=compress))
        opt.max_grad_norm = float(limit)  # (before the first step builds the flat buffers)
        norms = []
        if graph:
            step.capture(dev, merged, warmup=2)
            for _ in range(2):
                step.replay()
                norms.append(step.grad_norm_stats(reset=False)["last_norm"])
        else:
            for _ in range(4):
                step.step(dev, merged)
                norms.append(step.grad_norm_stats(reset=False)["last_norm"])
        torch.cuda.synchronize()
        kind = "staged graphs" if isinstance(step._graph, list) else "eager" if step._graph is None else "one graph"
        return norms, opt.flat_p.detach().cpu().clone(), step.grad_norm_stats(), kind

    def same_on_both(t):
        both = [torch.empty_like(t) for _ in range(2)]
        dist.all_gather(both, t)
        return bool(torch.equal(both[0].view(torch.int16), both[1].view(torch.int16)))
    first, _, _, _ = run(1e30, False)
    limit = 0.5 * first[0]
    res = {"first_norms": first, "limit": limit}
    for name, graph, compress in (("eager", False, "none"), ("graph", True, "none"), ("graph_bf16", True, "bf16")):
        norms, par, stats, kind = run(limit, graph, compress=compress)
        res[name] = {"norms": norms, "stats": stats, "kind": kind, "finite": bool(torch.isfinite(par).all()),
                     "norms_bit_identical": same_on_both(torch.tensor(norms, dtype=torch.float64)),
                     "params_bit_identical": same_on_both(par)}
        res[name + "_par"] = par
    res["graph_vs_eager_max_abs"] = float((res.pop("graph_par") - res.pop("eager_par")).abs().max())
    res.pop("graph_bf16_par")
    try:
        run(limit, False, shard=True)
        res["sharded"] = "no error"
    except RuntimeError as e:
        res["sharded"] = str(e)
    dist.barrier()
    if rank == 0:
        Path(out_path).write_text(json.dumps(res))
    dist.barrier()
    dist.destroy_process_group()


def run_ranks(out_path):
    import socket
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    procs = [subprocess.Popen([sys.executable, str(Path(__file__).resolve()), "rank", str(r), str(port), str(out_path)], env=env)
             for r in range(2)]
    rcs = [p.wait() for p in procs]
    sys.exit(0 if rcs == [0, 0] else 1)


if __name__ == "__main__":
    mode = sys.argv[1]
    if mode == "main":
        run_main(sys.argv[2], json.loads(sys.argv[3]))
    elif mode == "ranks":
        run_ranks(sys.argv[2])
    else:
        run_rank(int(sys.argv[2]), int(sys.argv[3]), sys.argv[4])
