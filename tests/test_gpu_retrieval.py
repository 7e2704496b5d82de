"""The retrieval report launch (include/egopack_retrieval.h) and ``GraphONE.record_retrieval`` on the GPU.

``wins`` must be, bit for bit, the histogram of the ``arg`` that ``egk_gather_max_fwd`` writes on the same inputs (called through
``_lib``), and the host model's (tests/retrieval_common.py) on inputs with planted ties.  ``dist`` is compared with the same formula
in float64 from the same f32 inputs, N(0, 1) values, under ``retrieval_common.dist_bound``: (H / 64 + 16) * 2^-24, absolute for the
cosine distance and relative for l2 (the derivation is in that module).  The largest observed error is printed.

Every (H, k) pair of HS x KS is a case; inside it the rows, the bank size, the number of tasks, the distance and the activation type
rotate so that every value of each meets every H and every k."""
import ctypes as C
import itertools

import numpy as np
import pytest
import torch

from tests import retrieval_common as RC

pytestmark = pytest.mark.gpu
DEV = "cuda"
f32, bf16, i64 = torch.float32, torch.bfloat16, torch.int64


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


def _gather_max_arg(f_act, bank, nn):
    """uint8 [N, H]: the winners egk_gather_max_fwd writes (contiguous operands, the launch's own stream)."""
    from egopack_amd import _lib, ops
    N, H = f_act.shape
    m = torch.empty_like(f_act)
    arg = torch.empty((N, H), dtype=torch.uint8, device=f_act.device)
    p = lambda t: C.c_void_p(t.data_ptr())
    rc = _lib.load().egk_gather_max_fwd(C.c_void_p(torch.cuda.current_stream().cuda_stream), p(f_act), p(bank), p(nn), p(m), p(arg), N, H,
                                        nn.shape[1], ops._dt(f_act))
    assert rc == 0, _lib.last_error()
    return arg


def _histogram(arg, k):
    return torch.stack([(arg == j).sum(1) for j in range(k + 1)], 1).to(torch.int32)


def _problem(g, N, H, k, K, dt, ties=False):
    """(f f32, f_act dt, bank f32, nn) on the device.  ``ties``: half-integer grid values, the activation row equal to the f32 row."""
    make = RC.grid if ties else (lambda r, c, g: torch.randn(r, c, generator=g))
    f, bank = make(N, H, g), make(K, H, g)
    f_act = f.to(dt) if ties else torch.randn(N, H, generator=g).to(dt)
    return f.to(DEV), f_act.to(DEV), bank.to(DEV), RC.lists(N, K, k, g).to(DEV)


def _check(f, f_act, bank, nn, distance, dist, wins, worst):
    H, k = f.shape[1], nn.shape[1]
    # wins: the histogram of the gather-max's own winners, bit for bit, and the host model
    arg = _gather_max_arg(f_act.contiguous(), bank.contiguous(), nn.contiguous())
    assert wins.dtype == torch.int32 and torch.equal(wins, _histogram(arg, k))
    assert np.array_equal(wins.cpu().numpy(), RC.wins_model(RC.widen(f_act), RC.widen(bank), nn.cpu().numpy()))
    assert bool((wins.sum(1) == H).all())
    # dist against float64
    ref = RC.dist_model(RC.widen(f), RC.widen(bank), nn.cpu().numpy(), distance)
    err = np.abs(dist.cpu().numpy().astype(np.float64) - ref)
    if distance == "l2":
        err = err / ref
    worst[distance] = max(worst.get(distance, 0.0), float(err.max()))
    assert float(err.max()) <= RC.dist_bound(H), (distance, H, k, float(err.max()), RC.dist_bound(H))


@pytest.mark.parametrize("H,k", list(itertools.product(RC.HS, RC.KS)))
def test_report_equals_the_gather_max_winners_and_the_float64_distances(H, k):
    _need_gpu()
    from egopack_amd import ops
    g = torch.Generator().manual_seed(1000 * H + k)
    turn = RC.HS.index(H) + RC.KS.index(k)
    worst = {}
    combos = list(itertools.product(("cosine", "l2"), (f32, bf16)))
    for i, rows in enumerate(RC.ROWS):
        for j, (distance, dt) in enumerate(combos):
            K = (k, 37, 500)[(turn + i + j) % 3]
            n_tasks = (1, 3)[(turn + i + j // 2) % 2]
            probs = [_problem(g, rows, H, k, K, dt) for _ in range(n_tasks)]
            outs = ops.retrieval_report([p[0] for p in probs], [p[1] for p in probs], [p[2] for p in probs], [p[3] for p in probs],
                                        distance_func=distance)
            assert len(outs) == n_tasks
            for (f, f_act, bank, nn), (dist, wins) in zip(probs, outs):
                assert dist.shape == (rows, k) and dist.dtype == f32 and wins.shape == (rows, k + 1)
                _check(f, f_act, bank, nn, distance, dist, wins, worst)
    for distance, e in worst.items():
        print(f"retrieval_report H={H} k={k} {distance}: largest error {e:.3e} ({e / RC.U:.2f} u), bound {RC.dist_bound(H):.3e} "
              f"({RC.dist_bound(H) / RC.U:.2f} u)")


@pytest.mark.parametrize("dt", [f32, bf16], ids=["f32", "bf16"])
@pytest.mark.parametrize("H,k,K", [(200, 4, 37), (8, 1, 1), (1024, 32, 500), (64, 4, 4)])
def test_wins_on_planted_ties_equal_the_host_model(H, k, K, dt):
    """bf16-representable grid values: most channels have several sources at the maximum, the node's own row included; an all-NaN
    channel, an all -inf channel and a node that equals one of its prototypes are planted."""
    _need_gpu()
    from egopack_amd import ops
    g = torch.Generator().manual_seed(H + k)
    f, f_act, bank, nn = _problem(g, 67, H, k, K, dt, ties=True)
    bank[:, 3], f_act[:, 3], f[:, 3] = float("nan"), float("nan"), float("nan")
    bank[:, 5], f_act[:, 5], f[:, 5] = float("-inf"), float("-inf"), float("-inf")
    f_act[7] = bank[nn[7, k - 1]].to(dt)
    (dist, wins), = ops.retrieval_report([f], [f_act], [bank], [nn])
    want = RC.wins_model(RC.widen(f_act), RC.widen(bank), nn.cpu().numpy())
    assert np.array_equal(wins.cpu().numpy(), want) and bool((wins.sum(1) == H).all())
    assert torch.equal(wins, _histogram(_gather_max_arg(f_act, bank, nn), k))
    assert int(wins[7, k]) == 0 and int(wins[:, 0].min()) >= 2  # (the copy never wins; the NaN and the -inf channel go to source 0)
    assert int((wins[:, 1:] > 0).sum()) > 0 or k == 1 and K == 1
    assert bool(torch.isnan(dist).all())  # (a NaN channel in every row: what the reference's formula gives)


@pytest.mark.parametrize("distance", ["cosine", "l2"])
@pytest.mark.parametrize("dt", [f32, bf16], ids=["f32", "bf16"])
def test_bits_do_not_depend_on_grouping_layout_or_the_outputs_asked_for(distance, dt):
    _need_gpu()
    from egopack_amd import ops
    g = torch.Generator().manual_seed(11)
    N, H, k = 67, 200, 4
    probs = [_problem(g, N, H, k, K, dt) for K in (37, 500, 4)]
    cols = lambda i: [p[i] for p in probs]
    group = ops.retrieval_report(cols(0), cols(1), cols(2), cols(3), distance_func=distance)
    for p, (dist, wins) in zip(probs, group):
        # alone
        (d1, w1), = ops.retrieval_report([p[0]], [p[1]], [p[2]], [p[3]], distance_func=distance)
        assert torch.equal(d1.view(torch.int32), dist.view(torch.int32)) and torch.equal(w1, wins)
        # one output only
        (d2, none), = ops.retrieval_report([p[0]], [p[1]], [p[2]], [p[3]], distance_func=distance, want_wins=False)
        (nothing, w2), = ops.retrieval_report([p[0]], [p[1]], [p[2]], [p[3]], distance_func=distance, want_dist=False)
        assert none is None and nothing is None
        assert torch.equal(d2.view(torch.int32), dist.view(torch.int32)) and torch.equal(w2, wins)
        # padded, offset views: an offset of whole 16-byte groups (rows stay vector-aligned) and an odd one (element loads)
        for off, pad in ((8, 16), (1, 3)):
            def view(t, fill):
                wide = torch.full((t.shape[0] + 2, t.shape[1] + off + pad), fill, dtype=t.dtype, device=t.device)
                wide[1:-1, off:off + t.shape[1]] = t
                v = wide[1:-1, off:off + t.shape[1]]
                assert not v.is_contiguous() and v.stride(0) > t.shape[1]
                return v
            args = [view(p[0], float("nan")), view(p[1], float("nan")), view(p[2], float("nan")), view(p[3], 0)]
            (d3, w3), = ops.retrieval_report(*[[a] for a in args], distance_func=distance)
            assert torch.equal(d3.view(torch.int32), dist.view(torch.int32)) and torch.equal(w3, wins), (off, pad)


# ---- GraphONE.record_retrieval --------------------------------------------------------------------------------------------------------
def _graphone(mode, k=4, H=64, K=37):
    from egopack_amd import ops
    from egopack_amd.models.graphONE.graphONE import GraphONE
    gen = torch.Generator(device=DEV).manual_seed(5)
    banks = {t: torch.randn(K, H, device=DEV, generator=gen) for t in ("ar", "lta", "pnr")}
    torch.manual_seed(3)
    go = GraphONE(banks, features_size=H, hidden_size=H, k=k, depth=2, residual=True).to(DEV)
    feats = {t: torch.randn(21, H, device=DEV, generator=gen) for t in ("ar", "lta", "pnr")}
    return go, feats


@pytest.mark.parametrize("mode", ["f32", "bf16"])
@pytest.mark.parametrize("parallel", [True, False], ids=["task-streams", "one-stream"])
def test_record_retrieval_keeps_what_the_interaction_used_and_changes_nothing(mode, parallel):
    _need_gpu()
    from egopack_amd import ops
    with ops.compute_mode(mode):
        go, feats = _graphone(mode)
        go.parallel_tasks = parallel
        go.eval()
        assert go.last_retrieval == {}
        with torch.no_grad():
            plain, closest0 = go.interact(feats)
            assert go.last_retrieval == {}  # (off by default)
            with go.record_retrieval() as kept:
                out, closest = go.interact(feats)
            torch.cuda.synchronize()
            assert kept is go.last_retrieval and sorted(kept) == ["ar", "lta", "pnr"]
            for t in feats:
                assert out[t].dtype == plain[t].dtype and torch.equal(out[t].float(), plain[t].float()), t  # bit-identical outputs
                assert torch.equal(closest[t][0], closest0[t][0])
                r = kept[t]
                assert sorted(r) == ["features", "features_act", "nn"]
                assert r["features"].dtype == f32 and torch.equal(r["features"], feats[t])
                assert r["features_act"].dtype == ops.act_dtype() and torch.equal(r["features_act"].float(), feats[t].to(ops.act_dtype()).float())
                assert r["nn"].shape == (21, 4) and r["nn"].dtype == i64 and torch.equal(r["nn"][:, 0], closest[t][0])
                assert torch.equal(r["nn"], ops.nearest_prototypes(r["features"], go.embeddings[t].weight, 4, go.distance_func))
            # after the block nothing more is kept, and what was kept stays readable
            again, _ = go.interact({t: f + 1 for t, f in feats.items()})
            assert all(torch.equal(go.last_retrieval[t]["features"], feats[t]) for t in feats)
            # the report on the kept tensors: the nearest prototype is the first entry, the distances ascend within the bound
            tasks = list(kept)
            rep = ops.retrieval_report([kept[t]["features"] for t in tasks], [kept[t]["features_act"] for t in tasks],
                                       [go.embeddings[t].weight for t in tasks], [kept[t]["nn"] for t in tasks], go.distance_func)
            for t, (dist, wins) in zip(tasks, rep):
                assert bool((wins.sum(1) == 64).all())
                assert bool((dist[:, 1:] - dist[:, :-1] >= -2 * RC.dist_bound(64)).all())
        # grad mode or training: nothing is recorded (and a new block starts empty)
        with go.record_retrieval() as kept:
            assert kept == {}
            go.interact(feats)
            assert kept == {}
            go.train()
            with torch.no_grad():
                go.interact(feats)
            assert kept == {} and go.last_retrieval == {}
            go.eval()
