"""The seeded sampler of the LTA futures on the GPU (include/egopack_sample.h) against the host model of
tests/lta_sampling_common.py.

  exact       with the optional outputs, lo <= t < hi for every sample, t = fl32(u_host * total_dev) recomputed in numpy: the
              selection logic and the Philox stream bit for bit, no tolerance, and no sample takes the fallback
  tolerance   lo / total and hi / total within (C + 8) * 2^-23 of the fp64 CDF (C terms of f32 accumulation in any association
              plus a few ulp of expf: derived, not measured), hence the device sample IS the fp64 model's wherever u is farther
              than that from every CDF boundary, and the model's or an adjacent live class elsewhere -- no case is left out
  shapes      rows {1, 3, 5, 44} x C {1, 2, 7, 63, 64, 65, 115, 478, 513} x K {1, 4, 5, 8, 9} (K = 5, 8, 9 cross a Philox call; 513
              classes take a second chunk), f32 and bf16, ld > C with NaN in the padding columns, logits on a 2^-10 grid in
              [-8, 8] (x - max is exact in f32; the bf16 rounding of a grid value is a grid value)

then zero-probability classes, invalid rows, the chi-square test of the CPU file on the device's samples, the counter identities,
the dtype twin, views, the rank invariance of the LTA meter and the loop-level repeatability.

Largest share of samples inside the tolerance band of a CDF boundary over the shape grid (checked like all others, never skipped;
printed by the last case of the grid): profiles/lta_sampling_cost.txt."""
import numpy as np
import pytest
import torch

from tests import lta_sampling_common as LS

pytestmark = pytest.mark.gpu

DEV = "cuda"
ROWS, CS, KS = (1, 3, 5, 44), (1, 2, 7, 63, 64, 65, 115, 478, 513), (1, 4, 5, 8, 9)
SEED = 1234
TRN_CFG = {"_target_": "egopack_amd.models.temporal_pooling.trn_pooling.TRNPooling", "dropout": 0.0, "hidden_size": 64}
BAND = {"near": 0, "all": 0, "worst": 0.0, "cases": 0}  # samples inside the tolerance band of a boundary, over the shape grid


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from egopack_amd import ops
    return ops


def grid_logits(rows, C, dtype, seed):
    """Random logits on the 2^-10 grid in [-8, 8] as a [rows, C] VIEW of a wider buffer whose padding columns hold NaN; the
    float64 values the device sees."""
    g = torch.Generator().manual_seed(seed)
    x = (torch.randint(-8192, 8193, (rows, C), generator=g).float() / 1024.0).to(dtype)
    buf = torch.full((rows, C + 5), float("nan"), dtype=dtype)
    buf[:, :C] = x
    return buf.to(DEV)[:, :C], x.double().numpy()


def launch(ops, views, K, seed, ordinal, row0=0):
    outs, dbg = ops.categorical_sample_multi(views, K, seed, ordinal, row0, debug=True)
    return [o.cpu().numpy() for o in outs], [tuple(d.cpu().numpy() for d in t) for t in dbg]


@pytest.mark.parametrize("C", CS)
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_samples_are_exact_against_the_host_stream_and_within_the_derived_tolerance(ops, dtype, C):
    near = total = 0
    for rows in ROWS:
        for K in KS:
            h, ordinal = (rows + K) % 3, rows * 7 + K
            view, x64 = grid_logits(rows, C, dtype, seed=C * 1000 + rows * 10 + K)
            assert view.stride(0) == C + 5 and view.shape == (rows, C)
            # the head index is the position in the list: heads in front of it get one-class rows
            heads = [torch.zeros(rows, 1, device=DEV, dtype=dtype) for _ in range(h)] + [view]
            outs, dbg = launch(ops, heads, K, SEED, ordinal)
            u = LS.uniforms(SEED, ordinal, 0, rows, h, K)
            n, t = LS.check_launch(outs[h], *dbg[h], x64, u)
            near, total = near + n, total + t
            for j in range(h):  # (a one-class row: always class 0, lo = 0, hi = total = 1)
                assert (outs[j] == 0).all() and (dbg[j][0] == 0).all() and (dbg[j][1] == 1).all() and (dbg[j][2] == 1).all()
    share = near / total
    BAND["near"], BAND["all"], BAND["worst"], BAND["cases"] = BAND["near"] + near, BAND["all"] + total, max(BAND["worst"], share), BAND["cases"] + 1
    print(f"tolerance band: C={C} {str(dtype)[6:]}: {near} of {total} samples ({share:.3e})")
    if BAND["cases"] == 2 * len(CS):
        print(f"tolerance band over the grid: {BAND['near']} of {BAND['all']} samples, largest share of a case {BAND['worst']:.3e}")


@pytest.mark.parametrize("C,alive", [(7, (0,)), (7, (6,)), (65, (0, 64)), (115, (3, 64, 114)), (513, (0, 511, 512)), (513, (512,)),
                                     (478, (0, 8, 477))])
def test_zero_probability_classes_never_come_back(ops, C, alive):
    """-inf on all but 1, 2 or 3 scattered classes (class 0 and class C - 1 among them; 511 | 512 straddles the chunks): only those
    come back, and the optional outputs satisfy everything they satisfy on dense rows."""
    rows, K = 5, 9
    view, x64 = grid_logits(rows, C, torch.float32, seed=C + len(alive))
    dead = np.ones(C, dtype=bool)
    dead[list(alive)] = False
    x64[:, dead] = -np.inf
    view[:, torch.from_numpy(dead).to(DEV)] = float("-inf")
    # the live classes of a row get comparable weights: logits in [-0.5, 0.5], still on the grid
    x64[:, ~dead] = np.round(x64[:, ~dead] / 16.0 * 1024.0) / 1024.0
    view[:, torch.from_numpy(~dead).to(DEV)] = torch.from_numpy(x64[:, ~dead]).float().to(DEV)
    outs, dbg = launch(ops, [view], K, SEED, 2)
    assert set(np.unique(outs[0]).tolist()) <= set(alive)
    LS.check_launch(outs[0], *dbg[0], x64, LS.uniforms(SEED, 2, 0, rows, 0, K))
    if len(alive) > 1:
        assert len(np.unique(outs[0])) == len(alive)  # (45 draws over 2 or 3 classes of comparable weight: each one is drawn)


@pytest.mark.parametrize("C", [7, 513])
def test_invalid_rows_get_minus_one_and_leave_their_neighbours_alone(ops, C):
    rows, K = 5, 9
    view, x64 = grid_logits(rows, C, torch.float32, seed=C)
    x64[1, :] = -np.inf
    view[1, :] = float("-inf")
    x64[3, C - 1] = np.nan
    view[3, C - 1] = float("nan")
    clean, clean64 = grid_logits(rows, C, torch.float32, seed=C)
    outs, dbg = launch(ops, [view], K, SEED, 4)
    assert (outs[0][[1, 3]] == -1).all() and (outs[0][[0, 2, 4]] >= 0).all()
    assert all((d[[1, 3]] == 0).all() for d in dbg[0])
    LS.check_launch(outs[0], *dbg[0], x64, LS.uniforms(SEED, 4, 0, rows, 0, K))
    ref, _ = launch(ops, [clean], K, SEED, 4)
    assert np.array_equal(outs[0][[0, 2, 4]], ref[0][[0, 2, 4]])
    view[3, C - 1] = float("inf")  # a +inf: no finite maximum either
    outs, _ = launch(ops, [view], K, SEED, 4)
    assert (outs[0][[1, 3]] == -1).all() and np.array_equal(outs[0][[0, 2, 4]], ref[0][[0, 2, 4]])


@pytest.mark.parametrize("C", [7, 115])
def test_device_samples_pass_the_chi_square_test_of_the_host_model(ops, C):
    """tests/test_lta_sampling_cpu.py's case on the device's samples, against the same constant."""
    x = torch.from_numpy(np.repeat(LS.CHI_LOGITS[C][None], LS.CHI_ROWS, 0)).float().to(DEV)
    outs, dbg = launch(ops, [x], LS.CHI_K, LS.CHI_SEED, LS.CHI_ORDINAL)
    u = LS.uniforms(LS.CHI_SEED, LS.CHI_ORDINAL, 0, LS.CHI_ROWS, 0, LS.CHI_K)
    near, total = LS.check_launch(outs[0], *dbg[0], x.double().cpu().numpy(), u)
    stat = LS.chi_square(outs[0], C)
    print(f"chi-square C={C}: {stat:.3f} (bound {LS.CHI_BOUND[C]:.3f}); {near} of {total} samples inside the tolerance band")
    assert stat < LS.CHI_BOUND[C], (stat, LS.CHI_BOUND[C])


def test_counter_identities(ops):
    rows, K = 44, 9
    a, _ = grid_logits(rows, 115, torch.float32, seed=1)
    b, _ = grid_logits(rows, 478, torch.float32, seed=2)
    both = ops.categorical_sample_multi([a, b], K, SEED, 6)
    # row r of a launch from row0 = 0 is row 0 of a launch over the slice that starts at r, with row0 = r
    for r in (1, 17, 43):
        part = ops.categorical_sample_multi([a[r:], b[r:]], K, SEED, 6, row0=r)
        assert torch.equal(part[0], both[0][r:]) and torch.equal(part[1], both[1][r:])
    # two heads in one launch = two single-head launches (the second as head 1: a one-class head in front of it)
    one = ops.categorical_sample_multi([a], K, SEED, 6)
    two = ops.categorical_sample_multi([torch.zeros(rows, 1, device=DEV), b], K, SEED, 6)
    assert torch.equal(one[0], both[0]) and torch.equal(two[1], both[1])
    # the seed, the ordinal and the head index each change the draws; the same arguments repeat them
    assert torch.equal(ops.categorical_sample_multi([a, b], K, SEED, 6)[1], both[1])
    assert not torch.equal(ops.categorical_sample_multi([a, b], K, SEED + 1, 6)[0], both[0])
    assert not torch.equal(ops.categorical_sample_multi([a, b], K, SEED, 7)[0], both[0])
    assert not torch.equal(ops.categorical_sample_multi([b, a], K, SEED, 6)[1], both[0])  # (a as head 1)
    # a smaller K is a prefix of a larger one
    assert torch.equal(ops.categorical_sample_multi([a, b], 5, SEED, 6)[0], both[0][:, :5])
    assert both[0].dtype == torch.int64 and both[0].shape == (rows, K) and both[0].is_contiguous()


@pytest.mark.parametrize("C", [7, 115, 478, 513])
def test_bf16_logits_and_their_f32_widening_give_the_same_samples(ops, C):
    g = torch.Generator().manual_seed(C)
    x16 = (torch.randn(44, C, generator=g) * 3).to(torch.bfloat16).to(DEV)  # (any bf16 values, not only grid values)
    a = ops.categorical_sample_multi([x16], 9, SEED, 1)[0]
    b = ops.categorical_sample_multi([x16.float()], 9, SEED, 1)[0]
    assert torch.equal(a, b) and int(a.min()) >= 0
    mixed = ops.categorical_sample_multi([x16, x16.float()], 9, SEED, 1)  # (a mixed list is widened: head 0 is unchanged)
    assert torch.equal(mixed[0], a)


def test_strided_row_stepped_and_offset_views_are_read_in_place(ops):
    g = torch.Generator().manual_seed(3)
    big = torch.full((90, 140), float("nan"))
    x = torch.randn(44, 115, generator=g) * 2
    big[1:89:2, 9:124] = x
    big = big.to(DEV)
    view = big[1:89:2, 9:124]  # offset, padded and every second row: unit class stride, so no copy
    assert view.stride() == (280, 1) and torch.equal(view.cpu(), x)
    want = ops.categorical_sample_multi([x.to(DEV)], 5, SEED, 0)[0]
    assert torch.equal(ops.categorical_sample_multi([view], 5, SEED, 0)[0], want)
    t = x.t().contiguous().to(DEV).t()  # class stride 44: the one layout that is copied
    assert t.stride() == (1, 44)
    assert torch.equal(ops.categorical_sample_multi([t], 5, SEED, 0)[0], want)
    assert ops.categorical_sample_multi([x.to(DEV)[:0]], 5, SEED, 0)[0].shape == (0, 5)  # no rows: nothing launched
    with pytest.raises(RuntimeError, match="K in 1 .. 1024"):
        ops.categorical_sample_multi([view], 1025, SEED, 0)
    with pytest.raises(RuntimeError, match="batch ordinal"):
        ops.categorical_sample_multi([view], 5, SEED, 1 << 24)


def _lta_setup():
    import egopack_amd.data as data
    from egopack_amd.models import Graph
    from egopack_amd.models.tasks import LTATask
    H = 64
    ds = data.SyntheticTaskDataset("lta", 22, 8, 3, 48, (7, 11), k=1, seed=5)
    torch.manual_seed(1)
    model = Graph(48, hidden_size=H, depth=2, temporal_pooling=TRN_CFG, num_segments=3).to(DEV)
    return ds, model, LTATask(H, H, (7, 11)).to(DEV)


def test_sharded_lta_validation_merges_to_the_single_pass_numbers_with_a_sampler(ops):
    """The setup of test_batch_sharded_validation_merges_to_the_single_pass_numbers (tests/test_gpu_meters.py), which has to skip
    the f64 edit-distance sums of the LTA meter because the futures come from torch's generator.  With a FutureSampler the merged
    two-rank meter equals the single pass on EVERY sum, and a second single pass equals the first."""
    import egopack_amd.data as data
    import egopack_amd.meters as meters
    import egopack_amd.validate as validate
    ds, model, task = _lta_setup()

    def run(rank, world, sampler):
        dl = data.build_dataloader(ds, 4, False, 0, False, 1, rank=rank, world_size=world, shard="batches")
        meter = meters.build_meter_for_dataset(ds, device=DEV)
        validate.validate_lta(model, dl, meter, task, device=DEV, sampler=sampler)
        return meter

    sampler = ops.FutureSampler(11)
    whole, again = run(0, 1, sampler), run(0, 1, sampler)
    merged = run(0, 2, sampler).merge(run(1, 2, sampler))
    assert merged.counter == whole.counter == again.counter and merged.loss_n == whole.loss_n
    n64 = 0
    for a, b, c in zip(merged._sums(), whole._sums(), again._sums()):
        n64 += a.dtype == torch.float64
        assert torch.equal(b, c), "two single passes differ"
        if a.dtype == torch.int64:
            assert torch.equal(a, b)
        else:
            torch.testing.assert_close(a, b, rtol=1e-12, atol=1e-12)
    assert n64 >= 1  # (the f64 sums -- the edit distances among them -- were compared, not skipped)
    got, want = merged.get_logs(), whole.get_logs()
    for k, v in want.items():
        if isinstance(v, (int, float)):
            assert got[k] == pytest.approx(v, rel=1e-12, abs=1e-12), k
    assert 0 < want["verbs_ed"] <= 1 and 0 < want["nouns_ed"] <= 1
    other = run(0, 1, ops.FutureSampler(12)).get_logs()
    assert (other["verbs_ed"], other["nouns_ed"]) != (want["verbs_ed"], want["nouns_ed"])  # (the seed matters)
    # without a sampler the torch path still runs
    old = run(0, 1, None)
    assert old.counter == whole.counter and 0 < old.get_logs()["verbs_ed"] <= 1


def test_validate_metrics_with_philox_sampling_repeats_itself(ops):
    import egopack_amd.data as data
    import main_temporal
    from egopack_amd import train as T
    ds, model, task = _lta_setup()
    sampler = T.build_lta_sampler(T.load_config(["lta_sampling.mode=philox", "lta_sampling.seed=3"]))
    assert isinstance(sampler, ops.FutureSampler) and sampler.seed == 3
    runs = []
    for _ in range(2):
        dl = {"lta": data.build_dataloader(ds, 4, False, 0, False, 1)}
        torch.manual_seed(len(runs))  # (torch's generator is not what the futures come from)
        runs.append(main_temporal.validate_metrics(1, model, {"lta": task}, ["lta"], {"lta": ds}, dl, DEV, sampler=sampler)["lta"])
    assert runs[0]["verbs_ed"] == runs[1]["verbs_ed"] and runs[0]["nouns_ed"] == runs[1]["nouns_ed"]
    assert runs[0] == runs[1] and 0 < runs[0]["verbs_ed"] <= 1
