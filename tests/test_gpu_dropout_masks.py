"""Every dropout keep mask, bit for bit, against the host Philox model of tests/philox_ref.py.

The three places that draw -- the one-wave row LayerNorm, the workgroup-per-row LayerNorm, the flat dropout kernel -- at every
width class and on both sides of its boundaries; host offsets and device offset words beyond 2^32; the host stream's
bookkeeping (reservations cover what a launch consumes, launches are disjoint, ``rng_replay`` / ``manual_seed`` repeat); and
whole training steps, eager and replayed from a captured graph: which counters every launch of every step drew, and that the
device offset word moved exactly once per replay.  Philox is integer arithmetic and the keep decision is exact in f32: every
comparison is ``torch.equal``."""
import functools
import re
from pathlib import Path

import numpy as np
import pytest
import torch

from tests import philox_ref as P

pytestmark = pytest.mark.gpu
DEV = "cuda"
CSRC = Path(__file__).resolve().parents[1] / "egopack_amd" / "csrc"
DTYPES = [torch.float32, torch.bfloat16]


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


@pytest.fixture
def ops():
    """The ops module; the state of the dropout streams (host seed / offset, device offset word) is put back afterwards."""
    from egopack_amd import ops as _ops
    _ops.rng_device_offset(_device())
    state = _ops.get_rng_state()
    yield _ops
    _ops.set_rng_state(state)
    torch.cuda.synchronize()


def _device():
    return torch.device("cuda", torch.cuda.current_device())


def _word(ops) -> int:
    """The device offset word (one synchronisation)."""
    return int(ops.rng_device_offset(_device()).item())


def _set_stream(ops, seed, offset, word):
    ops.set_rng_state({"seed": seed, "offset": offset, "device": {_device().index: word}})


# the model's masks, computed once per (seed, offset, shape, p) and shared by the element types and the kernels that must agree
@functools.lru_cache(maxsize=None)
def _model_rows(seed, offset, rows, cols, p):
    m = torch.from_numpy(P.keep_mask_rows(seed, offset, rows, cols, p))
    return m


@functools.lru_cache(maxsize=None)
def _model_flat(seed, offset, n, p):
    return torch.from_numpy(P.keep_mask_flat(seed, offset, n, p))


@functools.lru_cache(maxsize=None)
def _rowln_inputs(rows, cols):
    g = torch.Generator().manual_seed(rows * 10007 + cols)
    x = torch.randn(rows, cols, generator=g) * 2 + 0.3
    return x.to(DEV), torch.randn(cols, generator=g).to(DEV), torch.randn(cols, generator=g).to(DEV)


def _rowln(ops, rows, cols, dt, p, relu=True):
    """One fused LayerNorm + dropout launch: (y, its saved keep mask) on the host."""
    x, w, b = _rowln_inputs(rows, cols)
    xi = x.to(dt).requires_grad_(True)
    with ops.compute_mode("bf16" if dt == torch.bfloat16 else "f32"):
        y = ops.row_layernorm(xi, w, b, 1e-5, relu=relu, p=p, training=True)
    mask = ops.last_rowln_mask(y)
    assert mask.dtype == torch.uint8 and mask.shape == (rows, cols)
    return y.detach().float().cpu(), mask.cpu()


def _flat(ops, n, dt, p):
    """One flat dropout launch over ones: (y != 0, its saved keep mask) on the host."""
    x = torch.ones(n, device=DEV, dtype=dt, requires_grad=True)
    y = ops.dropout(x, p, True)
    mask = y.grad_fn.saved_tensors[0]
    assert mask.dtype == torch.uint8 and mask.shape == (n,)
    return (y.detach() != 0).cpu(), mask.cpu()


def _check_rows(ops, seed, rows, cols, dt, p, word=0):
    """A launch at the stream's current position against the model at (that position + ``word``)."""
    snap = ops.rng_snapshot()
    y, mask = _rowln(ops, rows, cols, dt, p)
    want = _model_rows(seed, (snap + word) & P.MASK64, rows, cols, p)
    assert torch.equal(mask, want), (f"rows {rows} cols {cols} {dt} p {p} offset {snap} word {word}: "
                                     f"{int((mask != want).sum())} of {mask.numel()} mask elements differ from the model")
    assert bool((y[mask == 0] == 0).all())  # a dropped element is exactly 0
    return mask


# ---- a. row LayerNorm masks -----------------------------------------------------------------------------------------------------
WIDTHS = [40, 250, 256, 260, 1024, 1028, 1280, 2048, 3072, 4096]


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("cols", WIDTHS)
def test_row_layernorm_masks_equal_the_model(ops, cols, dt):
    """37 rows at every width class (S = 64 / 256 / 1024), both sides of its boundaries, the scalar mask stores of cols % 4 != 0,
    the FULL instantiation (1024) and the workgroup-per-row kernels (2048 / 3072 / 4096); three launches in a row, so that all but
    the first draw at a host offset that is not 0."""
    seed = 0x5EED0000 + cols
    ops.manual_seed(seed)
    for p in (0.1, 0.25, 0.5) + ((0.999,) if cols == 1024 else ()):
        mask = _check_rows(ops, seed, 37, cols, dt, p)
        assert 0 < int(mask.sum()) < mask.numel()


def _csrc_int(file, pattern, what):
    """An integer constant of a launcher, read from the source when a test needs it (a rewritten launcher fails that test with
    a message, not the collection of this file)."""
    m = re.search(pattern, (CSRC / file).read_text())
    if m is None:
        pytest.fail(f"{file}: {what} no longer matches /{pattern}/ -- choose the sizes of this test from the launcher as it is now")
    return int(m.group(1))


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("cols", [1024, 4096])
def test_row_layernorm_masks_at_1031_rows(ops, cols, dt):
    """1031 rows: more workgroups than the other cases, still one row per wave (one-wave kernel: 258 workgroups of 4 waves) or per
    workgroup (workgroup-per-row kernel: 1031 workgroups), dealt round-robin -- neither grid is a multiple of 8.  The cases in
    which a wave or workgroup walks several rows follow."""
    seed = 0xBEEF00 + cols
    ops.manual_seed(seed)
    _check_rows(ops, seed, 1031, cols, dt, 0.5)


# Row counts beyond one pass of the capped grids.  Workgroup-per-row kernels: grid = min(rows, 1536), a multiple of 8 once capped,
# so ``row_walk`` gives XCD x the contiguous rows [x * per, (x + 1) * per), per = ceil(rows / 8), and a workgroup walks them 192
# apart, two rows in flight.  1600 rows: per = 200, slots 0 .. 7 of every XCD have a pair, the others a single row.  3100 rows:
# per = 388, slots 0 .. 3 have a pair and then a single row (a ragged last pair), the others one pair; the last XCD owns 384 rows.
# One-wave kernels: grid = min(ceil(rows / 4), 768) workgroups of 4 waves; 3100 rows cap it, the walk is the ownership walk with
# per = 388 and step 384: the waves of slot 0 take a second row.
MANY_ROWS = 3100


def _wide_grid_cap():
    return _csrc_int("norm_ops.hip", r"const int grid = rows < (\d+) \? rows : \1;", "the grid of the workgroup-per-row LayerNorm forward")


def _one_wave_grid_cap():
    return _csrc_int("norm_ops.hip", r"CAP_WIDE = (\d+)[;,]", "the grid cap of the one-wave row kernels (CAP_WIDE)")


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("rows,cols", [(1600, 2048), (1600, 3072), (MANY_ROWS, 4096)])
def test_workgroup_per_row_kernel_masks_with_two_rows_in_flight(ops, rows, cols, dt):
    """A capped grid (a multiple of 8: the XCD-ownership walk) whose workgroups take a second row with the first: the counter of
    the second row in flight, of a single row behind a pair, and of every row the ownership walk hands out."""
    cap = _wide_grid_cap()
    assert cap % 8 == 0 and rows > cap and (rows + 7) // 8 > cap // 8  # (capped, owned by XCD, some workgroup has two rows)
    if rows == MANY_ROWS:
        assert 2 * (cap // 8) < (rows + 7) // 8 < 3 * (cap // 8)  # (some workgroups: a pair and then a single row)
    seed = 0xC0FFEE00 + cols
    ops.manual_seed(seed)
    _check_rows(ops, seed, rows, cols, dt, 0.5)


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("cols,one_wave", [(1024, False), (250, False), (4096, True)])
def test_one_wave_kernel_masks_with_several_rows_per_wave(ops, cols, one_wave, dt):
    """More rows than one pass of the capped grid of the one-wave kernels (768 workgroups x 4 waves): the ownership walk, and
    waves that take a second row.  1024 is the FULL instantiation, 250 the scalar mask stores; 4096 runs with egk_tune 7 = 0
    and shares its model with the workgroup-per-row case above."""
    from egopack_amd import _lib
    lib = _lib.load()
    cap = _one_wave_grid_cap()
    assert cap % 8 == 0 and MANY_ROWS > 4 * cap
    seed = 0xC0FFEE00 + cols
    prev = lib.egk_tune(7, 0) if one_wave else None
    try:
        ops.manual_seed(seed)
        _check_rows(ops, seed, MANY_ROWS, cols, dt, 0.5)
    finally:
        if one_wave:
            lib.egk_tune(7, prev)


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("rows,cols", [(37, 2048), (37, 4096), (1031, 4096)])
def test_one_wave_reference_kernel_masks_equal_the_model(ops, rows, cols, dt):
    """The one-wave-per-row kernels at the widths the workgroup-per-row kernels normally take (egk_tune 7 = 0)."""
    from egopack_amd import _lib
    lib = _lib.load()
    seed = (0xBEEF00 + cols) if rows == 1031 else (0x5EED0000 + cols)  # (the seeds of the tests above: their models are reused)
    prev = lib.egk_tune(7, 0)
    try:
        ops.manual_seed(seed)
        for p in (0.5,) if rows == 1031 else (0.1, 0.25, 0.5):
            _check_rows(ops, seed, rows, cols, dt, p)
    finally:
        lib.egk_tune(7, prev)


# ---- b. flat dropout masks ------------------------------------------------------------------------------------------------------
def _ew_grid_cap() -> int:
    """The workgroup cap of ``ew_grid`` (csrc/loss_optim.hip): beyond 4 * 256 * cap elements the grid-stride loop takes a second lap."""
    return _csrc_int("loss_optim.hip", r"return \(unsigned\)\(b < 1 \? 1 : b > (\d+) \? \1 : b\);", "the workgroup cap of ew_grid")


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("n", [1, 3, 4, 1021, 1 << 16])
def test_flat_dropout_masks_equal_the_model(ops, n, dt):
    _check_flat(ops, n, dt)


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("extra", [3, 4 * 1025 + 3])
def test_flat_dropout_masks_on_the_second_lap_of_the_grid_stride_loop(ops, extra, dt):
    """4 * 256 * (the workgroup cap of ``ew_grid``) elements fill one lap of the capped grid; ``extra`` more start the second:
    3 (one thread, a tail of three elements) and 4 * 1025 + 3 (five workgroups, the last with one full group and the tail)."""
    _check_flat(ops, 4 * 256 * _ew_grid_cap() + extra, dt)


def _check_flat(ops, n, dt):
    seed = 0xF1A70000 + (n & 0xFFFF)
    ops.manual_seed(seed)
    for p in (0.25, 0.5):
        snap = ops.rng_snapshot()
        nonzero, mask = _flat(ops, n, dt, p)
        want = _model_flat(seed, snap, n, p)
        assert torch.equal(mask, want), f"n {n} {dt} p {p} offset {snap}: {int((mask != want).sum())} mask elements differ from the model"
        assert torch.equal(nonzero, want.bool())  # the output of an all-ones input carries the same pattern


# ---- c. offsets beyond 32 bits ----------------------------------------------------------------------------------------------------
HOST_OFFSET = 2 ** 32 - 100  # 37 rows of 1024 columns (S = 256) and 1021 flat elements (256 counters) both cross 2^32 from here


def _offset_cases(ops):
    word = 3 * ops.RNG_DEVICE_STRIDE + 5  # high counter word not 0, low word a multiple of nothing
    return {"host": (HOST_OFFSET, 0), "device": (0, word), "both": (HOST_OFFSET, word)}


def _wrapped_32(counters, seed, shape, p):
    """The mask a kernel would draw whose counter arithmetic is 32 bits wide (what the offset cases must tell from the model)."""
    words = P.philox_u64(counters & np.uint64(P.MASK32), seed)
    flat = words.reshape(shape[0], -1)[:, :shape[1]]
    return torch.from_numpy(P.keep_from_words(flat, p))


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("which", ["host", "device", "both"])
def test_row_layernorm_masks_at_offsets_beyond_32_bits(ops, which, dt):
    host, word = _offset_cases(ops)[which]
    seed = 0x0FF5E7
    _set_stream(ops, seed, host, word)
    assert ops.rng_snapshot() == host and _word(ops) == word
    got = _check_rows(ops, seed, 37, 1024, dt, 0.5, word=word)
    # the case discriminates: the model at the host offset alone, or at the truncated sum, is another mask
    if word:
        assert not torch.equal(got, _model_rows(seed, host, 37, 1024, 0.5))
    assert not torch.equal(got, _wrapped_32(P.row_counters(host + word, 37, 1024), seed, (37, 1024), 0.5))
    assert _word(ops) == word  # (a dropout launch reads the word, nothing else)


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("which", ["host", "device", "both"])
def test_flat_dropout_masks_at_offsets_beyond_32_bits(ops, which, dt):
    host, word = _offset_cases(ops)[which]
    seed = 0x0FF5E8
    _set_stream(ops, seed, host, word)
    _, mask = _flat(ops, 1021, dt, 0.5)
    assert torch.equal(mask, _model_flat(seed, host + word, 1021, 0.5))
    if word:
        assert not torch.equal(mask, _model_flat(seed, host, 1021, 0.5))
    assert not torch.equal(mask, _wrapped_32(P.flat_counters(host + word, 1021)[None, :], seed, (1, 1021), 0.5)[0])


# ---- d. the host stream's bookkeeping ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cols", [40, 250, 1024, 1028, 4096])
def test_stream_bookkeeping(ops, cols):
    """Launches of different shapes back to back (a LayerNorm of the width under test, a flat dropout, a LayerNorm of another
    class): each mask is the model's at its own snapshot, the counters the model says a launch consumed lie inside what the
    launch reserved -- at cols = 40 the rows are 64 counters apart, S * rows > rows * cols / 4 -- and no two launches share one;
    ``rng_replay`` and a second ``manual_seed`` give the same masks again."""
    seed, rows, p = 0xB00C + cols, 37, 0.5
    other = 250 if cols != 250 else 1280

    def run():
        out, snaps = [], [ops.rng_snapshot()]
        out.append(_rowln(ops, rows, cols, torch.float32, p)[1])
        snaps.append(ops.rng_snapshot())
        out.append(_flat(ops, 1021, torch.float32, p)[1])
        snaps.append(ops.rng_snapshot())
        out.append(_rowln(ops, 5, other, torch.float32, p)[1])
        snaps.append(ops.rng_snapshot())
        return out, snaps

    ops.manual_seed(seed)
    assert ops.rng_snapshot() == 0 and _word(ops) == 0
    first, snaps = run()
    assert snaps[0] == 0 and snaps == sorted(set(snaps))
    assert torch.equal(first[0], _model_rows(seed, snaps[0], rows, cols, p))
    assert torch.equal(first[1], _model_flat(seed, snaps[1], 1021, p))
    assert torch.equal(first[2], _model_rows(seed, snaps[2], 5, other, p))
    used = [P.row_intervals(snaps[0], rows, cols), P.flat_intervals(snaps[1], 1021), P.row_intervals(snaps[2], 5, other)]
    for k, iv in enumerate(used):
        lo, hi = P.span(iv)
        assert snaps[k] <= lo and hi <= snaps[k + 1], f"launch {k} drew [{lo}, {hi}) but reserved [{snaps[k]}, {snaps[k + 1]})"
    assert P.disjoint([i for iv in used for i in iv])
    # a second pass over the same calls under rng_replay: the same masks, and the stream ends where the first pass ended
    with ops.rng_replay(snaps[0]):
        again, snaps2 = run()
    assert snaps2 == snaps and ops.rng_snapshot() == snaps[-1]
    assert all(torch.equal(a, b) for a, b in zip(first, again))
    # replayed from the middle: the launches behind that snapshot only
    with ops.rng_replay(snaps[1]):
        assert torch.equal(_flat(ops, 1021, torch.float32, p)[1], first[1])
    after = _rowln(ops, 5, other, torch.float32, p)[1]  # (behind the replay the stream goes on where it was: fresh counters)
    assert torch.equal(after, _model_rows(seed, snaps[-1], 5, other, p)) and not torch.equal(after, first[2])
    ops.manual_seed(seed)
    third, snaps3 = run()
    assert snaps3 == snaps and all(torch.equal(a, b) for a, b in zip(first, third))


# ---- e. whole training steps --------------------------------------------------------------------------------------------------------
@pytest.fixture
def compute_restored():
    from egopack_amd import ops
    prev = ops.get_compute()
    yield
    ops.set_compute(prev)


def _build(compute, max_grad_norm):
    """The small MTL workload of tests/test_gpu_grad_clip.py with dropout 0.5: two fused LayerNorm + dropout launches per step,
    the second on a slab input.  (The builder seeds the dropout streams: host offset 0, device word 0.)"""
    from tests.test_gpu_grad_clip import _build as build
    return build("mtl", compute, max_grad_norm, dropout="0.5")


def _launch_model(rec, word):
    kind, seed, off, rows, cols = rec
    assert kind == "rows"
    return _model_rows(seed, (off + word) & P.MASK64, rows, cols, 0.5)


def _launch_intervals(rec, word):
    kind, seed, off, rows, cols = rec
    return P.row_intervals(off + word, rows, cols) if kind == "rows" else P.flat_intervals(off + word, cols)


@pytest.mark.parametrize("compute", ["f32", "bf16"])
def test_eager_steps_draw_the_model_masks(ops, compute, compute_restored):
    """Three eager steps: every tapped mask is the model's at the recorded (seed, host offset, rows, cols); the steps' counters
    are pairwise disjoint.  An eager step does not touch the device offset word -- its masks move on with the host offset."""
    step, opt, batches, merged = _build(compute, None)
    seed = ops.get_rng_state()["seed"]
    assert seed == 11 and ops.rng_snapshot() == 0 and _word(ops) == 0
    tap = ops.tap_dropout_masks()
    ends = []
    with tap as masks:
        for j in range(3):
            step.step(batches, merged)
            torch.cuda.synchronize()
            assert _word(ops) == 0
            ends.append((len(tap.launches), ops.rng_snapshot()))
    recs = list(tap.launches)
    rows_recs = [r for r in recs if r[0] == "rows"]
    per = ends[0][0]
    assert [e[0] for e in ends] == [per, 2 * per, 3 * per] and len(rows_recs) == len(masks) == 3 * 2
    assert all(r[1] == seed for r in recs)
    for rec, mask in zip(rows_recs, masks):
        assert torch.equal(mask.cpu(), _launch_model(rec, 0)), rec
    assert [r[3:] for r in recs[:per]] == [r[3:] for r in recs[per:2 * per]] == [r[3:] for r in recs[2 * per:]]
    # every launch draws inside its step's slice of the host stream, and no two launches of the run share a counter
    lo = 0
    for j, (n, hi) in enumerate(ends):
        for rec in recs[n - per:n]:
            a, b = P.span(_launch_intervals(rec, 0))
            assert lo <= a and b <= hi, (j, rec)
        lo = hi
    assert P.disjoint([i for rec in recs for i in _launch_intervals(rec, 0)])


@pytest.mark.parametrize("clip", [False, True])
def test_replayed_steps_draw_the_model_masks(ops, clip, compute_restored):
    """capture(warmup=2) + four replays: mask i of replay k is the model's at the host offset baked into the graph and the device
    word of that replay, and not at the neighbouring words; the word moves by exactly one stride per replay -- with clipping on it
    rides in the single gated optimizer launch, without in the first early one -- also in a replay whose step the gate skips; the
    counters of all launches of the run are pairwise disjoint; an eager step at replay k's stream state taps replay k's masks."""
    STRIDE = ops.RNG_DEVICE_STRIDE
    step, opt, batches, merged = _build("bf16", 1e-3 if clip else None)  # (a bound far below the gradient norm: every step is clipped)
    tap = ops.tap_dropout_masks()
    with tap as masks:
        step.capture(batches, merged, warmup=2)
    torch.cuda.synchronize()
    recs = list(tap.launches)
    per = len(recs) // 3
    assert per >= 2 and len(recs) == 3 * per and [r[3:] for r in recs[:per]] == [r[3:] for r in recs[2 * per:]]  # two eager steps + the capture
    rows_recs = [r for r in recs if r[0] == "rows"]
    assert len(rows_recs) == len(masks) == 3 * 2
    seed = 11
    assert all(r[1] == seed for r in recs)
    assert _word(ops) == 0  # (the eager warm-up steps leave the word alone, and issuing the captured step runs nothing)
    for rec, mask in zip(rows_recs[:4], masks[:4]):  # the warm-up steps
        assert torch.equal(mask.cpu(), _launch_model(rec, 0)), rec
    baked, static = rows_recs[4:], masks[4:]  # what the graph's launches were given, and the buffers they write
    snap = recs[2 * per][2]  # the host stream's position when the captured step was issued
    assert snap == min(r[2] for r in recs[2 * per:]) > max(r[2] for r in recs[:2 * per])
    drawn = [i for rec in recs[:2 * per] for i in _launch_intervals(rec, 0)]
    seen = {}
    x = merged.x
    for k in range(4):
        w0 = _word(ops)
        assert w0 == k * STRIDE
        poisoned = clip and k == 2
        if poisoned:  # a step the clipping gate skips (tests/test_gpu_grad_clip.py::test_skipped_step_inside_a_replayed_graph)
            keep = x[5, 1, 9].clone()
            x[5, 1, 9] = float("inf")
        step.replay()
        torch.cuda.synchronize()
        if poisoned:
            x[5, 1, 9] = keep
        assert _word(ops) - w0 == STRIDE, f"replay {k}: the device offset word moved by {_word(ops) - w0}"
        seen[k] = [m.cpu().clone() for m in static]
        for i, (rec, got) in enumerate(zip(baked, seen[k])):
            assert torch.equal(got, _launch_model(rec, w0)), f"replay {k} mask {i}"
            assert not torch.equal(got, _launch_model(rec, (w0 + STRIDE) & P.MASK64)), f"replay {k} mask {i}: the masks of replay {k + 1}"
            assert not torch.equal(got, _launch_model(rec, (w0 - STRIDE) & P.MASK64)), f"replay {k} mask {i}: the masks of replay {k - 1}"
        drawn += [i for rec in recs[2 * per:] for i in _launch_intervals(rec, w0)]
    assert P.disjoint(drawn), "two launches of the run drew the same counters"
    if clip:
        stats = step.grad_norm_stats()
        assert stats["skipped"] == 1 and stats["clipped"] >= 1 and stats["steps"] == 6, stats
    # eager against replay: the stream state replay 1 saw, the same sequence of launches issued eagerly
    state = ops.get_rng_state()
    _set_stream(ops, seed, state["offset"], 1 * STRIDE)
    with ops.rng_replay(snap), ops.tap_dropout_masks() as eager:
        step.step(batches, merged)
    torch.cuda.synchronize()
    assert len(eager) == len(static) and all(torch.equal(e.cpu(), s) for e, s in zip(eager, seen[1]))
    assert _word(ops) == STRIDE and ops.rng_snapshot() == state["offset"]
