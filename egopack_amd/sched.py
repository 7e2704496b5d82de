"""The step's launch scheduler: on which stream and in which launch a weight gradient, a norm reduction or a "rider" is issued --
late forks, the weight-gradient side streams, the parking queue with its grouped launches, the step's tail, the per-step scope.
The ops say what their weight gradient is (``issue_*``); the engine sets a step's schedule (``step_schedule``, the hooks, the joins)."""
from __future__ import annotations

import contextlib
from collections import namedtuple
from types import SimpleNamespace

import torch

F32 = 0  # EGK_COMPUTE_F32 (ops.F32)
# parked work: a dW contraction ``gemm(*args, **kw)`` (``out``: its gradient slot; ``tiles``: its output tiles, counted when it is parked)
# and a norm layer's dw / db reduction (the arguments of egk_ln_bwd_reduce)
Problem = namedtuple("Problem", "args kw out tiles")
Reduction = namedtuple("Reduction", "ws dw db rows cols n_seg")
Fork = namedtuple("Fork", "key event fn")  # a deferred fork: ``fn(event)`` goes out behind the next launch of the stream ``key``


def _ops():  # (the launches a flush issues -- gemm, gemm_grouped, the reduction launch: nothing of ops is imported at module level)
    from . import ops
    return ops


def stream_key(stream) -> tuple:
    return (stream.device.index, stream.cuda_stream)


def tiles(M: int, N: int) -> int:  # (128 x 128 output tiles of an M x N contraction)
    return ((M + 127) // 128) * ((N + 127) // 128)


# ---- late forks --------------------------------------------------------------------------------------------------------------
# Launches forked to another stream are ISSUED one launch late: after the forking stream's NEXT library launch, behind an event
# recorded at the fork point.  Same dependencies, same work -- but under hipGraph capture the child of a fork that is created first
# stays on the parent's hardware queue and the other pays a cross-queue hand-off.  A backward pass issues the forked weight gradient
# first, so the dX CHAIN hopped at every fork (tools/exp/fork_order.py: 12 links with a forked weight gradient each, 601 us per
# replay side-launch-first, 500 us chain-first).  ``on``: switched per step (``step_schedule``).
_deferred = SimpleNamespace(items=[], busy=False, on=True)


def defer_after_next_launch(fn) -> None:
    """Run ``fn(event)`` right after the current stream's next library launch (``event``: recorded on the current stream now);
    immediately if the mechanism is off.  ``fn`` issues work on OTHER streams behind ``event``."""
    cur = torch.cuda.current_stream()
    ev = torch.cuda.Event()
    ev.record(cur)
    if not _deferred.on:
        fn(ev)
        return
    _deferred.items.append(Fork(stream_key(cur), ev, fn))


def drain_deferred(all_streams: bool = True) -> None:
    """Issue the deferred side launches now (every join point calls this first; ``ops._ck`` after every launch, for its stream only)."""
    if _deferred.busy or not _deferred.items:
        return
    key = stream_key(torch.cuda.current_stream())
    take = [it for it in _deferred.items if all_streams or it.key == key]
    _deferred.items = [it for it in _deferred.items if not (all_streams or it.key == key)]
    _deferred.busy = True
    try:
        for it in take:
            it.fn(it.event)
    finally:
        _deferred.busy = False


# ---- weight-gradient side streams --------------------------------------------------------------------------------
# A dW contraction (64 tiles of 128 x 128, walked as <= 256 workgroups) feeds nothing but the optimizer, while the dX chain it would
# sit in is a strict dependency chain of launches, many of them small.  When the gradient lands in the flat buffer (no tensor goes
# back to autograd) the launch goes to a side stream forked from the backward stream there; ``join_wgrad()`` (queued as an
# end-of-backward callback of the autograd engine) joins every side stream with the stream that called backward().  Off by default:
# measured on MI355X it gains 3-4 % on the multi-task steps (M = 6144 backbone rows, heads on their own streams) and loses 3-5 % on
# single-task steps (M = 2048: every launch is already a partial-chip launch); the engine turns it on per step (``step_schedule``).
# ``handoff``: the end of a backward() call does NOT make the backward stream wait for the side streams: the engine takes them over
# (``take_wgrad_streams``) and orders its gradient exchange behind them, so the next stage's dX chain starts beside these gradients.
_wgrad = SimpleNamespace(enabled=False, streams={}, pending=[], queued=False, exclude=set(), handoff=False)


def exclude_wgrad_streams(streams) -> None:
    """Backward work running on these streams keeps its weight-gradient launches (the task-head streams of the engine already
    overlap each other; forking each of them again oversubscribes the hardware queues)."""
    _wgrad.exclude.update(stream_key(st) for st in streams)


def scope_excluded_streams(streams) -> None:
    """The excluded set becomes exactly ``streams`` (a step calls this with ITS head / task / side streams when it starts issuing: stream
    handles are pooled and handed out round-robin, so in a process that builds many steps -- a test suite -- the handles excluded by steps
    long gone would pile up until the next step's backward stream counts as a head stream and its weight gradients take other paths)."""
    _wgrad.exclude = {stream_key(st) for st in streams if st is not None}


def unexcluded_stream() -> torch.cuda.Stream:
    """A stream from the pool whose handle is not registered as a head / task stream (torch hands pooled handles out round-robin:
    a fresh ``torch.cuda.Stream()`` may alias one an earlier step excluded) -- for graph captures."""
    keep = []
    for _ in range(64):
        st = torch.cuda.Stream()
        if stream_key(st) not in _wgrad.exclude:
            return st
        keep.append(st)
    return keep[-1]


def _on_excluded_stream() -> bool:
    return stream_key(torch.cuda.current_stream()) in _wgrad.exclude


def wgrad_side_stream(main) -> torch.cuda.Stream | None:
    """The weight-gradient side stream of ``main`` if one has been created."""
    return _wgrad.streams.get(stream_key(main))


def _wgrad_launch(in_place: bool, tensors, launch, in_backward: bool = True):
    """Run ``launch()`` (weight / bias gradient kernels that only write persistent gradient slots) on the side stream of the current
    stream; ``tensors`` are the temporaries it reads (kept alive for that stream).  ``in_backward`` False: called from ``join_wgrad``
    itself (possibly after backward has returned): no end-of-backward callback is installed, the caller joins right away."""
    on = _wgrad.enabled and in_place and tensors and tensors[0].is_cuda
    main = torch.cuda.current_stream() if on else None
    key = stream_key(main) if on else None
    if not on or key in _wgrad.exclude:
        launch()
        return
    side = _wgrad.streams.get(key)
    if side is None:
        side = _wgrad.streams[key] = torch.cuda.Stream(device=main.device)

    def issue(ev):
        side.wait_event(ev)
        with torch.cuda.stream(side):
            launch()
        for t in tensors:
            if t is not None:
                t.record_stream(side)
    defer_after_next_launch(issue)  # (the closure keeps the operands alive until then)
    if side not in _wgrad.pending:
        _wgrad.pending.append(side)
    if in_backward and not _wgrad.queued:  # join at the end of THIS backward pass, on the stream of the thread that called it
        _wgrad.queued = True
        torch.autograd.Variable._execution_engine.queue_callback(join_wgrad)


def join_wgrad(force: bool = False):
    """The current stream waits for every weight-gradient side stream with work in flight (after backward, before the gradients are
    read: optimizer step, gradient exchange, end of a capture).  ``force``: the caller IS the step's backward stream (see flush_wgrad)."""
    if _wgrad.handoff and not force:
        return  # (end-of-backward callback while the engine hands the side streams to its exchange: take_wgrad_streams)
    for side in take_wgrad_streams(force):
        torch.cuda.current_stream().wait_stream(side)


def take_wgrad_streams(force: bool = True) -> list:
    """Issue whatever is parked, then hand over the side streams with weight-gradient work in flight: the CALLER orders its
    consumer of the gradients behind them (and eventually joins that consumer into the backward stream)."""
    flush_wgrad(in_backward=False, force=force)
    drain_deferred()
    streams, _wgrad.pending, _wgrad.queued = _wgrad.pending, [], False
    return streams


# ---- deferred, grouped weight gradients ------------------------------------------------------------------------------------
# A weight gradient of an H x H layer is a 64-tile contraction over K = all nodes: alone it fills a quarter of the chip, and split-K
# to fill it costs slabs plus a second launch (23 us + 8.7 us per launch, 12 of them in the headline step, all competing with the dX
# chain for the CUs).  With the queue on, such launches are PARKED (operands kept alive) and issued SIX AT A TIME as one grouped
# launch on the side stream: 384 workgroups, no slabs, no reduce launch, a sixth of the forks.  ``flush_wgrad`` issues what is parked.
# ``count``: bf16 problems per grouped launch for this step (None: WGRAD_GROUP_COUNT); ``items`` / ``reds``: Problem / Reduction
# records; ``riders``: callables; ``hold``: the tensors all of them read.
_wq = SimpleNamespace(on=False, count=None, items=[], tiles=0, hold=[], reds=[], riders=[])
# Six per launch: alone, six H x H problems in one launch of two 4-wave workgroups per CU run at 900 TF/s against 740 for four on
# one 8-wave workgroup per CU (tools/gemm_group_bench.py: x4 70 us, x6 85 us, x8 133 us at K = 6144).  Inside the step: 4 / 5 / 6 /
# 7 / 8 -> 1.558 / 1.60 / 1.538 / 1.60 / 1.595 ms (three alternating rounds of 200 steps; 12 H x H weight gradients = two launches of
# six).  Before the dX chain kept its hardware queue at the forks (defer_after_next_launch) six measured WORSE than four (1.75 vs
# 1.68).  The library takes up to 8 per launch.  A full group is issued at once, on the side stream: 1.474-1.477 ms, against
# 1.598-1.604 on the backward stream itself and 1.774-1.782 right before a backward row kernel, joined behind it (HISTORY.md).
WGRAD_GROUP_COUNT = 6
F32_WGRAD_GROUP_COUNT = 8


def _empty_queue():  # (nothing is parked from here on; returns what was: problems, reductions, riders, held tensors)
    was = (_wq.items, _wq.reds, _wq.riders, _wq.hold)
    _wq.items, _wq.reds, _wq.riders, _wq.hold, _wq.tiles = [], [], [], [], 0
    return was


def park_rider(fn, hold=()) -> None:
    """``fn()`` -- a launch that feeds nothing on the backward chain (a reported vector, say) -- rides with the next flush of the
    parked weight gradients: issued on their side stream, in front of the grouped launch.  Run at once when nothing can be parked
    (queue or side streams off, or on a task-head stream, whose parked work is issued by another stream)."""
    if not (_wq.on and _wgrad.enabled) or _on_excluded_stream():
        fn()
        return
    _wq.riders.append(fn)
    _wq.hold.extend(t for t in hold if t is not None)


def _wgrad_groupable(M, N, A, lda, B, ldb, K, compute=None) -> bool:
    if not (_wq.on and _wgrad.enabled) or A.dtype != B.dtype:
        return False
    if A.dtype == torch.bfloat16:
        ok = K % 64 == 0 and lda % 8 == 0 and ldb % 8 == 0
    elif A.dtype == torch.float32 and compute == F32:
        ok = K % 32 == 0 and lda % 4 == 0 and ldb % 4 == 0  # exact-f32 problems: the grouped f32 kernel (egk_gemm_grouped)
    else:
        return False
    return ok and A.data_ptr() % 16 == 0 and B.data_ptr() % 16 == 0 and tiles(M, N) <= 128


def _park(args, kw, tensors) -> None:
    M, N, out = args[0], args[1], args[7]  # (gemm's positional arguments: M, N, A, lda, B, ldb, K, out, ldc)
    _wq.items.append(Problem(args, kw, out, tiles(M, N)))
    _wq.hold.extend(t for t in tensors if t is not None)
    _wq.tiles += _wq.items[-1].tiles


def _wgrad_defer(args, kw, tensors, park_on_excluded: bool = False, park_only: bool = False) -> bool:
    """Park the dW contraction ``gemm(*args, **kw)`` (transA, transB, accumulate into a gradient slot) for the next grouped launch.
    False: not eligible (the caller launches it itself).  On an excluded stream (the engine's task-head streams) nothing is parked
    unless ``park_on_excluded``: such a problem is only PARKED there -- a later flush from the backward stream, which by then has
    joined the head streams (engine._run_heads), issues it, never the head stream itself, which would race the OTHER heads' operands."""
    excluded = _on_excluded_stream()
    if not _wgrad_groupable(*args[:7], kw.get("compute")) or (excluded and not park_on_excluded):
        return False
    _park(args, kw, tensors)
    if excluded or park_only:  # (park_only: a later weight-gradient launch of the same step takes it along, see _take_parked)
        return True
    # exact-f32 problems are matrix-pipe bound (a launch lasts as long as its fullest CU): EIGHT H x H problems, 512 tiles = two per CU
    count = F32_WGRAD_GROUP_COUNT if args[2].dtype == torch.float32 else (_wq.count or WGRAD_GROUP_COUNT)
    if len(_wq.items) >= count or _wq.tiles >= 64 * count:
        flush_wgrad()
    # (no end-of-backward join is scheduled for a parked problem: whoever switched the queue on -- engine.StepBase -- ends the step's
    #  LAST backward() call with ``join_wgrad(force=True)``, which issues what is parked.  A join after every backward() call made the
    #  next call's dX chain wait for weight gradients that feed only the optimizer: single-task step 0.915 -> 0.880 ms, multi-task neutral)
    return True


def issue_wgrad(args, kw, hold, *, park_on_excluded=False, park_only=False, eligible=True, in_place=True) -> bool:
    """An op's weight gradient ``gemm(*args, **kw)`` (``hold``: the temporaries it reads): parked for the next grouped launch if the
    op calls it ``eligible`` and the queue takes it (True), else launched -- on the side stream if it lands ``in_place`` in a slot."""
    if eligible and _wgrad_defer(args, kw, hold, park_on_excluded, park_only):
        return True
    _wgrad_launch(in_place, hold, lambda: _ops().gemm(*args, **kw))
    return False


def _take_parked(max_items: int):
    """Remove and return up to ``max_items`` parked weight-gradient problems as (args, kw) pairs (all of them or none: a partial
    take would reorder accumulations into one slot) for a caller that is about to issue a grouped launch of the same layout."""
    items = _wq.items
    if not items or len(items) > max_items:
        return []
    _wq.items, _wq.tiles = [], 0
    return [(p.args, p.kw) for p in items]


def issue_ln_reduce(ws, dw, db, rows, cols, n_seg) -> None:
    """A norm layer's dw / db reduction that goes to the side stream (``_ln_reduce_on_side`` said so): parked with the next grouped
    launch (the parked reductions are issued as ONE launch, egk_ln_bwd_reduce_multi), else launched there."""
    red = Reduction(ws, dw, db, rows, cols, n_seg)
    if _wq.on and _wgrad.enabled:
        _wq.reds.append(red)
        _wq.hold.append(ws)
    else:
        _wgrad_launch(True, (ws,), lambda: _ops()._launch_reductions([red]))


def reduction_batches(reds) -> list:
    """``reds`` in order, cut into batches of at most 8 reductions with DISTINCT targets: a parameter used several times in one step
    (per-task backbone passes) has several reductions accumulating into the same dw / db -- those stay in separate, ordered launches."""
    batches, seen = [], set()
    for r in reds:
        key = {r.dw.data_ptr(), r.db.data_ptr()}
        if not batches or len(batches[-1]) == 8 or key & seen:
            batches.append([])
            seen = set()
        batches[-1].append(r)
        seen |= key
    return batches


def flush_wgrad(in_backward: bool = True, force: bool = False, before_tail: bool = False):
    """Issue what is parked (``before_tail``: only if a tail range is set).  On an excluded (task-head) stream nothing is issued -- unless
    ``force``: the engine's own calls from the backward stream (end of a step's backward, the last-weight-gradient hook) must never leave
    parked work behind, whatever handle that stream has (a capture stream may alias a pooled handle an earlier step registered as excluded)."""
    if not (_wq.items or _wq.reds or _wq.riders) or (_on_excluded_stream() and not force) or (before_tail and _last_wgrad["tail"] is None):
        return  # (a head stream never issues what others parked)
    items, reds, riders, hold = _empty_queue()
    if any(_in_tail(p.out) for p in items) or any(_in_tail(r.dw) or _in_tail(r.db) for r in reds):
        _last_wgrad["leaked"] = True  # (a gradient of the tail range leaves for the side stream: see last_wgrad_tail_on_backward_stream)
    ops = _ops()

    def launch():
        ops.stamp("wgrad_flush", seq=True)  # (on the side stream: when this flush's launches can start)
        for fn in riders:
            fn()
        for i in range(0, len(items), 8):
            chunk = items[i:i + 8]
            ops.stamp("wgrad_group", seq=True)
            if len(chunk) == 1:
                ops.gemm(*chunk[0].args, **chunk[0].kw)
            else:
                # beside the dX chain a group runs on 4-WAVE workgroups also when it has <= 256 tiles (alone the 8-wave two-wave-group
                # variant is faster there: 70 vs 85 us for four H x H problems): an 8-wave workgroup takes 2 x 208 VGPRs of every SIMD
                # of its CU and the chain's row kernels (96-193 VGPRs) wait for it to leave -- a 13 us row-LayerNorm backward took 82 us
                # behind such a launch; 4 waves leave 304.  Step 1.511 -> 1.498 ms (six alternating runs of 300 steps, every pair)
                ops.gemm_grouped([(p.args, p.kw) for p in chunk], four_wave=len(chunk) <= 4)
        if reds:
            ops._launch_reductions(reds)
        ops.stamp("wgrad_flush_end", seq=True)
    _wgrad_launch(True, hold, launch, in_backward)


# ---- the step's tail and the per-step scope ------------------------------------------------------------------------------------
_last_wgrad = {"param": None, "hook": None, "pre": None, "inline": True, "tail": None, "leaked": False}
_wgrad_ln = {"side": True}  # (bench.py --ln-reduce-inline: False)
_g1_hook = {"fn": None}  # (the graphONE backward hook, ``set_graphone_backward_hook``)


def set_last_wgrad_tail(lo_ptr: int, hi_ptr: int) -> None:
    """With a last-weight-gradient hook installed: parked weight gradients and norm reductions whose gradient slots lie in the address
    range [lo_ptr, hi_ptr) are issued TOGETHER WITH the last weight gradient as one grouped launch on the backward stream (the caller's
    hook starts the optimizer on everything OUTSIDE that range meanwhile and steps the range after the launch).  Stand-alone, the first
    TRN linear's weight gradient takes 120 us and the two other TRN weight gradients as a group of their own 66 us; the three in one
    launch 123 us (tools/exp/tail_group_bench.py).  (0, 0): only the last weight gradient itself (the default)."""
    _last_wgrad["tail"] = (int(lo_ptr), int(hi_ptr)) if hi_ptr > lo_ptr else None
    _last_wgrad["leaked"] = False


def last_wgrad_tail_on_backward_stream() -> bool:
    """Every gradient of the tail range (``set_last_wgrad_tail``) was issued on the BACKWARD stream: no parked problem or reduction of
    the range left with an earlier flush for the side stream, no weight gradient of the range was launched there directly.  The optimizer
    slice over the range may then follow the last weight gradient on the backward stream without waiting for the side stream's queue."""
    return _last_wgrad["tail"] is not None and not _last_wgrad["leaked"]


def _in_tail(t) -> bool:
    rng = _last_wgrad["tail"]
    return rng is not None and rng[0] <= t.data_ptr() < rng[1]


def _take_tail_items():
    """Split what is parked by gradient-slot address: (contractions, reductions) inside the tail range are returned and removed
    from the queue; the rest stays parked (everything, when no tail range is set)."""
    red_in = lambda r: _in_tail(r.dw) and _in_tail(r.db)
    items = [p for p in _wq.items if _in_tail(p.out)]
    _wq.items = [p for p in _wq.items if not _in_tail(p.out)]
    reds = [r for r in _wq.reds if red_in(r)]
    _wq.reds = [r for r in _wq.reds if not red_in(r)]
    _wq.tiles = sum(p.tiles for p in _wq.items)
    return items, reds


def set_last_wgrad_hook(param, hook, pre=None) -> None:
    """``hook()`` is called (on the backward stream) just before the weight-gradient launch of ``param`` -- the engine marks the LAST
    weight gradient of the step with it to start the optimizer on everything else meanwhile.  ``pre()`` runs first, before what is parked
    is issued: a step joins there the backward branches still running on other streams (their parked problems read operands made there)."""
    _last_wgrad["param"], _last_wgrad["hook"], _last_wgrad["pre"] = param, hook, pre
    if hook is None:
        _last_wgrad["tail"] = None


def issue_last_or_wgrad(param, out, args, kw, hold, in_place: bool, eligible: bool) -> None:
    """The weight gradient ``gemm(*args, **kw)`` of a linear layer into ``out`` (``in_place``: it and the bias gradient are gradient slots;
    ``eligible``: a compute type the grouped launches serve): parked, else launched on the side stream.  The step's LAST one stays on the
    backward stream: nothing is left to overlap it with, and the hop to the side stream and back costs two hand-offs (~10 us each)."""
    last = param is _last_wgrad["param"] and _last_wgrad["hook"] is not None
    tail_items, tail_reds = [], []
    if last:
        if _last_wgrad["pre"] is not None:
            _last_wgrad["pre"]()
        tail_items, tail_reds = _take_tail_items()  # (issued below; the argument tuples keep their operands alive)
        flush_wgrad(force=True)  # (the hook starts the optimizer on every other slot: their gradients must be issued)
        _last_wgrad["hook"]()
    if last and (tail_items or tail_reds) and in_place and eligible:
        # the step's tail as ONE grouped launch on the backward stream: the range's parked weight gradients + this one (the largest
        # last), then the range's norm reductions
        if tail_items:
            _ops().gemm_grouped([(p.args, p.kw) for p in tail_items] + [(args, kw)])
        else:
            _ops().gemm(*args, **kw)
        if tail_reds:
            _ops()._launch_reductions(tail_reds)
    elif not (in_place and not last and eligible and _wgrad_defer(args, kw, hold)):
        if not last and _in_tail(out):
            _last_wgrad["leaked"] = True  # (launched below on the side stream)
        for p in tail_items:  # (not eligible after all: issue what was taken, in order)
            _ops().gemm(*p.args, **p.kw)
        if tail_reds:
            _ops()._launch_reductions(tail_reds)
        _wgrad_launch(in_place and not (last and _last_wgrad["inline"]), hold, lambda: _ops().gemm(*args, **kw))


def _ln_reduce_on_side(slot_w, slot_b, x) -> bool:
    """The norm layers' dw / db reduction moves to the weight-gradient side stream when there is one for this stream (side
    streams on, stream not one of the excluded head / task streams) and both gradients accumulate in place."""
    on = _wgrad.enabled and _wgrad_ln["side"] and slot_w is not None and slot_b is not None and x.is_cuda
    return bool(on) and not _on_excluded_stream()


def set_graphone_backward_hook(fn) -> None:
    """``fn()`` is called on the backward stream at the end of the grouped GraphONE backward (``ops._GraphOneStages``), when
    every gradient of the stage parameters is either issued or parked -- the engine starts the optimizer on that region there."""
    _g1_hook["fn"] = fn


@contextlib.contextmanager
def step_schedule(side_streams: bool, grouping: bool, count: int | None = None, deferred_forks: bool = True, handoff: bool = False):
    """The scheduler's settings for ONE step being issued (egopack_amd.engine: every eager step and every capture runs inside one): weight
    gradients on side streams, the parking queue with ``count`` bf16 problems per grouped launch (None: WGRAD_GROUP_COUNT), the late issue
    of forked launches, the hand-over of the side streams to a gradient exchange.  Entering and leaving both drop whatever is parked or
    deferred: a step ends with ``join_wgrad`` (which issues it), so something is left only when a step was abandoned by an exception --
    its launches must not surface in, and its weight gradients must not be accumulated by, the next step.  Leaving also clears the hooks
    a step installs while it runs (``set_last_wgrad_hook`` with its ``pre`` and tail range, ``set_graphone_backward_hook``): no hook
    outlives its step.  Scopes nest: the inner one hands the outer one's settings back."""
    def install(enabled, on, per_launch, late, hand):
        _wgrad.enabled, _wgrad.handoff = bool(enabled), bool(hand)
        _wq.on, _wq.count = bool(on), None if per_launch is None else int(per_launch)
        _deferred.on, _deferred.items = bool(late), []
        _empty_queue()
    prev = (_wgrad.enabled, _wq.on, _wq.count, _deferred.on, _wgrad.handoff)
    install(side_streams, grouping, count, deferred_forks, handoff)
    try:
        yield
    finally:
        set_last_wgrad_hook(None, None)
        set_graphone_backward_hook(None)
        install(*prev)
