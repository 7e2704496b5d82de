"""Training steps of the hot path (reference main_temporal.train :49-134, main_egopack.train
:64-159 and train_step_task :45-61) re-designed for MI355X:

  * the backbone runs ONCE per step over the node sets of all enabled task batches (fused pass,
    per-task graph-LayerNorm statistics), then each task's head / loss runs on its row slice;
  * the objective ``sum_t weight_t * loss_t.mean()`` is one deterministic reduction chain;
  * gradients accumulate inside the backward kernels into the optimiser's flat buffer, are
    exchanged by dist.GradSync (RCCL) when world_size > 1, and Adam is one launch;
  * ``capture()`` records forward + backward (+ Adam when single-GPU) of a fixed-shape step into a
    hipGraph (torch.cuda.CUDAGraph) so a replayed step costs one graph launch instead of ~300
    kernel launches from Python.
"""
from __future__ import annotations

import contextlib
import math
import queue
import threading
from typing import Dict, Mapping, Optional, Sequence

import torch

from . import ops, sched, switches
from .data import Data, merge_batches
from .criterion import MetricSelectorWrapper
from .dist import GradSync
from .optim import TASK_WEIGHTING_MODES

TASK_ORDER = ("ar", "lta", "oscc", "pnr")  # order of the loss terms in main_temporal.train


STRUCTURE_FIELDS = ("edge_index", "batch", "ptr", "ptr32", "graph")


def structure_key(b: Data) -> int:
    """Host-side fingerprint of a batch's graph structure: sequence boundaries and edges (the CSR arrays derive from them)."""
    if b.__dict__.get("_arena") is not None and b.__dict__.get("_struct_key"):
        return b.__dict__["_struct_key"]  # (the native builder's: a hash of the samples' graph templates)
    parts = []
    for name in ("edge_index", "ptr"):
        v = getattr(b, name, None)
        if torch.is_tensor(v) and v.device.type == "cpu":
            parts.append((name, tuple(v.shape), hash(v.contiguous().numpy().tobytes())))
        elif torch.is_tensor(v):
            return 0  # (already on a device: no cheap fingerprint -- 0 never matches, everything is copied)
    return hash(tuple(parts)) or 1


def stage_batches(host, device, order=TASK_ORDER, pin: bool = True, store=None, dtype=None, features: bool = True):
    """Host -> device transfer of one step's task batches for the fused pass: the feature blocks are packed
    into ONE (pinned) buffer and moved with ONE copy; the returned per-task batches view row ranges of the
    device buffer and ``merged`` exposes the whole buffer (first contraction at M = all nodes).

    With a ``feature_store.FeatureStore`` and batches that carry ``x_idx`` instead of ``x`` nothing but the index
    matrices crosses PCIe: ONE gather launch builds the packed ``[sum N, S, F]`` buffer in HBM."""
    live = [t for t in order if host.get(t) is not None]
    resident = store is not None and all(getattr(host[t], "x", None) is None and getattr(host[t], "x_idx", None) is not None
                                         for t in live)
    if resident and all(host[t].__dict__.get("_arena") is not None for t in live):
        return _stage_arenas([host[t] for t in live], live, device, store, dtype, features)
    if resident:
        idx = torch.cat([host[t].x_idx for t in live])
        if pin and idx.device.type == "cpu":
            idx = idx.pin_memory()
        dbuf = store.gather(idx.to(device, non_blocking=True), dtype=dtype)
        rows = [host[t].x_idx.shape[0] for t in live]
    else:
        from .data import pack_features
        slot = []
        buf = pack_features([host[t] for t in live], pin=pin, ring_slot=slot)
        dbuf = buf.to(device, non_blocking=True)
        if slot and dbuf.is_cuda:  # the pinned staging buffer may be handed out again once this copy has completed
            ev = torch.cuda.Event()
            ev.record(torch.cuda.current_stream())
            slot[0][1] = ev
        rows = [host[t].x.shape[0] for t in live]
    from .data import to_device_packed
    dev, off = {}, 0
    saved = {}
    for t in live:  # everything but the features (they are already on the device) travels in ONE packed copy
        b = host[t]
        saved[t] = (b.x, getattr(b, "x_base", None), getattr(b, "x_idx", None))
        b.x = b.x_base = b.x_idx = None
        b._struct_key = structure_key(b)  # (lets merge_batches reuse the merged CSR of equal structures)
    placeholder = [torch.empty(0)] * len(live)
    for t, ph in zip(live, placeholder):  # merge on the host; the packed device buffer becomes its x below
        host[t].x, host[t].x_base = ph, None
    merged = merge_batches([host[t] for t in live])
    merged.x = None
    for t in live:
        host[t].x = host[t].x_base = None
    moved = to_device_packed([*(host[t] for t in live), merged], device)
    for t, n, d in zip(live, rows, moved[:-1]):
        d.x = dbuf[off:off + n]
        d.x_base = dbuf
        off += n
        dev[t] = d
    for t in live:
        host[t].x, host[t].x_base, host[t].x_idx = saved[t]
    md = moved[-1]
    md.x = md.x_base = dbuf
    if getattr(md, "_blob", None) is not None:
        md._blob.names = [*live, "merged"]
    # fingerprint of everything that describes the graphs (not the features / labels): equal keys = equal structure, so a
    # replay on static buffers (StepBase.train_step) need not rewrite the CSR arrays, edge lists and batch vectors
    for t in live:
        dev[t]._struct_key = host[t]._struct_key
    md._struct_key = hash(tuple(dev[t]._struct_key for t in live)) or 1
    return dev, md


def _stage_arenas(hs, live, device, store, dtype, features: bool = True):
    """``stage_batches`` for batches the native builder wrote into arenas (data.Arena): the merged batch comes from one host call,
    every batch travels as one memcpy into the transfer buffer -- the store rows with it -- and the packed feature block is gathered
    task by task from the device copy of those rows.  No tensor of the step is touched on the host.  ``features=False``: the block
    is NOT gathered here -- the transfer carries the store (``BlobRef.store``) and whoever consumes the batches gathers the rows
    where it wants them (a captured training step: straight into its idle input buffers, StepBase._input_slot;
    ``ensure_features`` for anything else)."""
    from .data import to_device_packed
    merged = merge_batches(hs)
    merged.x = None
    moved = to_device_packed([*hs, merged], device)
    rows = [h._arena.meta["num_nodes"] for h in hs]
    idx0 = moved[0].__dict__["x_idx"]
    x_dtype = dtype or store.table.dtype
    dbuf = torch.empty((sum(rows), idx0.shape[1], store.features_size), dtype=x_dtype, device=idx0.device) if features else None
    dev, off = {}, 0
    for t, n, h, d in zip(live, rows, hs, moved[:-1]):
        if features:
            store.gather(d.__dict__["x_idx"], out=dbuf[off:off + n], dtype=dtype)
            d.x = dbuf[off:off + n]
        d.x_base = dbuf
        d._struct_key = h.__dict__.get("_struct_key", 0)
        dev[t] = d
        off += n
    md = moved[-1]
    md.x = md.x_base = dbuf
    ref = getattr(md, "_blob", None)
    if ref is not None:
        ref.names = [*live, "merged"]
        ref.store, ref.x_dtype = store, x_dtype  # (what a consumer that gathers the rows itself needs)
    md._struct_key = hash(tuple(dev[t]._struct_key for t in live)) or 1
    return dev, md


def ensure_features(batches, merged=None) -> None:
    """Give batches that were staged without their feature block (``stage_batches(features=False)``) the block: gathered from the
    transfer's store on the current stream (no-op for batches that have it)."""
    live = [(t, b) for t, b in batches.items() if b is not None]
    if not live or all(b.__dict__.get("x") is not None for _, b in live):
        return
    ref = _shared_blob(batches, merged)
    store = getattr(ref, "store", None) if ref is not None else None
    if store is None:
        raise RuntimeError("batches without features and without a feature store to gather them from")
    idx = [b.__dict__["x_idx"] for _, b in live]
    dbuf = torch.empty((sum(i.shape[0] for i in idx), idx[0].shape[1], store.features_size), dtype=ref.x_dtype, device=idx[0].device)
    off = 0
    for (t, b), i in zip(live, idx):
        n = i.shape[0]
        store.gather(i, out=dbuf[off:off + n], dtype=ref.x_dtype)
        b.x, b.x_base = dbuf[off:off + n], (dbuf if merged is not None else None)
        off += n
    if merged is not None:
        merged.x = merged.x_base = dbuf


_COPY_STREAMS = {}  # device index -> the staging copy stream (StagedBatches)


STAGE_LOCK = threading.RLock()  # held by StagedBatches' thread while it stages, and by eager steps / captures (see ``_ahead``)


class StagedBatches:
    """Iterate a host-batch iterator one step AHEAD on a copy stream: while the device runs step i, the host collates batch
    i + 1 and its tensors cross PCIe (the packed feature block is 57 MB per step of the headline workload: 1.0 ms at 56
    GB/s, which would otherwise sit between two steps on the compute stream).  Yields ``(batches, merged)`` as
    ``stage_batches`` returns them (``merged`` None for a single task / per-task backbone passes), already ordered behind
    the copy on the consumer's stream."""

    def __init__(self, host_iter, device, order=TASK_ORDER, fused: bool = True, store=None, dtype=None, depth: Optional[int] = None,
                 step=None):
        self.it, self.device, self.order, self.fused, self.store, self.dtype = iter(host_iter), device, order, fused, store, dtype
        # the training step these batches feed (optional): once it gathers the store rows into its own input buffers
        # (``StepBase.gathers_inputs``) the feature block is no longer gathered here
        self.step = step
        # steps staged ahead by the staging thread (0: staged inline, right behind the consumer's launch of the step before)
        self.depth = 2 if depth is None else int(depth)
        # ONE copy stream per device for the life of the process: the caching allocator keeps a pool per stream, so a fresh
        # stream per epoch stranded every epoch's staging blocks in a pool nobody allocates from again (reserved memory grew
        # by ~130 MB per epoch of the headline workload while the allocated bytes stayed flat)
        self.copy_stream = None
        if torch.device(device).type == "cuda":
            key = torch.device(device).index if torch.device(device).index is not None else torch.cuda.current_device()
            self.copy_stream = _COPY_STREAMS.get(key)
            if self.copy_stream is None:
                # (a priority stream: the runtime keeps hardware queues per priority level, so the staging launches do not sit in a
                #  queue behind a branch of the replayed graph that is waiting for its dependencies)
                self.copy_stream = _COPY_STREAMS[key] = torch.cuda.Stream(device=device, priority=-1)

    def _stage(self, host):
        live = {t: b for t, b in host.items() if b is not None}
        features = not (self.store is not None and getattr(self.step, "gathers_inputs", False))
        if self.fused and len(live) > 1:
            return stage_batches(live, self.device, self.order, store=self.store, dtype=self.dtype, features=features)
        from .data import to_device_packed
        moved = to_device_packed([live[t] for t in live], self.device)  # (one copy for all of a step's tensors)
        ref = getattr(moved[0], "_blob", None) if moved else None
        if ref is not None:
            ref.names = list(live)
            if self.store is not None:
                ref.store, ref.x_dtype = self.store, self.dtype or self.store.table.dtype
        for t, d in zip(live, moved):
            d._struct_key = structure_key(live[t])
            if self.store is not None and getattr(d, "x", None) is None and getattr(d, "x_idx", None) is not None:
                if features or ref is None or "x_idx" not in d.__dict__:
                    d.x = self.store.gather(d.x_idx, dtype=self.dtype)  # features from the device-resident table
        return dict(zip(live, moved)), None

    def _fetch(self):
        try:
            host = next(self.it)
        except StopIteration:
            return None
        if self.copy_stream is None:
            return self._stage(host), None
        # (no wait for the compute stream: the caching allocator keeps per-stream pools, and what is allocated here is
        #  marked as used by the consumer's stream below)
        with torch.cuda.stream(self.copy_stream):
            staged = self._stage(host)
            done = torch.cuda.Event()
            done.record(self.copy_stream)
        return staged, done

    def _ahead(self):
        """``_fetch`` results from a thread of their own, ``depth`` steps ahead (None ends the walk, an exception is re-raised in
        the consumer).  The thread holds ``STAGE_LOCK`` while it stages: eager steps and captures take the same lock, so that
        nothing of another thread touches the HIP runtime while a capture is open and the launch-order bookkeeping of ``ops``
        has ONE writer; replays of the captured step -- every steady-state step -- do not take it and overlap the staging."""
        q, stop = queue.Queue(maxsize=self.depth), threading.Event()

        def put(item):
            while not stop.is_set():
                try:
                    q.put(item, timeout=0.05)
                    return True
                except queue.Full:
                    pass
            return False

        def produce():
            try:
                torch.cuda.set_device(self.copy_stream.device)
                while not stop.is_set():
                    with STAGE_LOCK:
                        nxt = self._fetch()
                    if not put(nxt) or nxt is None:
                        return
            except BaseException as e:  # noqa: BLE001 (handed to the consumer)
                put(e)
        if switches.debug("stage_profile"):
            inner = produce

            def produce():  # noqa: F811 (development: where the staging thread's time goes)
                import cProfile
                import pstats
                pr = cProfile.Profile()
                try:
                    pr.runcall(inner)
                finally:
                    pstats.Stats(pr).sort_stats("tottime").print_stats(35)
        th = threading.Thread(target=produce, name="egk-staging", daemon=True)
        th.start()
        try:
            while True:
                nxt = q.get()
                if nxt is None:
                    return
                if isinstance(nxt, BaseException):
                    raise nxt
                yield nxt
        finally:
            stop.set()
            th.join(timeout=10.0)

    def __iter__(self):
        def inline():
            nxt = self._fetch()
            while nxt is not None:
                yield nxt
                nxt = self._fetch()  # issued right after the consumer launched its step: overlaps it
        for nxt in (self._ahead() if (self.copy_stream is not None and self.depth > 0) else inline()):
            (batches, merged), done = nxt
            if done is not None:
                cur = torch.cuda.current_stream()
                cur.wait_event(done)
                ref = _shared_blob(batches, merged)
                if ref is not None:  # every tensor but the features is a view of the transfer's one buffer
                    ref.ready = done  # (what a consumer on another stream waits for: StepBase._input_slot)
                    used = [ref.dev, *(getattr(b, k, None) for b in [*batches.values(), merged] if b is not None
                                       for k in ("x", "x_base"))]
                else:
                    used = [v for _, v in [*(kv for b in batches.values() for kv in _walk(b)), *_walk(merged)]]
                for v in used:
                    if torch.is_tensor(v) and v.is_cuda:
                        v.record_stream(cur)  # allocated on the copy stream, consumed here
            yield batches, merged


# ---- static-shape batches: what a captured step may be replayed on ----------------------------------------------------
def _walk(obj, prefix=""):
    """(path, value) for every tensor / plain scalar reachable from a Data / CSRGraph (lists of tensors included)."""
    from dataclasses import fields, is_dataclass
    if obj is None:
        return
    if torch.is_tensor(obj):
        yield prefix, obj
    elif is_dataclass(obj):
        for f in fields(obj):
            yield from _walk(getattr(obj, f.name), f"{prefix}.{f.name}")
    elif isinstance(obj, Data):
        obj.materialise()
        for k in sorted(obj.__dict__):
            yield from _walk(obj.__dict__[k], f"{prefix}.{k}")
    elif isinstance(obj, (list, tuple)):
        for i, v in enumerate(obj):
            yield from _walk(v, f"{prefix}[{i}]")
    elif isinstance(obj, (int, float, bool, str)):
        yield prefix, obj


# Edge-sized arrays live in the static buffers of a captured step at a CAPACITY (data.EDGE_FIELDS / EDGE_BUCKET): the LTA edge
# count moves by a few entries from batch to batch, no kernel takes E, and the signature compares capacities.
from .data import EDGE_BUCKET, EDGE_FIELDS, VALUE_FIELDS, edge_capacity as _edge_capacity  # noqa: E402


def _is_edge_field(path: str) -> bool:
    return path.endswith(EDGE_FIELDS)


def batch_signature(batches: Mapping[str, Data], merged=None) -> tuple:
    """Everything a capture bakes in: the shape / dtype of every tensor (edge-sized arrays: their capacity) and every plain
    scalar (node counts, heavy-row modes ...) of the step's batches.  Two steps with equal signatures differ in tensor
    VALUES only.  Private attributes (``_struct_key`` ...) describe values, not shapes: they are not part of it."""
    sig = []
    for name, obj in [*sorted(batches.items()), ("merged", merged)]:
        for path, v in _walk(obj, name):
            if "._" in path or (torch.is_tensor(v) and v.dim() >= 1 and path.endswith(".x_base")):  # (x_base aliases x)
                continue
            if path.endswith(VALUE_FIELDS):  # (the batch ordinal: a value, baked into nothing)
                continue
            if torch.is_tensor(v):
                shape = tuple(v.shape)
                if _is_edge_field(path) and v.dim() >= 1:
                    shape = shape[:-1] + (_edge_capacity(shape[-1]),)
                sig.append((path, (shape, v.dtype)))
            else:
                sig.append((path, v))
    return tuple(sig)


def _fast_key(batches, merged):
    """A cheap stand-in for ``batch_signature`` when every batch carries a structure fingerprint: the fingerprints and the
    feature blocks' shapes / types (None: some batch has no fingerprint -- take the full signature)."""
    parts = []
    for name, b in [*sorted(batches.items()), ("merged", merged)]:
        if b is None:
            parts.append((name, None))
            continue
        k = getattr(b, "_struct_key", 0)
        x = getattr(b, "x", None)
        if not k or not torch.is_tensor(x):
            return None
        y = getattr(b, "y", None)
        # the labelled-row set of a compacted head is baked into a capture too (the strided row view ``live_ap`` and the padded
        # height of ``live_idx`` / ``live_y``): it depends on label VALUES, which the structure fingerprint does not cover
        li = getattr(b, "live_idx", None)
        parts.append((name, k, tuple(x.shape), x.dtype, tuple(y.shape) if torch.is_tensor(y) else None,
                      getattr(b, "live_ap", None), tuple(li.shape) if torch.is_tensor(li) else None))
    return tuple(parts)


def _shared_blob(batches, merged):
    """The ``data.BlobRef`` of a step whose batches all came out of ONE packed transfer with a layout signature, else None."""
    objs = [b for b in [*batches.values(), merged] if b is not None]
    ref = getattr(objs[0], "_blob", None) if objs else None
    if ref is None or ref.gsig is None or ref.names is None or any(getattr(b, "_blob", None) is not ref for b in objs):
        return None
    return ref


def _feature_key(batches, merged):
    """(name, shape, dtype) of every feature block of a step's batches -- also for batches staged without their block
    (``stage_batches(features=False)``): its shape follows from the store rows, its type is the transfer's."""
    ref = None
    out = []
    for name, b in [*sorted(batches.items()), ("merged", merged)]:
        if b is None:
            continue
        x = b.__dict__.get("x", None) if "x" in b.__dict__ else getattr(b, "x", None)
        if torch.is_tensor(x):
            out.append((name, tuple(x.shape), x.dtype))
            continue
        ref = ref or _shared_blob(batches, merged)
        store = getattr(ref, "store", None) if ref is not None else None
        if store is None:
            continue
        if name == "merged":
            idx = [bb.__dict__.get("x_idx") for _, bb in sorted(batches.items()) if bb is not None]
            if all(torch.is_tensor(i) for i in idx):
                out.append((name, (sum(i.shape[0] for i in idx), idx[0].shape[1], store.features_size), ref.x_dtype))
        else:
            i = b.__dict__.get("x_idx")
            if torch.is_tensor(i):
                out.append((name, (*i.shape, store.features_size), ref.x_dtype))
    return tuple(out)


def _static_from_blob(ref, batches, merged):
    """Private buffers for a capture out of a packed transfer: ONE byte buffer of the transfer's layout (edge-sized arrays at
    capacity) + clones of the feature blocks.  -> (buffer, static batches, static merged)."""
    blob = torch.empty_like(ref.dev)
    blob.copy_(ref.dev)
    outs = dict(zip(ref.names, ref.rebuild(blob, True)))
    static_m = outs.pop("merged", None) if merged is not None else None
    static_b = {t: outs.get(t) for t in batches}
    for dst, src in [*((static_b[t], batches[t]) for t in batches if batches[t] is not None), (static_m, merged)]:
        if dst is None:
            continue
        for k, v in src.__dict__.items():  # what was attached after the transfer (features, fingerprints)
            if k in ("_blob", "_fill") or k in dst.__dict__ and dst.__dict__[k] is not None:
                continue
            setattr(dst, k, v)
    if static_m is not None and torch.is_tensor(merged.x):
        static_m.x = merged.x.clone()
        _rewire_packed(static_b, static_m)
    else:
        for t, b in static_b.items():
            if b is not None and torch.is_tensor(b.x):
                b.x = batches[t].x.clone()
                b.x_base = None
    return blob, static_b, static_m


@torch.no_grad()
def copy_batch_values(dst_batches, dst_merged, src_batches, src_merged, dst_walks=None) -> None:
    """dst <- src for every tensor of two sets of batches with the same signature (device to device).  Per-task feature
    blocks that are row ranges of a packed buffer (``x_base``) are written once, through the buffer; edge-sized arrays are
    written into the first E entries of their capacity.  Graph-structure arrays are skipped when both sides carry the same
    non-zero structure fingerprint; after a full copy the destination takes over the source's fingerprint."""
    done = set()
    pairs = [(dst_batches[t], src_batches[t]) for t in sorted(dst_batches) if dst_batches[t] is not None]
    if dst_merged is not None:
        pairs.append((dst_merged, src_merged))
    for dst, src in pairs:
        smap = dict(_walk(src))
        base = getattr(dst, "x_base", None)
        k_dst, k_src = getattr(dst, "_struct_key", 0), getattr(src, "_struct_key", 0)
        same_structure = bool(k_dst) and k_dst == k_src
        if dst_walks is not None:  # (the destination's tensors never change: walked once per static batch)
            walk = dst_walks.get(id(dst))
            if walk is None:
                walk = dst_walks[id(dst)] = [(p_, d_) for p_, d_ in _walk(dst) if torch.is_tensor(d_) and not p_.endswith(".x_base")]
        else:
            walk = _walk(dst)
        for path, d in walk:
            if not torch.is_tensor(d) or path.endswith(".x_base"):
                continue
            if same_structure and path.split(".")[1].split("[")[0] in STRUCTURE_FIELDS:
                continue  # equal fingerprints (stage_batches): the graph arrays already hold these values
            s_ = smap.get(path)
            if s_ is None or d.data_ptr() == s_.data_ptr():
                continue
            if (path == ".x" and torch.is_tensor(base) and base.untyped_storage().data_ptr() == d.untyped_storage().data_ptr()
                    and d.numel() != base.numel()):
                continue  # a row range of the packed buffer: the buffer itself is copied as the merged batch's x
            key = (d.untyped_storage().data_ptr(), d.storage_offset(), tuple(d.shape))
            if key not in done:
                if d.shape != s_.shape and _is_edge_field(path):
                    d[..., :s_.shape[-1]].copy_(s_, non_blocking=True)  # (the tail keeps stale entries no row range reaches)
                else:
                    d.copy_(s_, non_blocking=True)
                done.add(key)
        if not same_structure:
            dst._struct_key = k_src  # (0 when the source's structure is unknown: the next copy is a full one again)


def _clone_batch(d: Data, pad_edges: bool = False) -> Data:
    """Deep copy of a device batch (own storage for every tensor; scalars shared).  ``pad_edges``: edge-sized arrays are
    allocated at their capacity (zeros behind the copied entries) -- the static buffers of a captured training step."""
    from dataclasses import fields, is_dataclass, replace

    def dup(path, t):
        if pad_edges and _is_edge_field(path) and t.dim() >= 1 and _edge_capacity(t.shape[-1]) != t.shape[-1]:
            out = torch.zeros(t.shape[:-1] + (_edge_capacity(t.shape[-1]),), dtype=t.dtype, device=t.device)
            out[..., :t.shape[-1]].copy_(t)
            return out
        return t.clone()
    out = Data()
    for k, v in d.materialise().__dict__.items():
        if torch.is_tensor(v):
            v = dup(f".{k}", v)
        elif is_dataclass(v):
            v = replace(v, **{f.name: (dup(f".{k}.{f.name}", getattr(v, f.name)) if torch.is_tensor(getattr(v, f.name))
                                       else getattr(v, f.name)) for f in fields(v)})
        elif isinstance(v, (list, tuple)) and v and all(torch.is_tensor(t) for t in v):
            v = [t.clone() for t in v]
        setattr(out, k, v)
    return out


def _rewire_packed(static_b, static_m) -> None:
    """After cloning: the per-task feature blocks become row ranges of the merged batch's packed buffer again."""
    if static_m is None or not torch.is_tensor(getattr(static_m, "x", None)):
        return
    off = 0
    for t in [t for t in TASK_ORDER if static_b.get(t) is not None]:
        b = static_b[t]
        n = b.x.shape[0]
        b.x = static_m.x[off:off + n]
        b.x_base = static_m.x
        off += n
    static_m.x_base = static_m.x


# hipGraph capture mode.  'thread_local': HIP calls of OTHER threads stay legal while this thread captures -- the
# process-group watchdog of torch.distributed polls its events (hipEventQuery) from its own thread at any time, and
# under the default 'global' mode that query is an error that aborts the process.
CAPTURE_MODE = "thread_local"


class StepBase:
    """Shared machinery of the two training steps: fused multi-task backbone pass, eager step with gradient
    exchange + flat Adam, hipGraph capture / replay.  Subclasses implement ``losses(batches, merged)`` returning
    ``(total, vectors, extra)``."""

    order: Sequence[str] = TASK_ORDER
    headwise_backward = False  # (MTLStep: the heads' backward inside their stream contexts, the backbone's as a call of its own)
    wgrad_grouping_default = True
    wgrad_group_count = None  # bf16 weight-gradient problems per grouped launch (None: _wgrad_count's policy)

    def _wgrad_count(self, batches, merged=None):
        """H x H weight-gradient problems per grouped launch.  Eight problems are 512 tiles = two whole rounds of the chip (16.4 us per
        problem at 6144 rows against 20 for six = 1.5 rounds), but such a launch holds EVERY CU for both rounds and the backward chain's
        launches wait behind it: worth it while the K walk is short.  Measured, 6 against 8 on one box, alternating
        (round 6, HISTORY.md): fused three-task step at 6144 rows 1.308 -> 1.287 ms (its 8-rank dry run 1.360 -> 1.317,
        sharded 1.282 -> 1.247), four tasks at 8192 rows 1.636 -> 1.644, at 16384 rows 2.945 -> 3.013, one task at 2048 rows
        0.837 -> 0.847 -- so: eight for a fused multi-task pass of fewer than 8192 rows, else the module default (six)."""
        if self.wgrad_group_count is not None:
            return self.wgrad_group_count
        live = [b for b in batches.values() if b is not None]
        if self.fused and merged is not None and len(live) > 1:
            rows = getattr(merged, "pos", None)
            if rows is not None and int(rows.shape[0]) < 8192:
                return 8
        return None
    # forked launches (weight gradients, early Adam) issued one launch late so that the dX chain keeps its hardware queue under
    # capture (sched.defer_after_next_launch): -4 % on the multi-task steps, -1.6 % on the single-task step; the EgoPack step,
    # whose GraphONE chains already occupy three queues, measured 4.04 vs 3.51 ms with it and leaves it off
    deferred_forks_default = True

    def _init_base(self, model, tasks, weights, optimizer, fused_backbone, sync, parallel_heads):
        self.model, self.tasks = model, dict(tasks)
        self.weights = {t: float(w) for t, w in weights.items()}
        self.optimizer, self.fused, self.sync = optimizer, fused_backbone, sync
        self.enabled = [t for t in self.order if self.weights.get(t, 0) > 0 and t in self.tasks]
        self.parallel_heads = parallel_heads
        # ---- everything a step object holds besides its configuration, at its idle value ----
        # streams of its own, created on first use (a step may be built before its device is chosen): ``_own_stream``
        self._head_streams = []     # one per task head (``_run_heads``)
        self.max_head_streams = None  # cap on them (None: one per head)
        self._zero_stream = None    # clears the gradient buffer beside a captured forward pass (``_fork_grad_clear``)
        self._adam_stream = None    # optimizer slices beside the step's last weight gradient (``_early_adam_plan``)
        self._input_stream = None   # fills the idle set of input buffers (``_input_slot``)
        # the captured step
        self._graph = None          # the hipGraph (staged: a list of three)
        self._static_out = None     # (objective, loss vectors) the graph writes
        self._static_in = None      # everything the graph reads, kept alive
        self._fuse_adam = True      # the optimizer is inside the graph
        self._graph_has_exchange = False  # ... and so are the gradient exchange's collectives
        self._graph_adam_lo = False  # the captured Adam launches write the low halves of the weights
        self._hyper_in_graph = False  # the graph computes the step's Adam constants itself
        self._rng_in_graph = False  # the graph moves the dropout offset word on itself
        self._grad_store_off = False  # a capture with stored gradient slots failed its check: every slot is cleared + accumulated
        self._grad_store_slots = 0  # gradient slots the last capture stored instead
        self.capture_notes = []     # what a capture fell back from (empty: nothing)
        # the step being issued
        self._stage_state, self._cuts = None, []  # the staged backward's leaves between its stages
        self._zero_pending = False  # the gradient clear is forked and not yet joined (``_join_zero``)
        self._handoff = False       # the weight-gradient side streams are handed to the gradient exchange (``_issuing``)
        self._live_last = list(self.enabled)  # tasks with a batch in the last one-piece eager step
        self._grad_one = None       # the persistent 1.0 the objective's backward starts from
        # running loss sums (``loss_sums``)
        self._loss_acc = self._loss_scratch = None
        self._loss_counts = {}
        # the training loop (``train_step``)
        self._steps_seen = 0
        self.loop_counts = {"replayed": 0, "eager": 0}  # per training loop; the entry points log and reset it per epoch
        self._train_static = None   # the static batches of the captured step and its sets of input buffers
        # task weighting (MTLStep ``task_weighting``; include/egopack_task_scale.h) -- idle: off
        self.task_mode = "none"       # none | manual | uncertainty
        self.task_scale = None        # f32 [len(enabled)] on the device: the factor of every head's backward seed, read by the kernels
        self.task_log_var = None      # uncertainty: the models.TaskLogVariance whose parameter the optimizer steps
        self._task_scale_host = None  # the scales as last set from the host (manual; 1.0 each before that)
        self.captures = 0             # captures taken by this step object (a changed task scale must not add one)
        # optional launch(es) in front of every step, inside the captured graph too: e.g. the feature-store gather that
        # materialises the step's input block from its index matrix (feature_store.FeatureStore.gather(idx, out=buffer))
        self.input_hook = None
        # weight-gradient launches of the backbone on a side stream (they feed nothing but the optimizer): 2-4 % on the
        # multi-task steps, 1.8 % on the single-task step (1.236 -> 1.214 ms), neutral on the EgoPack step
        self.wgrad_side_streams = bool(parallel_heads)
        # H x H weight gradients parked and issued four at a time as ONE grouped launch of 256 workgroups (sched._wgrad_defer):
        # -4 % on the 3-task step, -12 % on the single-task step; the EgoPack step measured 3.59 vs 3.46-3.52 ms with it in round 1
        # and left it off until round 4 (EgoPackStep.wgrad_grouping_default)
        self.wgrad_grouping = type(self).wgrad_grouping_default
        self.deferred_forks = type(self).deferred_forks_default
        # development switches (egopack_amd/switches.py): the environment overrides the step class's defaults
        for name in ("wgrad_grouping", "deferred_forks"):
            forced = switches.override(name)
            if forced is not None:
                setattr(self, name, forced)

    # ---- backbone ------------------------------------------------------------------------------------
    def features(self, batches: Mapping[str, Data], merged: Optional[Data] = None) -> Dict[str, torch.Tensor]:
        live = self._live(batches)
        if self.fused and len(live) > 1:
            if merged is None:
                merged = merge_batches([batches[t] for t in live])
                merged = merged.to(batches[live[0]].pos.device)
            feat = self.model(merged)
            parts = ops.split_rows(feat, [batches[t].pos.shape[0] for t in live])
            return dict(zip(live, parts))
        return {t: self.model(batches[t]) for t in live}

    def _run_heads(self, feats, head_fn, main_job=None):
        """``head_fn(t, feat) -> (loss_vector, extra)`` for every task; on side streams when there are several
        (independent half-chip contractions: they overlap).  A head_fn that also runs the head's BACKWARD (see
        ``_backward_pass``) must do so here, inside the head's stream context: one ``backward()`` over several streams
        replays the branches one after the other (tools/exp/branch_overlap.py: 676 us against 441 us for three chains of
        20 contractions), one call per branch inside its stream context lets them overlap."""
        vectors, extras = {}, {}
        if main_job is not None and not feats:
            main_job()
            return vectors, extras
        if self.parallel_heads and (len(feats) > 1 or main_job is not None) and next(iter(feats.values())).is_cuda:
            main = torch.cuda.current_stream()
            fork = torch.cuda.Event()
            fork.record(main)
            n_streams = min(len(feats), self.max_head_streams or len(feats))
            while len(self._head_streams) < n_streams:
                self._head_streams.append(torch.cuda.Stream())
                sched.exclude_wgrad_streams(self._head_streams[-1:])
            used = self._head_streams[:n_streams]
            for st in used:
                st.wait_event(fork)
            if main_job is not None:  # a chain that stays on the main stream, beside the forked ones; issued FIRST: under
                main_job()            # capture the child of a fork that is created first keeps the parent's hardware queue
            for i, (t, feat) in enumerate(feats.items()):
                st = used[i % n_streams]
                feat.record_stream(st)
                with torch.cuda.stream(st):
                    vectors[t], extras[t] = head_fn(t, feat)
            for st in used:
                main.wait_stream(st)
        else:
            for t, feat in feats.items():
                vectors[t], extras[t] = head_fn(t, feat)
            if main_job is not None:
                main_job()
        return vectors, extras

    def _adam_keeps_lo(self) -> bool:
        opt = self.optimizer
        return bool(getattr(opt, "adam_writes_lo", False) and getattr(opt, "flat_w16lo", None) is not None)

    def _own_stream(self, name: str, **kw) -> torch.cuda.Stream:
        """The step's stream ``self.<name>`` (declared None in ``_init_base``), created on first use."""
        st = getattr(self, name)
        if st is None:
            st = torch.cuda.Stream(**kw)
            setattr(self, name, st)
        return st

    def _branch_streams(self):
        """The step's own head / task / side streams: backward work on them keeps its weight-gradient launches."""
        return list(self._head_streams)

    def _scope_streams(self) -> None:
        """This step's own head / task / side streams are the excluded ones from here on (sched.scope_excluded_streams)."""
        sched.scope_excluded_streams(self._branch_streams())

    # ---- running per-task loss sums (what a training loop logs per epoch: reference main_temporal.py:129-134) -----------------------
    # The reference keeps them with ``.item()`` per step; kept as ``sum()`` + ``add_`` launches between two replays of the captured
    # step they were nine launches (48 us) on the stream every replay waits for.  They accumulate INSIDE the step instead: one f64
    # slot per enabled task, added to by the objective's launch (or a one-workgroup launch of their own) beside the parked weight
    # gradients; the host only counts elements.  ``loss_sums()`` reads (and clears) them: one synchronisation per epoch.
    def _loss_acc_for(self, device):
        acc = self._loss_acc
        if acc is None or acc.device != device:
            if torch.cuda.is_current_stream_capturing():
                raise RuntimeError("the loss accumulators must exist before a capture (run one eager step, or loss_sums(), first)")
            acc = self._loss_acc = torch.zeros(max(len(self.enabled), 1), dtype=torch.float64, device=device)
            self._loss_scratch = torch.zeros(1, dtype=torch.float32, device=device)
        return acc

    @torch.no_grad()
    def _ride_loss_sums(self, vectors) -> None:
        live = [v for v in vectors.values() if v is not None]
        if not live or not live[0].is_cuda:
            return
        acc, order = self._loss_acc_for(live[0].device), list(self.enabled)
        src = {t: v.detach() for t, v in vectors.items()}
        sched.park_rider(lambda: ops.weighted_mean_sum_into(self._loss_scratch, [src.get(t) for t in order], [0.0] * len(order), acc=acc),
                         tuple(src.values()))

    def _count_losses(self, vectors) -> None:
        cnt = self._loss_counts
        for t, v in vectors.items():
            cnt[t] = cnt.get(t, 0) + int(v.numel())

    def loss_sums(self, reset: bool = True) -> Dict[str, tuple]:
        """{task: (sum of its per-element losses, elements)} over the steps since the last reset (one device synchronisation)."""
        acc, cnt = self._loss_acc, self._loss_counts
        vals = acc.tolist() if acc is not None else [0.0] * len(self.enabled)
        out = {t: (float(vals[k]), int(cnt.get(t, 0))) for k, t in enumerate(self.enabled)}
        if reset:
            if acc is not None:
                acc.zero_()
            cnt.clear()
        return out

    # ---- global-norm gradient clipping (optim.FlatAdam max_grad_norm) ------------------------------------------------------------------
    # The norm's partial sums are taken piece by piece as backward finishes the pieces of the flat gradient, on the stream and at the
    # points where the unclipped step starts its early Adam slices (GraphONE's slice beside the backbone's backward, everything but the
    # temporal pooling beside the step's last weight-gradient group); only the pooling's partial sums, the one-workgroup finalize and
    # ONE Adam launch over the whole buffer are left behind backward: no Adam launch may start before the coefficient exists.  The
    # eager step sums the same pieces in the same order (``_clip_pieces``), so eager and replayed steps report the same bits.
    def _clip_on(self) -> bool:
        return bool(getattr(self.optimizer, "clipping", False))

    def grad_norm_stats(self, reset: bool = True) -> dict:
        """Gradient-norm statistics of the steps since the last reset (optim.FlatAdam.grad_norm_stats; one synchronisation)."""
        return self.optimizer.grad_norm_stats(reset)

    def _clip_pieces(self, live, plan=None):
        """[lo, hi) pieces of the flat gradient in the order a one-rank step sums them."""
        opt = self.optimizer
        total = opt.flat_p.numel()
        plan = self._early_adam_plan(live) if plan is None else plan
        if plan is None:
            return [(0, total)]
        first = [plan["graphone_region"]] if plan.get("graphone_region") else []
        return first + _minus([(0, plan["lo"]), (plan["hi"], total)], first) + [(plan["lo"], plan["hi"])]

    def _objective(self, vectors, counts=None):
        order = [t for t in self.enabled if t in vectors]
        return ops.weighted_mean_sum([vectors[t] for t in order], [self.weights[t] for t in order],
                                     None if counts is None else [counts.get(t) for t in order])

    # ---- eager step -------------------------------------------------------------------------------------
    # Exact cross-rank graph-LayerNorm statistics (SURVEY 8e caveat 1, optional): with several ranks every graph LayerNorm
    # sums its segment statistics over the ranks (forward and backward, ops.set_graph_ln_exchange), so the step computes
    # what ONE process computes on the global batch -- the reference's semantics at that batch size -- instead of the
    # default per-rank statistics (each replica = the reference at its local batch size).  Six small collectives per step
    # on the compute stream.  On an RCCL group they are captured with the rest of the N-rank step (one graph incl. the
    # exchange, _capture_exchange_graph); on a group whose collectives cannot be captured (gloo) the mode steps eagerly.
    exact_graph_ln = False

    def _exact_ln_on(self) -> bool:
        return bool(self.exact_graph_ln and self.sync is not None and self.sync.world > 1)

    @contextlib.contextmanager
    def _ln_exchange_scope(self):
        prev = ops.set_graph_ln_exchange(self.sync.sum_small) if self._exact_ln_on() else ops.set_graph_ln_exchange(None)
        try:
            yield
        finally:
            ops.set_graph_ln_exchange(prev)

    def _live(self, batches):
        """The enabled tasks that have a batch in this step, in the step's order."""
        return [t for t in self.enabled if batches.get(t) is not None]

    # ---- the one way into issuing a step: eager (one piece, staged) and captured (one rank, exchange graph, staged graphs) ----------
    # sched.step_schedule keeps three rules for every one of them: nothing parked or deferred survives a step that was abandoned by an
    # exception, no hook outlives its step, and the settings of whoever issued before come back.
    @contextlib.contextmanager
    def _issuing(self, batches, merged, *, handoff: bool = False, store: bool = False):
        """Issue one step inside: this step's streams are the excluded ones, the weight-gradient / fork scheduler (``sched``) runs
        with this step's settings.  ``handoff``: the side streams are handed to the gradient exchange at the end of every backward
        stage (``_exchange_region``) instead of joined.  ``store`` (captures): gradient slots learnt to have one writer per step
        (``_learn_single_writers``) are stored, not cleared + accumulated -- the provider is installed for the body (not at all:
        switched off, or nothing learnt), ``zero_flat_grads`` leaves those slots out meanwhile, and the optimizer checks at the end
        that every slot left uncleared was written exactly once (EGK_DISABLE=grad_store)."""
        opt = self.optimizer
        self._scope_streams()
        prev_handoff, stored, ok = self._handoff, None, False
        try:
            with sched.step_schedule(self.wgrad_side_streams, self.wgrad_grouping, self._wgrad_count(batches, merged), self.deferred_forks,
                                     handoff):
                self._handoff = handoff
                if store and not self._grad_store_off and hasattr(opt, "store_begin") and switches.enabled("grad_store"):
                    provider = opt.store_begin()
                    if provider is not None:
                        stored = (ops.set_grad_slot_provider(provider),)
                yield
            ok = True
        finally:
            self._handoff = prev_handoff
            if stored is not None:
                ops.set_grad_slot_provider(stored[0])
                opt.store_end(ok=ok)
                self._grad_store_slots = len(opt.store_slots)

    def forward_backward(self, batches, merged=None):
        self._live_last = self._live(batches)
        self.optimizer.zero_grad()
        self._task_scale_head()
        if self.input_hook is not None:
            self.input_hook()
        with self._issuing(batches, merged):
            # (eagerly issued steps end with the same grouped tail launch as captured ones: same tile variants, same bits)
            self._install_tail(self._tail_only_plan(self._live(batches)))
            with self._ln_exchange_scope():
                total, vectors = self._backward_pass(batches, merged)
            sched.join_wgrad(force=True)
        return total, vectors

    def step(self, batches: Mapping[str, Data], merged: Optional[Data] = None):
        with STAGE_LOCK:
            if self._use_stages():
                out = self._staged_step(batches, merged)
            else:
                with self._learn_single_writers():
                    total, vectors = self.forward_backward(batches, merged)
                self._exchange_and_update()
                out = total.detach(), {t: v.detach() for t, v in vectors.items()}
            self._count_losses(out[1])
            return out

    # ---- gradient slots with one writer per step: stored, not cleared + accumulated (optim.FlatAdam.learn_begin / store_begin) ------
    # Learnt from the EAGER steps of every execution structure (one-piece and staged), applied to every CAPTURE (one rank, the
    # staged graphs of the N-rank step, the one-graph exchange): the gradient exchange reads the flat buffer region by region
    # once backward has finished it -- whether a slot was cleared and added into or stored makes no difference to what it reads.
    @contextlib.contextmanager
    def _learn_single_writers(self):
        opt = self.optimizer
        learn = (getattr(opt, "materialised", False) and hasattr(opt, "learn_begin") and not torch.cuda.is_current_stream_capturing()
                 and switches.enabled("grad_store"))
        prev = ops.set_grad_slot_provider(opt.learn_begin()) if learn else None  # (which gradient slots have ONE writer per step)
        try:
            yield
        finally:
            if learn:
                ops.set_grad_slot_provider(prev)
                opt.learn_end()

    def _fork_grad_clear(self, hyper: bool) -> None:
        """Captured steps clear the gradient buffer BESIDE the forward pass (nothing writes a gradient before the first backward
        launch): 100 MB of memset off the chain's head, forked behind the forward pass's first launch (sched.defer_after_next_launch)
        and joined by ``_join_zero`` before backward starts.  ``hyper``: the step's Adam constants (one thread, from the device-side
        step counter) ride along."""
        opt, side = self.optimizer, self._own_stream("_zero_stream")

        def issue_zero(ev):
            side.wait_event(ev)
            with torch.cuda.stream(side):
                opt.zero_flat_grads()
                if hyper:
                    opt.prepare_hyper(in_capture=True)
                self._task_scale_head()  # (uncertainty: scale = exp(-log_var), joined with the clear before the heads read it)
        sched.defer_after_next_launch(issue_zero)
        self._zero_pending = True

    def _task_scale_head(self) -> None:
        """The launch at the head of a step with learned task weights (MTLStep); nothing otherwise."""

    def _task_scale_for(self, device):
        """The per-task scale vector of the heads' seeds on ``device`` (MTLStep with task weighting); None otherwise."""
        return None

    def _join_zero(self):
        """Wait for the gradient clear forked by ``_fork_grad_clear`` before the first launch that writes a gradient."""
        if self._zero_pending:
            sched.drain_deferred()
            torch.cuda.current_stream().wait_stream(self._zero_stream)
            self._zero_pending = False

    def _backward_pass(self, batches, merged=None):
        """Forward + backward of the objective (gradients accumulate into the parameters' slots): (objective, loss vectors)."""
        total, vectors, _ = self.losses(batches, merged)
        self._ride_loss_sums(vectors)
        self._join_zero()
        # (the seed of the objective's backward is a persistent 1.0: ``backward()`` without it fills a fresh tensor with a torch
        #  kernel on the chain, between the loss and the first backward launch)
        one = self._grad_one
        if one is None or one.device != total.device or one.dtype != total.dtype:
            one = self._grad_one = torch.ones((), dtype=total.dtype, device=total.device)
        total.backward(gradient=one)
        return total, vectors

    # ---- staged backward: gradient exchange overlapped with the rest of backward --------------------------------------
    # With several ranks the flat gradient is exchanged REGION BY REGION as backward finishes it: the task heads'
    # region after stage A (forward + heads' backward), the SAGE stack's after stage B, the TRN's after stage C.  The
    # stages are pieces of ONE backward pass, cut at detached leaves (the backbone output per task, the TRN output),
    # so every gradient is what the single pass computes; each stage is its own hipGraph under capture and the
    # collectives run between the graph launches, on the communication stream, while the next stage computes.
    staged = None  # None: automatic (several ranks, flat buffers laid out [TRN | SAGE stack | heads]); True / False: forced

    def _stage_regions(self):
        return None  # steps that support stages return [(lo, hi) heads, (lo, hi) SAGE stack, (lo, hi) TRN]

    def _use_stages(self) -> bool:
        if self.staged is False or not getattr(self.optimizer, "materialised", False):
            return False
        if self.staged is None and (self.sync is None or self.sync.world <= 1):
            return False
        # (the sharded update is region-wise too: each region is reduce-scattered when backward has finished it, dist.GradSync.start)
        return self._stage_regions() is not None

    def _exchange_region(self, region):
        if self.sync is not None and self.sync.world > 1:
            # (handoff: the region's weight gradients may still be running on their side streams -- the communication stream
            #  waits for them, the backward stream goes straight on with the next stage)
            after = sched.take_wgrad_streams() if self._handoff else ()
            self.sync.start(self.optimizer, *region, after=after)

    def _stage_join(self):
        """End of a backward stage: the stage's gradients are complete once the weight-gradient side streams are joined."""
        if not self._handoff:
            sched.join_wgrad(force=True)

    def _finish_staged(self):
        if self.sync is not None and self.sync.world > 1:
            self.sync.finish_and_step(self.optimizer)
        else:
            self.optimizer.step()

    def _staged_step(self, batches, merged=None):
        regions = self._stage_regions()
        if self.sync is not None:
            self.sync.begin_step()
        self.optimizer.zero_grad()
        self._task_scale_head()
        if self.input_hook is not None:
            self.input_hook()
        with self._issuing(batches, merged):
            self._install_tail(self._tail_only_plan(self._live(batches)))
            with self._ln_exchange_scope(), self._learn_single_writers():
                total, vectors = self._stage_a(batches, merged)
                self._exchange_region(regions[0])
                self._stage_b()
                self._exchange_region(regions[1])
                self._stage_c()
                self._exchange_region(regions[2])
        self._finish_staged()
        return total.detach(), {t: v.detach() for t, v in vectors.items()}

    def _exchange_and_update(self):
        opt = self.optimizer
        if hasattr(opt, "materialised") and not opt.materialised:
            opt._materialise()
        if self.sync is not None and self.sync.world > 1:
            regions = self._stage_regions() if getattr(self.sync, "shard_update", False) else None
            if regions is not None:
                # sharded update: WHICH rank steps which slice must not depend on how the step was issued -- the moments of a slice
                # live on its rank -- so a one-piece backward (the first step, before the flat buffers exist) shards region by
                # region exactly as the staged steps that follow it do
                self.sync.begin_step()
                for region in regions:
                    self.sync.start(opt, *region)
                self.sync.finish_and_step(opt)
            else:
                self.sync.reduce_and_step(opt)  # chunked: Adam of chunk i overlaps the collectives of the later chunks
        else:
            if self._clip_on():
                opt.norm_regions = self._clip_pieces(self._live_last)
            opt.step()

    # ---- training loop entry: eager for the first steps, then the captured step on static-shape batches -------------
    use_graph = True
    graph_after = 2  # eager steps before the capture (they build the flat optimizer buffers and warm the allocator)

    def train_step(self, batches: Mapping[str, Data], merged: Optional[Data] = None):
        """One optimizer step on device batches, for training loops (main_temporal / main_egopack).

        The first ``graph_after`` steps run eagerly.  The next one is captured on private copies of its batches, and every
        later step whose batches have the SAME signature (``batch_signature``: shapes, dtypes, node counts, edge CAPACITIES
        -- the loaders deliver fixed-size batches of fixed-length sequences, so that is every step but a short last one,
        also for LTA batches whose edge count moves with the labels) copies its
        values into those buffers and replays the graph: the step the benchmark measures instead of ~150 launches issued
        from Python.  Anything else (different shapes, several ranks with an eager exchange path, ``use_graph`` off) takes
        the eager step.  Returns what ``step`` returns; after a replay the loss vectors are the graph's static outputs,
        valid until the next call.  ``loop_counts`` tallies replayed vs eager steps."""
        self._steps_seen += 1
        st = self._train_static
        ref = _shared_blob(batches, merged)
        if not (ref is not None and st is not None and self.use_graph and st.get("gsig") == ref.gsig and len(st.get("slots", ())) > 1
                and st["xkey"] == _feature_key(batches, merged)):
            ensure_features(batches, merged)  # (staged without their feature block, and this step is not a replay that gathers it)
        first = next(iter(batches.values()))
        on_device = first.x.is_cuda if torch.is_tensor(first.__dict__.get("x", None) if "x" in first.__dict__ else first.x) else (
            ref is not None and ref.dev.is_cuda)
        if (not self.use_graph or self._steps_seen <= self.graph_after or not on_device
                or (self._exact_ln_on() and not self._one_graph_exchange_ok())):
            self.loop_counts["eager"] += 1
            return self.step(batches, merged)
        if self.fused and len(self._live(batches)) > 1 and merged is None:
            self.loop_counts["eager"] += 1
            return self.step(batches, merged)  # (the caller did not stage a merged batch: nothing static to replay on)
        # batches out of ONE packed transfer (data.to_device_packed) with the layout the static buffers were built from: one
        # device-to-device copy of the byte buffer + one of the feature block instead of a copy per tensor, no signature walk
        if ref is not None and st is not None and st.get("gsig") == ref.gsig and st["xkey"] == _feature_key(batches, merged):
            slot = self._input_slot(st, ref, batches, merged)
            st["fast"] = None
            self.loop_counts["replayed"] += 1
            self._select_slot(slot)
            total = self.replay()
            slot["done"] = torch.cuda.current_stream().record_event()  # (this slot's buffers are read until here)
            return total.detach(), {t: v.detach() for t, v in self._static_out[1].items()}
        # equal structure fingerprints (stage_batches attaches them) + equal feature shapes = equal signature: the walk over
        # every tensor of the step's batches (0.2-0.3 ms of host time per step) is skipped for such a step
        fast = _fast_key(batches, merged)
        sig = st["sig"] if (st is not None and fast is not None and fast == st.get("fast")) else batch_signature(batches, merged)
        if st is None:
            blob = None
            if ref is not None:
                blob, static_b, static_m = _static_from_blob(ref, batches, merged)
            else:
                clone = lambda d: None if d is None else _clone_batch(d, pad_edges=True)
                static_b = {t: clone(b) for t, b in batches.items()}
                static_m = clone(merged)
                _rewire_packed(static_b, static_m)
                copy_batch_values(static_b, static_m, batches, merged)
            self.capture(static_b, static_m, warmup=0)
            st = self._train_static = {"sig": batch_signature(static_b, static_m), "batches": static_b, "merged": static_m,
                                       "fast": fast}
            if blob is not None:
                st.update(blob=blob, gsig=ref.gsig, xkey=_feature_key(batches, merged))
            st["slots"] = [self._slot_of_capture(blob, static_b, static_m)]
            if st["sig"] != sig:  # (cannot happen: the clones mirror the originals)
                self._train_static = None
                self.loop_counts["eager"] += 1
                return self.step(batches, merged)
        elif st["sig"] != sig:
            self.loop_counts["eager"] += 1
            return self.step(batches, merged)
        else:
            copy_batch_values(st["batches"], st["merged"], batches, merged, dst_walks=st.setdefault("walks", {}))
            if fast is not None and st.get("fast") != fast:
                st["fast"] = fast  # (the static buffers now hold this structure)
        self.loop_counts["replayed"] += 1
        self._select_slot(st["slots"][0])
        total = self.replay()
        st["slots"][0]["done"] = torch.cuda.current_stream().record_event()
        return total.detach(), {t: v.detach() for t, v in self._static_out[1].items()}

    # ---- two captured steps on alternating input buffers ------------------------------------------------------------------------------
    # A replay reads its batch from fixed buffers, and it reads the feature block at both ends of the step (first contraction, last
    # weight gradient): the next batch cannot be written there while the step runs, and written between two replays the copies (57 MB
    # of features + the index buffer) were 30 us on the stream both replays are ordered on.  A loop that feeds packed transfers
    # (data.to_device_packed) therefore captures the step TWICE, on two sets of input buffers, and alternates: while the replay on
    # one set runs, the next batch is copied into the other on a stream of its own (behind the event that ends the last replay that
    # read that set, and behind the staging of the batch).  The two graphs share everything else -- parameters, optimizer state,
    # gradient buffer, dropout offset word, loss accumulators -- and run one after the other on the training stream.
    gathers_inputs = False  # set once the step gathers the store rows into its own input buffers (see _input_slot)

    def _slot_of_capture(self, blob, static_b, static_m) -> dict:
        return {"graph": self._graph, "out": self._static_out, "static_in": self._static_in, "blob": blob,
                "batches": static_b, "merged": static_m, "done": None}

    def _select_slot(self, slot) -> None:
        self._graph, self._static_out, self._static_in = slot["graph"], slot["out"], slot["static_in"]

    def _double_buffer_ok(self) -> bool:  # (one-rank steps whose optimizer is in the graph)
        return bool(self._fuse_adam and not isinstance(self._graph, list))

    def _input_slot(self, st, ref, batches, merged) -> dict:
        """The set of input buffers this step's replay reads, holding this step's batch (see above)."""
        slots = st["slots"]
        cur = torch.cuda.current_stream()
        if self._double_buffer_ok():
            k = st["turn"] = (st.get("turn", 0) + 1) % 2
            if k == len(slots):  # the second capture, on private copies of THIS batch (they hold its values: nothing to fill)
                self._select_slot(slots[0])
                blob, static_b, static_m = _static_from_blob(ref, batches, merged)
                self.capture(static_b, static_m, warmup=0)
                slots.append(self._slot_of_capture(blob, static_b, static_m))
                return slots[k]
        else:
            k = 0
        slot = slots[k]
        side = cur
        if len(slots) > 1:
            side = self._own_stream("_input_stream", priority=-1)
            ready = getattr(ref, "ready", None)
            if ready is not None:
                side.wait_event(ready)  # (the staging of this batch: engine.StagedBatches)
            else:
                side.wait_stream(cur)  # (staged on the training stream by the caller)
            if slot["done"] is not None:
                side.wait_event(slot["done"])
        store = getattr(ref, "store", None)
        with torch.no_grad(), torch.cuda.stream(side):
            slot["blob"].copy_(ref.dev, non_blocking=True)
            if merged is not None:
                if torch.is_tensor(merged.__dict__.get("x")):
                    slot["merged"].x.copy_(merged.x, non_blocking=True)
                slot["merged"]._struct_key = getattr(merged, "_struct_key", 0)
            for t, b in batches.items():
                if b is not None:
                    dst = slot["batches"][t]
                    if not torch.is_tensor(b.__dict__.get("x")):
                        # staged without its feature block: the store rows (they arrived with the transfer) are gathered straight
                        # into this set's block -- one pass over the rows instead of a gather + a copy of the block
                        store.gather(b.__dict__["x_idx"], out=dst.x, dtype=dst.x.dtype)
                    elif merged is None:
                        dst.x.copy_(b.x, non_blocking=True)
                    dst._struct_key = getattr(b, "_struct_key", 0)
        if len(slots) > 1 and store is not None:
            self.gathers_inputs = True  # (from now on a StagedBatches that feeds this step leaves the gathers to it)
        if side is not cur:
            for v in (ref.dev, getattr(merged, "x", None), *(getattr(b, "x", None) for b in batches.values() if b is not None)):
                if torch.is_tensor(v) and v.is_cuda:
                    v.record_stream(side)
            cur.wait_event(side.record_event())
        return slot

    # ---- hipGraph capture ---------------------------------------------------------------------------------
    def capture(self, batches: Mapping[str, Data], merged: Optional[Data] = None, warmup: int = 2):
        """Capture forward+backward(+Adam if no gradient exchange) for THESE device tensors (static
        shapes and addresses: refill them in place between replays).

        The stored gradient slots (``_issuing``) are whatever the last EAGER step learnt; when the captured batches
        write them differently (another live-task set: MTL loaders of unequal length, per-task backbone passes) the provider or
        its end-of-capture check raises -- the capture is then taken once more with every slot cleared and accumulated, and
        ``capture_notes`` says so: a slower step, never a crash of the training loop and never a wrong gradient."""
        with STAGE_LOCK:  # (a staging thread makes no HIP call while a capture is open: StagedBatches._ahead)
            try:
                return self._capture_once(batches, merged, warmup)
            except RuntimeError as e:
                if not str(e).startswith("grad_store:") or self._grad_store_off:
                    raise
                if self.sync is not None and self.sync.world > 1 and self._one_graph_exchange_ok():
                    raise  # (a failed capture that holds collectives is not retried in this process: see one_graph_exchange)
                torch.cuda.synchronize()
                self._grad_store_off = True
                self.capture_notes = [*self.capture_notes, f"stored gradient slots off for this step ({e})"]
                return self._capture_once(batches, merged, 0)

    def _capture_once(self, batches, merged, warmup):
        opt = self.optimizer
        self.captures += 1
        self._loss_acc_for(next(self.model.parameters()).device)  # (the running loss sums' slots: allocated outside the capture)
        self._task_scale_for(next(self.model.parameters()).device)  # (likewise the task-scale vector, when there is one)
        if self._exact_ln_on() and not self._one_graph_exchange_ok():
            raise RuntimeError("exact_graph_ln sums the graph-LayerNorm statistics over the ranks inside the step: this process "
                               "group's collectives cannot be captured in a hipGraph -- use step() / train_step() (eager) in this mode")
        live = self._live(batches)
        if self.fused and len(live) > 1 and merged is None:  # index work must stay outside the capture
            merged = merge_batches([batches[t] for t in live]).to(batches[live[0]].pos.device)
        if warmup > 0 or not getattr(opt, "materialised", True):
            self._scope_streams()
            side = sched.unexcluded_stream()  # (a pooled handle that is not one of this step's head / task streams)
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                for _ in range(max(warmup, 1)):  # also materialises the flat buffers
                    self.step(batches, merged)
            torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        if self.sync is not None and self.sync.world > 1 and ((self._use_stages() and self._one_graph_exchange_ok()) or self._exact_ln_on()):
            # the eager steps above issued collectives and THIS capture records collectives (the opt-in one-graph exchange, the
            # exact cross-rank LayerNorm statistics): the process group's watchdog must have retired the eager ones before the
            # capture takes the communicator's stream into capture mode (dist.quiesce_before_capture: the round-3 abort).  The
            # staged graphs -- the N-rank default -- and the one-piece captures issue their collectives BETWEEN graph launches and
            # never capture that stream: they do not pay the settle time (a heuristic: one watchdog sweep, see the docstring).
            self.sync.quiesce()
        if hasattr(opt, "invalidate_lo_shadows") and not self._adam_keeps_lo():
            opt.invalidate_lo_shadows()  # (a captured step must contain every refresh of the low halves it relies on)
        # (when the Adam launch itself writes the low halves -- FlatAdam.adam_writes_lo, once they exist -- the warm-up steps left
        #  them fresh and every replay's Adam leaves them fresh for the next one: no split launch in the captured step)
        self._graph_has_exchange = False
        self._graph_adam_lo = False
        if self._use_stages():
            return self._capture_staged(batches, merged)
        fuse_adam = self.sync is None or self.sync.world <= 1
        g = torch.cuda.CUDAGraph()
        opt.sync_hyper_source()  # (the step constants are computed inside the graph from a device-side step counter)
        ops.rng_device_offset(opt.flat_p.device)  # (the dropout offset word exists BEFORE the capture: created inside, its fill is a node)
        self._hyper_in_graph = False
        # gradient slots with one writer per step (learnt from the eager steps above, FlatAdam.learn_begin) are stored, not cleared +
        # accumulated (``store``): the step's buffer clear shrinks to what is still added into; also when the optimizer follows a
        # gradient exchange outside the graph
        with self._issuing(batches, merged, store=True):
            early = self._early_adam_plan(live) if fuse_adam else None
            clip = fuse_adam and self._clip_on()
            if clip and early is not None:
                early["clip"], early["normed"] = True, []  # (its hooks take partial sums of the norm where they would start Adam slices)
            with torch.cuda.graph(g, stream=sched.unexcluded_stream(), capture_error_mode=CAPTURE_MODE):
                ops.stamp("step_start")
                self._hyper_in_graph = fuse_adam
                self._fork_grad_clear(hyper=fuse_adam)  # (with the step's Adam constants when the optimizer is in the graph)
                self._rng_in_graph = False
                if self.input_hook is not None:
                    self.input_hook()
                if early is None and not fuse_adam:
                    self._install_tail(self._tail_only_plan(live))
                if early is not None:
                    sched.set_last_wgrad_hook(early["param"], early["hook"], pre=self._join_gradient_branches)
                    sched.set_graphone_backward_hook(early.get("graphone_hook"))
                    if early["tail"]:
                        g0 = opt.flat_g.data_ptr()
                        sched.set_last_wgrad_tail(g0 + 4 * early["lo"], g0 + 4 * early["hi"])
                # (no join with the weight-gradient side stream when a backward() call returns: the gradients are read below, behind
                #  ``sched.join_wgrad(force=True)``)
                total, vectors = self._backward_pass(batches, merged)
                self._join_zero()  # (a backward path that did not: the memset must at least precede the optimizer)
                sched.set_last_wgrad_hook(None, None)
                sched.join_wgrad(force=True)
                ops.stamp("backward_done")
                # the Philox offset word of the dropout launches moves on INSIDE the graph (beside nothing that reads it: every
                # dropout launch of the step is done when the optimizer starts): replay k draws the masks of offset base + k * stride
                # without a separate launch in front of every replay -- and without a launch of its own: it rides in an optimizer
                # launch (egk_adam_step_bump)
                rng_here = not (early is not None and early.get("rng_done"))
                bump = (ops.rng_device_offset(opt.flat_p.device), ops.RNG_DEVICE_STRIDE) if rng_here else None
                if clip:
                    # every Adam launch waits for the norm: the pieces summed beside backward are joined, the rest (the temporal
                    # pooling, final only now) is summed here, then finalize and ONE Adam launch behind its gate
                    if early is not None and (early["fired"] or early.get("done")):
                        torch.cuda.current_stream().wait_stream(early["stream"])
                    for a, b in _minus([(0, opt.flat_p.numel())], early["normed"] if early is not None else ()):
                        opt.norm_partials(None, a, b)
                    opt.norm_finalize()
                    ops.stamp("norm_done")
                    opt.launch(bump=bump)
                    bump = None
                    ops.stamp("adam_done")
                elif fuse_adam:
                    if early is not None and early["fired"]:
                        torch.cuda.current_stream().wait_stream(early["stream"])
                        opt.launch(None, early["lo"], early["hi"], bump=bump if early["hi"] > early["lo"] else None)
                        bump = None if early["hi"] > early["lo"] else bump
                    elif early is not None and early.get("done"):  # (a slice was stepped, the last weight gradient's hook never ran)
                        torch.cuda.current_stream().wait_stream(early["stream"])
                        for a, b in _minus([(0, opt.flat_p.numel())], early["done"]):
                            opt.launch(None, a, b, bump=bump)
                            bump = None
                    else:
                        opt.launch(bump=bump)
                        bump = None
                    ops.stamp("adam_done")
                if bump is not None:
                    ops.advance_rng_device(opt.flat_p.device)
                self._rng_in_graph = True
        self._graph, self._static_out, self._fuse_adam = g, (total, vectors), fuse_adam
        self._graph_adam_lo = bool(fuse_adam and self._adam_keeps_lo())  # (the captured Adam launches write the low halves)
        # the graph holds raw addresses: keep every tensor it reads alive for as long as the graph exists
        # (in particular the merged batch -- CSR arrays, positions, segment pointers -- when it was built here)
        self._static_in = (batches, merged)
        return g

    # captured single-GPU step: start Adam on everything but the last weight gradient's slots beside that launch.  Only
    # for steps that have JOINED every other gradient producer into the backward stream by then (MTLStep with its
    # head-wise backward does; a step whose branches are still running on their own streams at that point must not)
    early_adam = False

    def _tail_only_plan(self, live):
        """(first TRN weight, flat range of the temporal pooling's slots) when the step can end with ONE grouped launch of the
        pooling's weight gradients (sched.set_last_wgrad_tail) although no optimizer slice runs beside it -- the steps whose
        Adam follows a gradient exchange.  None when the layout does not allow it."""
        opt = self.optimizer
        tp = getattr(self.model, "temporal_pooling", None)
        first = getattr(tp, "proj", [None])[0] if tp is not None else None
        if (first is None or not hasattr(opt, "region_of") or not getattr(opt, "materialised", False) or not (self.fused or len(live) == 1)
                or not self.headwise_backward_ok()
                or first.weight.numel() >= 512 * 128 * 128):  # (a wide first linear's weight gradient stays a launch of its own)
            return None
        params = [p for p in tp.parameters() if p.requires_grad]
        lo, hi = opt.region_of(params)
        slots = [opt._slot_of[id(p)] for p in params if id(p) in opt._slot_of]
        if not (hi > lo and lo % 8 == 0 and hi % 8 == 0 and sum(n for _, n in slots) == hi - lo):
            return None
        return first.weight, lo, hi

    def headwise_backward_ok(self) -> bool:
        return bool(self.headwise_backward)

    def _install_tail(self, plan, hook=None) -> None:
        if plan is None:
            return
        g0 = self.optimizer.flat_g.data_ptr()
        sched.set_last_wgrad_hook(plan[0], hook or (lambda: None))
        sched.set_last_wgrad_tail(g0 + 4 * plan[1], g0 + 4 * plan[2])

    def _early_adam_plan(self, live):
        """The step ends with two launches that have the chip to themselves one after the other: the weight gradient of
        the first TRN linear (the last node of backward, 58 GFLOP, compute-bound) and Adam (750 MB, HBM-bound).  When the
        backbone runs once per step (fused pass or a single task) every other gradient is final when that weight gradient
        is launched: Adam over the rest of the flat buffers starts beside it on its own stream, Adam over the slots of
        that weight and bias follows it.  Elementwise: the same update, bit for bit."""
        opt = self.optimizer
        tp = getattr(self.model, "temporal_pooling", None)
        first = getattr(tp, "proj", [None])[0] if tp is not None else None
        if not (self._early_adam_ok() and first is not None and hasattr(opt, "region_of") and (self.fused or len(live) == 1)):
            return None
        total = opt.flat_p.numel()

        def region(params):
            lo, hi = opt.region_of(params)
            slots = [opt._slot_of[id(p)] for p in params if id(p) in opt._slot_of]
            ok = hi > lo and lo % 8 == 0 and hi % 8 == 0 and sum(n for _, n in slots) == hi - lo  # (adjacent slots)
            return (lo, hi) if ok else None
        # the late Adam slice: the whole temporal pooling when its slots are one block (then the step's tail is ONE grouped
        # launch of its weight gradients, sched.set_last_wgrad_tail), else the first linear alone
        # (a first linear whose weight gradient alone is >= 512 tiles of 128 x 128 -- the shipped pooling width 4096: 1152 -- fills
        #  the chip by itself: its launch stays alone and the late slice is that layer's, so that Adam over the rest of the pooling
        #  runs beside it; Hp = 4096 step 2.785-2.796 -> 2.770-2.772 ms.  At Hp = 1024 (288 tiles) the pooling's three weight
        #  gradients are one grouped launch, 123 against 120 + 66 us.)
        tail = None
        if first.weight.numel() < 512 * 128 * 128:
            tail = region([p for p in tp.parameters() if p.requires_grad])
        reg = tail or region([p for p in (getattr(first, "weight", None), getattr(first, "bias", None)) if p is not None])
        if reg is None:
            return None
        lo, hi = reg
        plan = {"param": first.weight, "lo": lo, "hi": hi, "stream": self._own_stream("_adam_stream"), "fired": False, "tail": tail is not None}
        def hook():
            if plan["fired"]:
                return
            main = torch.cuda.current_stream()

            def issue(ev):
                # (issued AFTER the last weight gradient's own launch, behind an event recorded here: see
                #  sched.defer_after_next_launch -- the launch created first keeps the backward stream's hardware queue)
                side = sched.wgrad_side_stream(main)
                plan["stream"].wait_event(ev)
                if side is not None:
                    plan["stream"].wait_stream(side)
                with torch.cuda.stream(plan["stream"]):
                    if plan.get("clip"):  # (clipping: no Adam before the norm exists -- this piece's partial sums instead)
                        for a, b in _minus([(0, lo), (hi, total)], plan.get("done", ())):
                            opt.norm_partials(None, a, b)
                            plan["normed"].append((a, b))
                        return
                    # the dropout offset word moves on here, beside the last weight gradient (every dropout launch of the step
                    # is long done), INSIDE the first optimizer launch: no launch of its own
                    bump = (ops.rng_device_offset(opt.flat_p.device), ops.RNG_DEVICE_STRIDE)
                    for a, b in _minus([(0, lo), (hi, total)], plan.get("done", ())):  # (``done``: slices stepped earlier in the step)
                        opt.launch(None, a, b, bump=bump)
                        bump = None
                    if bump is not None:  # (no slice left to step here: the word still moves on)
                        ops.advance_rng_device(opt.flat_p.device)
            plan["rng_done"] = not plan.get("clip")  # (every dropout launch of the step has been issued: this is backward's end)
            sched.defer_after_next_launch(issue)
            plan["fired"] = True
        plan["hook"] = hook
        return plan

    # (measured and not kept: Adam over the SAGE + head slots started when backward enters the temporal pooling, beside the
    #  TRN backward chain: 1.85 vs 1.75 ms -- the HBM-bound launch slows the chain more than the shorter tail saves)

    def _early_adam_ok(self) -> bool:
        return bool(self.early_adam)

    def _gradient_branch_streams(self):
        """Streams on which parts of backward may still be running when the LAST weight gradient of the step is launched."""
        return []

    def _join_gradient_branches(self) -> None:
        """Called on the backward stream right before the step's last weight gradient (sched.set_last_wgrad_hook ``pre``): the
        branches of a one-call backward that run on other streams are joined HERE -- what they parked for the grouped
        weight-gradient launches (operands made on their streams) is issued next, and the optimizer slice that starts beside the
        last weight gradient reads every gradient they wrote.  (Autograd itself joins them only when backward() returns.)"""
        main = torch.cuda.current_stream()
        for st in self._gradient_branch_streams():
            with torch.cuda.stream(st):
                live_branch = torch.cuda.is_current_stream_capturing()
            if live_branch and st != main:
                main.wait_stream(st)

    # The N-rank step as ONE hipGraph: the three stages, the region-wise collectives between them (communication stream, forked
    # and joined inside the capture) and the per-chunk Adam launches.  Three graph launches + ~13 collectives + ~13 Adam
    # launches issued from Python per step become one graph launch (--exchange-dry-run 8 on one GPU: 1.69 -> 1.53 ms).
    # RCCL collectives enqueue device work only and are capturable; the process group's watchdog keeps polling its events from
    # its own thread, legal under CAPTURE_MODE 'thread_local'.
    #
    # OPT-IN.  The default for several ranks is the path with the most evidence: three staged graphs with the collectives
    # issued eagerly between the graph launches (two real rank processes run it, tools/two_rank_check.py).  This mode has only
    # ever met a 1-rank RCCL group, so it is taken when the caller asks for it -- the attribute, or EGK_ENABLE=one_graph_exchange
    # -- typically after a pre-flight child process per rank has captured and replayed it with exit code 0 (bench.py
    # ``one_graph_probe``).  A capture that holds collectives and FAILS is not retried in this process: the exception reaches
    # the caller (after a failed capture nothing guarantees that the stream / communicator is reusable; the round-3 catch-and-
    # continue onto the staged graphs is gone), who ends the attempt -- the parent picks the next mode for ALL ranks.
    one_graph_exchange = False

    def _one_graph_exchange_ok(self) -> bool:
        forced = switches.override("one_graph_exchange")  # (EGK_ENABLE / EGK_DISABLE win over the attribute)
        want = self.one_graph_exchange if forced is None else forced
        return bool(want and self.sync is not None and self.sync.world > 1 and self.sync.capturable())

    def _capture_exchange_graph(self, batches, merged):
        opt, sync = self.optimizer, self.sync
        regions = self._stage_regions()
        live = self._live(batches)
        g = torch.cuda.CUDAGraph()
        opt.grad_scale = 1.0 / sync.world
        opt.sync_hyper_source()
        self._hyper_in_graph = True
        count = opt.step_count
        sync.begin_step()
        sync.hyper_ready = True
        try:
            # (handoff: every stage's side streams go to its region's collectives; single-writer gradient slots are stored: the
            #  collectives read final values either way)
            with (self._issuing(batches, merged, handoff=True, store=True),
                  torch.cuda.graph(g, stream=sched.unexcluded_stream(), capture_error_mode=CAPTURE_MODE)):
                ops.stamp("step_start")
                # (the gradient buffer is cleared beside the forward pass, as in the one-rank capture: joined by _join_zero()
                #  before the heads' backward writes the first gradient)
                self._fork_grad_clear(hyper=True)
                self._rng_in_graph = False
                if self.input_hook is not None:
                    self.input_hook()
                with self._ln_exchange_scope():  # (exact cross-rank graph-LN statistics: their collectives are captured too)
                    total, vectors = self._stage_a(batches, merged)
                    self._join_zero()
                    ops.stamp("heads_done")
                    self._exchange_region(regions[0])
                    # beside the step's LAST weight-gradient launch (the grouped tail of the temporal pooling): the Adam slices of
                    # the regions exchanged by then, each behind its collective -- what the one-rank capture does with its early
                    # Adam launch; only the pooling's own slices are left for the end of the step
                    fired = []

                    def early_adam_hook():
                        if fired:
                            return
                        fired.append(True)
                        side = self._own_stream("_adam_stream")

                        def issue(ev):
                            side.wait_event(ev)
                            sync.step_started_chunks(opt, side)
                        sched.defer_after_next_launch(issue)
                    self._install_tail(self._tail_only_plan(live), early_adam_hook if self._early_adam_ok() else None)
                    self._stage_b()
                    ops.stamp("stack_done")
                    self._exchange_region(regions[1])
                    self._stage_c()
                ops.stamp("backward_done")
                self._exchange_region(regions[2])
                sync.finish_and_step(opt)
                ops.stamp("adam_done")
                ops.advance_rng_device(opt.flat_p.device)
                self._rng_in_graph = True
        finally:
            sync.hyper_ready = False
            sync.begin_step()
            opt.step_count = count  # (finish_and_step counted the capture; replay() counts the steps that run)
        self._graph, self._static_out, self._fuse_adam = g, (total, vectors), True
        self._graph_adam_lo = self._adam_keeps_lo()  # (every chunk's captured Adam launch writes the low halves of its slice)
        self._graph_has_exchange = True
        self._static_in = (batches, merged, self._stage_state, self._cuts)
        return g

    def _capture_staged(self, batches, merged):
        """Three graphs (one per backward stage) from one memory pool; the gradient exchange sits between them."""
        self._graph_has_exchange = False
        if self._one_graph_exchange_ok():
            return self._capture_exchange_graph(batches, merged)  # (an exception ends the attempt: see one_graph_exchange)
        gs = [torch.cuda.CUDAGraph() for _ in range(3)]
        self._rng_in_graph = False  # (no staged graph advances the Philox offset word: replay() does, also after a one-piece capture)
        # (``store``: one provider over the three captures -- every learnt slot is written in exactly one of them)
        with self._issuing(batches, merged, store=True):
            live = self._live(batches)
            cap = sched.unexcluded_stream()  # (one capture stream for the three graphs, never a registered head / task stream)
            with torch.cuda.graph(gs[0], stream=cap, capture_error_mode=CAPTURE_MODE):
                # the gradient buffer is cleared BESIDE the forward pass, as in the one-rank capture (a fork and a join inside
                # the first graph; _stage_a joins it before the heads' backward writes the first gradient)
                self._fork_grad_clear(hyper=False)
                if self.input_hook is not None:
                    self.input_hook()
                total, vectors = self._stage_a(batches, merged)
                self._join_zero()  # (a stage A that did not: the fork must end inside this graph)
            pool = gs[0].pool()
            with torch.cuda.graph(gs[1], pool=pool, stream=cap, capture_error_mode=CAPTURE_MODE):
                self._install_tail(self._tail_only_plan(live))  # (stage B ends with the stack's flush, stage C is the tail launch)
                self._stage_b()
            with torch.cuda.graph(gs[2], pool=pool, stream=cap, capture_error_mode=CAPTURE_MODE):
                self._stage_c()
        self._graph, self._static_out, self._fuse_adam = gs, (total, vectors), False
        self._static_in = (batches, merged, self._stage_state, self._cuts)  # everything the graphs read stays alive
        return gs

    def replay(self):
        """One training step from the captured graph(s)."""
        opt = self.optimizer
        if getattr(opt, "_ema_swapped", False):  # (the graph's optimizer launch runs without ``opt.launch`` on the host: its check is made here)
            raise RuntimeError("replay(): inside optimizer.ema_weights() the parameters hold the average -- no step there")
        self._count_losses(self._static_out[1])
        if not self._rng_in_graph:
            ops.advance_rng_device(opt.flat_p.device)
        if isinstance(self._graph, list):
            regions = self._stage_regions()
            if self.sync is not None:
                self.sync.begin_step()
            for g, region in zip(self._graph, regions):
                g.replay()
                self._exchange_region(region)
            self._finish_staged()
            return self._static_out[0]
        if self._fuse_adam:
            if self._hyper_in_graph:
                opt.sync_hyper_source()  # (host -> device only when lr / grad_scale changed or the step count was set)
                self._graph.replay()
                opt.note_captured_step()
            else:
                opt.prepare_hyper()
                self._graph.replay()
            opt.step_count += 1
            # the graph's Adam launch moved flat_p on the DEVICE without opt.launch() running on the host: every low half a
            # 'bf16x3' contraction marked fresh before this replay (validation's precise pass between two epochs) is stale now --
            # unless the captured Adam launches write the low halves themselves: then ALL of them are fresh behind a replay
            if self._graph_adam_lo:
                opt._lo_fresh = [(0, opt.flat_p.numel())]
            else:
                opt.invalidate_lo_shadows()
        else:
            self._graph.replay()
            self._exchange_and_update()  # (one-piece graph, the exchange and the optimizer behind it)
        return self._static_out[0]


class MTLStep(StepBase):
    """One multi-task pre-training step (BASELINE configs 2, 3, 5; reference main_temporal.train :49-134)."""

    def __init__(self, model, tasks: Mapping[str, torch.nn.Module], criteria: Mapping[str, torch.nn.Module],
                 weights: Mapping[str, float], optimizer, fused_backbone: bool = True, sync: Optional[GradSync] = None,
                 parallel_heads: bool = True, task_weighting: str = "none", log_var=None):
        """``task_weighting``: none | manual | uncertainty.  ``manual``: ``set_task_scale`` changes the balance of the
        tasks between two steps, replays included.  ``uncertainty``: ``log_var``, a models.TaskLogVariance over ``enabled`` whose
        parameter is the LAST parameter of ``optimizer`` (train.build_optimizer), is learned with the weights."""
        self._init_base(model, tasks, weights, optimizer, fused_backbone, sync, parallel_heads)
        self.criteria = dict(criteria)
        self._head_batches = None  # the batches of the step being issued, for the heads (``_heads_forward_backward``)
        self._coef_grads = {}      # per task the constant its head's backward starts from (w_t / numel), filled once
        self._init_task_weighting(task_weighting, log_var)

    # ---- task weights in device memory (include/egopack_task_scale.h) ---------------------------------------------------
    # Every head's backward seed w_t / N_t is multiplied INSIDE its kernel by task_scale[i] (i: the task's place in ``enabled``), one
    # separately rounded f32 product.  manual: the host writes the vector; uncertainty: exp(-log_var), written by one launch at the
    # head of the step, and the rider that reports the objective also stores d J / d log_var into the parameter's gradient slot.
    def _init_task_weighting(self, mode, log_var) -> None:
        mode = str(mode or "none").lower()
        if mode not in TASK_WEIGHTING_MODES:
            raise ValueError(f"task_weighting: unknown mode '{mode}' ({' | '.join(TASK_WEIGHTING_MODES)})")
        if mode == "uncertainty":
            if log_var is None or tuple(getattr(log_var, "tasks", ())) != tuple(self.enabled):
                raise ValueError(f"task_weighting uncertainty: log_var must be a TaskLogVariance over the enabled tasks {self.enabled}, "
                                 f"got {None if log_var is None else tuple(getattr(log_var, 'tasks', ()))}")
            known = {id(p) for g in self.optimizer.param_groups for p in g["params"]}
            if id(log_var.log_var) not in known:
                raise ValueError("task_weighting uncertainty: log_var is not a parameter of the optimizer (train.build_optimizer(log_var=...))")
        elif log_var is not None:
            raise ValueError(f"task_weighting {mode}: log_var is for the uncertainty mode")
        if mode != "none":
            if not (self.headwise_backward and self.enabled):
                raise ValueError("task_weighting needs the head-wise backward (headwise_backward) and an enabled task")
            self._task_scale_host = [1.0] * len(self.enabled)
        self.task_mode, self.task_log_var = mode, (log_var if mode == "uncertainty" else None)
        if hasattr(self.optimizer, "task_weighting"):
            self.optimizer.task_weighting = mode  # (dist.GradSync refuses the sharded update by name)

    def _task_scale_for(self, device):
        """The scale vector on ``device`` (None when the feature is off), created outside captures."""
        if self.task_mode == "none":
            return None
        sc = self.task_scale
        if sc is None or sc.device != device:
            if torch.cuda.is_current_stream_capturing():
                raise RuntimeError("the task-scale vector must exist before a capture (run one eager step first)")
            sc = self.task_scale = torch.tensor(self._task_scale_host, dtype=torch.float32, device=device)
        return sc

    def set_task_scale(self, scales: Mapping[str, float]) -> None:
        """manual mode: task t's share of the objective becomes w_t * scales[t] from the next step on -- eager or replayed, no new
        capture.  One small asynchronous copy from a fresh pinned buffer on the current stream; tasks not named keep their scale."""
        if self.task_mode != "manual":
            raise ValueError(f"set_task_scale: task_weighting.mode is '{self.task_mode}' (manual sets scales from the host)")
        if torch.cuda.is_available() and torch.cuda.is_current_stream_capturing():
            raise RuntimeError("set_task_scale: not inside a capture (the copy would become a node with today's values)")
        unknown = [t for t in scales if t not in self.enabled]
        if unknown:
            raise ValueError(f"set_task_scale: {unknown} not among the enabled tasks {self.enabled}")
        for t, v in scales.items():
            v = float(v)
            if not (math.isfinite(v) and v >= 0.0):
                raise ValueError(f"set_task_scale: the scale of {t} must be finite and >= 0, got {v}")
            self._task_scale_host[self.enabled.index(t)] = v
        if self.task_scale is not None:
            host = torch.tensor(self._task_scale_host, dtype=torch.float32)
            self.task_scale.copy_(host.pin_memory() if self.task_scale.is_cuda else host, non_blocking=True)

    def task_scales(self) -> Dict[str, float]:
        """{task: the scale the kernels read now} (one device synchronisation; 1.0 each when the feature is off)."""
        if self.task_scale is None:
            return {t: (1.0 if self._task_scale_host is None else self._task_scale_host[i]) for i, t in enumerate(self.enabled)}
        return dict(zip(self.enabled, self.task_scale.tolist()))

    def _task_scale_head(self) -> None:
        if self.task_mode == "uncertainty":
            p = self.task_log_var.log_var
            ops.task_scale_prepare(p.detach(), self._task_scale_for(p.device))

    def _seed_grad(self, key, v, t, coef, scale):
        """The tensor head ``t``'s backward starts from: the constant ``coef`` filled once -- with a task scale, fl32(coef * scale)
        filled by one launch per step (egk_fill_scaled_from), and only when the head left the announced-seed paths (a head on
        them never reads the tensor)."""
        g = self._coef_grads.get(key)
        if g is None or g._egk_coef != coef:
            g = self._coef_grads[key] = torch.full_like(v, coef, dtype=v.dtype).detach()
            g._egk_coef = coef
        if scale is not None and not ops.seed_consumed(v):
            if v.dtype != torch.float32:
                raise RuntimeError(f"head {t}: a {v.dtype} loss vector cannot start from a scaled seed")
            ops.fill_scaled_from(g, coef, scale)
        return g

    # ---- sequence mixup (include/egopack_mixup.h) -------------------------------------------------------------------------
    # A training batch of a mixed task carries mix_src / mix_lam / mix_y (data.BatchLoader); batches without them run exactly the
    # launches they ran before.  ONE launch in front of the backbone writes the mixed rows of all task batches into a second input
    # buffer (out of place: the staged input stays as it was, so a replay over it mixes the same rows again, not the mix), an
    # unmixed task's rows are copied by the same launch; the heads hand both labels and lambda to their cross entropy.
    def _mix_of(self, d):
        """(mix_y, mix_lam) of a batch that carries the fields while the model trains, else None."""
        if d is None or not self.model.training or getattr(d, "mix_src", None) is None:
            return None
        return d.mix_y, d.mix_lam

    @staticmethod
    def _mix_rows_of(xs, ds):
        """The mixed copies of the input blocks ``xs`` ([N, ...] each) of the batches ``ds``: one launch over all of them."""
        outs = [torch.empty_like(x) for x in xs]
        flat = lambda x: x.reshape(x.shape[0], -1)
        mixed = [getattr(d, "mix_src", None) is not None for d in ds]
        ops.mix_rows([flat(x) for x in xs], [flat(o) for o in outs], [d.mix_src if m else None for d, m in zip(ds, mixed)],
                     [d.mix_lam if m else None for d, m in zip(ds, mixed)])
        return outs

    def features(self, batches, merged=None):
        live = self._live(batches)
        if not any(self._mix_of(batches[t]) is not None for t in live):
            return super().features(batches, merged)
        if self.fused and len(live) > 1:
            if merged is None:
                merged = merge_batches([batches[t] for t in live])
                merged = merged.to(batches[live[0]].pos.device)
            x = merged.x
            if isinstance(x, (list, tuple)):
                x = torch.cat(list(x))
            rows = [batches[t].pos.shape[0] for t in live]
            offs = [sum(rows[:i]) for i in range(len(rows) + 1)]
            out = torch.empty_like(x)
            flat = lambda v: v.reshape(v.shape[0], -1)
            ds = [batches[t] for t in live]
            mixed = [self._mix_of(d) is not None for d in ds]
            ops.mix_rows([flat(x[a:b]) for a, b in zip(offs, offs[1:])], [flat(out[a:b]) for a, b in zip(offs, offs[1:])],
                         [d.mix_src if m else None for d, m in zip(ds, mixed)], [d.mix_lam if m else None for d, m in zip(ds, mixed)])
            keep = (merged.__dict__.get("x"), merged.__dict__.get("x_base"))
            merged.x = merged.x_base = out
            try:
                feat = self.model(merged)
            finally:
                merged.x, merged.x_base = keep
            return dict(zip(live, ops.split_rows(feat, rows)))
        feats = {}
        for t in live:
            d = batches[t]
            if self._mix_of(d) is None:
                feats[t] = self.model(d)
                continue
            keep = (d.__dict__.get("x"), d.__dict__.get("x_base"))
            d.x, = self._mix_rows_of([d.x], [d])
            d.x_base = None
            try:
                feats[t] = self.model(d)
            finally:
                d.x, d.x_base = keep
        return feats

    def _head(self, t: str, feat, d):
        task = self.tasks[t]
        f = task.forward_features(feat)
        logits = task.forward_logits(f, d) if t == "oscc" else task.forward_logits(f)
        return self.criteria[t](logits, d.y), logits

    def losses(self, batches: Mapping[str, Data], merged: Optional[Data] = None):
        feats = self.features(batches, merged)
        vectors, logits_out = self._run_heads(feats, lambda t, feat: self._head(t, feat, batches[t]))
        return self._objective(vectors), vectors, logits_out

    # the projection heads of the task batches as ONE chain of grouped launches (ops.grouped_projection) instead of one
    # chain per task on its own stream: same shapes, different rows, different weights -- 3 x 2048-row launches that each
    # fill half of the chip become one 6144-row launch per stage (bf16 mode, once the optimizer's flat buffers exist)
    grouped_heads = True

    # a head whose classifier has ONE logit under BCE-with-logits (PNR) runs classifier + loss + their gradients as one row
    # pass (ops.linear1_bce) instead of ten launches of [N, H] x [H, 1] matrix work: same-box A/B of the headline step
    # 1.650 -> 1.624 ms.  Same values up to summation order (a row reduction instead of an MFMA K walk), so the bitwise
    # equalities between execution structures (tests/test_gpu_dist.py) are stated with it off
    one_pass_heads = True

    def _one_pass_head_ok(self, t: str) -> bool:
        from .criterion import BCEWithLogitsNone
        return self.one_pass_heads and hasattr(self.tasks[t], "fused_head_loss") and type(self.criteria[t]) is BCEWithLogitsNone

    def _one_pass_oscc_ok(self, t: str) -> bool:
        """The OSCC head (max pool -> 2-logit classifier -> cross entropy, one loss element per SEQUENCE) as pool + one launch
        (ops.linear2_ce): its eleven short launches sat on the critical path of the 4-task step between forward and backward."""
        from .criterion import CrossEntropyNone
        return (t == "oscc" and self.one_pass_heads and hasattr(self.tasks[t], "fused_head_loss")
                and type(self.criteria[t]) is CrossEntropyNone and switches.enabled("oscc_one_pass"))

    def _banked_tasks(self, order, proj_leaves):
        """Tasks whose multi-head classifier banks can share grouped launches (ops.grouped_classifier_banks): at least two."""
        cand = []
        for t in order:
            task = self.tasks[t]
            cls = getattr(task, "classifiers", None)
            if cls is None or (task.training and any(c[0].p > 0 for c in cls)):
                continue  # (no multi-head bank, or classifier dropout active: the per-task path)
            if getattr(cls[0][1].weight, "_egk_bank_views", None) is None or not isinstance(self.criteria[t], MetricSelectorWrapper):
                continue
            cand.append(t)
        if len(cand) < 2:
            return []
        views = [self.tasks[t].classifiers[0][1].weight._egk_bank_views for t in cand]
        return cand if ops.grouped_classifier_banks_ok([proj_leaves[t] for t in cand], views) else []

    def _heads_forward_backward(self, feats):
        """Heads' forward AND backward, every head inside its own stream context, on detached copies of the backbone
        features: returns (objective, loss vectors, {task: leaf}) with d(objective)/d(features) in ``leaf.grad``.
        The objective is sum_t w_t * mean(v_t) (main_temporal.py:99-128), so head t's backward starts from the
        constant w_t / numel(v_t) -- the value the one-call backward of the objective hands it, bit for bit."""
        leaves = {t: f.detach().requires_grad_(True) for t, f in feats.items()}
        batches = self._head_batches
        order = list(leaves)
        nets = [self.tasks[t].net for t in order]
        # Row compaction (exact): the heads are row-wise and a node whose labels are all ``ignore_index`` has loss 0 and gradient 0
        # (AR labels the centre node of a sequence only, data/ego4d_fho.py:222-223): such a task's projection, classifiers, loss and
        # their backward run on its labelled rows (data.live_label_rows, padded with all-zero rows / ignored labels to a multiple of
        # 64) and the feature gradient goes back to full height with zero rows elsewhere.  Loss vectors keep one element per node.
        live = {t: batches[t] for t in order if self._compact_head_ok(t, batches[t], leaves[t])}
        n_full = {t: leaves[t].shape[0] for t in order}
        labels = {t: (live[t].live_y if t in live else batches[t].y) for t in order}
        compact_v = {}  # the compacted heads' loss vectors as computed (the objective sums these; n_full divides)

        def full_vector(t, v):
            if t not in live:
                return v.detach()
            # one element per node for the caller (meters); the launch feeds nothing on the chain: it rides with the parked weight
            # gradients' next flush, on their stream
            compact_v[t] = v.detach()
            out = torch.empty(n_full[t], dtype=v.dtype, device=v.device)
            inv, src = live[t].live_inv, compact_v[t]
            sched.park_rider(lambda: ops.expand_rows(src, inv, out=out), (src, inv, out))
            return out
        # (a task whose labelled rows are an arithmetic progression -- one labelled node per sequence -- hands the grouped
        #  projection its full-height features and a row spec: a strided view stands for the gathered rows, no launch)
        specs, grouped = {}, False
        if self.grouped_heads and len(order) > 1:
            specs = {t: (*live[t].live_ap, live[t].live_inv) for t in live if getattr(live[t], "live_ap", None) is not None}
            grouped = ops.grouped_projection_ok([leaves[t] for t in order], nets, [specs.get(t) for t in order])
            if not grouped:
                specs = {}
        heads_in = {t: (leaves[t] if (t not in live or t in specs) else ops.live_rows(leaves[t], live[t].live_idx, live[t].live_inv))
                    for t in order}
        if self.grouped_heads and len(order) > 1 and not grouped:
            grouped = ops.grouped_projection_ok([heads_in[t] for t in order], nets)
        proj = proj_leaves = None
        if grouped:
            proj = ops.grouped_projection([heads_in[t] for t in order], nets, specs=[specs.get(t) for t in order])
            proj_leaves = {t: f.detach().requires_grad_(True) for t, f in zip(order, proj)}
            ops.stamp("heads_proj_fwd_done")
        else:
            specs = {}

        sc_vec = self._task_scale_for(next(iter(leaves.values())).device) if leaves else None
        sc = {t: (None if sc_vec is None else sc_vec[i:i + 1]) for i, t in enumerate(self.enabled)}  # each task's word of the vector

        def head(t, leaf):
            # AR / LTA: one loss element per node, back-propagated below with the constant w_t / numel -- known before the
            # loss is computed, so the cross entropy emits its gradient in the same launch (ops.loss_seed)
            # (the loss vector has one element per NODE, so the seed divides by the full node count also for a compacted head)
            n_loss = n_full[t] if t in ("ar", "lta", "pnr") else 0
            oscc_one = self._one_pass_oscc_ok(t) and batches[t].y.dim() == 1
            if oscc_one:
                n_loss = int(batches[t].y.numel())  # one loss element per sequence
            with ops.loss_seed(self.weights[t] / n_loss if n_loss else None, scale=sc[t]):
                task, d = self.tasks[t], batches[t]
                f = leaf if grouped else task.forward_features(leaf)  # grouped: ``leaf`` is the projected feature block
                one_pass = None
                if oscc_one:
                    one_pass = task.fused_head_loss(f, d, d.y, getattr(self.criteria[t], "label_smoothing", 0.0))
                elif n_loss and self._one_pass_head_ok(t):
                    # one-logit classifier + BCE + their gradients: one row pass (with the criterion's pos / neg / gamma, if any)
                    one_pass = task.fused_head_loss(f, d.y, balance=self.criteria[t].balance())
                if one_pass is not None:
                    v, logits = one_pass
                elif oscc_one:  # (did not apply after all: the contraction path WITHOUT an announced seed, as before)
                    with ops.loss_seed(None):
                        logits = task.forward_logits(f, d)
                        v = self.criteria[t](logits, d.y)
                    n_loss = 0
                else:
                    logits = task.forward_logits(f, d) if t == "oscc" else task.forward_logits(f)
                    mix = self._mix_of(d) if isinstance(self.criteria[t], MetricSelectorWrapper) else None
                    v = self.criteria[t](logits, labels[t]) if mix is None else self.criteria[t](logits, labels[t], mix=mix)
            n_out = v.numel() if t not in live else n_full[t]  # elements of the loss vector the objective averages over
            if n_loss and n_out != n_loss:
                raise RuntimeError(f"head {t}: {n_out} loss elements where {n_loss} were announced to the fused loss")
            if v.numel():
                # the constant the objective's backward hands this head (w_t / numel): one tensor per task, filled once
                g = self._seed_grad((t, v.numel(), n_out, v.dtype, v.device), v, t, self.weights[t] / n_out, sc[t])
                v.backward(gradient=g)
            return full_vector(t, v), logits
        # the multi-head classifier banks of several tasks (AR and LTA: same widths, own rows and weights) as ONE chain of
        # grouped launches on the main stream -- grouped classifier contraction, one fused cross entropy per task, grouped dX --
        # instead of one chain per task on its own stream (each fork / join of a stream costs more than these launches)
        banked = self._banked_tasks(order, proj_leaves) if grouped else []
        banked_vectors = {}

        def banked_chain():
            views = [self.tasks[t].classifiers[0][1].weight._egk_bank_views for t in banked]
            n_loss = {t: n_full[t] for t in banked}  # (one loss element per NODE: a compacted head's seed divides by the full count)
            all_logits = ops.grouped_classifier_banks([proj_leaves[t] for t in banked], views, fused_loss=True)
            vs, gs = [], []
            multi = None
            # the cross entropies of the banked tasks as ONE launch (each writes its own loss vector and gradient operand)
            sel = [self.criteria[t].select(logits, labels[t]) for t, logits in zip(banked, all_logits)]
            if len({s_[2] for s_ in sel}) == 1:
                # (the criteria's class-balance vectors, margins and focal exponents ride in the same launch; without any it is the
                #  launch it always was)
                bal = [self.criteria[t].select_balance(logits) for t, logits in zip(banked, all_logits)]
                shp = [self.criteria[t].select_shape(logits) for t, logits in zip(banked, all_logits)]
                mixes = [self.criteria[t].select_mix(logits, self._mix_of(batches[t])) for t, logits in zip(banked, all_logits)]
                multi = ops.cross_entropy_multi([(s_[0], s_[1]) for s_ in sel], [self.weights[t] / n_loss[t] for t in banked],
                                                sel[0][2], weights=[w for w, _ in bal], offsets=[a for _, a in bal],
                                                scales=None if sc_vec is None else [sc[t] for t in banked],
                                                margins=[m for m, _ in shp], gammas=[g for _, g in shp],
                                                mixes=mixes if any(m is not None for m in mixes) else None)
            for i, (t, logits) in enumerate(zip(banked, all_logits)):
                if multi is not None:
                    v = multi[i]
                else:
                    with ops.loss_seed(self.weights[t] / n_loss[t], scale=sc[t]):
                        mix = self._mix_of(batches[t])
                        v = self.criteria[t](logits, labels[t]) if mix is None else self.criteria[t](logits, labels[t], mix=mix)
                if v.numel() != proj_leaves[t].shape[0]:
                    raise RuntimeError(f"head {t}: {v.numel()} loss elements for {proj_leaves[t].shape[0]} rows")
                g = self._seed_grad((t, v.numel(), n_loss[t], v.dtype, v.device), v, t, self.weights[t] / n_loss[t], sc[t])
                vs.append(v)
                gs.append(g)
                banked_vectors[t] = full_vector(t, v)
            torch.autograd.backward(vs, gs)  # ONE pass: both cross entropies, then the grouped banks' backward once
        with ops.bank_grad_handoff():  # every head's logits feed exactly one loss node here
            src = proj_leaves if grouped else heads_in
            rest = {t: f for t, f in src.items() if t not in banked}
            vectors, _ = self._run_heads(rest, head, main_job=banked_chain if banked else None)
            vectors.update(banked_vectors)
            vectors = {t: vectors[t] for t in order if t in vectors}
        if grouped:  # back on the main stream: the grouped projection's backward down to the backbone features
            ops.stamp("heads_classifiers_done")
            live = [t for t in order if proj_leaves[t].grad is not None]
            if live:
                outs = dict(zip(order, proj))
                torch.autograd.backward([outs[t] for t in live], [proj_leaves[t].grad for t in live])
        with torch.no_grad():
            # the reported objective feeds nothing on the chain (every head's backward started from its known seed): its one-workgroup
            # reduction rides with the parked weight gradients' next flush, on their stream, instead of sitting between the heads'
            # backward and the backbone's
            src = {t: compact_v.get(t, v) for t, v in vectors.items()}
            cnt = {t: (n_full[t] if t in compact_v else None) for t in vectors}
            if not src:
                total = self._objective(src, cnt)
                self._ride_loss_sums(src)
            else:
                # (every enabled task has its slot in the launch -- absent ones add exactly 0 -- so that the running per-task loss
                #  sums, ``loss_sums``, accumulate in the same launch at fixed positions)
                order = list(self.enabled)
                total = torch.empty((), dtype=torch.float32, device=next(iter(src.values())).device)
                acc = self._loss_acc_for(total.device)
                if sc_vec is None:
                    sched.park_rider(lambda: ops.weighted_mean_sum_into(total, [src.get(t) for t in order], [self.weights[t] for t in order],
                                                                        [cnt.get(t) for t in order], acc=acc),
                                     (total, *[src[t] for t in order if t in src]))
                else:
                    # with task scales the rider is egk_task_scale_grad: the objective under the scales, the RAW loss sums, and in the
                    # uncertainty mode d J / d log_var stored into the parameter's gradient slot (its one writer: final with the
                    # heads' weight gradients it rides beside, before anything reads the heads' region of the flat gradient)
                    lv = ds = None
                    if self.task_mode == "uncertainty":
                        p = self.task_log_var.log_var
                        lv, ds = p.detach(), ops._grad_slot(p)
                        if ds is None:  # (the first step, before the flat buffers exist: an ordinary .grad)
                            ds = p.grad = torch.zeros_like(p)
                    out1 = total.view(1)
                    sched.park_rider(lambda: ops.task_scale_grad_into(out1, [src.get(t) for t in order], [self.weights[t] for t in order],
                                                                      sc_vec, [cnt.get(t) for t in order], log_var=lv, ds=ds, acc=acc),
                                     (total, *[src[t] for t in order if t in src]))
        return total, vectors, leaves

    compact_heads = True  # heads on the labelled rows only (data.live_label_rows); False: every row

    def _compact_head_ok(self, t: str, d, leaf) -> bool:
        """Task ``t``'s head runs on its labelled rows: a multi-head cross-entropy head (MetricSelectorWrapper over
        CrossEntropyNone with ignore_index -1: the row's loss and gradient are exactly zero when every head's label is -1 --
        with the wrapper's class-balance vectors too: an ignored row's loss and gradient are 0 whatever its weights and offsets),
        no active dropout in the head (its masks are drawn by row position), the batch built by data.collate with its
        ``live_*`` index arrays on the features' device."""
        if not self.compact_heads or t not in ("ar", "lta"):
            return False
        if self._mix_of(d) is not None:  # (mixup: a row is live if EITHER label is; the live_* arrays know the first only)
            return False
        idx = getattr(d, "live_idx", None)
        if idx is None or getattr(d, "live_inv", None) is None or getattr(d, "live_y", None) is None:
            return False
        if not (idx.is_cuda and idx.device == leaf.device and d.live_inv.numel() == leaf.shape[0]):
            return False
        from .criterion import CrossEntropyNone
        crit = self.criteria.get(t)
        if not isinstance(crit, MetricSelectorWrapper) or type(getattr(crit, "criterion", None)) is not CrossEntropyNone:
            return False
        # (a row labelled only in a column the wrapper does not select is kept: its loss and gradient are still exactly zero)
        task = self.tasks[t]
        drops = [m for m in task.modules() if isinstance(m, torch.nn.Dropout) or type(m).__name__ == "Dropout"]
        return not (task.training and any(getattr(m, "p", 0) > 0 for m in drops))

    headwise_backward = True  # False: one backward() call over all streams (kept for A/B measurements)
    early_adam = True

    def _early_adam_ok(self) -> bool:  # the heads are joined into the main stream before the backbone's backward starts
        return bool(self.early_adam and self.headwise_backward)

    def _backward_pass(self, batches, merged=None):
        if not self.headwise_backward:
            if self.task_mode != "none":
                raise RuntimeError("task weighting scales the seeds of the head-wise backward: headwise_backward must stay on")
            return super()._backward_pass(batches, merged)
        self._head_batches = batches
        feats = self.features(batches, merged)
        ops.stamp("fwd_backbone_done")
        self._join_zero()
        total, vectors, leaves = self._heads_forward_backward(feats)
        ops.stamp("heads_done")
        # the heads' parked weight gradients (classifier banks, projections) go out as one launch NOW, beside the first
        # links of the backbone's dX chain; left parked, the backbone's first weight gradient would flush nine problems
        # as 8 + 1
        sched.flush_wgrad(in_backward=False, force=True)
        order = [t for t in feats if leaves[t].grad is not None]
        torch.autograd.backward([feats[t] for t in order], [leaves[t].grad for t in order])
        return total, vectors

    # ---- the three backward stages (StepBase._staged_step) ---------------------------------------------------------
    def _stage_regions(self):
        opt, model = self.optimizer, self.model
        if not hasattr(opt, "region_of") or not hasattr(model, "net") or getattr(model, "temporal_pooling", None) is None:
            return None
        head_params = [p for t in self.enabled for p in self.tasks[t].parameters()]
        if self.task_log_var is not None:  # (the log-variances' slot follows the heads' slots: one region)
            head_params += list(self.task_log_var.parameters())
        mid_params = list(model.net.parameters())
        mid_ids = {id(p) for p in mid_params}
        trn_params = [p for p in model.parameters() if id(p) not in mid_ids]
        heads, mid, trn = opt.region_of(head_params), opt.region_of(mid_params), opt.region_of(trn_params)
        total = opt.flat_p.numel()
        tiles = sorted(r for r in (trn, mid, heads) if r[1] > r[0])
        ok = tiles and tiles[0][0] == 0 and tiles[-1][1] == total and all(a[1] == b[0] for a, b in zip(tiles, tiles[1:]))
        return [heads, mid, trn] if ok else None  # (any other layout: the one-piece backward + pipelined exchange)

    def _stage_a(self, batches, merged):
        """Forward, heads' forward / backward: final gradients of the head parameters + d(objective)/d(features)."""
        self._cuts = []

        def cut(x):
            leaf = x.detach().requires_grad_(True)
            self._cuts.append((x, leaf))
            return leaf
        self.model.stage_cut = cut
        try:
            feats = self.features(batches, merged)
        finally:
            self.model.stage_cut = None
        self._head_batches = batches
        self._join_zero()  # (a capture that clears the gradient buffer beside the forward pass: before the first gradient)
        total, vectors, leaves = self._heads_forward_backward(feats)
        self._stage_join()
        self._stage_state = (feats, leaves)
        return total, vectors

    def _stage_b(self):
        """Backbone output -> TRN output: final gradients of the SAGE stack."""
        feats, leaves = self._stage_state
        order = list(feats)
        torch.autograd.backward([feats[t] for t in order], [leaves[t].grad for t in order])
        self._stage_join()

    def _stage_c(self):
        """TRN output -> inputs: final gradients of the temporal pooling."""
        if self._cuts:
            torch.autograd.backward([x for x, _ in self._cuts], [leaf.grad for _, leaf in self._cuts])
            self._stage_join()


def _minus(ranges, holes):
    """The element ranges ``ranges`` without the ranges ``holes`` (lists of [lo, hi))."""
    out = list(ranges)
    for h0, h1 in holes:
        nxt = []
        for a, b in out:
            if h1 <= a or b <= h0:
                nxt.append((a, b))
                continue
            if a < h0:
                nxt.append((a, h0))
            if h1 < b:
                nxt.append((h1, b))
        out = nxt
    return [(a, b) for a, b in out if b > a]


class EgoPackStep(StepBase):
    """One novel-task step of main_egopack.train with late fusion (BASELINE configs 4, 5; reference
    main_egopack.py:45-159): backbone (train/eval mode and grad mode as configured) -> primary projection; aux
    projections DETACHED -> GraphONE.interact -> fused logits -> primary.compute_loss."""

    order = ("ar", "oscc", "lta", "pnr")  # order of the loss terms in main_egopack.train
    # grouped weight gradients and late forks: OFF until round 4 (3.77-3.89 against 3.62-3.72 ms then); with the OSCC head as six
    # launches and the three GraphONE backward chains on three queues they measure 3.20-3.24 against 3.47-3.48 ms
    wgrad_grouping_default = True
    deferred_forks_default = True
    wgrad_group_count = 8  # 2048-row batches: eight H x H problems = 512 tiles = two per CU (3.16 -> 3.09 ms; six on the 3-task step)
    AUX_ORDER = {"ar": ("lta", "oscc", "pnr"), "oscc": ("ar", "lta", "pnr"), "lta": ("ar", "oscc", "pnr"),
                 "pnr": ("ar", "oscc", "lta")}  # main_egopack.py:121-147

    def __init__(self, model, tasks: Mapping[str, torch.nn.Module], graphone, weights: Mapping[str, float], optimizer,
                 backprop_temporal_graph: bool = True, temporal_graph_train_mode: bool = False,
                 sync: Optional[GradSync] = None, fused_backbone: bool = True, parallel_heads: bool = True,
                 task_weighting: str = "none"):
        if str(task_weighting or "none").lower() != "none":
            raise ValueError(f"task_weighting.mode '{task_weighting}': the EgoPack step trains ONE primary task -- there is no balance "
                             "between tasks to adjust or learn (task weighting is for the multi-task step of main_temporal.py)")
        self._init_base(model, tasks, weights, optimizer, fused_backbone, sync, parallel_heads)
        self.graphone = graphone
        self.backprop, self.train_mode = backprop_temporal_graph, temporal_graph_train_mode
        self._precise_side = None  # the stream of the precise pass beside the training pass's forward, created on first use (``losses``)
        # Tasks that are not trained here only lend their projection heads to the detached auxiliary features (reference
        # main_egopack.py:53: ``.detach()``): their parameters never receive a gradient and the reference's Adam skips them
        # (grad is None).  They are marked frozen, which changes no result and lets the operand copies of their weights (bf16
        # copies, bf16 halves of the three-product path) be made once instead of at every use.
        for t, task in self.tasks.items():
            if t not in self.enabled:
                for p in task.parameters():
                    p.requires_grad_(False)

    # The nearest-prototype search is an INDEX op (reference graphONE.py:119-141: argsort of the cosine distances): its lists must
    # be the reference's, whatever the storage type of the training pass.  With bf16 activations the detached auxiliary features
    # carry the rounding of a dozen bf16 layers (~1 % relative), enough to flip ~5 % of the neighbour positions at K = 4096.  In
    # the bf16 modes they therefore come from a second, forward-only pass over the same batch in 'bf16x3' mode (f32 activations,
    # every contraction as three bf16 products of split operands: f32-grade at ~3x the bf16 cost, ops.precise_scope): backbone
    # + auxiliary projections, no gradient -- the reference detaches these features (main_egopack.py:53).  The GraphONE stages
    # consume the same values (rounded to the activation type).
    precise_search = True
    # Adam over everything but the temporal pooling's slots beside the step's last weight-gradient launch (StepBase._early_adam_plan):
    # the step is ONE backward() call whose last node is the first TRN linear -- every other node has been issued by then, on
    # the backward stream or on the branch streams below, which the optimizer slice waits for.  Config 4: 55 M parameters,
    # Adam alone at the end of the step lasted 261 us of 2.84 ms
    early_adam = True

    def _early_adam_ok(self) -> bool:
        return bool(self.early_adam and self.backprop)

    def _branch_streams(self):
        return [*self._head_streams, *getattr(self.graphone, "_task_streams", ()), self._precise_side]

    def _gradient_branch_streams(self):
        return [*getattr(self.graphone, "_task_streams", ()), *self._head_streams]

    def _early_adam_plan(self, live):
        """+ GraphONE's own slice (``graphone_adam`` off: none): its stage parameters (half of the step's parameters in config
        4) have their final gradients when the grouped GraphONE backward returns (sched.set_graphone_backward_hook) -- Adam over
        that slice then runs beside the backbone's backward instead of in the step's tail.  Round 4: the tail shrank from 275 to
        114 us and the backbone's backward grew by as much (2.746-2.751 against 2.72-2.80 ms, HISTORY.md: the
        memory-bound launch slows the chain it runs beside) -- opt-in then.  Round 5, with the searches grouped and the precise pass
        first: 2.42-2.45 against 2.475-2.478 ms (three alternating rounds): the default.  Elementwise, the same update bit for bit
        (tests/test_gpu_configs.py::test_config4_graphone_optimizer_slice_is_the_same_update)."""
        plan = super()._early_adam_plan(live)
        opt = self.optimizer
        if plan is None or not switches.enabled("graphone_adam") or len(live) != 1:
            return plan
        params = [p for p in self.graphone.parameters() if p.requires_grad and id(p) in opt._slot_of]
        if not params:
            return plan
        g0, g1 = opt.region_of(params)
        slots = [opt._slot_of[id(p)] for p in params]
        if not (g1 > g0 and g0 % 8 == 0 and g1 % 8 == 0 and sum(n for _, n in slots) == g1 - g0 and (g1 <= plan["lo"] or g0 >= plan["hi"])):
            return plan
        plan["done"] = []
        plan["graphone_region"] = (g0, g1)

        def graphone_done():
            if plan["fired"] or plan["done"]:
                return
            sched.flush_wgrad(force=True)  # (what the interaction left parked; issued behind the backward stream's next launch)
            main = torch.cuda.current_stream()

            def issue(ev):
                side = sched.wgrad_side_stream(main)
                plan["stream"].wait_event(ev)
                if side is not None:
                    plan["stream"].wait_stream(side)
                with torch.cuda.stream(plan["stream"]):
                    if plan.get("clip"):
                        opt.norm_partials(None, g0, g1)
                        plan["normed"].append((g0, g1))
                    else:
                        opt.launch(None, g0, g1)
            sched.defer_after_next_launch(issue)
            plan["done"].append((g0, g1))
        plan["graphone_hook"] = graphone_done
        return plan

    def _precise_on(self) -> bool:
        return bool(self.precise_search and ops.get_compute() in ("bf16", "bf16_f32act") and switches.enabled("precise_search"))

    def _aux_names(self, primary: str):
        return [t for t in self.AUX_ORDER[primary] if t in self.graphone.task_labels]

    @torch.no_grad()
    def precise_aux_features(self, batches, merged=None, rng_snap=None, tape=None):
        """{primary: {aux task: f32 [N, H]}}: the auxiliary projections of every enabled task batch from the 'bf16x3' pass.
        ``tape`` (a list): the backbone's nodes leave their results in it (ops.dual_record) for the one-pass step."""
        opt = self.optimizer
        live = self._live(batches)
        with ops.precise_scope(), ops.rng_replay(ops.rng_snapshot() if rng_snap is None else rng_snap):
            if getattr(opt, "materialised", False):
                opt.refresh_lo_shadows(list(self.model.parameters()))  # the backbone's low halves: one launch
            if tape is not None:
                with ops.dual_record() as rec:
                    feats = self.features(batches, merged)
                tape.extend(rec)
            else:
                feats = self.features(batches, merged)
            out = {}
            for t in live:
                others = self._aux_names(t)
                # the auxiliary projections of one batch as three grouped launches (+ one operand split) instead of ~5 per task at
                # the END of the precise chain, which the GraphONE stages wait for
                grouped = ops.grouped_projection_infer(feats[t], [self.tasks[o].net for o in others], out_f32=True) if len(others) > 1 else None
                out[t] = (dict(zip(others, grouped)) if grouped is not None
                          else {o: self.tasks[o].forward_features(feats[t], out_f32=True) for o in others})
        return out

    one_pass = True  # the bf16 training graph from the precise pass's results instead of a second backbone pass (see _one_pass_ok)

    def _one_pass_ok(self, batches, merged) -> bool:
        """ONE backbone pass per step (ops.dual_record / dual_replay) applies: a single task batch with bf16 features, gradients
        through the backbone, no active dropout in it (the keep masks of the two passes would have to be shared), statistics
        local to the rank.  ``one_pass`` off: the two-pass step of rounds 3-5."""
        if not (self.one_pass and self.backprop) or not switches.enabled("one_pass"):
            return False
        live = [batches[t] for t in self._live(batches)]
        if len(live) != 1 or isinstance(live[0].x, (list, tuple)) or live[0].x.dtype != torch.bfloat16 or ops.graph_ln_exchange_on():
            return False
        if ops.get_compute() != "bf16" or getattr(self.model, "stage_cut", None) is not None:
            return False
        drops = [m for m in self.model.modules() if type(m).__name__ == "Dropout" or isinstance(m, torch.nn.Dropout)]
        if self.model.training and any(getattr(m, "p", 0) > 0 for m in drops):
            return False
        tp = getattr(self.model, "temporal_pooling", None)
        return not (self.model.training and float(getattr(tp, "dropout", 0) or 0) > 0)

    def _search_ahead(self, precise) -> None:
        """The prototype searches of the coming ``GraphONE.interact`` calls on the CURRENT stream (the precise pass's): they need
        the precise features only, so they start when that pass ends -- not behind the join with the training pass's forward chain,
        which (created second) ends later: profiles/r05_c4_replay_timeline.txt vs r05b: the searches 907 -> 7xx us."""
        self.graphone.drop_searched()
        for d in precise.values():
            self.graphone.search_ahead(d)

    def task_loss(self, primary: str, feat, data, aux_in=None, f_primary=None):
        task = self.tasks[primary]
        others = self._aux_names(primary)
        if f_primary is None:
            f_primary = task.forward_features(feat)
        if aux_in is None:
            with torch.no_grad():
                # f32 out of the projections' last contraction: the nearest-prototype search (an index op) ranks the f32
                # accumulators in every compute mode; GraphONE brings them to the activation type for its stages
                grouped = ops.grouped_projection_infer(ops.to_act(feat), [self.tasks[t].net for t in others], out_f32=True)
                aux_in = (dict(zip(others, grouped)) if grouped is not None
                          else {t: self.tasks[t].forward_features(feat, out_f32=True) for t in others})
        aux, closest = self.graphone.interact(aux_in)
        ops.stamp("stages_done")
        if (primary == "oscc" and getattr(task, "loss_func", None) == "ce" and hasattr(task, "fused_head_loss") and data.y.dim() == 1
                and switches.enabled("oscc_one_pass")):
            # the four 2-logit classifiers (primary + one per auxiliary task) behind their max pools, the logit fusion, the loss and
            # every gradient as ONE launch: the objective is sum_t w_t mean(loss_t), so the loss vector's backward seed is the
            # constant w / B (ops.loss_seed) -- ~35 short launches of the contraction path otherwise
            with ops.loss_seed(self.weights[primary] / max(int(data.y.numel()), 1)):
                one = task.fused_head_loss(f_primary, data, data.y, smoothing=0.1, aux_features=aux,
                                           aux_streams=getattr(self.graphone, "stream_of", None))
            if one is not None:
                return one[0], one[1], aux, closest
        if primary == "oscc":
            logits = task.forward_logits(features=f_primary, batch=data, aux_features=aux)
        else:
            logits = task.forward_logits(features=f_primary, batch=getattr(data, "batch", None), aux_features=aux)
        return task.compute_loss(logits, data.y), logits, aux, closest

    def losses(self, batches: Mapping[str, Data], merged: Optional[Data] = None):
        self.model.train(self.train_mode)
        for t in self.tasks.values():
            t.train(True)
        self.graphone.train()
        snap = ops.rng_snapshot()
        precise, side = {}, None
        tape = None
        first = next((b for b in batches.values() if b is not None), None)
        on_side = self._precise_on() and first is not None and first.pos.is_cuda
        # Which chain is CREATED first keeps the launch queue under capture: the precise pass IS the step's critical chain and goes
        # first (2.529-2.549 against 2.565-2.586 ms with the training pass's forward chain created first, four alternating rounds).
        if self._precise_on():
            if on_side:
                # the precise pass is a chain of ~50 launches over the same few thousand rows as the training pass's forward:
                # forked onto its own stream, the two chains run side by side (each alone leaves most of the chip idle)
                main = torch.cuda.current_stream()
                if self._precise_side is None:  # (a high-priority stream: 5.05-5.26 against 2.53-2.55 ms in the captured step)
                    sched.exclude_wgrad_streams([self._own_stream("_precise_side")])
                side = self._precise_side
                side.wait_stream(main)
                tape = [] if self._one_pass_ok(batches, merged) else None
                with torch.cuda.stream(side):
                    precise = self.precise_aux_features(batches, merged, rng_snap=snap, tape=tape)
                    ops.stamp("precise_done")
                    self._search_ahead(precise)
                    ops.stamp("search_done")
            else:
                precise = self.precise_aux_features(batches, merged, rng_snap=snap)
        # (the two passes draw the same dropout offsets: same keep masks when the backbone is in train mode)
        tape = tape if side is not None else None
        if tape:
            # ONE backbone pass: the training graph is built from the precise pass's taped results (ops.dual_replay) -- its nodes
            # launch roundings, no contractions -- behind the precise backbone, beside its auxiliary projections and the searches
            cur = torch.cuda.current_stream()
            for _, ts in tape:  # (every node of the replay waits for its own taped node: ops._tape_take)
                for t in ts.values():
                    if torch.is_tensor(t):
                        t.record_stream(cur)
            with ops.dual_replay(tape), torch.set_grad_enabled(self.backprop):
                feats = self.features(batches, merged)
        else:
            with (ops.rng_replay(snap) if self._precise_on() else contextlib.nullcontext()), torch.set_grad_enabled(self.backprop):
                feats = self.features(batches, merged)
        # the primary projection heads need nothing of the precise pass: issued BEFORE the join with its stream, so that they run
        # beside its tail instead of behind it (profiles/r04_c4_replay_timeline.txt: 896-990 us, 95 us in which nothing else ran)
        f_prim = {}
        if side is not None and len(feats) == 1:
            f_prim = {t: self.tasks[t].forward_features(f) for t, f in feats.items()}
        ops.stamp("train_fwd_done")
        if side is not None:
            main.wait_stream(side)
            ops.stamp("precise_joined")
            for d in precise.values():
                for a in d.values():
                    a.record_stream(main)
            for st in self.graphone.ahead_streams():
                main.wait_stream(st)  # (the searches forked off ``side``; joined HERE, into the origin stream: GraphONE.search_ahead)
            for a in self.graphone.searched_tensors():
                a.record_stream(main)

        def head(t, feat):
            loss, logits, _, _ = self.task_loss(t, feat, batches[t], aux_in=precise.get(t), f_primary=f_prim.get(t))
            return loss, logits
        vectors, logits_out = self._run_heads(feats, head)
        return self._objective(vectors), vectors, logits_out
