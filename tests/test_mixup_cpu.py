"""Sequence mixup without a GPU: the host draw (egopack_amd.data.mixup_fields) against its numpy restatement in tests/mixup_common.py
and against the properties it promises, the argument refusals of both launches of include/egopack_mixup.h (they come before any
launch: no device is touched), and the argument checks of the ops wrappers."""
import ctypes as C

import numpy as np
import pytest
import torch

from egopack_amd import data as D
from tests import mixup_common as MC


def batch_of(lengths, heads=2, seed=0):
    lengths = np.asarray(lengths, dtype=np.int64)
    ptr = np.concatenate([[0], np.cumsum(lengths)])
    y = torch.randint(-1, 50, (int(lengths.sum()), heads), generator=MC.gen(seed))
    return lengths, ptr, y


def fields(lengths, ptr, y, **kw):
    args = dict(seed=7, epoch=2, ordinal=5, task="ar", alpha=0.4)
    args.update(kw)
    return D.mixup_fields(ptr, y, **args)


@pytest.mark.parametrize("lengths", [[5] * 8, [5, 3, 5, 7, 3, 5, 3, 9], [4], [2, 2]])
@pytest.mark.parametrize("per_sequence", [True, False])
def test_the_draw_pairs_whole_sequences_of_equal_length(lengths, per_sequence):
    lengths, ptr, y = batch_of(lengths)
    src, lam, my = fields(lengths, ptr, y, per_sequence=per_sequence)
    N = int(lengths.sum())
    assert src.dtype == torch.int32 and lam.dtype == torch.float32 and my.dtype == y.dtype
    assert src.shape == (N,) and lam.shape == (N,) and my.shape == y.shape
    assert sorted(src.tolist()) == list(range(N)), "mix_src is a permutation of the rows"
    assert torch.equal(my, y[src.long()]), "mix_y == y[mix_src]"
    assert bool(((lam >= 0) & (lam <= 1)).all())
    seq_of = np.repeat(np.arange(len(lengths)), lengths)
    for s in range(len(lengths)):
        a, n = int(ptr[s]), int(lengths[s])
        partner = int(seq_of[int(src[a])])
        assert lengths[partner] == n, "a sequence is paired with a sequence of the same node count"
        assert src[a:a + n].tolist() == list(range(int(ptr[partner]), int(ptr[partner]) + n)), "node i maps to node i of the partner"
        assert len(set(lam[a:a + n].tolist())) == 1, "mix_lam is constant over a sequence"
        if (lengths == n).sum() == 1:
            assert partner == s, "a lone length maps to itself"
    if not per_sequence:
        assert len(set(lam.tolist())) == 1, "one lambda per batch"


def test_the_draw_is_the_restatement_and_depends_on_its_key_only():
    lengths, ptr, y = batch_of([5, 3, 5, 7, 3, 5, 3, 9])
    for kw in (dict(), dict(per_sequence=False), dict(prob=0.5, ordinal=11), dict(task="lta", alpha=2.0)):
        src, lam, my = fields(lengths, ptr, y, **kw)
        args = dict(seed=7, epoch=2, ordinal=5, task="ar", alpha=0.4)
        args.update(kw)
        rsrc, rlam, rmy = MC.draw(lengths, y.numpy(), **args)
        assert np.array_equal(src.numpy(), rsrc) and np.array_equal(lam.numpy().view(np.int32), rlam.view(np.int32))
        assert np.array_equal(my.numpy(), rmy)
    base = fields(lengths, ptr, y)
    again = fields(lengths, ptr, y)
    assert all(torch.equal(a, b) for a, b in zip(base, again)), "the same (seed, epoch, ordinal, task): the same fields"
    torch.manual_seed(123)  # (no global generator takes part)
    np.random.seed(5)
    assert all(torch.equal(a, b) for a, b in zip(base, fields(lengths, ptr, y)))
    for kw in (dict(ordinal=6), dict(epoch=3), dict(task="lta"), dict(seed=8)):
        other = fields(lengths, ptr, y, **kw)
        assert not (torch.equal(base[0], other[0]) and torch.equal(base[1], other[1])), f"{kw}: other fields"


def test_prob_zero_mixes_nothing_and_bad_arguments_are_refused():
    lengths, ptr, y = batch_of([5] * 6)
    src, lam, my = fields(lengths, ptr, y, prob=0.0)
    assert bool((lam == 1).all()) and torch.equal(my, y[src.long()])
    for ordinal in range(20):  # prob = 1: every batch is mixed (a Beta draw is 1 with probability 0)
        assert not bool((fields(lengths, ptr, y, ordinal=ordinal)[1] == 1).all())
    with pytest.raises(ValueError, match="alpha"):
        fields(lengths, ptr, y, alpha=0.0)
    with pytest.raises(ValueError, match="pnr"):
        fields(lengths, ptr, y, task="pnr")


# ---- the launches' refusals: before any launch, no device ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from egopack_amd import _lib
    return _lib.load()


def refused(rc, *needles):
    from egopack_amd import _lib
    assert rc == -1, (rc, _lib.last_error())
    for n in needles:
        assert n in _lib.last_error(), (n, _lib.last_error())


A, B_ = 0x10000, 0x90000  # aligned addresses nobody dereferences: every call below is refused on the host


@pytest.mark.parametrize("rows", [0, 5])
def test_mix_rows_refusals(lib, rows):
    cols = 8
    seg = lambda **kw: (kw.get("xin", A), kw.get("out", B_), kw.get("ld_in", cols), kw.get("ld_out", cols), kw.get("rows", rows),
                        kw.get("src", A + 0x1000), kw.get("lam", A + 0x2000))
    call = lambda segs, cols_=cols, dt=MC.F32: MC.call_mix_rows(lib, segs, cols_, dt, None)
    refused(call([seg()], cols_=0), "egk_mix_rows_multi", "cols must be >= 1")
    refused(call([seg(ld_in=7)]), "egk_mix_rows_multi", "ld_in >= cols")
    refused(call([seg(ld_out=7)]), "egk_mix_rows_multi", "ld_out >= cols")
    refused(call([seg()] * 5), "egk_mix_rows_multi", "1 .. 4 segments")
    refused(call([seg()], dt=3), "egk_mix_rows_multi", "unknown element dtype")
    refused(call([seg(lam=None)]), "egk_mix_rows_multi", "src is given without lam")
    refused(call([seg(src=None)]), "egk_mix_rows_multi", "lam is given without src")
    refused(call([seg(out=A)]), "egk_mix_rows_multi", "out of place")
    refused(call([seg(out=A + 4)]), "egk_mix_rows_multi", "out of place")
    refused(call([seg(xin=A + 2)]), "egk_mix_rows_multi", "not aligned to their element")
    refused(call([seg(src=A + 0x1002)]), "egk_mix_rows_multi", "not 4-byte aligned")
    refused(call([seg(), seg(xin=B_ + 0x100000, out=B_ + 16)]), "egk_mix_rows_multi", "x_out of segment")
    if rows == 0:
        assert call([seg()]) == 0, "rows == 0 passes the checks and launches nothing"


def test_ce_mix_refusals(lib):
    for rows in (0, 5):
        t = dict(logits=[(A, 20, 20, 24, 0)], y=A, y_b=A, y_stride=1, lam=A, loss=B_, dlogits=B_, ldd=24, rows=rows, gscale=1.0, scale=None)
        call = lambda ts, dt=MC.F32: MC.call_ce_mix(lib, ts, 0.1, dt, None)
        refused(call([dict(t, y_b=None)]), "egk_ce_mix_fused_multi", "y or y_b")
        refused(call([dict(t, lam=None)]), "egk_ce_mix_fused_multi", "lam")
        refused(call([dict(t, dlogits=None)]), "egk_ce_mix_fused_multi", "loss or dlogits")
        refused(call([dict(t, rows=-1)]), "egk_ce_mix_fused_multi", "rows must be >= 0")
        refused(call([dict(t, logits=[])]), "egk_ce_mix_fused_multi", "1 .. 4 heads")
        refused(call([dict(t, logits=[(A, 20, 0, 0, 0)])]), "egk_ce_mix_fused_multi", "C must be >= 1")
        refused(call([dict(t, logits=[(A, 20, 20, 19, 0)])]), "egk_ce_mix_fused_multi", "pad must be >= C")
        refused(call([dict(t, logits=[(None, 20, 20, 20, 0)])]), "egk_ce_mix_fused_multi", "logits of head 0")
        refused(call([dict(t, lam=A + 2)]), "egk_ce_mix_fused_multi", "not 4-byte aligned")
        refused(call([dict(t, scale=A + 1)]), "egk_ce_mix_fused_multi", "scale of task 0")
        refused(call([t] * 5), "egk_ce_mix_fused_multi", "1 .. 4 tasks")
        refused(call([t], dt=2), "egk_ce_mix_fused_multi", "unknown activation dtype")
    assert MC.call_ce_mix(lib, [dict(t, rows=0)], 0.1, MC.F32, None) == 0, "rows == 0 passes the checks and launches nothing"


def test_profile_ids_and_header_constants(lib):
    from egopack_amd import _lib
    text = _lib.ADDON_HEADERS["mixup"].read_text()
    for name, v in (("EGK_MIX_MAX_SEGMENTS", _lib.MIX_MAX_SEGMENTS), ("EGK_CE_MIX_MAX_TASKS", _lib.CE_MIX_MAX_TASKS),
                    ("EGK_CE_MIX_MAX_HEADS", _lib.CE_MIX_MAX_HEADS)):
        assert f"#define {name} {v}" in text


# ---- the ops wrappers' own checks (they raise before anything reaches a device) -------------------------------------------------------
def test_ops_argument_checks():
    from egopack_amd import ops
    z, y = torch.zeros(4, 3), torch.zeros(4, 1, dtype=torch.int64)
    lam = torch.ones(4)
    with pytest.raises(ValueError, match="mix does not combine with weight / offset / margin / gamma"):
        ops.cross_entropy((z,), y, weight=(torch.ones(3),), mix=(y, lam))
    with pytest.raises(ValueError, match="mix does not combine"):
        ops.cross_entropy((z,), y, gamma=2.0, mix=(y, lam))
    with pytest.raises(ValueError, match="mix y_b"):
        ops.cross_entropy((z,), y, mix=(y[:2], lam))
    with pytest.raises(ValueError, match="mix lam"):
        ops.cross_entropy((z,), y, mix=(y, lam.double()))
    with pytest.raises(ValueError, match="pair"):
        ops.cross_entropy((z,), y, mix=y)
    with pytest.raises(ValueError, match="mixes has 1 entries for 2 tasks"):
        ops.cross_entropy_multi([((z,), y), ((z,), y)], [1.0, 1.0], mixes=[(y, lam)])


# ---- the loader: the fields travel with the batch, the same on every path -------------------------------------------------------------
MIX = dict(task="ar", alpha=0.4, per_sequence=True, prob=1.0, seed=3)


def loader(ds, mixup=MIX, workers=0, rank=0, world=1, shard="samples", shuffle=False):
    dl = D.build_dataloader(ds, 4, shuffle, 0, True, seed=1, rank=rank, world_size=world, shard=shard, workers=workers)
    dl.mixup = None if mixup is None else dict(mixup)
    return dl


def fields_of(dl, epoch=0):
    dl.mix_epoch = epoch
    out = {}
    for b in dl:
        out[b.ordinal] = (b.mix_src.clone(), b.mix_lam.clone(), b.mix_y.clone(), b.ptr.clone(), b.y.clone())
    return out


def same_fields(a, b):
    assert sorted(a) == sorted(b)
    for k in a:
        assert all(torch.equal(x, y) for x, y in zip(a[k][:3], b[k][:3])), k


def test_the_fields_are_the_same_through_every_loader_path():
    ds = D.SyntheticTaskDataset("ar", 16, 5, 3, 8, (7, 11), k=1, seed=3)
    plain = fields_of(loader(ds))
    assert len(plain) == 4
    for o, (src, lam, my, ptr, y) in plain.items():  # ... and they are the restatement's, from the batch's ptr and y alone
        rsrc, rlam, rmy = MC.draw(np.diff(ptr.numpy()), y.numpy(), 3, 0, o, "ar", 0.4)
        assert np.array_equal(src.numpy(), rsrc) and np.array_equal(lam.numpy(), rlam) and np.array_equal(my.numpy(), rmy)
    pool = loader(ds, workers=2)
    try:
        same_fields(fields_of(pool), plain)
    finally:
        pool.close()
    halves = {}
    for rank in (0, 1):  # a 2-way batch shard keeps the single-process ordinals: together the ranks hold the same fields
        halves.update(fields_of(loader(ds, rank=rank, world=2, shard="batches")))
    same_fields(halves, plain)
    other = fields_of(loader(ds), epoch=1)
    assert not all(torch.equal(other[k][1], plain[k][1]) for k in plain), "another epoch: other fields"
    again = loader(ds)
    first = fields_of(again, epoch=0)
    second = {b.ordinal: b.mix_lam.clone() for b in again}  # (a second pass without setting the epoch: the epoch moved on by itself)
    assert all(torch.equal(second[k], other[k][1]) for k in other) and again.mix_lam_mean() is not None
    same_fields(first, plain)


def test_the_native_builder_carries_the_same_fields():
    kw = dict(task="ar", length=16, T=5, num_segments=3, features_size=8, num_class_labels=(7, 11), k=1, seed=3, n_videos=2, frames=64)
    native, numpy_ = D.SyntheticResidentDataset(**kw), D.SyntheticResidentDataset(**kw)
    numpy_.native_batches = False
    a, b = fields_of(loader(native)), fields_of(loader(numpy_))
    same_fields(a, b)
    for o, (src, lam, my, ptr, y) in a.items():
        rsrc, rlam, rmy = MC.draw(np.diff(ptr.numpy()), y.numpy(), 3, 0, o, "ar", 0.4)
        assert np.array_equal(src.numpy(), rsrc) and np.array_equal(lam.numpy(), rlam) and np.array_equal(my.numpy(), rmy)


def test_alpha_zero_and_validation_loaders_carry_no_field():
    from egopack_amd import train as T
    ds = {"ar": D.SyntheticTaskDataset("ar", 8, 5, 3, 8, (7, 11), k=1, seed=3), "pnr": D.SyntheticTaskDataset("pnr", 8, 5, 3, 8, (7, 11), k=1, seed=3)}

    class Cfg(dict):
        batch_size, num_workers, seed = 4, 0, 1
    has = lambda loaders, t: [hasattr(b, "mix_src") or hasattr(b, "mix_lam") or hasattr(b, "mix_y") for b in loaders[t]]
    off = T.build_loaders(Cfg(), ds, True, 0, 1)
    assert not any(has(off, "ar")) and off["ar"].mixup is None and off["ar"].mix_lam_mean() is None
    on = T.build_loaders(Cfg(mixup={"alpha": 0.4}), ds, True, 0, 1)
    assert all(has(on, "ar")) and not any(has(on, "pnr")), "a mixed task's training batches carry the fields, no other task's"
    assert on["ar"].mixup["seed"] == 1, "seed null: the run's seed"
    val = T.build_loaders(Cfg(mixup={"alpha": 0.4}), ds, False, 0, 1)
    assert not any(has(val, "ar")), "validation batches carry none of the fields"
    only = T.build_loaders(Cfg(mixup={"alpha": 0.4, "tasks": []}), ds, True, 0, 1)
    assert not any(has(only, "ar"))


@pytest.mark.parametrize("over, keys", [
    ({"mixup": {"alpha": 0.4}, "class_balance": {"mode": "weight"}}, ("mixup.tasks", "class_balance.mode")),
    ({"mixup": {"alpha": 0.4, "tasks": ["lta"]}, "class_balance": {"mode": "logit_adjust", "tasks": ["lta"]}}, ("mixup.tasks", "class_balance.mode")),
    ({"mixup": {"alpha": 0.4}, "ce_shape": {"margin": "ldam"}}, ("mixup.tasks", "ce_shape.margin")),
    ({"mixup": {"alpha": 0.4}, "ce_shape": {"gamma": 2.0}}, ("mixup.tasks", "ce_shape.gamma")),
    ({"mixup": {"alpha": 0.4}, "enable_graphone": True}, ("mixup.alpha", "enable_graphone")),
    ({"mixup": {"alpha": -0.1}}, ("mixup.alpha",)),
    ({"mixup": {"prob": 1.5}}, ("mixup.prob",)),
    ({"mixup": {"prob": -0.1}}, ("mixup.prob",)),
    ({"mixup": {"tasks": ["ar", "pnr"]}}, ("mixup.tasks", "pnr")),
    ({"mixup": {"beta": 1.0}}, ("mixup", "beta")),
])
def test_every_refusal_at_build_time_names_its_keys(over, keys):
    from egopack_amd import train as T
    with pytest.raises(ValueError) as e:
        T.check_mixup(dict(over), enable_graphone=bool(over.get("enable_graphone", False)))
    assert all(k in str(e.value) for k in keys), str(e.value)


def test_combinations_that_are_not_refused():
    from egopack_amd import train as T
    assert T.check_mixup({})["alpha"] == 0.0
    T.check_mixup({"class_balance": {"mode": "weight"}, "enable_graphone": True}, enable_graphone=True)  # (alpha 0: off, nothing to refuse)
    T.check_mixup({"mixup": {"alpha": 0.4, "tasks": ["ar"]}, "class_balance": {"mode": "weight", "tasks": ["lta"]}})  # (other tasks)
    T.check_mixup({"mixup": {"alpha": 0.4}, "pnr_balance": {"mode": "focal"}, "task_weighting": {"mode": "uncertainty"}})
    with pytest.raises(ValueError, match="main_egopack.py"):
        T.check_mixup({"mixup": {"alpha": 0.4}}, enable_graphone=True, entry="main_egopack.py")
