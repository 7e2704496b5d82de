"""The seeded sampler of the LTA futures without a GPU: what include/egopack_sample.h pins beyond the one ledger (tests/test_cabi.py),
the host-side refusals of its entry point, the counter layout and the uniform conversion of the host model
(tests/lta_sampling_common.py), the ``lta_sampling:`` config block, the batch ordinal of data.BatchLoader, and the chi-square test
of the host model alone against the bounds the GPU test uses."""
import ctypes

import numpy as np
import pytest
import torch

from tests import lta_sampling_common as LS
from tests import philox_ref as PR

# ---- 1. include/egopack_sample.h beyond the common ledger ------------------------------------------------------------------------
# (names, exports, bound types, the bounds ledger and the struct fields of this header: the one ledger, tests/test_cabi.py)


def test_sample_task_struct_size_and_limits():
    from egopack_amd import _lib
    text = _lib.HEADERS["sample"].read_text()
    assert ctypes.sizeof(_lib.SampleTask) == 72 and _lib.SampleTask.head.offset == 20 and _lib.SampleTask.out.offset == 24
    assert f"#define EGK_SAMPLE_MAX_TASKS {_lib.SAMPLE_MAX_TASKS}" in text and f"#define EGK_SAMPLE_MAX_K {_lib.SAMPLE_MAX_K}" in text


def test_categorical_sample_has_a_profile_id_of_its_own():
    from egopack_amd import _lib
    lib = _lib.load()
    name = ctypes.create_string_buffer(64)
    n, ms, fl, by = ctypes.c_int64(), ctypes.c_double(), ctypes.c_double(), ctypes.c_double()
    names = []
    for i in range(lib.egk_prof_count()):
        assert lib.egk_prof_get(i, name, 64, ctypes.byref(n), ctypes.byref(ms), ctypes.byref(fl), ctypes.byref(by)) == 0
        names.append(name.value.decode())
    assert {"categorical_sample", "task_scale", "dropout_fwd"} <= set(names) and len(set(names)) == len(names)


# ---- 2. host-side refusals (small fake non-null pointers: every check precedes the first dereference and the first launch) ---------
def _tasks(n=1, **kw):
    from egopack_amd import _lib
    arr = (_lib.SampleTask * n)()
    for h, t in enumerate(arr):
        t.logits, t.ld, t.C, t.head, t.out, t.out_row_stride, t.out_k_stride = 0x1000, 8, 7, h, 0x2000, 5, 1
        for k, v in kw.items():
            setattr(t, k, v)
    return arr


def test_categorical_sample_refuses_bad_arguments_before_any_launch():
    from egopack_amd import _lib
    lib = _lib.load()
    F32, BF16 = 0, 1

    def call(tasks, count=1, rows=4, K=5, seed=1, ordinal=0, row0=0, dtype=F32):
        return lib.egk_categorical_sample(None, tasks, count, rows, K, seed, ordinal, row0, dtype)

    def refused(rc, needle):
        assert rc == -1 and needle in _lib.last_error() and "egk_categorical_sample" in _lib.last_error(), (rc, _lib.last_error())

    refused(call(None), "null task list")
    for count in (0, -1, 9):
        refused(call(_tasks(8), count=count), "1 .. 8 tasks")
    refused(call(_tasks(), rows=-1), "rows >= 0")
    for K in (0, -3, 1025):
        refused(call(_tasks(), K=K), "K in 1 .. 1024")
    for b in (-1, 1 << 24):
        refused(call(_tasks(), ordinal=b), "batch ordinal")
    refused(call(_tasks(), row0=-1), "inside [0, 2^24)")
    refused(call(_tasks(), row0=(1 << 24) - 3, rows=4), "inside [0, 2^24)")
    refused(call(_tasks(), dtype=2), "unknown logits dtype")
    refused(call(_tasks(logits=None)), "null pointer")
    refused(call(_tasks(out=None)), "null pointer")
    refused(call(_tasks(C=0)), "class count")
    refused(call(_tasks(ld=6)), "leading dimension")
    for h in (-1, 256):
        refused(call(_tasks(head=h)), "head index in [0, 256)")
    refused(call(_tasks(out_k_stride=-1)), "negative output stride")
    refused(call(_tasks(lo=0x3000)), "given together")
    refused(call(_tasks(lo=0x3000, hi=0x4000)), "given together")
    refused(call(_tasks(logits=0x1002)), "misaligned pointer")
    refused(call(_tasks(out=0x2004)), "misaligned pointer")
    refused(call(_tasks(lo=0x3002, hi=0x4000, total=0x5000)), "misaligned pointer")
    bad_second = _tasks(2)
    bad_second[1].head = 300
    refused(call(bad_second, count=2), "task 1")
    # the limits themselves pass the checks; without rows nothing is launched (and no pointer is followed)
    assert call(_tasks(8), count=8, rows=0, K=1024, ordinal=(1 << 24) - 1, row0=1 << 24) == 0
    assert call(_tasks(logits=0x1002, head=255, lo=0x3000, hi=0x4000, total=0x5000), rows=0, dtype=BF16) == 0
    # ... and the refusals hold without rows too
    refused(call(_tasks(), rows=0, K=1025), "K in 1 .. 1024")
    refused(call(_tasks(head=256), rows=0), "head index")
    refused(call(_tasks(out=None), rows=0), "null pointer")


# ---- 3. the counter layout and the uniform conversion --------------------------------------------------------------------------------
def test_counters_of_distinct_samples_are_distinct_across_every_field_boundary():
    """(b, r, h, k >> 2) sit in disjoint bit fields: over a box that straddles each field's boundary no two samples share a
    (counter, word) pair, and a field at its limit does not reach into the next one."""
    bs, rs, hs = [0, 1, (1 << 24) - 1], [0, 1, (1 << 16) - 1, 1 << 16, (1 << 24) - 1], [0, 1, 255]
    ks = [0, 3, 4, 7, 8, 255, 256, 1020, 1023]
    seen = {}
    for b in bs:
        for r in rs:
            for h in hs:
                for k in ks:
                    draw = (LS.counter(b, r, h, k), k & 3)
                    assert draw not in seen, (seen[draw], (b, r, h, k))
                    seen[draw] = (b, r, h, k)
    assert len(seen) == len(bs) * len(rs) * len(hs) * len(ks)
    assert LS.counter((1 << 24) - 1, (1 << 24) - 1, 255, 1023) == (1 << 64) - 1  # the fields tile the 64 bits exactly
    assert LS.counter(0, 0, 0, 1023) == 255 and LS.counter(0, 0, 1, 0) == 1 << 8 and LS.counter(0, 1, 0, 0) == 1 << 16
    assert LS.counter(1, 0, 0, 0) == 1 << 40
    for bad in ((1 << 24, 0, 0, 0), (0, 1 << 24, 0, 0), (0, 0, 256, 0), (0, 0, 0, 1024), (-1, 0, 0, 0)):
        with pytest.raises(ValueError):
            LS.counter(*bad)
    # samples 0..3 share a counter and take its four words; sample 4 starts the next one
    w = LS.words(9, 2, 5, 1, 1, 9)[0]
    first = PR.philox_u64_scalar(LS.counter(2, 5, 1, 0), LS.key(9))
    second = PR.philox_u64_scalar(LS.counter(2, 5, 1, 4), LS.key(9))
    assert w.tolist() == [*first, *second, PR.philox_u64_scalar(LS.counter(2, 5, 1, 8), LS.key(9))[0]]
    # rows of a launch that starts at row0 are the rows row0 + r of a launch that starts at 0
    assert np.array_equal(LS.words(9, 2, 3, 4, 1, 9), LS.words(9, 2, 0, 7, 1, 9)[3:])


def test_the_sampler_key_is_not_the_dropout_key_and_the_package_agrees():
    from egopack_amd import ops
    assert ops.SAMPLER_KEY_SALT == LS.KEY_SALT == int.from_bytes(b"LTA_SAMP", "big")
    for seed in (0, 1, 0x5EEDE60, (1 << 64) - 1):
        assert ops.sampler_key(seed) == LS.key(seed) != seed and 0 <= LS.key(seed) < 1 << 64


def test_known_answers_of_the_uniform_conversion():
    u = LS.uniform_from_words(np.array([0, 255, 256, 0x80000000, 0xFFFFFFFF, 0xFFFFFF00], dtype=np.uint32))
    assert u.dtype == np.float32
    assert u.tolist() == [0.0, 0.0, 2.0 ** -24, 0.5, 1.0 - 2.0 ** -24, 1.0 - 2.0 ** -24]
    # Philox4x32-10 known answer (Random123 kat_vectors: counter 0, key 0) through the library's 64-bit wrapper
    assert PR.philox_u64_scalar(0, 0) == (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)
    w = PR.philox_u64_scalar(LS.counter(0, 0, 0, 0), LS.key(0))
    assert LS.uniforms(0, 0, 0, 1, 0, 4)[0].tolist() == [float(np.float32(x >> 8) * np.float32(2.0 ** -24)) for x in w]
    u = LS.uniforms(3, 1, 0, 64, 1, 9)
    assert u.shape == (64, 9) and float(u.min()) >= 0.0 and float(u.max()) < 1.0


def test_the_fp64_sampler_on_hand_made_rows():
    ninf = -np.inf
    x = np.array([[ninf, 0.0, ninf, 0.0, ninf], [0.0, 0.0, 0.0, 0.0, 0.0], [np.nan, 0, 0, 0, 0], [ninf] * 5, [np.inf, 0, 0, 0, 0]])
    u = np.array([[0.0, 0.49, 0.5, 0.99]] * 5)
    got = LS.sample64(x, u)
    assert got[0].tolist() == [1, 1, 3, 3]          # dead classes never come back, class 0 and class C - 1 included
    assert got[1].tolist() == [0, 2, 2, 4]          # cdf 0.2 0.4 0.6 0.8 1.0: the smallest c with cdf > u
    assert (got[2:] == -1).all()                    # a NaN, no finite maximum (all -inf, a +inf)


# ---- 4. the configuration ----------------------------------------------------------------------------------------------------------
def test_lta_sampling_config_accepts_and_rejects_as_documented():
    from egopack_amd import train as T
    from egopack_amd.ops import FutureSampler
    cfg = T.load_config([])
    assert dict(cfg.lta_sampling) == {"mode": "torch", "seed": 0}
    assert T.lta_sampling_config(cfg) == {"mode": "torch", "seed": 0} and T.build_lta_sampler(cfg) is None
    cfg = T.load_config(["lta_sampling.mode=philox", "lta_sampling.seed=7"])
    assert T.lta_sampling_config(cfg) == {"mode": "philox", "seed": 7}
    s = T.build_lta_sampler(cfg)
    assert isinstance(s, FutureSampler) and s.seed == 7 and not hasattr(s, "state_dict")  # (stateless: nothing to checkpoint)
    assert T.lta_sampling_config(T.load_config(["lta_sampling.mode=PHILOX"]))["mode"] == "philox"
    assert T.lta_sampling_config({}) == {"mode": "torch", "seed": 0}  # (a config without the block: the defaults)
    with pytest.raises(ValueError) as e:
        T.lta_sampling_config(T.load_config(["+lta_sampling.temperature=2"]))
    assert "temperature" in str(e.value) and "mode" in str(e.value) and "seed" in str(e.value)
    with pytest.raises(ValueError) as e:
        T.build_lta_sampler(T.load_config(["lta_sampling.mode=gumbel"]))
    assert "gumbel" in str(e.value) and "torch | philox" in str(e.value)
    for bad in ("-1", "1.5", "abc", str(1 << 64)):
        with pytest.raises(ValueError, match="lta_sampling.seed"):
            T.lta_sampling_config(T.load_config([f"lta_sampling.seed={bad}"]))


def test_generate_from_logits_without_a_sampler_is_the_torch_path_and_a_sampler_needs_an_ordinal():
    from egopack_amd.models.tasks import LTATask
    task = LTATask(16, 16, (7, 11))
    lv = torch.full((6, 7), -30.0)
    lv[:, 3] = 30.0
    ln = torch.full((6, 11), -30.0)
    ln[:, 9] = 30.0
    preds, logits = task.generate_from_logits((lv, ln))
    assert logits[0] is lv and preds[0].shape == (6, 5) and bool((preds[0] == 3).all()) and bool((preds[1] == 9).all())
    preds, _ = task.generate_from_logits((lv, ln), K=2, sampler=None)
    assert preds[1].shape == (6, 2)
    calls = []
    preds, _ = task.generate_from_logits((lv, ln), K=3, sampler=lambda *a: calls.append(a) or "drawn", ordinal=4)
    assert preds == "drawn" and calls[0][1:] == (3, 4, 0) and calls[0][0][0] is lv
    with pytest.raises(ValueError, match="ordinal"):
        task.generate_from_logits((lv, ln), sampler=lambda *a: None)


# ---- 5. the batch ordinal ------------------------------------------------------------------------------------------------------------
def test_the_loader_stamps_every_batch_with_its_index_in_the_single_process_order():
    from egopack_amd import data as D
    from egopack_amd import engine
    ds = D.SyntheticTaskDataset("lta", 22, 8, 3, 16, (7, 11), k=1, seed=5)
    whole = list(D.build_dataloader(ds, 4, False, 0, False, 1, shard="batches"))
    assert [b.ordinal for b in whole] == [0, 1, 2, 3, 4, 5] and all(type(b.ordinal) is int for b in whole)
    for world in (2, 3):
        for rank in range(world):
            part = list(D.build_dataloader(ds, 4, False, 0, False, 1, rank=rank, world_size=world, shard="batches"))
            assert [b.ordinal for b in part] == list(range(rank, 6, world))
            for b in part:  # the batch a rank gets under an ordinal IS the single pass's batch of that ordinal
                assert torch.equal(b.y, whole[b.ordinal].y) and torch.equal(b.pos, whole[b.ordinal].pos)
    assert [b.ordinal for b in D.build_dataloader(ds, 4, False, 0, True, 1)] == [0, 1, 2, 3, 4]  # drop_last
    # it survives the move to a device and the collation processes' packing, and carries no tensor
    moved = whole[3].to("cpu")
    assert moved.ordinal == 3 and moved is not whole[3]
    assert D.unpack_data(*D.pack_data(whole[2])).ordinal == 2
    packed = D.to_device_packed([whole[4]], "cpu", pack_on_cpu=True)[0]
    assert packed.ordinal == 4
    # it is a value, not a shape: the layout of a packed transfer and the signature of a captured step do not see it
    a, b = whole[1], whole[1].to("cpu")
    b.ordinal = 99
    assert engine.batch_signature({"lta": a}) == engine.batch_signature({"lta": b})
    assert not any("ordinal" in str(entry[0]) for entry in engine.batch_signature({"lta": a}))
    sig = lambda d: D.to_device_packed([d], "cpu", pack_on_cpu=True)[0]._blob.gsig
    assert sig(a) == sig(b) and sig(a) is not None and not any("ordinal" in str(entry[0]) for entry in sig(a))


def test_the_loader_stamps_on_the_worker_path_too():
    from egopack_amd import data as D
    ds = D.SyntheticTaskDataset("lta", 22, 8, 3, 16, (7, 11), k=1, seed=5)
    dl = D.build_dataloader(ds, 4, False, 0, False, 1, rank=1, world_size=2, shard="batches", workers=1)
    try:
        got = [(b.ordinal, b.y.clone()) for b in dl]
    finally:
        dl.close()
    whole = list(D.build_dataloader(ds, 4, False, 0, False, 1, shard="batches"))
    assert [o for o, _ in got] == [1, 3, 5]
    assert all(torch.equal(y, whole[o].y) for o, y in got)


# ---- 6. the host model alone stays inside the chi-square bound ---------------------------------------------------------------------
@pytest.mark.parametrize("C", [7, 115])
def test_the_host_model_passes_the_chi_square_test_the_device_samples_take(C):
    """4096 rows x K = 8 of one fixed distribution against the 1 - 1e-6 quantile of chi-square with C - 1 degrees of freedom
    (LS.CHI_BOUND: scipy.stats.chi2.ppf(1 - 1e-6, C - 1), written down as a constant).  Every expected count is at least 5."""
    p = LS.chi_probs(C)
    n = LS.CHI_ROWS * LS.CHI_K
    assert p.shape == (C,) and abs(p.sum() - 1.0) < 1e-12 and p.min() * n >= 5.0
    assert LS.CHI_BOUND == {7: 38.25833637714585, 115: 200.65036320850285}
    u = LS.uniforms(LS.CHI_SEED, LS.CHI_ORDINAL, 0, LS.CHI_ROWS, 0, LS.CHI_K)
    s = LS.sample64(np.repeat(LS.CHI_LOGITS[C][None], LS.CHI_ROWS, 0), u)
    assert s.shape == (LS.CHI_ROWS, LS.CHI_K) and s.min() >= 0 and s.max() < C
    stat = LS.chi_square(s, C)
    assert stat < LS.CHI_BOUND[C], (stat, LS.CHI_BOUND[C])
    # the statistic has teeth: the same samples against a shifted distribution are far outside
    assert LS.chi_square((s + 1) % C, C) > LS.CHI_BOUND[C]
