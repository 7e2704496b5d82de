"""Guard-band tests of include/egopack_sample.h: egk_categorical_sample touches only what its task list names.

The form of tests/test_gpu_bounds_ema.py (helpers and ``Guards`` of tests/test_gpu_bounds.py are imported; nothing is registered
there): every device argument -- the logits of both heads, the strided outputs, the optional lo / hi / total -- sits in a
sentinel-filled window: NaN in the guard rows and in the padding columns of the logits (a read beyond a window makes the row
invalid and its samples -1), a poison value in the int64 outputs (the gaps between the strided samples must keep it).  The
samples are compared with the host model through the optional outputs (tests/lta_sampling_common.py: exact, tolerance, model),
everything outside the windows must keep the sentinel bits, and a second run on plain buffers must give the same bits.  The
ledger of this header is in tests/test_lta_sampling_cpu.py; the module imports without a GPU."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import lta_sampling_common as LS
from tests import test_gpu_bounds as B
from tests.test_gpu_bounds import BF16, F32, Guards, S, bf16, f32, gen, i64, ok, refused

CASES = []  # (id, function, variant dict, covers, second run on plain buffers?) -- this header's own list
POISON = -7  # what the int64 output buffers hold wherever no sample belongs
SEED = 99


def case(*covers, variants=None, plain=True):
    def deco(fn):
        for v in variants or [dict()]:
            v = dict(v)
            second = v.pop("plain", plain)
            vid = v.pop("id", None) or "-".join(f"{k}={B._fmt(x)}" for k, x in v.items())
            CASES.append((fn.__name__ + ("-" + vid if vid else ""), fn, v, covers, second))
        fn.covers = covers
        return fn
    return deco


def covered():
    """Every entry point some case declares it covers (the ledger in tests/test_lta_sampling_cpu.py)."""
    return sorted({name for _, _, _, cov, _ in CASES for name in cov})


@case("egk_categorical_sample",
      variants=[dict(rows=44, Cs=(115, 478), K=5, dt=f32, debug=True), dict(rows=44, Cs=(115, 478), K=5, dt=bf16, debug=False),
                dict(rows=5, Cs=(513, 7), K=9, dt=f32, debug=True), dict(rows=3, Cs=(1, 65, 1030), K=8, dt=bf16, debug=True),
                dict(rows=1, Cs=(64,), K=1, dt=f32, debug=True), dict(rows=0, Cs=(115, 478), K=5, dt=f32, debug=True, plain=False)])
def categorical_sample(lib, ops, G, rows, Cs, K, dt, debug):
    """Padded leading dimensions (one 16-byte vector of NaN behind every row), outputs with a row stride of K * ks + 3 and a sample
    stride ks = 2, row0 = 3, heads numbered from 2.  ``rows = 0``: nothing is launched and nothing is touched."""
    from egopack_amd import _lib
    from egopack_amd.ops import sampler_key
    g = gen(rows * 31 + sum(Cs) + K)
    ks, ordinal, row0, h0 = 2, 5, 3, 2
    x = [(torch.randint(-8192, 8193, (rows, c), generator=g).float() / 1024.0).to(dt) for c in Cs]
    L = [G.m(f"logits{i}", rows, c, dt, pad=B.pad_cols(dt), init=x[i]) for i, c in enumerate(Cs)]
    O = [G.m(f"out{i}", rows, K * ks, i64, pad=3, poison=POISON) for i in range(len(Cs))]
    D = [[G.v(f"{n}{i}", rows * K, f32) for n in ("lo", "hi", "total")] for i in range(len(Cs))] if debug else None
    tasks = (_lib.SampleTask * len(Cs))()
    for i, t in enumerate(tasks):
        t.logits, t.ld, t.C, t.head = L[i].ptr, L[i].ld, Cs[i], h0 + i
        t.out, t.out_row_stride, t.out_k_stride = O[i].ptr, O[i].ld, ks
        if debug:
            t.lo, t.hi, t.total = (d.ptr for d in D[i])
    call = lambda **kw: lib.egk_categorical_sample(S(), tasks, kw.get("count", len(Cs)), rows, kw.get("K", K), sampler_key(SEED),
                                                   kw.get("ordinal", ordinal), row0, B.edt(dt))
    ok(call(), "egk_categorical_sample")
    G.check()
    for i, c in enumerate(Cs):
        got = O[i].view.cpu()
        assert bool((got[:, 1::ks] == POISON).all()), "a gap between two strided samples was written"
        s = got[:, 0::ks].numpy()
        assert s.shape == (rows, K) and (rows == 0 or (s.min() >= 0 and s.max() < c))
        if debug and rows:
            lo, hi, total = (d.view.cpu().numpy().reshape(rows, K) for d in D[i])
            LS.check_launch(s, lo, hi, total, x[i].double().numpy(), LS.uniforms(SEED, ordinal, row0, rows, h0 + i, K))
        elif rows:  # without the optional outputs: the same samples as the launch with them (the plain run compares bits too)
            u = LS.uniforms(SEED, ordinal, row0, rows, h0 + i, K)
            far = np.abs(LS.cdf64(x[i].double().numpy())[0][:, None, :] - u.astype(np.float64)[:, :, None]).min(axis=2) > LS.tolerance(c)
            assert (s[far] == LS.sample64(x[i].double().numpy(), u)[far]).all()
    # refused on the host, nothing launched: the windows and the guards keep their bits
    before = [o.bits() for o in O]
    refused(call(K=1025), "K in 1 .. 1024")
    refused(call(ordinal=1 << 24), "batch ordinal")
    refused(call(count=9), "1 .. 8 tasks")
    tasks[0].head = 256
    refused(call(), "head index in [0, 256)")
    tasks[0].head = h0
    keep, tasks[0].out = tasks[0].out, None
    refused(call(), "null pointer")
    tasks[0].out = keep
    keep, tasks[0].logits = tasks[0].logits, None
    refused(call(), "null pointer")
    tasks[0].logits = keep
    tasks[0].ld = Cs[0] - 1
    refused(call(), "leading dimension")
    tasks[0].ld = L[0].ld
    G.check()
    assert all(torch.equal(a, o.bits()) for a, o in zip(before, O)), "a refused call wrote samples"
    out = {f"out{i}": o for i, o in enumerate(O)}
    if debug:
        out.update({f"{n}{i}": d for i in range(len(Cs)) for n, d in zip(("lo", "hi", "total"), D[i])})
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("name,fn,variant,covers,plain", CASES, ids=[c[0] for c in CASES])
def test_bounds_lta_sampling(name, fn, variant, covers, plain):
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from egopack_amd import _lib, ops
    lib = _lib.load()
    try:
        G = Guards()
        out = fn(lib, ops, G, **variant)
        G.check()
        if plain and out:
            got = {k: B._bits(v) for k, v in out.items()}
            H = Guards(plain=True)
            base = fn(lib, ops, H, **variant)
            torch.cuda.synchronize()
            for k, v in base.items():
                b = B._bits(v)
                assert got[k].shape == b.shape and torch.equal(got[k], b), f"{k}: the guarded call and the contiguous call differ in bits"
    finally:
        torch.cuda.synchronize()
