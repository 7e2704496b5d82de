"""Guard-band tests: a launch touches only what its arguments name.

Every case embeds EVERY device argument of an entry point -- inputs, outputs, workspaces -- in a sentinel-filled buffer
(tests/guarded.py): guard rows in front of and behind the logical rows, pad columns where the entry point takes a leading
dimension, NaN (or a poison index that names a NaN row) everywhere outside the logical window.  A case then

  1. calls the entry point through the ctypes binding (``_lib.load()``) with the window's pointer and leading dimension;
  2. compares the output window with a plain high-precision reference of the same operation, at the tolerance of the
     existing parity test of that entry point (named next to each comparison) -- an element the kernel forgets keeps its NaN
     sentinel and fails here, a read beyond an input's window carries a NaN into the result and fails here;
  3. ``Guards.check()``: everything outside every window still holds the sentinel BITS (inputs must not be written either);
  4. the driver runs the case a second time on standalone contiguous buffers (no guard, no pad) and asserts that the outputs
     are bit-identical: strides change addresses, not arithmetic.

Workspaces are handed over at EXACTLY the size the library's query function (or the header's formula) gives; entry points
that take a size refuse one byte less (tests/test_cabi.py has the refusals that need no GPU).

Entry points that take a workspace but NO size argument (they cannot check; the exact-size guarded workspace is their test):
egk_colsum, egk_rowln_bwd, egk_rowln_group_bwd, egk_ln_bwd_reduce(_multi), egk_graphln_fwd / _bwd / _bwd_stats / _bwd_finish /
_bwd_apply / _stats, egk_csr_gather(_banded), egk_rowdot_bce, egk_rowdot_reduce, egk_rowdot_ce2(_multi), egk_gemm_reduce_slabs.

The module imports without a GPU (tests/test_cabi.py reads ``covered()`` for the ledger of entry points).
"""
import ctypes as C
import math

import pytest
import torch
import torch.nn.functional as F

from tests.guarded import GUARD_ELEMS, GUARD_ROWS, Guarded1D, Guarded2D, pad_cols

DEV = "cuda"
F32, BF16 = 0, 1                      # EGK_F32 / EGK_BF16
f32, bf16, i64, i32, u8, f64 = torch.float32, torch.bfloat16, torch.int64, torch.int32, torch.uint8, torch.float64
OUT16 = dict(rtol=8e-3, atol=8e-3)    # tests/test_gpu_kernels.py: the final rounding of a bf16 output


def gen(seed):
    return torch.Generator().manual_seed(seed)


def r16(t):
    return t.to(bf16).float()


def edt(dtype):
    return BF16 if dtype == bf16 else F32


def S():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def P(x, byte_offset=0):
    """Device pointer of a guarded buffer's window / a tensor / None."""
    if x is None:
        return None
    return C.c_void_p((x.ptr if isinstance(x, Guarded2D) else x.data_ptr()) + byte_offset)


def ptr_array(items):
    return (C.c_void_p * len(items))(*[None if t is None else (t.ptr if isinstance(t, Guarded2D) else t.data_ptr()) for t in items])


def ok(rc, what):
    from egopack_amd import _lib
    assert rc == 0, f"{what} returned {rc}: {_lib.last_error()}"


def refused(rc, needle):
    from egopack_amd import _lib
    assert rc != 0 and needle in _lib.last_error(), (rc, _lib.last_error())


def close(got, ref, what, **tol):
    torch.testing.assert_close(got.detach().float().cpu() if got.dtype != f64 else got.detach().cpu(), ref, msg=lambda s: f"{what}: {s}",
                               check_dtype=False, **tol)


def same(got, ref, what):
    got, ref = got.detach().cpu(), ref.detach().cpu()
    if got.shape == ref.shape and torch.equal(got, ref):
        return
    assert got.shape == ref.shape, f"{what}: shape {tuple(got.shape)}, expected {tuple(ref.shape)}"
    bad = (got != ref).nonzero()
    raise AssertionError(f"{what}: {bad.shape[0]} of {got.numel()} elements differ, first at {bad[:4].tolist()}: got "
                         f"{[got[tuple(i)].item() for i in bad[:4]]}, expected {[ref[tuple(i)].item() for i in bad[:4]]}")


class Guards:
    """The guarded buffers of one case.  ``plain``: standalone contiguous buffers instead (no guard, no pad, no offset) --
    the second run of a case, whose outputs must have the same bits."""

    def __init__(self, device=DEV, plain=False):
        self.device, self.plain, self.items = device, plain, []

    def m(self, name, rows, cols, dtype=f32, pad=0, init=None, guard_rows=GUARD_ROWS, offset_elems=0, poison=None):
        g = Guarded2D(rows, cols, dtype, self.device, ld=cols + (0 if self.plain else pad), guard_rows=0 if self.plain else guard_rows,
                      offset_elems=0 if self.plain else offset_elems, init=init, poison=poison)
        self.items.append((name, g))
        return g

    def v(self, name, n, dtype=f32, init=None, guard=GUARD_ELEMS, offset_elems=0, poison=None):
        g = Guarded1D(n, dtype, self.device, guard=0 if self.plain else guard, offset_elems=0 if self.plain else offset_elems,
                      init=init, poison=poison)
        self.items.append((name, g))
        return g

    def check(self):
        torch.cuda.synchronize()
        for name, g in self.items:
            g.assert_untouched(name)


CASES = []  # (id, function, variant dict, covers, second run on plain buffers?)


def _fmt(x):
    if isinstance(x, (tuple, list)):
        return "x".join(_fmt(e) for e in x) or "none"
    return str(x).replace("torch.", "")


def case(*covers, variants=None, plain=True):
    """Register one test per variant; a variant's ``plain=False`` leaves out the second run on standalone buffers."""
    def deco(fn):
        for v in variants or [dict()]:
            v = dict(v)
            second = v.pop("plain", plain)
            vid = v.pop("id", None) or "-".join(f"{k}={_fmt(x)}" for k, x in v.items())
            CASES.append((fn.__name__ + ("-" + vid if vid else ""), fn, v, covers, second))
        fn.covers = covers
        return fn
    return deco


def covered():
    """Every entry point some case declares it covers (the ledger in tests/test_cabi.py)."""
    return sorted({name for _, _, _, cov, _ in CASES for name in cov})


# =====================================================================================================================
# 5. losses
# =====================================================================================================================
def _ce_ref(logits, y, sm, gloss=None):
    z = logits.double().clone().requires_grad_(True)
    loss = F.cross_entropy(z, y, ignore_index=-1, reduction="none", label_smoothing=sm)
    if gloss is None:
        return loss.detach()
    (loss * gloss.double()).sum().backward()
    return loss.detach(), z.grad


@case("egk_ce_fwd", "egk_ce_bwd", variants=[
    dict(rows=64, Cn=128, pad=0, ys=1, sm=0.0, dt=f32, acc=0),
    dict(rows=77, Cn=115, pad=5, ys=2, sm=0.1, dt=bf16, acc=1),     # bf16 dlogits with ld = 125: rows not 16-byte aligned (the kernels are scalar)
    dict(rows=37, Cn=2, pad=4, ys=1, sm=0.1, dt=f32, acc=0),
    dict(rows=0, Cn=9, pad=4, ys=1, sm=0.0, dt=f32, acc=0)])
def ce(lib, ops, G, rows, Cn, pad, ys, sm, dt, acc):
    g = gen(rows * 7 + Cn)
    logits = torch.randn(rows, Cn, generator=g) * 3
    y = torch.randint(0, Cn, (rows, ys), generator=g)
    y[::3, 0] = -1                                                   # ignored rows
    gloss, loss0 = torch.randn(rows, generator=g), torch.randn(rows, generator=g)
    L = G.m("logits", rows, Cn, f32, pad=pad, init=logits)
    Y = G.v("y", rows * ys, i64, init=y, poison=(Cn - 1))            # (a label read beyond the list is a valid class)
    loss = G.v("loss", rows, f32, init=loss0 if acc else None)
    lse = G.v("lse", rows, f32)
    GL = G.v("gloss", rows, f32, init=gloss)
    D = G.m("dlogits", rows, Cn, dt, pad=2 * pad)
    ok(lib.egk_ce_fwd(S(), P(L), L.ld, P(Y), ys, P(loss), P(lse), rows, Cn, sm, acc), "egk_ce_fwd")
    ok(lib.egk_ce_bwd(S(), P(L), L.ld, P(Y), ys, P(lse), P(GL), P(D), D.ld, rows, Cn, sm, edt(dt)), "egk_ce_bwd")
    G.check()
    ref, dref = _ce_ref(logits, y[:, 0], sm, gloss)
    # tests/test_gpu_kernels.py::test_cross_entropy_heads_ignore_index
    close(loss.view, (ref + (loss0.double() if acc else 0)).float(), "loss", rtol=1e-5, atol=1e-5)
    close(lse.view, torch.logsumexp(logits.double(), 1).float(), "lse", rtol=1e-5, atol=1e-5)
    close(D.view, dref.float(), "dlogits", **(OUT16 if dt == bf16 else dict(rtol=1e-4, atol=1e-6)))
    return dict(loss=loss, lse=lse, dlogits=D)


def _ce_fused_task(G, tag, g, rows, Cs, pads, lpad, dpad, dt, sm, gscale, every_third=False):
    """One task of egk_ce_fused(_multi): n heads, their column blocks [dcol, dcol + pad) inside ONE gradient matrix, with
    sentinel columns in front of, between and behind the blocks."""
    n = len(Cs)
    logits = [torch.randn(rows, c, generator=g) * 3 for c in Cs]
    y = torch.stack([torch.randint(0, c, (rows,), generator=g) for c in Cs] + [torch.zeros(rows, dtype=i64)], 1)  # y_stride = n + 1
    y[1::4, 0] = -1
    y[2::5, n - 1] = -1
    if every_third:                                                   # every third label of every head, rows with one head ignored among them
        for h in range(n):
            y[h::3, h] = -1
    dcol, col = [], 3
    for p in pads:
        dcol.append(col)
        col += p + 2                                                  # two sentinel columns between the blocks
    width = col
    L = [G.m(f"{tag}logits{h}", rows, Cs[h], f32, pad=lpad, init=logits[h]) for h in range(n)]
    Y = G.v(tag + "y", rows * (n + 1), i64, init=y, poison=0)
    loss = G.v(tag + "loss", rows, f32)
    D = G.m(tag + "dlogits", rows, width, dt, pad=dpad)
    return dict(n=n, rows=rows, Cs=Cs, pads=pads, dcol=dcol, L=L, Y=Y, loss=loss, D=D, logits=logits, y=y, sm=sm, gscale=gscale, dt=dt)


def _ce_fused_check(t, tag):
    rows, n = t["rows"], t["n"]
    total = torch.zeros(rows, dtype=f64)
    inside = torch.zeros(t["D"].cols, dtype=torch.bool)
    for h in range(n):
        ref, dref = _ce_ref(t["logits"][h], t["y"][:, h], t["sm"], torch.full((rows,), t["gscale"]))
        total += ref
        c0, Cn, pd = t["dcol"][h], t["Cs"][h], t["pads"][h]
        inside[c0:c0 + pd] = True
        close(t["D"].view[:, c0:c0 + Cn], dref.float(), f"{tag}dlogits head {h}",
              **(OUT16 if t["dt"] == bf16 else dict(rtol=1e-4, atol=1e-6)))  # test_cross_entropy_heads_ignore_index
        assert not t["D"].view[:, c0 + Cn:c0 + pd].float().ne(0).any(), f"{tag}dlogits head {h}: pad columns [C, pad) are not zero"
    close(t["loss"].view, total.float(), tag + "loss", rtol=1e-5, atol=1e-5)
    keep = t["D"].is_sentinel()[:, ~inside]
    assert bool(keep.all()), f"{tag}dlogits: {int((~keep).sum())} element(s) outside every head's column block were written"


@case("egk_ce_fused", variants=[dict(rows=77, Cs=(115, 478), pads=(128, 512), lpad=0, dpad=0, dt=bf16, sm=0.1),
                                dict(rows=64, Cs=(7, 11, 2), pads=(7, 16, 8), lpad=3, dpad=5, dt=f32, sm=0.0),
                                dict(rows=0, Cs=(7,), pads=(8,), lpad=0, dpad=0, dt=f32, sm=0.0)])
def ce_fused(lib, ops, G, rows, Cs, pads, lpad, dpad, dt, sm):
    t = _ce_fused_task(G, "", gen(rows + sum(Cs)), rows, Cs, pads, lpad, dpad, dt, sm, 0.37)
    n = t["n"]
    ok(lib.egk_ce_fused(S(), ptr_array(t["L"]), (C.c_int64 * n)(*[l.ld for l in t["L"]]), (C.c_int32 * n)(*Cs), (C.c_int32 * n)(*pads),
                        (C.c_int64 * n)(*t["dcol"]), n, P(t["Y"]), n + 1, P(t["loss"]), P(t["D"]), t["D"].ld, rows, sm, 0.37, edt(dt)),
       "egk_ce_fused")
    G.check()
    _ce_fused_check(t, "")
    return dict(loss=t["loss"], dlogits=t["D"])


def _ce_task_array(tasks):
    from egopack_amd import _lib
    arr = (_lib.CETask * len(tasks))()
    for a, t in zip(arr, tasks):
        for h in range(t["n"]):
            a.logits[h], a.ld[h], a.C[h], a.pad[h], a.dcol[h] = t["L"][h].ptr, t["L"][h].ld, t["Cs"][h], t["pads"][h], t["dcol"][h]
        a.n_heads, a.y, a.y_stride, a.loss, a.dlogits, a.ldd = t["n"], t["Y"].ptr, t["n"] + 1, t["loss"].ptr, t["D"].ptr, t["D"].ld
        a.rows, a.gscale = t["rows"], t["gscale"]
    return arr


@case("egk_ce_fused_multi", variants=[dict(dt=bf16, lpad=0, dpad=0), dict(dt=f32, lpad=3, dpad=5)])
def ce_fused_multi(lib, ops, G, dt, lpad, dpad):
    from egopack_amd import _lib
    g = gen(91)
    specs = [(77, (115, 478), (128, 512), 0.5), (33, (20,), (64,), 0.25), (0, (5,), (8,), 1.0)]  # (the third task has no rows)
    tasks = [_ce_fused_task(G, f"task{i}.", g, r, cs, pd, lpad, dpad, dt, 0.1, gs) for i, (r, cs, pd, gs) in enumerate(specs)]
    ok(lib.egk_ce_fused_multi(S(), _ce_task_array(tasks), len(tasks), 0.1, edt(dt)), "egk_ce_fused_multi")
    G.check()
    out = {}
    for i, t in enumerate(tasks):
        _ce_fused_check(t, f"task{i}.")
        out[f"loss{i}"], out[f"dlogits{i}"] = t["loss"], t["D"]
    return out


@case("egk_ce_fused", "egk_ce_fused_multi", variants=[dict(rows=r, dt=dt, sm=sm) for r in (32, 77) for dt in (f32, bf16) for sm in (0.0, 0.1)])
def ce_fused_forms(lib, ops, G, rows, dt, sm):
    """include/egopack_hip.h: per task, egk_ce_fused_multi gives the bits of egk_ce_fused.  One task through egk_ce_fused, through
    egk_ce_fused_multi(count = 1), and as entry 0 and as entry 1 of a two-task launch beside a shorter task: loss and the whole
    gradient window (pad columns and the untouched sentinel columns included) have the same bits.  rows = 32: eight workgroups,
    the XCD-contiguous row walk; rows = 77: twenty workgroups, the round-robin walk (csrc/common.h: row_walk)."""
    Cs, pads, gs = (115, 478), (128, 512), 0.37
    A = [_ce_fused_task(G, f"form{i}.", gen(rows + 5), rows, Cs, pads, 0, 0, dt, sm, gs, every_third=True) for i in range(4)]
    B = [_ce_fused_task(G, f"other{i}.", gen(17), 21, (20,), (64,), 0, 0, dt, sm, 0.25) for i in range(2)]
    t, n = A[0], len(Cs)
    ok(lib.egk_ce_fused(S(), ptr_array(t["L"]), (C.c_int64 * n)(*[l.ld for l in t["L"]]), (C.c_int32 * n)(*Cs), (C.c_int32 * n)(*pads),
                        (C.c_int64 * n)(*t["dcol"]), n, P(t["Y"]), n + 1, P(t["loss"]), P(t["D"]), t["D"].ld, rows, sm, gs, edt(dt)),
       "egk_ce_fused")
    ok(lib.egk_ce_fused_multi(S(), _ce_task_array([A[1]]), 1, sm, edt(dt)), "egk_ce_fused_multi (one task)")
    ok(lib.egk_ce_fused_multi(S(), _ce_task_array([A[2], B[0]]), 2, sm, edt(dt)), "egk_ce_fused_multi (entry 0)")
    ok(lib.egk_ce_fused_multi(S(), _ce_task_array([B[1], A[3]]), 2, sm, edt(dt)), "egk_ce_fused_multi (entry 1)")
    G.check()
    _ce_fused_check(t, "egk_ce_fused: ")
    for other, what in zip(A[1:], ("count = 1", "entry 0 of 2", "entry 1 of 2")):
        same(other["loss"].bits(), t["loss"].bits(), f"loss, egk_ce_fused_multi {what} against egk_ce_fused")
        same(other["D"].bits(), t["D"].bits(), f"dlogits, egk_ce_fused_multi {what} against egk_ce_fused")
    same(B[1]["loss"].bits(), B[0]["loss"].bits(), "loss of the shorter task, entry 0 against entry 1")
    same(B[1]["D"].bits(), B[0]["D"].bits(), "dlogits of the shorter task, entry 0 against entry 1")
    return dict(loss=t["loss"], dlogits=t["D"])


@case("egk_bce_fwd", "egk_bce_bwd", variants=[dict(n=333, dt=f32), dict(n=256, dt=bf16), dict(n=0, dt=f32)])
def bce(lib, ops, G, n, dt):
    g = gen(53 + n)
    x, y, gl = torch.randn(n, generator=g) * 4, torch.randint(0, 2, (n,), generator=g), torch.randn(n, generator=g)
    X, Y, GL = G.v("logits", n, f32, init=x), G.v("y", n, i64, init=y, poison=1), G.v("gloss", n, f32, init=gl)
    loss, D = G.v("loss", n, f32), G.v("dlogits", n, dt)
    ok(lib.egk_bce_fwd(S(), P(X), P(Y), P(loss), n), "egk_bce_fwd")
    ok(lib.egk_bce_bwd(S(), P(X), P(Y), P(GL), P(D), n, edt(dt)), "egk_bce_bwd")
    G.check()
    z = x.double().requires_grad_(True)
    ref = F.binary_cross_entropy_with_logits(z, y.double(), reduction="none")
    (ref * gl.double()).sum().backward()
    close(loss.view, ref.detach().float(), "loss", rtol=1e-5, atol=1e-6)  # tests/test_gpu_kernels.py::test_bce_with_logits
    close(D.view, z.grad.float(), "dlogits", **(OUT16 if dt == bf16 else dict(rtol=1e-5, atol=1e-6)))
    return dict(loss=loss, dlogits=D)


@case("egk_onehot_sigmoid_loss_fwd", "egk_onehot_sigmoid_loss_bwd",
      variants=[dict(rows=37, Cn=2, kind=0, dt=f32), dict(rows=37, Cn=3, kind=1, dt=bf16), dict(rows=64, Cn=4, kind=1, dt=f32),
                dict(rows=0, Cn=2, kind=0, dt=f32)])
def onehot_sigmoid(lib, ops, G, rows, Cn, kind, dt):
    g = gen(rows + Cn + kind)
    alpha, gamma = 0.5, 2.0
    x, y = torch.randn(rows, Cn, generator=g) * 3, torch.randint(0, Cn, (rows,), generator=g)
    gl = torch.randn(rows, Cn, generator=g)
    X, Y, GL = G.v("logits", rows * Cn, f32, init=x), G.v("y", rows, i64, init=y, poison=0), G.v("gloss", rows * Cn, f32, init=gl)
    loss, D = G.v("loss", rows * Cn, f32), G.v("dlogits", rows * Cn, dt)
    ok(lib.egk_onehot_sigmoid_loss_fwd(S(), P(X), P(Y), P(loss), rows, Cn, kind, alpha, gamma), "egk_onehot_sigmoid_loss_fwd")
    ok(lib.egk_onehot_sigmoid_loss_bwd(S(), P(X), P(Y), P(GL), P(D), rows, Cn, kind, alpha, gamma, edt(dt)), "egk_onehot_sigmoid_loss_bwd")
    G.check()
    z, t = x.double().requires_grad_(True), F.one_hot(y, Cn).double()
    ce_ = F.binary_cross_entropy_with_logits(z, t, reduction="none")
    if kind == 1:  # torchvision.ops.sigmoid_focal_loss, written out
        p = torch.sigmoid(z)
        pt = p * t + (1 - p) * (1 - t)
        ref = ce_ * (1 - pt) ** gamma * (alpha * t + (1 - alpha) * (1 - t))
    else:
        ref = ce_
    (ref * gl.double()).sum().backward()
    # tests/test_gpu_configs.py compares these losses at rtol 1e-5 / atol 1e-6 (test_bce_with_logits' tolerance)
    close(loss.view.view(rows, Cn), ref.detach().float(), "loss", rtol=1e-5, atol=1e-6)
    close(D.view.view(rows, Cn), z.grad.float(), "dlogits", **(OUT16 if dt == bf16 else dict(rtol=1e-5, atol=1e-6)))
    return dict(loss=loss, dlogits=D)


@case("egk_weighted_sums", "egk_weighted_sums_acc", "egk_fill_scaled", "egk_fill_scaled_multi", "egk_sum_scale",
      variants=[dict(ns=(100, 37, 0, 2051)), dict(ns=(1,))])
def objective_sums(lib, ops, G, ns):
    g = gen(54 + len(ns))
    xs = [torch.randn(n, generator=g) for n in ns]
    coefs = [0.5 / max(n, 1) for n in ns]
    k = len(ns)
    X = [G.v(f"x{i}", n, f32, init=x) for i, (n, x) in enumerate(zip(ns, xs))]
    out, out2, acc = G.v("out", 1, f32), G.v("out_acc", 1, f32), G.v("acc", k, f64, init=torch.arange(k, dtype=f64))
    nsa, ca = (C.c_int64 * k)(*ns), (C.c_float * k)(*coefs)
    ok(lib.egk_weighted_sums(S(), ptr_array(X), nsa, ca, k, P(out)), "egk_weighted_sums")
    ok(lib.egk_weighted_sums_acc(S(), ptr_array(X), nsa, ca, k, P(out2), P(acc)), "egk_weighted_sums_acc")
    ref = sum(c * x.double().sum() for c, x in zip(coefs, xs))
    scalar = G.v("scalar", 1, f32, init=torch.tensor([1.7]))
    outs = [G.v(f"dx{i}", n, f32) for i, n in enumerate(ns)]
    ok(lib.egk_fill_scaled_multi(S(), P(scalar), ca, ptr_array(outs), nsa, k), "egk_fill_scaled_multi")
    one = G.v("fill", ns[-1], f32)
    ok(lib.egk_fill_scaled(S(), P(scalar), 0.25, P(one), ns[-1]), "egk_fill_scaled")
    ss, ss0 = G.v("sum_scale", 1, f32, init=torch.tensor([3.0])), G.v("sum_scale0", 1, f32)
    ok(lib.egk_sum_scale(S(), P(X[-1]), P(ss), ns[-1], 0.5, 1), "egk_sum_scale")
    ok(lib.egk_sum_scale(S(), P(X[0]), P(ss0), 0, 0.5, 0), "egk_sum_scale")  # n == 0: stores scale * 0
    G.check()
    # tests/test_gpu_kernels.py::test_weighted_mean_sum_and_sum_tensors
    close(out.view, torch.tensor([float(ref)]), "out", rtol=1e-5, atol=1e-6)
    same(out2.view, out.view, "out (acc form)")
    close(acc.view, torch.tensor([i + float(x.double().sum()) for i, x in enumerate(xs)], dtype=f64), "acc", rtol=1e-5, atol=1e-6)
    for o, c in zip(outs, coefs):
        same(o.view, torch.full((o.n,), 1.7, dtype=f32) * torch.tensor(c, dtype=f32), "fill_scaled_multi")
    same(one.view, torch.full((ns[-1],), 1.7, dtype=f32) * torch.tensor(0.25, dtype=f32), "fill_scaled")
    close(ss.view, torch.tensor([3.0 + 0.5 * float(xs[-1].double().sum())]), "sum_scale", rtol=1e-5, atol=1e-6)
    same(ss0.view, torch.zeros(1), "sum_scale of nothing")
    return dict(out=out, acc=acc, ss=ss, **{f"dx{i}": o for i, o in enumerate(outs)})


# =====================================================================================================================
# 6. elementwise and optimiser
# =====================================================================================================================
@case("egk_dropout_fwd", "egk_dropout_bwd", variants=[dict(n=4096, dt=f32, p=0.5), dict(n=1003, dt=bf16, p=0.25), dict(n=0, dt=f32, p=0.5)])
def dropout(lib, ops, G, n, dt, p):
    g = gen(n + 3)
    x, dy = r16(torch.randn(n, generator=g)) + 3.0, r16(torch.randn(n, generator=g))
    X, DY = G.v("x", n, dt, init=x), G.v("dy", n, dt, init=dy)
    Y, M, DX = G.v("y", n, dt), G.v("mask", n, u8), G.v("dx", n, dt)
    off = G.v("dev_offset", 1, i64, init=torch.tensor([5]), poison=0)
    ok(lib.egk_dropout_fwd(S(), P(X), P(Y), P(M), n, p, 1234, 8, P(off), edt(dt)), "egk_dropout_fwd")
    ok(lib.egk_dropout_bwd(S(), P(DY), P(M), P(DX), n, p, edt(dt)), "egk_dropout_bwd")
    G.check()
    m = M.view.cpu()
    assert set(m.unique().tolist()) <= {0, 1}, "mask: values other than 0 / 1 (a forgotten element keeps 0xA5)"
    inv = 1.0 / (1.0 - p)
    # the oracle applied with the kernel's own keep-mask (test_rowln_dropout_mask_semantics): rtol 1e-4 / atol 1e-5
    close(Y.view, x * m.float() * inv, "y", **(OUT16 if dt == bf16 else dict(rtol=1e-4, atol=1e-5)))
    close(DX.view, dy * m.float() * inv, "dx", **(OUT16 if dt == bf16 else dict(rtol=1e-4, atol=1e-5)))
    return dict(y=Y, mask=M, dx=DX)


@case("egk_relu_gate", "egk_axpby", variants=[dict(n=4096, dt=f32, off=0), dict(n=1003, dt=bf16, off=0), dict(n=1001, dt=f32, off=1),
                                              dict(n=0, dt=f32, off=0)])
def relu_gate_axpby(lib, ops, G, n, dt, off):
    """``off``: the buffers start one element past a 16-byte boundary -- both host functions compute ``vec`` from the pointers."""
    g = gen(n + 11)
    dy, y, b = r16(torch.randn(n, generator=g)), r16(torch.randn(n, generator=g)), torch.randn(n, generator=g)
    DY, Y, DX = G.v("dy", n, dt, init=dy, offset_elems=off), G.v("y", n, dt, init=y, offset_elems=off), G.v("dx", n, dt, offset_elems=off)
    ok(lib.egk_relu_gate(S(), P(DY), P(Y), P(DX), n, edt(dt)), "egk_relu_gate")
    A, B, O, O1 = (G.v("a", n, f32, init=dy, offset_elems=off), G.v("b", n, f32, init=b, offset_elems=off), G.v("out", n, f32, offset_elems=off),
                   G.v("out1", n, f32, offset_elems=off))
    ok(lib.egk_axpby(S(), P(A), P(B), P(O), n, 0.5, -2.0), "egk_axpby")
    ok(lib.egk_axpby(S(), P(A), None, P(O1), n, 0.5, 0.0), "egk_axpby")
    G.check()
    same(DX.view.float(), torch.where(y > 0, dy, torch.zeros(())), "dx")  # a selection: exact
    close(O.view, (0.5 * dy.double() - 2.0 * b.double()).float(), "axpby", rtol=1e-6, atol=1e-6)  # test_weighted_mean_sum_and_sum_tensors (sum_tensors)
    close(O1.view, (0.5 * dy.double()).float(), "axpby without y", rtol=1e-6, atol=1e-6)
    return dict(dx=DX, out=O, out1=O1)


@case("egk_copy_blocks", variants=[dict(nbytes=(4096, 0, 37, 1600, 3), null=(3,)), dict(nbytes=(16,), null=()), dict(nbytes=(5, 7), null=(0,))])
def copy_blocks(lib, ops, G, nbytes, null):
    g = gen(sum(nbytes))
    k, total = len(nbytes), sum(nbytes)
    srcs = [torch.randint(1, 256, (n,), generator=g, dtype=torch.int16).to(u8) for n in nbytes]
    X = [None if i in null else G.v(f"src{i}", n, u8, init=s) for i, (n, s) in enumerate(zip(nbytes, srcs))]
    D = G.v("dst", total, u8)
    ok(lib.egk_copy_blocks(S(), ptr_array(X), (C.c_int64 * k)(*nbytes), P(D), k), "egk_copy_blocks")
    G.check()
    same(D.view, torch.cat([torch.zeros(n, dtype=u8) if i in null else s for i, (n, s) in enumerate(zip(nbytes, srcs))]), "dst")
    return dict(dst=D)


@case("egk_zero_fill", "egk_zero_fill_ranges", variants=[dict(n16=1), dict(n16=1000)])
def zero_fill(lib, ops, G, n16):
    A = G.v("p", n16 * 4, f32, init=torch.ones(n16 * 4))
    ok(lib.egk_zero_fill(S(), P(A), n16 * 16), "egk_zero_fill")
    # ranges of an optimizer's flat gradient buffer: what lies between them keeps its bits
    B = G.v("base", 8192, f32, init=torch.arange(8192, dtype=f32) + 1)
    begin, nb = [0, 64, 4096 * 4 - 16, 1024], [16, 16 * n16 if n16 < 50 else 1600, 16, 0]
    ok(lib.egk_zero_fill_ranges(S(), P(B), (C.c_int64 * 4)(*begin), (C.c_int64 * 4)(*nb), 4), "egk_zero_fill_ranges")
    G.check()
    same(A.view, torch.zeros(n16 * 4), "zero_fill")
    ref = torch.arange(8192, dtype=f32) + 1
    for b0, n in zip(begin, nb):
        ref[b0 // 4:(b0 + n) // 4] = 0
    same(B.view, ref, "zero_fill_ranges")
    # refusals (host side, nothing launched): a pointer / a range that is not made of whole 16-byte groups
    refused(lib.egk_zero_fill(S(), P(A, 4), 16), "16-byte aligned")
    refused(lib.egk_zero_fill_ranges(S(), P(B, 8), (C.c_int64 * 1)(0), (C.c_int64 * 1)(16), 1), "16-byte aligned")
    refused(lib.egk_zero_fill_ranges(S(), P(B), (C.c_int64 * 1)(8), (C.c_int64 * 1)(16), 1), "whole 16-byte groups")
    G.check()
    same(B.view, ref, "zero_fill_ranges after the refused calls")
    return dict(p=A, base=B)


def _adam_ref(p, g, m, v, hyper, b1, b2, eps, wd):
    p, g, m, v = (t.double() for t in (p, g, m, v))
    lr, bc1, bc2s, gs = (float(h) for h in hyper)
    gg = g * gs + wd * p
    m = m + (gg - m) * (1 - b1)
    v = v * b2 + (1 - b2) * gg * gg
    return p - (lr / bc1) * (m / (v.sqrt() / bc2s + eps)), m, v


@case("egk_adam_step", "egk_adam_step_bump", "egk_adam_step_gated",
      variants=[dict(n=1003, gdt=f32, entry="step"), dict(n=4099, gdt=bf16, entry="bump"), dict(n=1003, gdt=f32, entry="gated", gate=1),
                dict(n=1003, gdt=bf16, entry="gated", gate=0), dict(n=4096, gdt=f32, entry="bump"), dict(n=0, gdt=f32, entry="bump")])
def adam(lib, ops, G, n, gdt, entry, gate=1):
    """The launch runs over an inner slice of larger flat buffers (the guards ARE the rest of the buffers), n % 4 != 0."""
    gn = gen(n + 61)
    p, g = torch.randn(n, generator=gn), r16(torch.randn(n, generator=gn))
    m, v = torch.randn(n, generator=gn) * 0.1, torch.rand(n, generator=gn) * 0.01
    hyper = torch.tensor([1e-2, 1 - 0.9 ** 3, math.sqrt(1 - 0.999 ** 3), 0.5])
    b1, b2, eps, wd = 0.9, 0.999, 1e-8, 1e-3
    Pp, Gg, M, V = G.v("p", n, f32, init=p), G.v("g", n, gdt, init=g), G.v("m", n, f32, init=m), G.v("v", n, f32, init=v)
    H = G.v("hyper", 4, f32, init=hyper)
    hi, lo = G.v("bf16_shadow", n, bf16), (G.v("bf16_lo_shadow", n, bf16) if entry != "step" else None)
    bump = G.v("bump_word", 1, i64, init=torch.tensor([100]), poison=0) if entry != "step" else None
    gt = G.v("gate", 1, i32, init=torch.tensor([gate]), poison=1) if entry == "gated" else None
    common = (S(), P(Pp), P(Gg), edt(gdt), P(M), P(V), n, P(H), b1, b2, eps, wd, P(hi))
    if entry == "step":
        ok(lib.egk_adam_step(*common), "egk_adam_step")
    elif entry == "bump":
        ok(lib.egk_adam_step_bump(*common, P(lo), P(bump), 7), "egk_adam_step_bump")
    else:
        ok(lib.egk_adam_step_gated(*common, P(lo), P(bump), 7, P(gt)), "egk_adam_step_gated")
    G.check()
    if bump is not None:
        assert bump.view.tolist() == [107 if n > 0 else 100], "bump_word"
    if entry == "gated" and gate == 0:  # a skipped step: nothing but *bump_word changes
        same(Pp.view, p, "p"), same(M.view, m, "m"), same(V.view, v, "v")
        assert bool(hi.is_sentinel().all()) and bool(lo.is_sentinel().all()), "a gated-off step wrote a bf16 copy"
    else:
        rp, rm, rv = _adam_ref(p, g, m, v, hyper, b1, b2, eps, wd)
        tol = dict(rtol=1e-5, atol=1e-6)  # tests/test_gpu_kernels.py::test_flat_adam_matches_torch_adam
        close(Pp.view, rp.float(), "p", **tol), close(M.view, rm.float(), "m", **tol), close(V.view, rv.float(), "v", **tol)
        pd = Pp.view.clone()
        same(hi.view.view(torch.int16), pd.to(bf16).view(torch.int16), "bf16_shadow")  # = bf16(p) of the stored p, bit for bit
        if lo is not None:
            same(lo.view.view(torch.int16), (pd - pd.to(bf16).float()).to(bf16).view(torch.int16), "bf16_lo_shadow")
    out = dict(p=Pp, m=M, v=V, hi=hi)
    if lo is not None:
        out["lo"] = lo
    return out


@case("egk_adam_hyper", "egk_grad_sumsq", "egk_grad_norm_finalize",
      variants=[dict(n=40003, gdt=f32, max_norm=1.0), dict(n=16384, gdt=bf16, max_norm=1e9), dict(n=7, gdt=f32, max_norm=1.0)])
def clip_chain(lib, ops, G, n, gdt, max_norm):
    g = r16(torch.randn(n, generator=gen(n)) * 3)
    slots = lib.egk_grad_sumsq_slots(n)
    assert slots == min(1024, (n + 16383) // 16384)
    X = G.v("g", n, gdt, init=g)
    part = G.v("partials", slots, f64)                                   # exactly egk_grad_sumsq_slots(n)
    src = G.v("src", 2, f32, init=torch.tensor([1e-3, 0.5]))
    t_dev = G.v("t_dev", 1, i64, init=torch.tensor([2]), poison=0)
    hyper, gate = G.v("hyper", 4, f32), G.v("gate", 1, i32, poison=7)
    stats = G.v("stats", 6, f64, init=torch.zeros(6, dtype=f64))
    ok(lib.egk_adam_hyper(S(), P(src), P(t_dev), 0.9, 0.999, P(hyper)), "egk_adam_hyper")
    ok(lib.egk_grad_sumsq(S(), P(X), edt(gdt), n, P(part), slots), "egk_grad_sumsq")
    ok(lib.egk_grad_norm_finalize(S(), P(part), slots, P(src), max_norm, P(hyper), P(t_dev), P(gate), P(stats)), "egk_grad_norm_finalize")
    G.check()
    want = float(g.double().pow(2).sum())
    got = math.fsum(part.view.tolist())
    assert abs(got - want) / want <= 2 * n * 2.0 ** -53, ("partials", got, want)  # tests/test_gpu_grad_clip.py::test_sum_of_squares_kernel
    norm = torch.tensor(0.5 * math.sqrt(want), dtype=f32)
    coef = torch.tensor(max_norm, dtype=f32) / (norm + torch.tensor(1e-6, dtype=f32))
    ref_h = torch.tensor([1e-3, 1 - 0.9 ** 3, math.sqrt(1 - 0.999 ** 3), float(torch.tensor(0.5) * coef) if float(coef) < 1 else 0.5])
    close(hyper.view, ref_h, "hyper", rtol=1e-5, atol=1e-6)  # tests/test_gpu_grad_clip.py TOL
    assert t_dev.view.tolist() == [3] and gate.view.tolist() == [1]
    close(stats.view, torch.tensor([1.0, float(norm), float(norm), 1.0 if float(coef) < 1 else 0.0, 0.0, float(norm)], dtype=f64), "stats",
          rtol=1e-5, atol=1e-6)
    # one slot less than the kernel writes: refused on the host, nothing launched
    refused(lib.egk_grad_sumsq(S(), P(X), edt(gdt), n, P(part), slots - 1), "partial sums")
    refused(lib.egk_grad_sumsq(S(), P(X, 4 if gdt == f32 else 2), edt(gdt), max(n - 1, 1), P(part), lib.egk_grad_sumsq_slots(max(n - 1, 1))),
            "16-byte aligned")
    G.check()
    return dict(partials=part, hyper=hyper, stats=stats)


@case("egk_stamp")
def stamp(lib, ops, G):
    buf = G.v("buf", 8, i64, poison=0)
    ok(lib.egk_stamp(S(), P(buf), 3), "egk_stamp")
    ok(lib.egk_stamp(S(), P(buf), 7), "egk_stamp")
    G.check()
    b = buf.view.tolist()
    assert b[3] != 0 and b[7] != 0 and b[7] >= b[3] and [b[i] for i in (0, 1, 2, 4, 5, 6)] == [0] * 6, b
    return None  # (a clock: nothing to compare between two runs)


# =====================================================================================================================
# 7. meters
# =====================================================================================================================
@case("egk_label_rank", variants=[dict(rows=77, Cn=115, pad=5, ys=2), dict(rows=64, Cn=128, pad=0, ys=1), dict(rows=0, Cn=5, pad=0, ys=1)])
def label_rank(lib, ops, G, rows, Cn, pad, ys):
    g = gen(rows + Cn)
    s = torch.randn(rows, Cn, generator=g).mul(4).round().div(4)  # many exact ties
    y = torch.randint(0, Cn, (rows, ys), generator=g)
    y[::7, 0] = -1
    if rows:
        y[1, 0] = Cn  # out of range: -1
    L = G.m("logits", rows, Cn, f32, pad=pad, init=s)
    Y = G.v("labels", rows * ys, i64, init=y, poison=0)
    R = G.v("rank", rows, i32, poison=-7)
    ok(lib.egk_label_rank(S(), P(L), L.ld, P(Y), ys, P(R), rows, Cn), "egk_label_rank")
    G.check()
    ref = torch.full((rows,), -1, dtype=i32)
    for r in range(rows):
        t = int(y[r, 0])
        if 0 <= t < Cn:
            ref[r] = int((s[r] > s[r, t]).sum()) + int((s[r, :t] == s[r, t]).sum())
    same(R.view, ref, "rank")
    refused(lib.egk_label_rank(S(), P(L), Cn - 1, P(Y), ys, P(R), rows, Cn), "leading dimension")
    return dict(rank=R)


def _levenshtein(a, b):
    prev = list(range(len(b) + 1))
    for i, x in enumerate(a, 1):
        cur = [i]
        for j, yv in enumerate(b, 1):
            cur.append(min(prev[j] + 1, cur[j - 1] + 1, prev[j - 1] + (x != yv)))
        prev = cur
    return prev[-1]


@case("egk_edit_distance", variants=[dict(N=5, Z=20, K=5), dict(N=3, Z=64, K=2), dict(N=4, Z=1, K=3), dict(N=0, Z=20, K=5)])
def edit_distance(lib, ops, G, N, Z, K):
    """pred is a [N, Z + 2, K] block of a wider prediction tensor (element strides (Z + 2) * K, K, 1 from its third row), label
    [N, Z] rows of a matrix with two spare columns."""
    g = gen(N + Z + K)
    pred, label = torch.randint(0, 6, (N, Z + 2, K), generator=g), torch.randint(0, 6, (N, Z + 2), generator=g)
    Pd = G.v("pred", N * (Z + 2) * K, i64, init=pred, poison=99)
    Lb = G.v("label", N * (Z + 2), i64, init=label, poison=98)
    out = G.v("out", N * K, i32, poison=-7)
    ok(lib.egk_edit_distance(S(), P(Pd, 2 * K * 8), (Z + 2) * K, K, 1, P(Lb, 8), Z + 2, 1, P(out), N, Z, K), "egk_edit_distance")
    G.check()
    ref = torch.tensor([_levenshtein(pred[n, 2:, k].tolist(), label[n, 1:Z + 1].tolist()) for n in range(N) for k in range(K)], dtype=i32)
    same(out.view, ref.reshape(-1), "out")  # tests/test_gpu_meters.py compares these distances exactly
    refused(lib.egk_edit_distance(S(), P(Pd), 1, 1, 1, P(Lb), 1, 1, P(out), N, 65, K), "unsupported")
    return dict(out=out)


# =====================================================================================================================
# 4. search
# =====================================================================================================================
GENERIC = dict(rtol=1e-4, atol=1e-5)  # tests/test_gpu_kernels.py (module docstring): every non-GEMM kernel against its f64 reference


@case("egk_row_inv_norm", "egk_row_sq_norm", "egk_row_inv_norm_cast",
      variants=[dict(rows=37, cols=260, dt=f32), dict(rows=64, cols=1024, dt=bf16), dict(rows=5, cols=250, dt=f32), dict(rows=9, cols=3, dt=bf16),
                dict(rows=6144, cols=1024, dt=f32), dict(rows=0, cols=64, dt=f32)])
def row_norms(lib, ops, G, rows, cols, dt):
    x = torch.randn(rows, cols, generator=gen(rows + cols)) * 2
    if rows:
        x[0, 0], x[rows - 1, cols - 1] = 1.0e5, -7.0e-6  # (inf in half / a half subnormal: test_search_prep_launch_equals_its_three_passes)
    x = r16(x) if dt == bf16 else x
    X = G.m("x", rows, cols, dt, init=x)
    inv, sq = G.v("inv_norm", rows), G.v("sq_norm", rows)
    ok(lib.egk_row_inv_norm(S(), P(X), P(inv), rows, cols, edt(dt)), "egk_row_inv_norm")
    ok(lib.egk_row_sq_norm(S(), P(X), P(sq), rows, cols, edt(dt)), "egk_row_sq_norm")
    G.check()
    ss = x.double().pow(2).sum(1)
    close(inv.view, ss.rsqrt().float(), "inv_norm", **GENERIC)
    close(sq.view, ss.float(), "sq_norm", **GENERIC)
    out = dict(inv=inv, sq=sq)
    if dt == f32:
        inv2, hi, h16 = G.v("inv_norm (cast launch)", rows), G.m("hi", rows, cols, bf16), G.m("h16", rows, cols, torch.int16)
        rc = lib.egk_row_inv_norm_cast(S(), P(X), P(inv2), P(hi), P(h16), rows, cols)
        if cols % 4:
            refused(rc, "multiple of 4")
            G.check()
            assert bool(hi.is_sentinel().all()) and bool(h16.is_sentinel().all()) and bool(inv2.is_sentinel().all())
        else:
            ok(rc, "egk_row_inv_norm_cast")
            G.check()
            same(inv2.view, inv.view, "inv_norm of the cast launch")  # test_search_prep_launch_equals_its_three_passes: the same bits
            same(hi.view.view(torch.int16), x.to(bf16).view(torch.int16), "hi")
            same(h16.view, x.to(torch.float16).view(torch.int16), "h16")
            out.update(hi=hi, h16=h16)
    return out


@case("egk_bf16_residual_ratio", "egk_residual_ratio16", variants=[dict(rows=57, cols=260, pad=4), dict(rows=8, cols=1024, pad=0),
                                                                   dict(rows=1, cols=3, pad=5)])
def residual_ratio(lib, ops, G, rows, cols, pad):
    x = torch.randn(rows, cols, generator=gen(rows * cols))
    X = G.m("x", rows, cols, f32, pad=pad, init=x)
    out = {}
    for f16 in (0, 1):
        r, rmax = G.v(f"r (f16 = {f16})", rows), G.v(f"rmax (f16 = {f16})", 1)
        if f16:
            ok(lib.egk_residual_ratio16(S(), P(X), X.ld, P(r), P(rmax), rows, cols, 1), "egk_residual_ratio16")
        else:
            ok(lib.egk_bf16_residual_ratio(S(), P(X), X.ld, P(r), P(rmax), rows, cols), "egk_bf16_residual_ratio")
        G.check()
        rounded = x.to(torch.float16 if f16 else bf16).double()
        ref = ((x.double() - rounded).norm(dim=1) / x.double().norm(dim=1)).float()
        close(r.view, ref, "r", **GENERIC)
        close(rmax.view, ref.max().reshape(1), "rmax", **GENERIC)
        out[f"r{f16}"], out[f"rmax{f16}"] = r, rmax
    refused(lib.egk_residual_ratio16(S(), P(X), cols - 1, P(r), P(rmax), rows, cols, 0), "bad shape")
    return out


@case("egk_cast", "egk_cast_f16", variants=[dict(n=4096, off=0), dict(n=1001, off=0), dict(n=1002, off=1), dict(n=1003, off=3), dict(n=0, off=0)])
def casts(lib, ops, G, n, off):
    """``off``: the buffers start ``off`` elements past a 16-byte boundary.  egk_cast computes ``vec`` from the pointers (scalar path);
    egk_cast_f16 refuses."""
    x = torch.randn(n, generator=gen(n + off)) * 3
    if n:
        x[0] = 1.0e5
    X, Y, Z = G.v("src", n, f32, init=x, offset_elems=off), G.v("dst bf16", n, bf16, offset_elems=off), G.v("dst f32", n, f32, offset_elems=off)
    H = G.v("dst f16", n, torch.int16, offset_elems=off)
    ok(lib.egk_cast(S(), P(X), F32, P(Y), BF16, n), "egk_cast")
    ok(lib.egk_cast(S(), P(Y), BF16, P(Z), F32, n), "egk_cast")
    rc = lib.egk_cast_f16(S(), P(X), P(H), n)
    G.check()
    same(Y.view.view(torch.int16), x.to(bf16).view(torch.int16), "f32 -> bf16")  # tests/test_gpu_kernels.py::test_cast_roundtrip: exact
    same(Z.view, x.to(bf16).float(), "bf16 -> f32")
    out = dict(y=Y, z=Z)
    if X.ptr % 16 or H.ptr % 8:
        refused(rc, "unaligned")
        assert bool(H.is_sentinel().all()), "a refused egk_cast_f16 wrote its output"
    else:
        ok(rc, "egk_cast_f16")
        same(H.view, x.to(torch.float16).view(torch.int16), "f32 -> f16")
        out["h"] = H
    refused(lib.egk_cast(S(), P(X), F32, P(Z), F32, n), "equal")
    return out


@case("egk_cos_dist", "egk_topk_smallest", "egk_topk_smallest_l2",
      variants=[dict(rows=33, K=257, k=4, pad=3), dict(rows=64, K=4096, k=4, pad=4), dict(rows=17, K=1000, k=16, pad=0),
                dict(rows=5, K=64, k=1, pad=8), dict(rows=0, K=64, k=4, pad=0)])
def cos_dist_topk(lib, ops, G, rows, K, k, pad):
    """tests/test_gpu_kernels.py::test_topk_selection_equals_full_lexicographic_sort: few distinct values and power-of-two scales, so
    every distance is exact in f32 and the picks must equal a full (distance, index) sort."""
    g = gen(rows * 1000 + K)
    dot = torch.randint(-3, 4, (rows, K), generator=g).float() / 4
    if rows:
        dot[0, :] = 0.5
    f_inv, b_inv = 2.0 ** torch.randint(-1, 2, (rows,), generator=g).float(), 2.0 ** torch.randint(-1, 2, (K,), generator=g).float()
    f_sq, b_sq = torch.randint(2, 6, (rows,), generator=g).float(), torch.randint(2, 6, (K,), generator=g).float()
    D = G.m("dot", rows, K, f32, pad=pad, init=dot)
    FI, BI, FS, BS = G.v("f_inv", rows, init=f_inv), G.v("b_inv", K, init=b_inv), G.v("f_sq", rows, init=f_sq), G.v("b_sq", K, init=b_sq)
    dist = G.m("dist", rows, K, f32)
    nn, nn2 = G.m("nn", rows, k, i64, poison=-7), G.m("nn (l2)", rows, k, i64, poison=-7)
    ok(lib.egk_cos_dist(S(), P(D), D.ld, P(FI), P(BI), P(dist), rows, K), "egk_cos_dist")
    ok(lib.egk_topk_smallest(S(), P(D), D.ld, P(FI), P(BI), P(nn), rows, K, k), "egk_topk_smallest")
    ok(lib.egk_topk_smallest_l2(S(), P(D), D.ld, P(FS), P(BS), P(nn2), rows, K, k), "egk_topk_smallest_l2")
    G.check()
    d = 1.0 - dot * f_inv[:, None] * b_inv[None, :]
    same(dist.view, d, "dist")
    same(nn.view, torch.sort(d, dim=1, stable=True).indices[:, :k], "nn")
    d2 = (f_sq[:, None] + b_sq[None, :] - 2.0 * dot).clamp(min=0).sqrt() * (1.0 / 4096.0)  # multiples of 1/2 below 12: distinct roots
    same(nn2.view, torch.sort(d2, dim=1, stable=True).indices[:, :k], "nn (l2)")
    refused(lib.egk_topk_smallest(S(), P(D), D.ld, P(FI), P(BI), P(nn), rows, K, 17), "k must be in")
    return dict(dist=dist, nn=nn, nn2=nn2)


@case("egk_topk_window", "egk_topk_window_group", "egk_topk_window_group16", variants=[
    dict(Gn=1, N=70, K=257, H=128, k=8, pd=4, pf=4, pb=4, entry="single"),
    dict(Gn=3, N=64, K=512, H=256, k=4, pd=0, pf=0, pb=0, entry="group"),
    dict(Gn=2, N=33, K=300, H=64, k=1, pd=3, pf=4, pb=8, entry="group16", plain=False),   # ldd % 4 != 0: the scalar screen
    dict(Gn=2, N=40, K=64, H=1024, k=16, pd=4, pf=8, pb=4, entry="group16"),
    dict(Gn=2, N=33, K=257, H=128, k=4, pd=4, pf=1, pb=3, entry="group", plain=False),    # ldf, ldb % 4 != 0: rows read by elements
    dict(Gn=8, N=0, K=64, H=64, k=4, pd=0, pf=0, pb=0, entry="group")])
def window_search(lib, ops, G, Gn, N, K, H, k, pd, pf, pb, entry):
    """tests/test_gpu_kernels.py::test_window_search_gives_the_lists_of_the_exact_distances: the lists must be those of the exact
    (f64) distances wherever the ranking gap exceeds the f32 key's rounding."""
    g = gen(Gn * 1000 + N + K)
    f16 = entry == "group16"
    rdt = torch.float16 if f16 else bf16
    f = torch.randn(Gn * N, H, generator=g)
    banks = [torch.randn(K, H, generator=g) for _ in range(Gn)]
    for b in banks:
        b[7] = b[6]                                                    # exact duplicates: ties -> lower index
    if N:
        f[3] = banks[0][6] + 0.2 * f[3]
    dot1 = torch.cat([(f[i * N:(i + 1) * N].to(rdt).double() @ banks[i].to(rdt).double().t()).float() for i in range(Gn)])
    f_inv = f.double().norm(dim=1).reciprocal().float()
    b_invs = [b.double().norm(dim=1).reciprocal().float() for b in banks]
    rbs = [((b.double() - b.to(rdt).double()).norm(dim=1) / b.double().norm(dim=1)).max().float().reshape(1) for b in banks]
    D1 = G.m("dot1", Gn * N, K, f32, pad=pd, init=dot1)
    Fm = G.m("f", Gn * N, H, f32, pad=pf, init=f)
    B = [G.m(f"bank{i}", K, H, f32, pad=pb, init=b) for i, b in enumerate(banks)]
    FI = G.v("f_inv", Gn * N, init=f_inv)
    BI = [G.v(f"b_inv{i}", K, init=b) for i, b in enumerate(b_invs)]
    RB = [G.v(f"rb_max{i}", 1, init=r) for i, r in enumerate(rbs)]
    nn, cand = G.m("nn", Gn * N, k, i64, poison=-7), G.v("cand", Gn * N, i32, poison=-7)
    if entry == "single":
        call = lambda fp, ldd: lib.egk_topk_window(S(), P(D1), ldd, fp, Fm.ld, P(B[0]), B[0].ld, P(FI), P(BI[0]), P(RB[0]), P(nn), P(cand),
                                                   N, K, H, k)
    elif entry == "group":
        call = lambda fp, ldd: lib.egk_topk_window_group(S(), P(D1), ldd, fp, Fm.ld, ptr_array(B), B[0].ld, P(FI), ptr_array(BI),
                                                         ptr_array(RB), P(nn), P(cand), Gn, N, K, H, k)
    else:
        call = lambda fp, ldd: lib.egk_topk_window_group16(S(), P(D1), ldd, fp, Fm.ld, ptr_array(B), B[0].ld, P(FI), ptr_array(BI),
                                                           ptr_array(RB), P(nn), P(cand), Gn, N, K, H, k, 1)
    ok(call(P(Fm), D1.ld), "egk_topk_window*")
    G.check()
    got, cnt = nn.view.cpu(), cand.view.cpu()
    for i in range(Gn):
        fi, bi = f[i * N:(i + 1) * N].double(), banks[i].double()
        dist = 1.0 - (fi / fi.norm(dim=1, keepdim=True)) @ (bi / bi.norm(dim=1, keepdim=True)).t()
        srt, order = torch.sort(dist, dim=1, stable=True)
        if k < K:
            safe = (srt[:, 1:k + 1] - srt[:, :k]).min(dim=1).values > 2e-6
        else:
            safe = (srt[:, 1:k] - srt[:, :k - 1]).min(dim=1).values > 2e-6
        gi = got[i * N:(i + 1) * N]
        same(gi[safe], order[safe][:, :k], f"nn of group {i}")
        if N:
            close(torch.gather(dist, 1, gi), srt[:, :k], f"selected distances of group {i}", rtol=0, atol=1e-6)
            assert int(cnt[i * N:(i + 1) * N].min()) >= k, "cand"
    if N:
        assert got[3, :2].tolist() == [6, 7][:k]
        refused(call(P(Fm, 4), D1.ld), "16-byte aligned")  # (after the empty-launch return: only with rows)
    refused(call(P(Fm), K - 1), "leading dimension")
    G.check()
    return dict(nn=nn, cand=cand)


# =====================================================================================================================
# 3. graph and row ops
# =====================================================================================================================
def _knob(lib, key):
    """Current value of an egk_tune knob (set and put back: the call returns the previous value)."""
    v = lib.egk_tune(key, 1)
    lib.egk_tune(key, v)
    return v


def _tee(lib, G, rows, cols, pad):
    """Arm the split tee for the next launch: hi / lo [rows, cols] bf16 with their own leading dimension."""
    hi, lo = G.m("tee hi", rows, cols, bf16, pad=pad), G.m("tee lo", rows, cols, bf16, pad=pad)
    ok(lib.egk_tee_split_next(P(hi), P(lo), hi.ld), "egk_tee_split_next")
    return hi, lo


def _tee_check(hi, lo, y, what):
    """hi = bf16(y), lo = bf16(y - hi) of the STORED f32 result, bit for bit (egk_split_bf16's arithmetic)."""
    yv = y.view.clone()
    same(hi.view.view(torch.int16), yv.to(bf16).view(torch.int16), what + ": tee hi")
    same(lo.view.view(torch.int16), (yv - yv.to(bf16).float()).to(bf16).view(torch.int16), what + ": tee lo")


@case("egk_pe_add", "egk_pe_table", "egk_pe_add_table", "egk_tee_split_next", "egk_slab_input_next",
      variants=[dict(rows=50, cols=64, dt=f32, tee=4, slab=True), dict(rows=37, cols=250, dt=f32, tee=3, slab=False),
                dict(rows=64, cols=1024, dt=bf16, tee=None, slab=False), dict(rows=130, cols=1024, dt=f32, tee=0, slab=True),
                dict(rows=33, cols=40, dt=bf16, tee=None, slab=False), dict(rows=0, cols=64, dt=f32, tee=None, slab=False)])
def positional_encoding(lib, ops, G, rows, cols, dt, tee, slab):
    """``tee``: pad of the split tee's halves (None: no tee; 3: a leading dimension that forces its element-wise stores);
    ``slab``: egk_pe_add_table reads its input as two slabs + bias (egk_slab_input_next).  bf16 rows of 1024 columns run on the
    rows1024 kernel (egk_tune 3)."""
    from oracle import pyg_ops as PO
    g = gen(rows + cols)
    x = r16(torch.randn(rows, cols, generator=g))
    pos = torch.randint(-128, 128, (rows,), generator=g)
    freq = PO.positional_encoding_frequency(cols)
    pos_min, n_pos = -8, 16                                          # most positions lie OUTSIDE the table
    if rows > 2:
        pos[0], pos[1], pos[2] = -8, 7, 8
    X, Pz, Fq = G.m("x", rows, cols, dt, init=x), G.v("pos", rows, i64, init=pos, poison=0), G.v("freq", cols // 2, f32, init=freq)
    Y, Y2, T = G.m("y", rows, cols, dt), G.m("y (table)", rows, cols, dt), G.m("table", n_pos, cols, f32)
    tol = OUT16 if dt == bf16 else dict(rtol=1e-5, atol=2e-5)        # tests/test_gpu_kernels.py::test_pe_add, test_graphln_csr_pe_bf16_activations
    halves = _tee(lib, G, rows, cols, tee) if tee is not None else None
    ok(lib.egk_pe_add(S(), P(X), P(Pz), P(Fq), P(Y), rows, cols, edt(dt)), "egk_pe_add")
    ok(lib.egk_pe_table(S(), P(Fq), pos_min, n_pos, cols, P(T)), "egk_pe_table")
    G.check()
    ref = x + PO.positional_encoding(pos, freq)
    close(Y.view, ref, "y", **tol)
    close(T.view, PO.positional_encoding(torch.arange(pos_min, pos_min + n_pos), freq), "table", rtol=1e-5, atol=2e-5)
    if halves and rows:
        _tee_check(*halves, Y, "egk_pe_add")
    out = dict(y=Y, table=T)
    if slab:
        x2, bias = torch.randn(rows, cols, generator=g), torch.randn(cols, generator=g)
        X2, Bs, XO = G.m("slab x2", rows, cols, f32, init=x2), G.v("slab bias", cols, f32, init=bias), G.m("slab x_out", rows, cols, f32)
        ok(lib.egk_slab_input_next(P(X2), P(Bs), P(XO)), "egk_slab_input_next")
        halves2 = _tee(lib, G, rows, cols, tee) if tee is not None else None
        Y3 = G.m("y (table, slab input)", rows, cols, dt)
        ok(lib.egk_pe_add_table(S(), P(X), P(Pz), P(Fq), P(T), pos_min, n_pos, P(Y3), rows, cols, edt(dt)), "egk_pe_add_table")
        G.check()
        same(XO.view, (x + x2) + bias, "slab x_out")                 # gemm_splitk_reduce's arithmetic: (x + x2) + bias, the same bits
        close(Y3.view, ((x + x2) + bias) + PO.positional_encoding(pos, freq), "y from a slab input", **tol)
        if halves2:
            _tee_check(*halves2, Y3, "egk_pe_add_table")
        out.update(x_out=XO, y3=Y3)
    ok(lib.egk_pe_add_table(S(), P(X), P(Pz), P(Fq), P(T), pos_min, n_pos, P(Y2), rows, cols, edt(dt)), "egk_pe_add_table")
    G.check()
    same(_bits(Y2), _bits(Y), "y through the table")                  # test_pe_add_table_is_bit_identical_to_the_direct_evaluation
    if dt == bf16 and cols == 1024:                                   # the generic kernel (egk_tune 3 = 0) gives the same bits
        # (the rows1024 kernel shares the counter id "pe_add": its launcher predicate -- knob 3, 16-byte aligned x / y / table -- is asserted)
        assert _knob(lib, 3) == 1 and all(t.ptr % 16 == 0 for t in (X, Y2, T))
        Y4 = G.m("y (table, generic kernel)", rows, cols, dt)
        prev = lib.egk_tune(3, 0)
        try:
            ok(lib.egk_pe_add_table(S(), P(X), P(Pz), P(Fq), P(T), pos_min, n_pos, P(Y4), rows, cols, edt(dt)), "egk_pe_add_table")
        finally:
            assert lib.egk_tune(3, prev) == 0
        G.check()
        same(_bits(Y4), _bits(Y2), "rows1024 kernel against the generic kernel")
    refused(lib.egk_pe_add(S(), P(X), P(Pz), P(Fq), P(Y), rows, cols + 1, edt(dt)), "odd channel count")
    out["y2"] = Y2
    return out


def _graphs(kind):
    """(edge_index, n) of the existing tests' graphs."""
    from egopack_amd import data as D
    g = gen(17)
    if kind == "banded":   # test_banded_gather_is_the_csr_gather_bit_for_bit: band sequences, LTA sequences, isolated rows, self loops
        parts, n = [], 0
        for T in (9, 32, 5, 1, 12):
            parts.append(D.radius_band_edges(torch.arange(T), 1) + n)
            n += T
        y = torch.stack([torch.randint(1, 5, (14,), generator=g), torch.randint(0, 5, (14,), generator=g)], 1)
        y[:3] = -1
        parts.append(D.lta_connectivity_edges(torch.arange(14), y, 1.5) + n)
        n += 14 + 3
        parts.append(torch.tensor([[2, 40, 20], [2, 40, 20]]))
        ei = torch.cat(parts, 1)
        keep = torch.ones(ei.shape[1], dtype=torch.bool)
        keep[-1] = False
        order = torch.argsort(ei[1, keep] * n + ei[0, keep])
        return torch.cat([ei[:, keep][:, order], ei[:, ~keep]], 1), n
    T, B = (70, 2) if kind == "heavy" else (32, 3)  # test_csr_gather_rows_with_hundreds_of_edges: fan-out / fan-in nodes
    eis, off = [], 0
    for _ in range(B):
        y = torch.ones(T, 2, dtype=torch.long)
        y[:2] = -1
        ei = D.lta_connectivity_edges(torch.arange(T), y, 1.5)
        eis.append(torch.cat([ei, torch.stack([torch.arange(3, T), torch.full((T - 3,), 2)])], 1) + off)
        off += T
    return torch.cat(eis, 1), off


@case("egk_csr_gather", "egk_csr_gather_banded", variants=[
    dict(kind="banded", cols=250, dt=f32, mode=0), dict(kind="banded", cols=1024, dt=bf16, mode=0), dict(kind="banded", cols=64, dt=f32, mode=0),
    dict(kind="heavy", cols=256, dt=f32, mode=0), dict(kind="heavy", cols=250, dt=bf16, mode=0), dict(kind="heavy", cols=1024, dt=bf16, mode=0),
    dict(kind="fan32", cols=1024, dt=bf16, mode=1), dict(kind="fan32", cols=260, dt=f32, mode=1), dict(kind="heavy", cols=2048, dt=f32, mode=1)])
def csr_gather(lib, ops, G, kind, cols, dt, mode):
    """Forward (mean) and transposed (weighted, gated) orientation; x carries one POISON ROW (NaN) behind its n rows, and ``col``'s
    sentinel names it.  bf16 rows of 1024 columns take the rows1024 kernels (egk_tune 3), compared with the generic ones."""
    from egopack_amd import data as D
    ei, n = _graphs(kind)
    gr = D.build_csr(ei, n)
    g = gen(n + cols)
    x, gate = r16(torch.randn(n, cols, generator=g)), r16(torch.randn(n, cols, generator=g))
    A = torch.zeros(n, n, dtype=f64)
    A.index_put_((ei[1], ei[0]), torch.ones(ei.shape[1], dtype=f64), accumulate=True)
    deg = A.sum(1).clamp(min=1)
    ref_f = ((A / deg[:, None]) @ x.double()).float()
    ref_b = (((A / deg[:, None]).t() @ x.double()) * (gate.double() > 0)).float()
    # test_csr_gather_rows_with_hundreds_of_edges (f32 1e-5 / 1e-5, bf16 1e-2 / 1e-2)
    tol = dict(rtol=1e-5, atol=1e-5) if dt == f32 else dict(rtol=1e-2, atol=1e-2)
    E = ei.shape[1]
    X = G.m("x (+ poison row)", n + 1, cols, dt, init=torch.cat([x, torch.full((1, cols), float("nan"))]))
    GT = G.m("relu_gate", n, cols, dt, init=gate)
    out = {}

    def run(tag, rowptr, col, wgt, gate_, heavy, band, knob):
        n_heavy = int(heavy.numel()) if mode == 1 or kind == "heavy" else 0
        if kind != "heavy" and mode == 0:
            heavy = heavy[:0]
        RP, CL = G.v(tag + "rowptr", n + 1, i32, init=rowptr, poison=E), G.v(tag + "col", E, i32, init=col, poison=n)
        W = G.v(tag + "wgt", E, f32, init=wgt) if wgt is not None else None
        HV = G.v(tag + "heavy_rows", n_heavy, i32, init=heavy[:n_heavy], poison=n) if n_heavy else None
        BD = G.v(tag + "band", n, u8, init=band) if band is not None else None
        ws_bytes = lib.egk_csr_heavy_ws_bytes(n_heavy, cols) if (n_heavy and mode == 0) else 0
        assert ws_bytes == (n_heavy * 8 * cols * 4 if mode == 0 else 0)
        WS = G.v(tag + "ws", ws_bytes // 4, f32) if ws_bytes else None          # exactly egk_csr_heavy_ws_bytes
        O = G.m(tag + "out", n, cols, dt)
        prev = lib.egk_tune(3, knob)
        try:
            if band is not None:
                ok(lib.egk_csr_gather_banded(S(), P(X), P(RP), P(CL), P(BD), P(O), n, cols, edt(dt), P(HV), n_heavy, P(WS), mode),
                   "egk_csr_gather_banded")
            else:
                ok(lib.egk_csr_gather(S(), P(X), P(RP), P(CL), P(W), P(gate_), P(O), n, cols, edt(dt), P(HV), n_heavy, P(WS), mode),
                   "egk_csr_gather")
        finally:
            lib.egk_tune(3, prev)
        G.check()
        return O

    lean = dt == bf16 and cols == 1024
    if lean:
        # The rows1024 kernels share the counter id "csr_gather" with the generic ones: selection is not observable through the ABI.
        # Their launcher predicate (knob 3 on, bf16, cols == 1024, 16-byte aligned x / out / gate) is asserted instead, and both knob
        # values are run below.
        assert _knob(lib, 3) == 1 and X.ptr % 16 == 0 and GT.ptr % 16 == 0
    for knob in ((1, 0) if lean else (1,)):
        t = f"[tune3={knob}] "
        fwd = run(t + "fwd ", gr.rowptr, gr.col, None, None, gr.heavy, None, knob)
        close(fwd.view, ref_f, t + "mean gather", **tol)
        bwd = run(t + "bwd ", gr.t_rowptr, gr.t_col, gr.t_wgt, GT, gr.t_heavy, None, knob)
        close(bwd.view, ref_b, t + "weighted gated gather", **tol)
        ungated = run(t + "bwd ungated ", gr.t_rowptr, gr.t_col, gr.t_wgt, None, gr.t_heavy, None, knob)
        close(ungated.view, ((A / deg[:, None]).t() @ x.double()).float(), t + "weighted gather", **tol)
        bnd = run(t + "banded ", gr.rowptr, gr.col, None, None, gr.heavy, gr.band, knob)
        same(_bits(bnd), _bits(fwd), t + "banded against the CSR walk")     # test_banded_gather_is_the_csr_gather_bit_for_bit
        out.update({f"fwd{knob}": fwd, f"bwd{knob}": bwd, f"bnd{knob}": bnd})
    if lean:
        same(_bits(out["bnd1"]), _bits(out["bnd0"]), "rows1024 banded kernel against the generic kernel")  # test_rows1024_gather_..._bit_identical
    if kind == "heavy":
        assert gr.t_heavy.numel() >= 2 and gr.heavy.numel() >= 2
    return out


@case("egk_gather_max_fwd", "egk_gather_max_bwd", "egk_gather_max_group_fwd", "egk_gather_max_bank_grad", variants=[
    dict(Gn=3, N=130, K=57, H=1024, k=4, dt=bf16), dict(Gn=2, N=37, K=57, H=256, k=8, dt=f32), dict(Gn=3, N=40, K=19, H=320, k=3, dt=f32),
    dict(Gn=1, N=70, K=19, H=250, k=4, dt=bf16), dict(Gn=4, N=33, K=57, H=512, k=4, dt=f32), dict(Gn=2, N=0, K=19, H=256, k=4, dt=f32)])
def gather_max(lib, ops, G, Gn, N, K, H, k, dt):
    """The banks carry one POISON ROW (NaN, number K) and ``nn``'s sentinel names it.  k in {4, 8} with H % 256 == 0 selects the
    loads-up-front kernel (egk_gather_max_tune), everything else the generic one: both are run and must agree bit for bit."""
    g = gen(Gn * 100 + N + H)
    banks = [torch.randn(K, H, generator=g) for _ in range(Gn)]
    nns = [torch.stack([torch.randperm(K, generator=g)[:k] for _ in range(N)]) if N else torch.zeros(0, k, dtype=i64) for _ in range(Gn)]
    f = torch.randn(Gn * N, H, generator=g)
    if N > 5:
        f[5] = banks[0][nns[0][5, 1]]                                 # an exact tie with a prototype row: the prototype wins
    f, dm = r16(f) if dt == bf16 else f, r16(torch.randn(Gn * N, H, generator=g))
    Fm = G.m("f", Gn * N, H, dt, init=f)
    B = [G.m(f"bank{i} (+ poison row)", K + 1, H, f32, init=torch.cat([b, torch.full((1, H), float("nan"))])) for i, b in enumerate(banks)]
    NN = [G.m(f"nn{i}", N, k, i64, init=nns[i], poison=K) for i in range(Gn)]
    up_front = k in (4, 8) and H % 256 == 0
    out = {}
    ref = torch.cat([torch.cat([banks[i][nns[i]], f[i * N:(i + 1) * N].unsqueeze(1)], 1) for i in range(Gn)]) if N else torch.zeros(0, k + 1, H)
    ref_m, ref_a = ref.max(1) if N else (torch.zeros(0, H), torch.zeros(0, H, dtype=i64))
    ref_a = (ref == ref_m.unsqueeze(1)).int().argmax(1).to(u8) if N else ref_a.to(u8)  # the FIRST maximum wins
    for knob in ((1, 0) if up_front else (1,)):
        prev = lib.egk_gather_max_tune(knob)
        try:
            M, Ar = G.m(f"[tune={knob}] m", Gn * N, H, dt), G.m(f"[tune={knob}] arg", Gn * N, H, u8)
            ok(lib.egk_gather_max_group_fwd(S(), P(Fm), ptr_array(B), ptr_array(NN), Gn, P(M), P(Ar), N, H, k, edt(dt)),
               "egk_gather_max_group_fwd")
            M1, A1 = G.m(f"[tune={knob}] m (one by one)", Gn * N, H, dt), G.m(f"[tune={knob}] arg (one by one)", Gn * N, H, u8)
            eb = 2 if dt == bf16 else 4
            for i in range(Gn):
                ok(lib.egk_gather_max_fwd(S(), P(Fm, i * N * H * eb), P(B[i]), P(NN[i]), P(M1, i * N * H * eb), P(A1, i * N * H), N, H, k,
                                          edt(dt)), "egk_gather_max_fwd")
        finally:
            lib.egk_gather_max_tune(prev)
        G.check()
        # test_gather_max_of_several_tasks_in_one_launch_with_every_load_up_front: values (rounded to the type) and winners exact
        same(M.view.float(), ref_m.to(dt).float(), f"[tune={knob}] m")
        same(Ar.view, ref_a, f"[tune={knob}] arg")
        same(_bits(M1), _bits(M), f"[tune={knob}] m one by one"), same(_bits(A1), _bits(Ar), f"[tune={knob}] arg one by one")
        out.update({f"m{knob}": M, f"arg{knob}": Ar})
    if N > 5:
        assert int(Ar.view[5].ne(k).sum()) > 0
    # backward: df = (arg == k) ? dm : 0 (+ df), and the trainable bank's gradient through the winners
    DM = G.m("dm", Gn * N, H, dt, init=dm)
    DF, DFa = G.m("df", Gn * N, H, dt), G.m("df (accumulate)", Gn * N, H, dt, init=f)
    ok(lib.egk_gather_max_bwd(S(), P(DM), P(Ar), P(DF), Gn * N, H, k, 0, edt(dt)), "egk_gather_max_bwd")
    ok(lib.egk_gather_max_bwd(S(), P(DM), P(Ar), P(DFa), Gn * N, H, k, 1, edt(dt)), "egk_gather_max_bwd")
    G.check()
    sel = torch.where(ref_a == k, dm, torch.zeros(()))
    same(DF.view.float(), sel, "df")                                   # test_gather_max_fwd_bwd: exact
    close(DFa.view, f + sel, "df accumulated", **(OUT16 if dt == bf16 else dict(rtol=1e-6, atol=1e-6)))  # test_gather_max_trainable_bank_gradient
    out.update(df=DF, dfa=DFa)
    if N:
        nn0, a0 = nns[0], ref_a[:N]
        edges = [[] for _ in range(K)]
        for r in range(N):
            for j in range(k):
                edges[int(nn0[r, j])].append(r * k + j)
        t_rowptr = torch.tensor([0] + [len(e) for e in edges]).cumsum(0).to(i32)
        t_edge = torch.tensor([e for es in edges for e in es], dtype=i32)
        TR, TE = G.v("t_rowptr", K + 1, i32, init=t_rowptr, poison=int(t_rowptr[-1])), G.v("t_edge", t_edge.numel(), i32, init=t_edge, poison=0)
        dbank0 = torch.randn(K, H, generator=g)
        DB = G.m("dbank", K, H, f32, init=dbank0)
        ok(lib.egk_gather_max_bank_grad(S(), P(DM), P(Ar), P(TR), P(TE), P(DB), K, H, k, edt(dt)), "egk_gather_max_bank_grad")
        G.check()
        refb = dbank0.double().clone()
        for j in range(k):
            refb.index_add_(0, nn0[:, j], torch.where(a0 == j, dm[:N], torch.zeros(())).double())
        close(DB.view, refb.float(), "dbank", rtol=1e-5, atol=1e-5)      # test_gather_max_trainable_bank_gradient
        out["dbank"] = DB
    return out


@case("egk_segment_max_fwd", "egk_segment_max_bwd", "egk_segment_max_multi_fwd", "egk_segment_max_multi_bwd", variants=[
    dict(lens=(4, 0, 5, 11), cols=96, dt=f32, n_src=1), dict(lens=(33, 1, 0, 70), cols=250, dt=bf16, n_src=2),
    dict(lens=(32,) * 7, cols=1024, dt=bf16, n_src=4), dict(lens=(5,) * 130, cols=256, dt=f32, n_src=3), dict(lens=(), cols=64, dt=f32, n_src=1)])
def segment_max(lib, ops, G, lens, cols, dt, n_src):
    """cols % 4 == 0 takes the four-columns-per-thread kernel (16 row lanes below 128 segments, 4 from there), else the serial walk;
    an empty sequence gives zeros and arg -1.  tests/test_gpu_kernels.py::test_segment_max_rows_shared_by_four_lanes: exact."""
    g = gen(len(lens) * 100 + cols)
    n_seg, rows = len(lens), sum(lens)
    ptr = torch.tensor((0,) + tuple(lens), dtype=i64).cumsum(0).to(i32)
    xs = [r16(torch.randn(rows, cols, generator=g)) for _ in range(n_src)]
    if rows > 1 and lens[0] > 1:
        xs[0][1] = xs[0][0]                                             # a tie: the first occurrence wins
    douts = [r16(torch.randn(n_seg, cols, generator=g)) for _ in range(n_src)]
    PT = G.v("ptr", n_seg + 1, i32, init=ptr, poison=rows)
    X = [G.m(f"x{i}", rows, cols, dt, init=x) for i, x in enumerate(xs)]
    O = [G.m(f"out{i}", n_seg, cols, dt) for i in range(n_src)]
    Ar = [G.m(f"arg{i}", n_seg, cols, i32, poison=-7) for i in range(n_src)]
    DO = [G.m(f"dout{i}", n_seg, cols, dt, init=d) for i, d in enumerate(douts)]
    DX = [G.m(f"dx{i}", rows, cols, dt) for i in range(n_src)]
    if n_src == 1:
        ok(lib.egk_segment_max_fwd(S(), P(X[0]), P(PT), P(O[0]), P(Ar[0]), n_seg, cols, edt(dt)), "egk_segment_max_fwd")
        ok(lib.egk_segment_max_bwd(S(), P(DO[0]), P(Ar[0]), P(PT), P(DX[0]), n_seg, rows, cols, edt(dt)), "egk_segment_max_bwd")
    else:
        ok(lib.egk_segment_max_multi_fwd(S(), ptr_array(X), P(PT), ptr_array(O), ptr_array(Ar), n_src, n_seg, cols, edt(dt)),
           "egk_segment_max_multi_fwd")
        ok(lib.egk_segment_max_multi_bwd(S(), ptr_array(DO), ptr_array(Ar), P(PT), ptr_array(DX), n_src, n_seg, rows, cols, edt(dt)),
           "egk_segment_max_multi_bwd")
    G.check()
    out = {}
    for i in range(n_src):
        ref_v, ref_a, ref_dx = torch.zeros(n_seg, cols), torch.full((n_seg, cols), -1, dtype=i32), torch.zeros(rows, cols)
        for s_, (a, b) in enumerate(zip(ptr[:-1].tolist(), ptr[1:].tolist())):
            if b > a:
                v, _ = xs[i][a:b].max(dim=0)
                first = (xs[i][a:b] == v).int().argmax(dim=0)
                ref_v[s_], ref_a[s_] = v, (first + a).int()
                ref_dx[first + a, torch.arange(cols)] = douts[i][s_]
        same(O[i].view.float(), ref_v, f"out{i}"), same(Ar[i].view, ref_a, f"arg{i}"), same(DX[i].view.float(), ref_dx, f"dx{i}")
        out.update({f"out{i}": O[i], f"arg{i}": Ar[i], f"dx{i}": DX[i]})
    return out


@case("egk_segment_sum_rows_f64", variants=[dict(rows=300, cols=1024, L=35, dt=f32), dict(rows=300, cols=37, L=35, dt=bf16),
                                            dict(rows=0, cols=64, L=5, dt=f32)])
def segment_sum_rows(lib, ops, G, rows, cols, L, dt):
    """tests/test_gpu_kernels.py::test_scatter_add_rows_f64: rows of one label summed in f32 in node order, added to the f64 bank --
    bit-exact against that restatement.  x carries a poison row (NaN) that ``order``'s sentinel names."""
    from oracle import pyg_ops as PO
    g = gen(41 + cols)
    x = r16(torch.randn(rows, cols, generator=g))
    label = torch.randint(-1, L, (rows,), generator=g)
    if rows:
        label[:40] = 7
    order = torch.argsort(label, stable=True)
    labs, counts = torch.unique_consecutive(label[order], return_counts=True)
    n_seg = labs.numel()
    seg_ptr = torch.cat([torch.zeros(1, dtype=i64), counts.cumsum(0)]).to(i32)
    bank0, count0 = torch.randn(L, cols, generator=g, dtype=f64), torch.randint(0, 9, (L,), generator=g)
    X = G.m("x (+ poison row)", rows + 1, cols, dt, init=torch.cat([x, torch.full((1, cols), float("nan"))]))
    OR, SP = G.v("order", rows, i32, init=order, poison=rows), G.v("seg_ptr", n_seg + 1, i32, init=seg_ptr, poison=rows)
    SL = G.v("seg_label", n_seg, i64, init=labs, poison=-1)            # (a label outside [0, n_labels): that group is skipped)
    BK, CT = G.m("bank", L, cols, f64, init=bank0), G.v("count", L, i64, init=count0, poison=-7)
    ok(lib.egk_segment_sum_rows_f64(S(), P(X), P(OR), P(SP), P(SL), P(BK), P(CT), n_seg, cols, L, edt(dt)), "egk_segment_sum_rows_f64")
    G.check()
    keep = label >= 0
    ref = bank0 + PO.scatter_sum(x[keep], label[keep], L) if rows else bank0
    same(BK.view, ref, "bank")
    same(CT.view, count0 + torch.bincount(label[keep], minlength=L), "count")
    return dict(bank=BK, count=CT)


@case("egk_gather_rows", "egk_gather_lerp_rows", variants=[
    dict(n=77, cols=1536, pad=8, tdt=bf16, odt=bf16), dict(n=77, cols=1536, pad=8, tdt=f32, odt=bf16), dict(n=33, cols=250, pad=3, tdt=f32, odt=f32),
    dict(n=33, cols=260, pad=4, tdt=bf16, odt=f32), dict(n=5, cols=1, pad=0, tdt=f32, odt=f32), dict(n=0, cols=64, pad=0, tdt=f32, odt=f32)])
def gather_rows(lib, ops, G, n, cols, pad, tdt, odt):
    """tests/test_gpu_feature_store.py: copies keep bits, f32 -> bf16 rounds to nearest even, indices outside the table give zeros;
    the interpolation is numpy's double arithmetic rounded once.  The table's last row is the POISON ROW the index sentinels name."""
    g = gen(n + cols)
    R = 40
    table = r16(torch.randn(R, cols, generator=g))
    idx = torch.randint(0, R, (n,), generator=g)
    lo_, hi_ = torch.randint(0, R, (n,), generator=g), torch.randint(0, R, (n,), generator=g)
    w = torch.rand(n, generator=g, dtype=f64)
    if n > 8:
        idx[1], idx[2] = -1, R + 1          # (R is the poison row: a valid index never selects it, R + 1 is out of range)
        lo_[3] = hi_[3]
        lo_[4], hi_[5] = -1, R + 1
    T = G.m("table (+ poison row)", R + 1, cols, tdt, pad=pad, init=torch.cat([table, torch.full((1, cols), float("nan"))]))
    IX, LO, HI = G.v("idx", n, i64, init=idx, poison=R), G.v("lo", n, i64, init=lo_, poison=R), G.v("hi", n, i64, init=hi_, poison=R)
    W = G.v("w", n, f64, init=w)
    O, O2 = G.m("out", n, cols, odt), G.m("out (lerp)", n, cols, odt)
    # the poison row lies INSIDE the allocation but outside table_rows = R: an index R gives zeros
    ok(lib.egk_gather_rows(S(), P(T), edt(tdt), T.ld, R, P(IX), P(O), edt(odt), n, cols), "egk_gather_rows")
    ok(lib.egk_gather_lerp_rows(S(), P(T), edt(tdt), T.ld, R, P(LO), P(HI), P(W), P(O2), edt(odt), n, cols), "egk_gather_lerp_rows")
    G.check()
    z = torch.zeros(1, cols)
    pick = lambda ix: torch.cat([table, z])[torch.where((ix >= 0) & (ix < R), ix, torch.full_like(ix, R))]
    same(O.view.float(), pick(idx).to(odt).float(), "out")
    a, b = pick(lo_).double(), pick(hi_).double()
    lerp = ((1.0 - w)[:, None] * a + w[:, None] * b).float()
    ref2 = torch.where((lo_ == hi_)[:, None], pick(lo_), lerp)
    # (bf16 output: the f32 result rounded ONCE more, tests/test_gpu_feature_store.py -- this comparison found the kernel rounding f64 -> bf16 in one step)
    same(O2.view.float(), ref2.to(odt).float(), "out (lerp)")
    refused(lib.egk_gather_rows(S(), P(T), edt(tdt), cols - 1, R, P(IX), P(O), edt(odt), n, cols), "leading dimension")
    return dict(out=O, out2=O2)


# =====================================================================================================================
# 2. normalisation
# =====================================================================================================================
def _pad8(n):
    return (n + 7) // 8 * 8


def _slots(G, name, cols, init):
    """dw / db as two adjacent slots of ONE guarded flat gradient buffer (optim.FlatAdam's layout: slots start at multiples of 8
    elements, the padding between them stays what it was); returns (buffer, byte offset of the second slot, the initial values)."""
    c8 = _pad8(cols)
    flat = G.v(name, 2 * c8, f32, init=init)
    return flat, c8 * 4


def _ws_guard(cols):
    """A workspace query that is one partial row short lets a kernel overrun by a whole partial row pair (2 * cols floats): the
    guard of a workspace covers that."""
    return max(GUARD_ELEMS, 4 * cols)


@case("egk_rowln_fwd", "egk_rowln_bwd", "egk_ln_bwd_reduce", "egk_tee_split_next", "egk_slab_input_next", variants=[
    dict(rows=37, cols=40, dt=f32, relu=1, p=0.0, tee=4, slab=True), dict(rows=5, cols=250, dt=f32, relu=0, p=0.25, tee=3, slab=False),
    dict(rows=130, cols=1024, dt=bf16, relu=1, p=0.5, tee=None, slab=False), dict(rows=130, cols=1024, dt=f32, relu=1, p=0.0, tee=0, slab=True),
    dict(rows=3, cols=1280, dt=f32, relu=1, p=0.25, tee=8, slab=False), dict(rows=70, cols=3072, dt=bf16, relu=1, p=0.25, tee=None, slab=False),
    dict(rows=64, cols=2048, dt=f32, relu=0, p=0.0, tee=4, slab=False), dict(rows=9, cols=4096, dt=f32, relu=1, p=0.25, tee=None, slab=False),
    dict(rows=2100, cols=64, dt=bf16, relu=1, p=0.0, tee=None, slab=False), dict(rows=0, cols=64, dt=f32, relu=1, p=0.0, tee=None, slab=False)])
def row_layernorm(lib, ops, G, rows, cols, dt, relu, p, tee, slab):
    """One-wave kernels (cols <= 256 / <= 1024 with the exact-1024 specialisation / <= 4096), the workgroup-per-row kernels of
    2048 / 3072 / 4096 columns, cols % 4 != 0 (element-wise accesses); dropout with the kernel's own keep mask; the tee halves and
    the slab input; dw / db accumulate into slots of a flat buffer, fused and through egk_ln_bwd_reduce."""
    g = gen(rows * cols + relu)
    x = r16(torch.randn(rows, cols, generator=g) * 2 + 0.3)
    w, b = torch.randn(cols, generator=g), torch.randn(cols, generator=g)
    dy = r16(torch.randn(rows, cols, generator=g))
    xin = x
    X = G.m("x", rows, cols, dt, init=x)
    W, B = G.v("w", cols, f32, init=w), G.v("b", cols, f32, init=b)
    Y, MEAN, RSTD = G.m("y", rows, cols, dt), G.v("mean", rows), G.v("rstd", rows)
    MASK = G.m("mask", rows, cols, u8) if p > 0 else None
    OFF = G.v("dev_offset", 1, i64, init=torch.tensor([3]), poison=0)
    out = dict(y=Y, mean=MEAN, rstd=RSTD)
    if slab:
        x2, bias = torch.randn(rows, cols, generator=g), torch.randn(cols, generator=g)
        X2, Bs, XO = G.m("slab x2", rows, cols, f32, init=x2), G.v("slab bias", cols, f32, init=bias), G.m("slab x_out", rows, cols, f32)
        ok(lib.egk_slab_input_next(P(X2), P(Bs), P(XO)), "egk_slab_input_next")
        xin = (x + x2) + bias
        out["x_out"] = XO
    halves = _tee(lib, G, rows, cols, tee) if tee is not None else None
    if cols in (2048, 3072, 4096):
        # The workgroup-per-row kernels share the launch counters' id with the one-wave kernels ("rowln_fwd" / "rowln_bwd"), so which
        # of them ran is not observable through the ABI.  What the launcher's predicate (wide_rows_ok: knob 7 on, cols a multiple of
        # 1024 above 1024, 16-byte aligned x / y / w / b, 4-byte aligned mask) reads is asserted here instead: it holds, so they run.
        assert _knob(lib, 7) == 1 and all(t.ptr % 16 == 0 for t in (X, Y, W, B)) and (MASK is None or MASK.ptr % 4 == 0)
    ok(lib.egk_rowln_fwd(S(), P(X), P(W), P(B), P(Y), P(MEAN), P(RSTD), P(MASK), rows, cols, 1e-5, relu, p, 1234, 16, P(OFF), edt(dt)),
       "egk_rowln_fwd")
    G.check()
    if slab:
        same(XO.view, xin, "slab x_out")
    if p > 0:
        m = MASK.view.cpu()
        assert set(m.unique().tolist()) <= {0, 1}, "mask: values other than 0 / 1 (a forgotten element keeps 0xA5)"
        out["mask"] = MASK
    else:
        m = torch.ones(rows, cols, dtype=u8)
    keep = m.double() / (1.0 - p)
    cx, cw, cb = (t.double().clone().requires_grad_(True) for t in (xin, w, b))
    ref = F.layer_norm(cx, (cols,), cw, cb, 1e-5)
    ref = (torch.relu(ref) if relu else ref) * keep
    (ref * dy.double()).sum().backward()
    # tests/test_gpu_kernels.py::test_rowln_fwd_bwd / test_rowln_dropout_mask_semantics / test_rowln_bf16_activations
    close(Y.view, ref.detach().float(), "y", **(OUT16 if dt == bf16 else dict(rtol=1e-4, atol=1e-5)))
    close(MEAN.view, xin.double().mean(1).float(), "mean", **GENERIC)
    close(RSTD.view, (xin.double().var(1, unbiased=False) + 1e-5).rsqrt().float(), "rstd", **GENERIC)
    if halves and rows:
        _tee_check(*halves, Y, "egk_rowln_fwd")
    # ---- backward (on the plain input x: a slab input is a forward matter)
    if slab:
        return out
    DY, DX = G.m("dy", rows, cols, dt, init=dy), G.m("dx", rows, cols, dt)
    slot0 = torch.randn(2 * _pad8(cols), generator=g)
    FL, db_off = _slots(G, "flat_g (dw | db slots)", cols, slot0)
    FL2, _ = _slots(G, "flat_g (dw | db slots, separate reduce)", cols, slot0)
    n_ws = 2 * lib.egk_rowln_bwd_ws_rows(rows) * cols
    WS, WS2 = G.v("ws", n_ws, f32, guard=_ws_guard(cols)), G.v("ws (separate reduce)", n_ws, f32, guard=_ws_guard(cols))   # exactly the header's formula
    DX2 = G.m("dx (separate reduce)", rows, cols, dt)
    if cols in (2048, 3072, 4096):  # (the backward's predicate also reads dy, dx, x and ws)
        assert all(t.ptr % 16 == 0 for t in (DY, DX, DX2, X, WS, WS2))
    ok(lib.egk_rowln_bwd(S(), P(DY), P(X), P(W), P(B), P(MEAN), P(RSTD), P(MASK), P(DX), P(FL), P(FL, db_off), P(WS), rows, cols, relu, p,
                         edt(dt)), "egk_rowln_bwd")
    ok(lib.egk_rowln_bwd(S(), P(DY), P(X), P(W), P(B), P(MEAN), P(RSTD), P(MASK), P(DX2), None, None, P(WS2), rows, cols, relu, p, edt(dt)),
       "egk_rowln_bwd")
    ok(lib.egk_ln_bwd_reduce(S(), P(WS2), P(FL2), P(FL2, db_off), rows, cols, 0), "egk_ln_bwd_reduce")
    G.check()
    c8 = _pad8(cols)
    bf = dt == bf16
    close(DX.view, cx.grad.float(), "dx", **(dict(rtol=2e-2, atol=2e-2) if bf else dict(rtol=1e-3, atol=1e-4)))
    ptol = dict(rtol=2e-2, atol=3e-2 * max(rows, 1) ** 0.5) if bf else dict(rtol=1e-3, atol=1e-3)
    got = FL.view.cpu()
    close(got[:cols], (slot0[:cols].double() + cw.grad).float(), "dw slot", **ptol)
    close(got[c8:c8 + cols], (slot0[c8:c8 + cols].double() + cb.grad).float(), "db slot", **ptol)
    same(got[cols:c8], slot0[cols:c8], "padding behind the dw slot"), same(got[c8 + cols:], slot0[c8 + cols:], "padding behind the db slot")
    same(_bits(DX2), _bits(DX), "dx with dw = db = NULL"), same(_bits(FL2), _bits(FL), "dw / db through egk_ln_bwd_reduce")
    out.update(dx=DX, flat=FL)
    return out


@case("egk_rowln_group_fwd", "egk_rowln_group_bwd", "egk_ln_bwd_reduce", "egk_ln_bwd_reduce_multi", "egk_tee_split_next", variants=[
    dict(row_ptr=(0, 40, 40, 77, 130), cols=256, dt=f32, relu=1, tee=4), dict(row_ptr=(0, 64, 200), cols=1024, dt=bf16, relu=1, tee=None),
    dict(row_ptr=(0, 5, 37, 38), cols=250, dt=f32, relu=0, tee=3), dict(row_ptr=(0, 0), cols=64, dt=f32, relu=1, tee=None)])
def row_layernorm_grouped(lib, ops, G, row_ptr, cols, dt, relu, tee):
    """Row ranges of ONE matrix, each with its own (w, b), a range of 0 rows included; tests/test_gpu_kernels.py::
    test_rowln_grouped_equals_per_range_launches compares with the per-range launches, this with torch directly."""
    g = gen(sum(row_ptr) + cols)
    ng, rows = len(row_ptr) - 1, row_ptr[-1]
    x, dy = r16(torch.randn(rows, cols, generator=g) * 2 + 0.3), r16(torch.randn(rows, cols, generator=g))
    ws_, bs_ = [torch.randn(cols, generator=g) for _ in range(ng)], [torch.randn(cols, generator=g) for _ in range(ng)]
    X, DY = G.m("x", rows, cols, dt, init=x), G.m("dy", rows, cols, dt, init=dy)
    W, B = [G.v(f"w{i}", cols, f32, init=t) for i, t in enumerate(ws_)], [G.v(f"b{i}", cols, f32, init=t) for i, t in enumerate(bs_)]
    RP = (C.c_int32 * (ng + 1))(*row_ptr)
    Y, MEAN, RSTD, DX = G.m("y", rows, cols, dt), G.v("mean", rows), G.v("rstd", rows), G.m("dx", rows, cols, dt)
    halves = _tee(lib, G, rows, cols, tee) if tee is not None else None
    ok(lib.egk_rowln_group_fwd(S(), P(X), ptr_array(W), ptr_array(B), RP, ng, P(Y), P(MEAN), P(RSTD), cols, 1e-5, relu, edt(dt)),
       "egk_rowln_group_fwd")
    max_rows = max(b - a for a, b in zip(row_ptr[:-1], row_ptr[1:]))
    blocks = lib.egk_rowln_bwd_ws_rows(max_rows)
    WS = G.v("ws", ng * blocks * 2 * cols, f32, guard=_ws_guard(cols))      # exactly the header's formula
    ok(lib.egk_rowln_group_bwd(S(), P(DY), P(X), ptr_array(W), ptr_array(B), RP, ng, P(MEAN), P(RSTD), P(DX), P(WS), cols, relu, edt(dt)),
       "egk_rowln_group_bwd")
    G.check()
    out = dict(y=Y, mean=MEAN, rstd=RSTD, dx=DX)
    if max_rows == 0:
        assert bool(Y.is_sentinel().all()) and bool(WS.is_sentinel().all())
        return out
    slot0 = torch.randn(2 * _pad8(cols), generator=g)
    FL = [_slots(G, f"flat_g of range {i}", cols, slot0) for i in range(ng)]
    FM = [_slots(G, f"flat_g of range {i} (one reduce launch)", cols, slot0) for i in range(ng)]
    for i in range(ng):
        ok(lib.egk_ln_bwd_reduce(S(), P(WS, i * blocks * 2 * cols * 4), P(FL[i][0]), P(FL[i][0], FL[i][1]), max_rows, cols, 0), "egk_ln_bwd_reduce")
    wsp = (C.c_void_p * ng)(*[WS.ptr + i * blocks * 2 * cols * 4 for i in range(ng)])
    ok(lib.egk_ln_bwd_reduce_multi(S(), wsp, ptr_array([f[0] for f in FM]), (C.c_void_p * ng)(*[f[0].ptr + f[1] for f in FM]),
                                   (C.c_int32 * ng)(*[max_rows] * ng), (C.c_int32 * ng)(*[cols] * ng), (C.c_int32 * ng)(*[0] * ng), ng),
       "egk_ln_bwd_reduce_multi")
    G.check()
    bf, c8 = dt == bf16, _pad8(cols)
    for i, (a, e) in enumerate(zip(row_ptr[:-1], row_ptr[1:])):
        cx, cw, cb = (t.double().clone().requires_grad_(True) for t in (x[a:e], ws_[i], bs_[i]))
        ref = F.layer_norm(cx, (cols,), cw, cb, 1e-5)
        ref = torch.relu(ref) if relu else ref
        (ref * dy[a:e].double()).sum().backward()
        close(Y.view[a:e], ref.detach().float(), f"y of range {i}", **(OUT16 if bf else dict(rtol=1e-4, atol=1e-5)))  # test_rowln_fwd_bwd
        close(MEAN.view[a:e], x[a:e].double().mean(1).float(), f"mean of range {i}", **GENERIC)
        close(DX.view[a:e], cx.grad.float(), f"dx of range {i}", **(dict(rtol=2e-2, atol=2e-2) if bf else dict(rtol=1e-3, atol=1e-4)))
        ptol = dict(rtol=2e-2, atol=3e-2 * max(e - a, 1) ** 0.5) if bf else dict(rtol=1e-3, atol=1e-3)
        got = FL[i][0].view.cpu()
        close(got[:cols], (slot0[:cols].double() + cw.grad).float(), f"dw of range {i}", **ptol)
        close(got[c8:c8 + cols], (slot0[c8:c8 + cols].double() + cb.grad).float(), f"db of range {i}", **ptol)
        same(got[cols:c8], slot0[cols:c8], "padding behind the dw slot")
        same(_bits(FM[i][0]), _bits(FL[i][0]), f"egk_ln_bwd_reduce_multi, range {i}")   # the header: same summation order, same bits
        out[f"flat{i}"] = FL[i][0]
    if halves:
        _tee_check(*halves, Y, "egk_rowln_group_fwd")
    return out


@case("egk_graphln_fwd", "egk_graphln_bwd", "egk_graphln_stats", "egk_graphln_fwd_apply", "egk_graphln_bwd_stats", "egk_graphln_bwd_apply",
      "egk_graphln_bwd_finish", "egk_ln_bwd_reduce", "egk_tee_split_next", "egk_slab_input_next", variants=[
    dict(rows=300, cols=256, segs=(0, 100, 101, 300), dt=f32, tee=4, slab=False), dict(rows=64, cols=1024, segs=(0, 64), dt=bf16, tee=None, slab=False),
    dict(rows=130, cols=250, segs=(0, 40, 40, 41, 130), dt=f32, tee=3, slab=False), dict(rows=64, cols=1024, segs=(0, 10, 64), dt=f32, tee=0, slab=True),
    dict(rows=200, cols=64, segs=(0, 12, 24, 36, 48, 60, 72, 84, 96, 108, 120, 132, 144, 144, 170, 199, 200), dt=bf16, tee=None, slab=False),
    dict(rows=2500, cols=40, segs=(0, 1000, 2500), dt=f32, tee=None, slab=False), dict(rows=0, cols=64, segs=(0, 0), dt=f32, tee=None, slab=False)])
def graph_layernorm(lib, ops, G, rows, cols, segs, dt, tee, slab):
    """1, 2, 3, 4 and 16 segments, a one-row segment and an empty one; tests/test_gpu_kernels.py::test_graphln_lrelu_fwd_bwd's reference
    (oracle.pyg_ops.graph_layer_norm per segment) and tolerances.  The whole-pass entry points and the separate passes must agree
    bit for bit (the header says they are the same launches)."""
    from oracle import pyg_ops as PO
    g = gen(rows + cols + len(segs))
    n_seg = len(segs) - 1
    x = r16(torch.randn(rows, cols, generator=g) * 1.5 + 0.2)
    w, b, dy = torch.randn(cols, generator=g), torch.randn(cols, generator=g), r16(torch.randn(rows, cols, generator=g))
    xin = x
    X, W, B = G.m("x", rows, cols, dt, init=x), G.v("w", cols, f32, init=w), G.v("b", cols, f32, init=b)
    SP = G.v("seg_ptr", n_seg + 1, i32, init=torch.tensor(segs), poison=rows)
    Y, ST = G.m("y", rows, cols, dt), G.v("stats", 2 * n_seg, f32)
    nws = lib.egk_graphln_ws_bytes(rows, cols, n_seg)
    blocks = lib.egk_graphln_stats_blocks(rows)
    assert nws == blocks * n_seg * 16 + lib.egk_rowln_bwd_ws_rows(rows) * 2 * cols * 4 and nws % 8 == 0
    WS = G.v("ws", nws // 8, f64, guard=_ws_guard(cols))                 # exactly egk_graphln_ws_bytes
    if slab:
        x2, bias = torch.randn(rows, cols, generator=g), torch.randn(cols, generator=g)
        X2, Bs, XO = G.m("slab x2", rows, cols, f32, init=x2), G.v("slab bias", cols, f32, init=bias), G.m("slab x_out", rows, cols, f32)
        ok(lib.egk_slab_input_next(P(X2), P(Bs), P(XO)), "egk_slab_input_next")
        xin = (x + x2) + bias
    halves = _tee(lib, G, rows, cols, tee) if tee is not None else None
    ok(lib.egk_graphln_fwd(S(), P(X), P(W), P(B), P(Y), P(ST), P(SP), n_seg, rows, cols, 1e-5, 0.2, P(WS), edt(dt)), "egk_graphln_fwd")
    G.check()
    out = dict(y=Y)
    if rows == 0:
        return out
    if slab:
        same(XO.view, xin, "slab x_out")
    live = [(s_, a, e) for s_, (a, e) in enumerate(zip(segs[:-1], segs[1:])) if e > a]
    cx, cw, cb = xin.double().clone().requires_grad_(True), w.double().clone().requires_grad_(True), b.double().clone().requires_grad_(True)
    ref = torch.cat([F.leaky_relu(PO.graph_layer_norm(cx[a:e], cw, cb), 0.2) for _, a, e in live])
    (ref * dy.double()).sum().backward()
    bf = dt == bf16
    close(Y.view, ref.detach().float(), "y", **(OUT16 if bf else dict(rtol=1e-4, atol=1e-5)))
    st = ST.view.cpu().view(n_seg, 2)
    for s_, a, e in live:
        seg = xin[a:e].double()
        close(st[s_], torch.stack([seg.mean(), 1.0 / (seg.std(unbiased=False) + 1e-5)]).float(), f"stats of segment {s_}", **GENERIC)
    if halves:
        _tee_check(*halves, Y, "egk_graphln_fwd")
    if slab:
        out["x_out"] = XO
        return out
    # the separate passes: statistics, then the normalising launch from the partials
    PT = G.v("partials", blocks * n_seg * 2, f64)                           # double [egk_graphln_stats_blocks(rows)][n_seg][2]
    Y2, ST2 = G.m("y (separate passes)", rows, cols, dt), G.v("stats (separate passes)", 2 * n_seg, f32)
    ok(lib.egk_graphln_stats(S(), P(X), P(SP), n_seg, rows, cols, P(PT), edt(dt)), "egk_graphln_stats")
    ok(lib.egk_graphln_fwd_apply(S(), P(X), P(W), P(B), P(Y2), P(ST2), P(SP), n_seg, rows, cols, 1e-5, 0.2, P(PT), blocks, edt(dt)),
       "egk_graphln_fwd_apply")
    G.check()
    same(_bits(Y2), _bits(Y), "y of stats + fwd_apply")
    tot = PT.view.cpu().view(blocks, n_seg, 2).sum(0)
    for s_, a, e in live:
        seg = x[a:e].double()
        close(tot[s_], torch.stack([seg.sum(), (seg * seg).sum()]), f"partial sums of segment {s_}", **GENERIC)
    # ---- backward: whole pass, stats + finish, and apply from the sums + the separate reduction
    DY = G.m("dy", rows, cols, dt, init=dy)
    slot0 = torch.randn(2 * _pad8(cols), generator=g)
    DX, (FL, db_off) = G.m("dx", rows, cols, dt), _slots(G, "flat_g (dw | db slots)", cols, slot0)
    WSB = G.v("ws (bwd)", nws // 8, f64, guard=_ws_guard(cols))
    ok(lib.egk_graphln_bwd(S(), P(DY), P(X), P(W), P(B), P(ST), P(DX), P(FL), P(FL, db_off), P(SP), n_seg, rows, cols, 1e-5, 0.2, P(WSB),
                           edt(dt)), "egk_graphln_bwd")
    DX2, (FL2, _) = G.m("dx (stats + finish)", rows, cols, dt), _slots(G, "flat_g (stats + finish)", cols, slot0)
    WS2 = G.v("ws (stats + finish)", nws // 8, f64, guard=_ws_guard(cols))
    ok(lib.egk_graphln_bwd_stats(S(), P(DY), P(X), P(W), P(B), P(ST), P(SP), n_seg, rows, cols, 0.2, P(WS2), edt(dt)), "egk_graphln_bwd_stats")
    ok(lib.egk_graphln_bwd_finish(S(), P(DY), P(X), P(W), P(B), P(ST), P(DX2), P(FL2), P(FL2, db_off), P(SP), n_seg, rows, cols, 1e-5, 0.2,
                                  P(WS2), blocks, P(WS2), edt(dt)), "egk_graphln_bwd_finish")
    DX3, (FL3, _) = G.m("dx (apply)", rows, cols, dt), _slots(G, "flat_g (apply + reduce)", cols, slot0)
    WSC = G.v("ws_col", lib.egk_rowln_bwd_ws_rows(rows) * 2 * cols, f32, guard=_ws_guard(cols))
    PB = G.v("partials (bwd)", blocks * n_seg * 2, f64, init=WS2.view[:blocks * n_seg * 2])
    ok(lib.egk_graphln_bwd_apply(S(), P(DY), P(X), P(W), P(B), P(ST), P(DX3), P(SP), n_seg, rows, cols, 1e-5, 0.2, P(PB), blocks, P(WSC),
                                 edt(dt)), "egk_graphln_bwd_apply")
    ok(lib.egk_ln_bwd_reduce(S(), P(WSC), P(FL3), P(FL3, db_off), rows, cols, 0), "egk_ln_bwd_reduce")
    FL4 = _slots(G, "flat_g (reduce of the whole-pass workspace)", cols, slot0)[0]
    DX4 = G.m("dx (dw = db = NULL)", rows, cols, dt)
    WS4 = G.v("ws (dw = db = NULL)", nws // 8, f64, guard=_ws_guard(cols))
    ok(lib.egk_graphln_bwd(S(), P(DY), P(X), P(W), P(B), P(ST), P(DX4), None, None, P(SP), n_seg, rows, cols, 1e-5, 0.2, P(WS4), edt(dt)),
       "egk_graphln_bwd")
    ok(lib.egk_ln_bwd_reduce(S(), P(WS4), P(FL4), P(FL4, db_off), rows, cols, n_seg), "egk_ln_bwd_reduce")
    G.check()
    c8 = _pad8(cols)
    # test_graphln_lrelu_fwd_bwd (f32); bf16 activations: test_rowln_bf16_activations' gradient tolerances
    dxtol = dict(rtol=2e-2, atol=2e-2) if bf else dict(rtol=1e-3, atol=1e-4)
    ptol = dict(rtol=2e-2, atol=3e-2 * rows ** 0.5) if bf else dict(rtol=1e-3, atol=2e-3)
    for name, dxv, fl in (("whole pass", DX, FL), ("stats + finish", DX2, FL2), ("apply + reduce", DX3, FL3), ("separate reduce", DX4, FL4)):
        close(dxv.view, cx.grad.float(), f"dx ({name})", **dxtol)
        got = fl.view.cpu()
        close(got[:cols], (slot0[:cols].double() + cw.grad).float(), f"dw ({name})", **ptol)
        close(got[c8:c8 + cols], (slot0[c8:c8 + cols].double() + cb.grad).float(), f"db ({name})", **ptol)
        same(got[cols:c8], slot0[cols:c8], f"padding behind the dw slot ({name})")
    same(_bits(DX2), _bits(DX), "dx of bwd_stats + bwd_finish"), same(_bits(FL2), _bits(FL), "dw / db of bwd_stats + bwd_finish")
    same(_bits(DX4), _bits(DX), "dx with dw = db = NULL"), same(_bits(FL4), _bits(FL), "dw / db through egk_ln_bwd_reduce(n_seg)")
    out.update(dx=DX, flat=FL, dx3=DX3, flat3=FL3)
    return out


# =====================================================================================================================
# 5b. the one- and two-logit heads (row reductions with their loss)
# =====================================================================================================================
@case("egk_rowdot_bce", "egk_rowdot_reduce", variants=[dict(rows=333, cols=256, dt=f32), dict(rows=77, cols=1000, dt=bf16), dict(rows=2048, cols=1024, dt=bf16),
                                                       dict(rows=37, cols=250, dt=f32), dict(rows=0, cols=64, dt=f32)])
def rowdot_bce(lib, ops, G, rows, cols, dt):
    """tests/test_gpu_kernels.py::test_one_logit_head_with_bce_in_one_row_pass: reference, tolerances and scales."""
    g = gen(rows + cols)
    f, w = r16(torch.randn(rows, cols, generator=g)), r16(torch.randn(cols, generator=g) * 0.05)
    bias, y = torch.randn(1, generator=g), torch.randint(0, 2, (rows,), generator=g)
    seed = 0.7 / max(rows, 1)
    Fm, W, Bz, Y = G.m("f", rows, cols, dt, init=f), G.v("w", cols, dt, init=w), G.v("bias", 1, f32, init=bias), G.v("y", rows, i64, init=y, poison=1)
    LG, LS, DF = G.v("logits", rows), G.v("loss", rows), G.m("df", rows, cols, dt)
    WS = G.v("ws", lib.egk_rowdot_ws_rows(rows) * (cols + 4), f32, guard=_ws_guard(cols))   # exactly egk_rowdot_ws_rows(rows) * (cols + 4)
    slot0 = torch.randn(_pad8(cols) + 8, generator=g)
    FL = G.v("flat_g (dw slot | db slot)", _pad8(cols) + 8, f32, init=slot0)
    ok(lib.egk_rowdot_bce(S(), P(Fm), P(W), P(Bz), P(Y), P(LG), P(LS), P(DF), P(WS), rows, cols, seed, edt(dt)), "egk_rowdot_bce")
    ok(lib.egk_rowdot_reduce(S(), P(WS), P(FL), P(FL, _pad8(cols) * 4), rows, cols), "egk_rowdot_reduce")
    LG2, LS2 = G.v("logits (forward only)", rows), G.v("loss (forward only)", rows)
    ok(lib.egk_rowdot_bce(S(), P(Fm), P(W), P(Bz), P(Y), P(LG2), P(LS2), None, None, rows, cols, seed, edt(dt)), "egk_rowdot_bce")
    G.check()
    cf, cW, cb = f.double().clone().requires_grad_(True), w.double().clone().requires_grad_(True), bias.double().clone().requires_grad_(True)
    z = cf @ cW + cb
    ref = F.binary_cross_entropy_with_logits(z, y.double(), reduction="none")
    ref.backward(torch.full_like(ref, seed))
    f32m = dt == f32
    lt = dict(rtol=1e-4, atol=1e-4) if f32m else dict(rtol=1e-2, atol=2e-2)
    close(LG.view, z.detach().float(), "logits", **lt), close(LS.view, ref.detach().float(), "loss", **lt)
    same(LG2.view, LG.view, "logits (forward only)"), same(LS2.view, LS.view, "loss (forward only)")
    out = dict(logits=LG, loss=LS, df=DF, flat=FL)
    if rows == 0:
        same(FL.view, slot0, "flat_g of an empty launch")
        return out
    gs, wsc = float(cf.grad.abs().max()), float(cW.grad.abs().max())
    c8, got = _pad8(cols), FL.view.cpu().double()
    assert (DF.view.float().cpu().double() - cf.grad).abs().max() <= (1e-5 if f32m else 1.5e-2) * gs, "df"
    assert (got[:cols] - slot0[:cols].double() - cW.grad).abs().max() <= (2e-5 if f32m else 1.5e-2) * wsc + 1e-6, "dw"
    assert abs(float(got[c8] - slot0[c8].double() - cb.grad[0])) <= (2e-5 if f32m else 1e-2) * max(1.0, abs(float(cb.grad)) * 100), "db"
    same(FL.view[cols:c8], slot0[cols:c8], "padding behind the dw slot"), same(FL.view[c8 + 1:], slot0[c8 + 1:], "behind the db word")
    return out


@case("egk_rowdot_ce2", "egk_rowdot_ce2_multi", variants=[
    dict(n_src=1, rows=1, cols=264, dt=f32, average=0, sm=0.1, entry="single"), dict(n_src=1, rows=256, cols=1024, dt=bf16, average=0, sm=0.0, entry="single"),
    dict(n_src=3, rows=256, cols=1024, dt=bf16, average=1, sm=0.1, entry="phases"), dict(n_src=2, rows=37, cols=250, dt=f32, average=0, sm=0.1, entry="multi"),
    dict(n_src=4, rows=1, cols=64, dt=f32, average=1, sm=0.0, entry="phases"), dict(n_src=2, rows=0, cols=64, dt=f32, average=1, sm=0.0, entry="multi")])
def rowdot_ce2(lib, ops, G, n_src, rows, cols, dt, average, sm, entry):
    """tests/test_gpu_kernels.py::test_two_logit_head_with_cross_entropy_in_one_launch / test_two_logit_heads_of_several_sources_in_one_
    launch: reference, tolerances and scales; 1 row and egk_rowdot_ce2_max_rows() rows, phases 1 and 2 as separate calls."""
    assert lib.egk_rowdot_ce2_max_rows() == 256
    g = gen(n_src * 7 + rows + cols)
    fs = [r16(torch.randn(rows, cols, generator=g)) for _ in range(n_src)]
    Ws = [r16(torch.randn(2, cols, generator=g) * 0.05) for _ in range(n_src)]
    bs = [torch.randn(2, generator=g) for _ in range(n_src)]
    y = torch.randint(0, 2, (rows,), generator=g)
    y[3::7] = -1
    seed = 1.3 / max(rows, 1)
    Fm = [G.m(f"f{k}", rows, cols, dt, init=t) for k, t in enumerate(fs)]
    Wm = [G.m(f"w{k}", 2, cols, dt, init=t) for k, t in enumerate(Ws)]
    Bz = [G.v(f"bias{k}", 2, f32, init=t) for k, t in enumerate(bs)]
    Y = G.v("y", rows, i64, init=y, poison=1)
    LG, LS, GWS = G.m("logits", rows, 2, f32), G.v("loss", rows), G.m("gws", rows, 2, f32)       # gws: float [rows][2]
    DF = [G.m(f"df{k}", rows, cols, dt) if k != 1 else None for k in range(n_src)]              # (source 1 wants no df)
    dw0 = [torch.randn(2, cols, generator=g) for _ in range(n_src)]
    db0 = [torch.randn(2, generator=g) for _ in range(n_src)]
    DW, DB = [G.m(f"dw{k}", 2, cols, f32, init=t) for k, t in enumerate(dw0)], [G.v(f"db{k}", 2, f32, init=t) for k, t in enumerate(db0)]
    if entry == "single":
        ok(lib.egk_rowdot_ce2(S(), P(Fm[0]), P(Wm[0]), P(Bz[0]), P(Y), P(LG), P(LS), P(DF[0]), P(DW[0]), P(DB[0]), P(GWS), rows, cols, sm, seed,
                              edt(dt)), "egk_rowdot_ce2")
    else:
        for phase in ((1, 2) if entry == "phases" else (0,)):
            ok(lib.egk_rowdot_ce2_multi(S(), n_src, ptr_array(Fm), ptr_array(Wm), ptr_array(Bz), P(Y), P(LG), P(LS), ptr_array(DF), ptr_array(DW),
                                        ptr_array(DB), P(GWS), rows, cols, average | (phase << 1), sm, seed, edt(dt)), "egk_rowdot_ce2_multi")
            G.check()
            if phase == 1:  # the row launch only: no parameter gradient yet
                for k in range(n_src):
                    same(DW[k].view, dw0[k], f"dw{k} after phase 1"), same(DB[k].view, db0[k], f"db{k} after phase 1")
    G.check()
    out = dict(logits=LG, loss=LS, gws=GWS, **{f"dw{k}": DW[k] for k in range(n_src)}, **{f"df{k}": d for k, d in enumerate(DF) if d is not None})
    if rows == 0:
        return out
    cf, cW, cb = ([t.double().clone().requires_grad_(True) for t in ts] for ts in (fs, Ws, bs))
    zs = torch.stack([f_ @ W_.t() + b_ for f_, W_, b_ in zip(cf, cW, cb)])
    z = zs.mean(0) if average else zs.sum(0)
    ref = F.cross_entropy(z, y, reduction="none", ignore_index=-1, label_smoothing=sm)
    ref.backward(torch.full_like(ref, seed))
    f32m = dt == f32
    lt = dict(rtol=1e-4, atol=1e-4) if f32m else dict(rtol=1e-2, atol=3e-2 if n_src > 1 else 2e-2)
    close(LG.view, z.detach().float(), "logits", **lt), close(LS.view, ref.detach().float(), "loss", **lt)
    for k in range(n_src):
        gs, wsc = float(cf[k].grad.abs().max()), float(cW[k].grad.abs().max())
        if DF[k] is not None:
            assert (DF[k].view.float().cpu().double() - cf[k].grad).abs().max() <= (1e-5 if f32m else 1.5e-2) * gs + 1e-12, f"df{k}"
        assert (DW[k].view.cpu().double() - dw0[k].double() - cW[k].grad).abs().max() <= (3e-5 if f32m else 1.5e-2) * wsc + 1e-6, f"dw{k}"
        assert (DB[k].view.cpu().double() - db0[k].double() - cb[k].grad).abs().max() <= \
            (3e-5 if f32m else 1e-2) * max(1.0, float(cb[k].grad.abs().max()) * 100), f"db{k}"
    refused(lib.egk_rowdot_ce2_multi(S(), n_src, ptr_array(Fm), ptr_array(Wm), ptr_array(Bz), P(Y), P(LG), P(LS), ptr_array(DF), ptr_array(DW),
                                     ptr_array(DB), P(GWS), 257, cols, average, sm, seed, edt(dt)), "at most 256 rows")
    return out


# =====================================================================================================================
# 1. contractions
# =====================================================================================================================
def _prof_launches(lib):
    """{kernel name: launches} of the library's launch counters."""
    out = {}
    name, n, ms, fl, by = C.create_string_buffer(64), C.c_int64(), C.c_double(), C.c_double(), C.c_double()
    for i in range(lib.egk_prof_count()):
        assert lib.egk_prof_get(i, name, 64, C.byref(n), C.byref(ms), C.byref(fl), C.byref(by)) == 0
        if n.value:
            out[name.value.decode()] = n.value
    return out


class _counted:
    """Launch counters around a block: ``.names`` = the kernels that ran (egk_prof_reset / egk_prof_get)."""

    def __init__(self, lib):
        self.lib, self.names = lib, {}

    def __enter__(self):
        self.lib.egk_prof_enable(1)
        self.lib.egk_prof_reset()
        return self

    def __exit__(self, *a):
        torch.cuda.synchronize()
        self.names = _prof_launches(self.lib)
        self.lib.egk_prof_enable(0)
        self.lib.egk_prof_reset()


def _gemm_problem(G, tag, g, M, N, Ks, tA, tB, odt, compute, cdt, rdt=None, pads=(0, 0, 0, 0), bias=False, act=0, alpha=1.0, acc=False,
                  dbias=False, scale=1.0, guard_rows=GUARD_ROWS):
    """Operands (every K source), C (with initial values when accumulated into), residual, bias, the dbias slot -- all guarded --
    and the f64 reference of  act(alpha * sum_s op(A_s) op(B_s)^T + C0 + bias) + residual  on the operands as the MFMA type
    sees them (bf16-rounded for EGK_COMPUTE_BF16)."""
    pa, pb, pc, pr = pads
    srcs, accum = [], torch.zeros(M, N, dtype=f64)
    rnd = (lambda t: t.to(bf16).double()) if compute == BF16 else (lambda t: t.double())
    for i, K in enumerate(Ks):
        a, b = torch.randn(M, K, generator=g) * scale, torch.randn(N, K, generator=g) * scale
        if odt == bf16:
            a, b = r16(a), r16(b)
        A = G.m(f"{tag}A{i}", K if tA else M, M if tA else K, odt, pad=pa, init=a.t() if tA else a, guard_rows=guard_rows)
        B = G.m(f"{tag}B{i}", K if tB else N, N if tB else K, odt, pad=pb, init=b.t() if tB else b, guard_rows=guard_rows)
        srcs.append((A, B, K))
        accum += (rnd(a).to(DEV) @ rnd(b).to(DEV).t()).cpu() if M * N * K > 1 << 30 else rnd(a) @ rnd(b).t()   # (big: torch's f64 matmul on the device)
        if i == 0:
            a0 = a
    c0 = torch.randn(M, N, generator=g) if acc else None
    Cm = G.m(tag + "C", M, N, cdt, pad=pc, init=c0, guard_rows=guard_rows)
    ref = alpha * accum + (c0.double() if acc else 0)
    Bs = None
    if bias:
        bv = torch.randn(N, generator=g)
        Bs = G.v(tag + "bias", N, f32, init=bv)
        ref = ref + bv.double()
    if act:
        ref = torch.relu(ref)
    R = None
    if rdt is not None:
        rv = r16(torch.randn(M, N, generator=g))
        R = G.m(tag + "residual", M, N, rdt, pad=pr, init=rv, guard_rows=guard_rows)
        ref = ref.float().double() + rv.double()
    DBs, db_ref = None, None
    if dbias:
        d0 = torch.randn(M, generator=g)
        DBs = G.v(tag + "dbias slot", M, f32, init=d0)
        db_ref = (d0.double() + rnd(a0).sum(1)).float()
    return dict(M=M, N=N, srcs=srcs, C=Cm, bias=Bs, R=R, dbias=DBs, ref=ref.float(), db_ref=db_ref, tA=tA, tB=tB, odt=odt, compute=compute,
                cdt=cdt, rdt=rdt, act=act, alpha=alpha, acc=acc)


def _gemm_desc(pr, d=None):
    from egopack_amd import _lib
    d = _lib.GemmDesc() if d is None else d
    d.M, d.N = pr["M"], pr["N"]
    s = pr["srcs"]
    d.A1, d.B1, d.lda1, d.ldb1, d.K1 = s[0][0].ptr, s[0][1].ptr, s[0][0].ld, s[0][1].ld, s[0][2]
    if len(s) > 1:
        d.A2, d.B2, d.lda2, d.ldb2, d.K2 = s[1][0].ptr, s[1][1].ptr, s[1][0].ld, s[1][1].ld, s[1][2]
    d.n_extra = max(len(s) - 2, 0)
    for i, (A, B, K) in enumerate(s[2:]):
        d.xA[i], d.xB[i], d.xlda[i], d.xldb[i], d.xK[i] = A.ptr, B.ptr, A.ld, B.ld, K
    d.transA, d.transB = int(pr["tA"]), int(pr["tB"])
    d.a_dtype = d.b_dtype = edt(pr["odt"])
    d.compute = pr["compute"]
    d.C, d.ldc, d.c_dtype = pr["C"].ptr, pr["C"].ld, edt(pr["cdt"])
    d.accumulate, d.act, d.alpha = int(pr["acc"]), pr["act"], pr["alpha"]
    d.bias = pr["bias"].ptr if pr["bias"] is not None else None
    if pr["R"] is not None:
        d.residual, d.ldr, d.r_dtype = pr["R"].ptr, pr["R"].ld, edt(pr["rdt"])
    d.dbias = pr["dbias"].ptr if pr["dbias"] is not None else None
    d.splitk = 1
    return d


def _gemm_tol(pr, deep=False):
    if pr["compute"] == F32:   # test_gemm_layouts / test_gemm_splitk_matches_single_pass (deep K, slabs)
        return dict(rtol=1e-4, atol=5e-4) if deep else dict(rtol=1e-4, atol=1e-4)
    if pr["cdt"] == bf16:      # test_gemm_bf16_memory_operands
        return OUT16
    return dict(rtol=2e-3, atol=5e-3) if deep else dict(rtol=1e-3, atol=1e-3)


_NN, _NT, _TT, _TN = (False, False), (False, True), (True, True), (True, False)
_GEMM = [  # M, N, Ks, layout, operand type, compute, C type, residual type, pads (A, B, C, residual), pipeline knob, extras
    # the generic kernels: K not a multiple of 64 / 32, ragged everything, N % 4 != 0 (c_vec false), leading dimensions that break alignment
    dict(M=130, N=70, Ks=(40,), lay=_NN, odt=f32, cmp=F32, cdt=f32, rdt=f32, pads=(4, 4, 4, 4), pipe=1, bias=True),
    dict(M=257, N=129, Ks=(144,), lay=_NT, odt=f32, cmp=F32, cdt=f32, rdt=f32, pads=(1, 3, 3, 1), pipe=1, bias=True, act=1),
    dict(M=33, N=1, Ks=(32,), lay=_TT, odt=f32, cmp=F32, cdt=f32, rdt=None, pads=(3, 3, 1, 0), pipe=1, acc=True, alpha=0.5),
    dict(M=64, N=7, Ks=(32, 40), lay=_TN, odt=f32, cmp=F32, cdt=f32, rdt=None, pads=(4, 4, 1, 0), pipe=1),
    dict(M=130, N=70, Ks=(40,), lay=_NN, odt=f32, cmp=BF16, cdt=f32, rdt=f32, pads=(4, 4, 2, 4), pipe=1, bias=True, id="generic bf16 kernel on f32 operands"),
    dict(M=257, N=129, Ks=(144,), lay=_TT, odt=bf16, cmp=BF16, cdt=bf16, rdt=bf16, pads=(8, 8, 3, 5), pipe=1, bias=True, want="gemm_bf16_generic"),
    dict(M=300, N=256, Ks=(200,), lay=_NT, odt=bf16, cmp=BF16, cdt=f32, rdt=None, pads=(1, 1, 0, 0), pipe=1, want="gemm_bf16_generic"),
    dict(M=128, N=128, Ks=(64,), lay=_NN, odt=bf16, cmp=BF16, cdt=f32, rdt=None, pads=(0, 0, 0, 0), pipe=0, want="gemm_bf16_generic"),
    dict(M=64, N=48, Ks=(0,), lay=_NN, odt=f32, cmp=F32, cdt=f32, rdt=None, pads=(0, 0, 4, 0), pipe=1, bias=True, act=1, id="K=0 stores epilogue(0)"),
    dict(M=64, N=48, Ks=(0,), lay=_NN, odt=bf16, cmp=BF16, cdt=bf16, rdt=None, pads=(0, 0, 8, 0), pipe=1, bias=True, id="K=0 bf16"),
    dict(M=0, N=48, Ks=(64,), lay=_NN, odt=bf16, cmp=BF16, cdt=f32, rdt=None, pads=(0, 0, 0, 0), pipe=1, id="M=0"),
    # the exact-f32 pipelined kernel: 128- and 96-row tiles (egk_gemm_set_pipeline 3 / 8), all four layouts, split-K
    dict(M=304, N=200, Ks=(256,), lay=_NN, odt=f32, cmp=F32, cdt=f32, rdt=f32, pads=(4, 4, 4, 4), pipe=3, bias=True, want="gemm_f32_nn"),
    dict(M=304, N=200, Ks=(256,), lay=_NN, odt=f32, cmp=F32, cdt=f32, rdt=None, pads=(4, 4, 3, 0), pipe=8, want="gemm_f32_nn", id="f32 96-row tiles"),
    dict(M=264, N=136, Ks=(128, 192), lay=_NT, odt=f32, cmp=F32, cdt=f32, rdt=None, pads=(4, 8, 4, 0), pipe=8, act=1, want="gemm_f32_nt"),
    dict(M=200, N=136, Ks=(512,), lay=_TT, odt=f32, cmp=F32, cdt=f32, rdt=None, pads=(4, 4, 4, 0), pipe=1, acc=True, splitk=4, dbias=True, want="gemm_f32_tt"),
    dict(M=200, N=131, Ks=(512,), lay=_TT, odt=f32, cmp=F32, cdt=f32, rdt=None, pads=(4, 2, 1, 0), pipe=1, acc=True, splitk=2, dbias=True,
         plain=False, id="f32 dW, unaligned B: generic kernel + column-sum route"),   # (contiguous, the fused route would run: other bits)
    dict(M=136, N=200, Ks=(128,), lay=_TN, odt=f32, cmp=F32, cdt=f32, rdt=None, pads=(4, 4, 4, 0), pipe=1, want="gemm_f32_tn"),
] + [  # every bf16 tile variant forced, ragged M and N for its tile height (64 / 96 / 128 / 192 / 256); c_vec / r_vec made false by a
       # leading dimension of C / the residual that is not a multiple of 4 (a transposed B needs N % 8 == 0 to stay on these kernels)
    dict(M=M, N=N, Ks=Ks, lay=lay, odt=bf16, cmp=BF16, cdt=cdt, rdt=rdt, pads=pads, pipe=pipe, want=want, **extra)
    for pipe, want, M, N, Ks, lay, cdt, rdt, pads, extra in [
        (3, "gemm_bf16_nn", 304, 200, (256,), _NN, f32, f32, (8, 8, 4, 4), dict(bias=True)),
        (3, "gemm_bf16_tt", 264, 136, (128, 192), _TT, f32, None, (8, 8, 3, 0), dict(acc=True, alpha=0.5)),
        (3, "gemm_bf16_tn", 136, 200, (64,), _TN, bf16, bf16, (8, 8, 8, 8), dict(act=1, bias=True)),
        (5, "gemm_bf16_nt_g2", 304, 200, (256,), _NT, bf16, None, (8, 8, 7, 0), dict()),
        (5, "gemm_bf16_tt_g2", 200, 136, (512,), _TT, f32, None, (8, 8, 4, 0), dict(acc=True, dbias=True)),
        (8, "gemm_bf16_nn_r96", 250, 200, (128,), _NN, f32, bf16, (8, 8, 4, 8), dict(bias=True, act=1)),
        (8, "gemm_bf16_nt_r96", 97, 136, (64, 64, 64), _NT, bf16, None, (8, 8, 5, 0), dict()),
        (11, "gemm_bf16_nn_r64", 130, 200, (128,), _NN, f32, None, (8, 8, 4, 0), dict(bias=True)),
        (11, "gemm_bf16_nt_r64", 65, 72, (64,), _NT, bf16, bf16, (8, 8, 1, 3), dict()),
        (12, "gemm_bf16_nn_g2", 130, 200, (256,), _NN, f32, None, (8, 8, 4, 0), dict()),
        (16, "gemm_bf16_nn_r192", 400, 200, (256,), _NN, bf16, None, (8, 8, 8, 0), dict(bias=True, loaders=1)),
        (16, "gemm_bf16_nt_r192", 193, 136, (128,), _NT, f32, f32, (8, 8, 1, 4), dict(loaders=0)),
        (16, "gemm_bf16_nn_r192", 400, 200, (512,), _NN, f32, None, (8, 8, 4, 0), dict(loaders=0)),
        (7, "gemm_bf16_nn_t256", 512, 256, (128,), _NN, f32, f32, (8, 8, 4, 4), dict(bias=True)),
        (7, "gemm_bf16_tt_t256", 256, 512, (128,), _TT, bf16, None, (8, 8, 8, 0), dict(act=1)),
        (7, "gemm_bf16_nt", 300, 256, (128,), _NT, f32, None, (8, 8, 4, 0), dict(id="256-row tile refused (ragged M): 128-row tiles")),
        (15, "gemm_bf16_nt_t256", 384, 512, (128,), _NT, f32, None, (8, 8, 4, 0), dict(bias=True)),
        (15, "gemm_bf16_nn_t256", 192, 256, (64, 64), _NN, bf16, bf16, (8, 8, 8, 8), dict()),
        # split-K on the pipelined kernels: the reduce launch must honour ldc, f32 and bf16 C, vector and scalar path
        (1, "gemm_splitk_reduce", 128, 256, (1024,), _TT, f32, None, (8, 8, 4, 0), dict(acc=True, splitk=4)),
        (1, "gemm_splitk_reduce", 130, 131, (512,), _TT, f32, None, (8, 8, 1, 0), dict(acc=True, splitk=2, dbias=True)),
        (3, "gemm_splitk_reduce", 200, 136, (512,), _NN, bf16, bf16, (8, 8, 8, 8), dict(splitk=3, bias=True, act=1)),
        (1, "gemm_splitk_reduce", 128, 256, (512, 512), _NT, f32, f32, (8, 8, 3, 4), dict(splitk=2, alpha=0.5)),
        # two K sources and the extra sources (six in all)
        (1, "gemm_bf16", 130, 200, (64, 128, 64, 64, 128, 64), _NN, f32, None, (8, 8, 4, 0), dict(bias=True)),
        (1, "gemm_bf16", 200, 136, (64, 64, 64), _TT, f32, None, (8, 8, 4, 0), dict(acc=True)),
    ]
]


@case("egk_gemm",
      variants=[dict(v, id=v.get("id") or f"{v.get('want', 'generic')}-pipe{v['pipe']}-{v['M']}x{v['N']}x{_fmt(v['Ks'])}-{i}") for i, v in enumerate(_GEMM)])
def gemm(lib, ops, G, M, N, Ks, lay, odt, cmp, cdt, rdt, pads, pipe, bias=False, act=0, alpha=1.0, acc=False, splitk=1, dbias=False, want=None,
         loaders=None):
    from egopack_amd import _lib
    g = gen(M * 1000 + N * 10 + sum(Ks) + pipe)
    pr = _gemm_problem(G, "", g, M, N, Ks, lay[0], lay[1], odt, cmp, cdt, rdt, pads, bias, act, alpha, acc, dbias)
    d = _gemm_desc(pr)
    d.splitk = splitk
    need = lib.egk_gemm_ws_bytes(C.byref(d))
    assert need >= (splitk * M * N * 4 if splitk > 1 else 0) and need % 4 == 0
    WS = G.v("ws", need // 4, f32, guard=max(GUARD_ELEMS, 2 * N)) if need else None        # exactly egk_gemm_ws_bytes
    d.ws, d.ws_bytes = (WS.ptr if WS else None), need
    prev = lib.egk_gemm_set_pipeline(pipe)
    if loaders is not None:
        # (the 192-row tile with and without its loader waves shares one counter id, "gemm_bf16_n?_r192", and the 870 / 871 switch
        #  returns the pipeline setting, not its own: which of the two instantiations ran is not observable through the ABI -- both
        #  switch positions are run, at K tiles on both sides of the launcher's ``nkt_slab >= 4``)
        lib.egk_gemm_set_pipeline(870 + loaders)
    try:
        if splitk > 1 and sum(Ks):   # one byte less than the slabs need: refused, nothing launched
            d.ws_bytes = splitk * M * N * 4 - 1
            refused(lib.egk_gemm(S(), C.byref(d)), "workspace too small")
            G.check()
            assert acc or bool(pr["C"].is_sentinel().all()), "a refused launch wrote C"
            d.ws_bytes = need
        with _counted(lib) as ran:
            ok(lib.egk_gemm(S(), C.byref(d)), "egk_gemm")
    finally:
        lib.egk_gemm_set_pipeline(871)
        lib.egk_gemm_set_pipeline(prev)
    G.check()
    if want and M and N:
        assert any(k.startswith(want) for k in ran.names), f"expected a {want}* launch, the counters show {ran.names}"
    if splitk > 1 and sum(Ks):
        assert "gemm_splitk_reduce" in ran.names, ran.names
    deep = splitk > 1
    close(pr["C"].view, pr["ref"], "C", **_gemm_tol(pr, deep))
    out = dict(C=pr["C"])
    if dbias:
        # test_gemm_dw_with_fused_bias_gradient (bf16) / test_gemm_f32_dw_with_fused_bias_gradient (f32)
        close(pr["dbias"].view, pr["db_ref"], "dbias", **(dict(rtol=1e-3, atol=2e-2) if cmp == BF16 else dict(rtol=1e-5, atol=1e-3)))
        out["dbias"] = pr["dbias"]
    return out


@case("egk_gemm", "egk_gemm_reduce_slabs", "egk_gemm_defer_reduce_next", "egk_rowln_fwd", "egk_slab_input_next",
      variants=[dict(M=130, N=256, K=512, pc=4), dict(M=64, N=136, K=1024, pc=1)])
def gemm_deferred_reduce(lib, ops, G, M, N, K, pc):
    """egk_gemm_defer_reduce_next: the split launch leaves its two slabs in ws = [2][M][N] (exactly that, guarded) and writes no C;
    egk_gemm_reduce_slabs sums them into a C with its own leading dimension; a slab-aware row kernel reads them directly."""
    g = gen(M + N + K)
    pr = _gemm_problem(G, "", g, M, N, (K,), False, False, bf16, BF16, f32, None, (8, 8, pc, 0), bias=True)
    d = _gemm_desc(pr)
    d.splitk, d.bias = 2, None
    need = lib.egk_gemm_ws_bytes(C.byref(d))
    assert need == 2 * M * N * 4
    WS = G.v("ws (slabs)", need // 4, f32)
    d.ws, d.ws_bytes = WS.ptr, need
    ok(lib.egk_gemm_defer_reduce_next(1), "egk_gemm_defer_reduce_next")
    try:
        with _counted(lib) as ran:
            ok(lib.egk_gemm(S(), C.byref(d)), "egk_gemm")
    finally:
        lib.egk_gemm_defer_reduce_next(0)
    G.check()
    assert "gemm_splitk_reduce" not in ran.names and bool(pr["C"].is_sentinel().all()), "a deferred reduce wrote C"
    ok(lib.egk_gemm_reduce_slabs(S(), P(WS), 2, M, N, P(pr["bias"]), P(pr["C"]), pr["C"].ld), "egk_gemm_reduce_slabs")
    G.check()
    close(pr["C"].view, pr["ref"], "C", rtol=2e-3, atol=5e-3)           # test_gemm_splitk_matches_single_pass
    refused(lib.egk_gemm_reduce_slabs(S(), P(WS), 2, M, N, P(pr["bias"]), P(pr["C"]), N - 1), "bad arguments")
    out = dict(C=pr["C"])
    if N % 4 == 0:  # the slabs as the input of a row LayerNorm: x = slab 0, x2 = slab 1, + bias, stored to x_out
        w, b = torch.randn(N, generator=g), torch.randn(N, generator=g)
        W, B = G.v("ln w", N, f32, init=w), G.v("ln b", N, f32, init=b)
        XO, Y, MEAN, RSTD = G.m("x_out", M, N, f32), G.m("y", M, N, f32), G.v("mean", M), G.v("rstd", M)
        ok(lib.egk_slab_input_next(P(WS, M * N * 4), P(pr["bias"]), P(XO)), "egk_slab_input_next")
        ok(lib.egk_rowln_fwd(S(), P(WS), P(W), P(B), P(Y), P(MEAN), P(RSTD), None, M, N, 1e-5, 0, 0.0, 0, 0, None, F32), "egk_rowln_fwd")
        G.check()
        same(XO.view, pr["C"].view, "x_out of the slab input against the reduce launch")   # the header: the same bits
        close(Y.view, F.layer_norm(pr["C"].view.cpu().double(), (N,), w.double(), b.double(), 1e-5).float(), "y", rtol=1e-4, atol=1e-5)
        out.update(x_out=XO, y=Y)
    return out


@case("egk_gemm", "egk_gemm_stats_blocks", "egk_graphln_fwd_apply", variants=[
    dict(M=1000, H=256, K=512, segs=(0, 300, 1000), pipe=1, pc=8), dict(M=600, H=256, K=256, segs=(0, 200, 600), pipe=8, pc=0),
    dict(M=1000, H=256, K=512, segs=(0, 300, 1000), pipe=11, pc=8), dict(M=768, H=256, K=256, segs=(0, 384, 768), pipe=16, pc=8)])
def gemm_segment_statistics(lib, ops, G, M, H, K, segs, pipe, pc):
    """st_mode 1 and 2 (tests/test_gpu_kernels.py::test_gemm_epilogue_segment_statistics_feed_graph_layernorm): st_ws holds exactly
    egk_gemm_stats_blocks(desc) * st_nseg * 2 doubles, st_x has its own leading dimension."""
    g = gen(M + pipe)
    n_seg, min_rows = len(segs) - 1, min(b - a for a, b in zip(segs, segs[1:]))
    SP = G.v("st_seg_ptr", n_seg + 1, i32, init=torch.tensor(segs), poison=M)
    prev = lib.egk_gemm_set_pipeline(pipe)
    try:
        pr = _gemm_problem(G, "fwd ", g, M, H, (K,), False, False, bf16, BF16, bf16, None, (8, 8, pc, 0), bias=True, scale=0.3)
        d = _gemm_desc(pr)
        d.st_mode, d.st_nseg, d.st_min_seg_rows, d.st_seg_ptr = 1, n_seg, min_rows, SP.ptr
        blocks = lib.egk_gemm_stats_blocks(C.byref(d))
        assert blocks > 0, "the rows-epilogue variants take the statistics at these shapes"
        ST = G.v("st_ws", blocks * n_seg * 2, f64)
        d.st_ws = ST.ptr
        ok(lib.egk_gemm(S(), C.byref(d)), "egk_gemm (st_mode 1)")
        G.check()
        close(pr["C"].view, pr["ref"], "C", **OUT16)
        o64 = pr["C"].view.double().cpu()
        part = ST.view.cpu().view(blocks, n_seg, 2).sum(0)
        for s_ in range(n_seg):
            blk = o64[segs[s_]:segs[s_ + 1]]
            close(part[s_], torch.stack([blk.sum(), (blk * blk).sum()]), f"sums of segment {s_}", rtol=1e-6, atol=1e-3)
        # the LayerNorm's normalising launch from these partials
        lw, lb = torch.randn(H, generator=g) * 0.5 + 1, torch.randn(H, generator=g) * 0.2
        LW, LB = G.v("ln w", H, f32, init=lw), G.v("ln b", H, f32, init=lb)
        Xc = G.m("x (contiguous copy of C)", M, H, bf16, init=pr["C"].view)
        Y, STATS = G.m("y", M, H, bf16), G.v("stats", 2 * n_seg, f32)
        ok(lib.egk_graphln_fwd_apply(S(), P(Xc), P(LW), P(LB), P(Y), P(STATS), P(SP), n_seg, M, H, 1e-5, 0.2, P(ST), blocks, BF16),
           "egk_graphln_fwd_apply")
        G.check()
        from oracle import pyg_ops as PO
        xs = pr["C"].view.float().cpu()
        yref = torch.cat([F.leaky_relu(PO.graph_layer_norm(xs[a:e], lw, lb), 0.2) for a, e in zip(segs[:-1], segs[1:])])
        close(Y.view, yref, "y from the epilogue's partials", **OUT16)
        # st_mode 2: dy of that LayerNorm from a dX-shaped contraction; st_x = the LayerNorm's input with its own leading dimension
        pr2 = _gemm_problem(G, "bwd ", g, M, H, (K,), False, True, bf16, BF16, bf16, None, (8, 8, pc, 0), scale=0.3)
        d2 = _gemm_desc(pr2)
        d2.st_mode, d2.st_nseg, d2.st_min_seg_rows, d2.st_seg_ptr = 2, n_seg, min_rows, SP.ptr
        d2.st_x, d2.st_ldx, d2.st_stats, d2.st_w, d2.st_b, d2.st_slope = pr["C"].ptr, pr["C"].ld, STATS.ptr, LW.ptr, LB.ptr, 0.2
        blocks2 = lib.egk_gemm_stats_blocks(C.byref(d2))
        assert blocks2 > 0
        ST2 = G.v("st_ws (mode 2)", blocks2 * n_seg * 2, f64)
        d2.st_ws = ST2.ptr
        ok(lib.egk_gemm(S(), C.byref(d2)), "egk_gemm (st_mode 2)")
        G.check()
    finally:
        lib.egk_gemm_set_pipeline(prev)
    close(pr2["C"].view, pr2["ref"], "dy", **OUT16)
    x64, dy64 = pr["C"].view.double().cpu(), pr2["C"].view.double().cpu()
    stats = STATS.view.double().cpu().view(n_seg, 2)
    part2 = ST2.view.cpu().view(blocks2, n_seg, 2).sum(0)
    for s_ in range(n_seg):
        xs_, ds = x64[segs[s_]:segs[s_ + 1]], dy64[segs[s_]:segs[s_ + 1]]
        xh = (xs_ - stats[s_, 0]) * stats[s_, 1]
        dxh = ds * torch.where(xh * lw.double() + lb.double() > 0, 1.0, 0.2) * lw.double()
        close(part2[s_], torch.stack([dxh.sum(), (dxh * xh).sum()]), f"backward sums of segment {s_}", rtol=2e-4, atol=5e-2)
    return dict(C=pr["C"], st=ST, y=Y, dy=pr2["C"], st2=ST2)


@case("egk_gemm_grouped", variants=[
    dict(lay=_TT, sizes=((256, 128, 64), (192, 256, 64), (64, 128, 128), (448, 128, 64), (136, 136, 64), (128, 128, 64), (200, 72, 128), (64, 64, 64)),
         odt=bf16, pipe=1, dbias=True, want="gemm_bf16_group_tt", id="eight dW problems"),
    dict(lay=_NN, sizes=((64, 1024, 1024), (2048, 1024, 1024), (2048, 1024, 1024)), odt=bf16, pipe=1, dbias=False, want="gemm_bf16_group_nn",
         id="192-row tiles with loader waves"),
    dict(lay=_TT, sizes=((1024, 4608, 4096), (1024, 1024, 4096), (1024, 1024, 4096)), odt=bf16, pipe=1, dbias=False, want="gemm_bf16_group_tt",
         id="tall tiles of an uneven weight-gradient group", plain=False),
    dict(lay=_NT, sizes=((130, 200, 128), (97, 136, 64)), odt=bf16, pipe=8, dbias=False, want="gemm_bf16_group_nt", id="96-row tiles"),
    dict(lay=_NN, sizes=((130, 200, 128), (65, 67, 64)), odt=bf16, pipe=11, dbias=False, want="gemm_bf16_group_nn", id="64-row tiles"),
    dict(lay=_NN, sizes=((130, 200, 128), (64, 72, 64)), odt=bf16, pipe=1, dbias=False, want="gemm_bf16_group_nn", f16=True, id="op_f16"),
    dict(lay=_TT, sizes=((200, 136, 64), (132, 72, 96)), odt=f32, pipe=1, dbias=True, want="gemm_f32_tt", id="exact-f32 group")])
def gemm_grouped(lib, ops, G, lay, sizes, odt, pipe, dbias, want, f16=False):
    """Every problem's operands, C and dbias slot in guarded buffers of their own; C with a padded leading dimension, ragged
    shapes.  tests/test_gpu_kernels.py::test_gemm_grouped_equals_separate_contractions / test_gemm_f32_grouped_launch_equals_the_single_
    launches compare with the single launches; this compares every problem with f64."""
    from egopack_amd import _lib
    g = gen(sum(m + n + k for m, n, k in sizes))
    n = len(sizes)
    arr = (_lib.GemmDesc * n)()
    cmp = F32 if odt == f32 else BF16
    prs = []
    for i, (M, N, K) in enumerate(sizes):
        big = M * N * K > 1 << 30
        if f16:   # IEEE-half operands in 16-bit words: values exactly representable in half AND compared against their own f64 product
            a, b = torch.randn(M, K, generator=g).to(torch.float16), torch.randn(N, K, generator=g).to(torch.float16)
            A, B = G.m(f"p{i} A", M, K, torch.int16, pad=8, init=a.view(torch.int16)), G.m(f"p{i} B", N, K, torch.int16, pad=8, init=b.view(torch.int16))
            Cm = G.m(f"p{i} C", M, N, f32, pad=4)
            pr = dict(M=M, N=N, srcs=[(A, B, K)], C=Cm, bias=None, R=None, dbias=None, ref=(a.double() @ b.double().t()).float(), db_ref=None,
                      tA=False, tB=False, odt=bf16, compute=BF16, cdt=f32, rdt=None, act=0, alpha=1.0, acc=False)
        else:
            pr = _gemm_problem(G, f"p{i} ", g, M, N, (K,), lay[0], lay[1], odt, cmp, f32, None, (8 if odt == bf16 else 4,) * 2 + (4 if i % 2 else 1, 0),
                               bias=not lay[0], acc=lay[0], dbias=dbias and lay[0], scale=0.25 if big else 1.0, guard_rows=GUARD_ROWS)
        _gemm_desc(pr, arr[i])
        arr[i].op_f16 = int(f16)
        prs.append(pr)
    prev = lib.egk_gemm_set_pipeline(pipe)
    try:
        with _counted(lib) as ran:
            ok(lib.egk_gemm_grouped(S(), arr, n), "egk_gemm_grouped")
    finally:
        lib.egk_gemm_set_pipeline(prev)
    G.check()
    assert any(k.startswith(want) for k in ran.names), f"expected a {want}* launch, the counters show {ran.names}"
    out = {}
    for i, pr in enumerate(prs):
        K = sizes[i][2]
        # test_gemm_dw_with_fused_bias_gradient's tolerances for the deep weight-gradient problems (K in the thousands)
        tol = dict(rtol=2e-3, atol=2e-2) if (cmp == BF16 and K >= 1024) else _gemm_tol(pr)
        close(pr["C"].view, pr["ref"], f"C of problem {i}", **tol)
        if pr["dbias"] is not None:
            close(pr["dbias"].view, pr["db_ref"], f"dbias of problem {i}", **(dict(rtol=1e-3, atol=2e-2) if cmp == BF16 else dict(rtol=1e-5, atol=1e-3)))
            out[f"dbias{i}"] = pr["dbias"]
        out[f"C{i}"] = pr["C"]
    bad = (_lib.GemmDesc * 2)()
    _gemm_desc(prs[0], bad[0]), _gemm_desc(prs[1], bad[1])
    bad[1].splitk = 2
    refused(lib.egk_gemm_grouped(S(), bad, 2), "no split-K")
    return out


@case("egk_gemm", variants=[
    dict(M=6144, N=1024, K=1024, lay=_NN, want="gemm_bf16_nn_r192", id="6144x1024: the 192-row tile by policy"),
    dict(M=6144, N=1024, K=256, lay=_NT, want="gemm_bf16_nt_r96", pipe=8, id="6144x1024: 96-row tiles"),
    dict(M=16384, N=1024, K=4608, lay=_NN, want="gemm_bf16_nn_t256", id="16384x1024x4608: the 256x256 tile by policy"),
    dict(M=6144, N=4096, K=1024, lay=_NN, want="gemm_bf16_nn_t256", id="6144x4096: the 192x256 tile by policy")], plain=False)
def gemm_full_size(lib, ops, G, M, N, K, lay, want, pipe=1):
    """One full-size shape per tile variant the policy only picks at full size.  The operands are built on the device; the
    reference (f64 on the CPU) is taken on a sample of rows that includes the first and last row of tiles of every height, and
    EVERY element of the window must have been written (no sentinel left)."""
    gd = torch.Generator(device=DEV).manual_seed(M + N + K)
    a = (torch.randn(M, K, device=DEV, generator=gd) * 0.25).to(bf16)
    b = (torch.randn(N, K, device=DEV, generator=gd) * 0.25).to(bf16)
    bias = torch.randn(N, device=DEV, generator=gd)
    A = G.m("A", M, K, bf16, pad=8, init=a)
    B = G.m("B", K if lay[1] else N, N if lay[1] else K, bf16, pad=8, init=b.t() if lay[1] else b)
    Cm, Bs = G.m("C", M, N, bf16, pad=8), G.v("bias", N, f32, init=bias)
    pr = dict(M=M, N=N, srcs=[(A, B, K)], C=Cm, bias=Bs, R=None, dbias=None, tA=False, tB=lay[1], odt=bf16, compute=BF16, cdt=bf16, rdt=None,
              act=0, alpha=1.0, acc=False)
    d = _gemm_desc(pr)
    prev = lib.egk_gemm_set_pipeline(pipe)
    try:
        with _counted(lib) as ran:
            ok(lib.egk_gemm(S(), C.byref(d)), "egk_gemm")
    finally:
        lib.egk_gemm_set_pipeline(prev)
    G.check()
    assert any(k.startswith(want) for k in ran.names), f"expected a {want}* launch, the counters show {ran.names}"
    assert not bool(Cm.is_sentinel().any()), "C: elements of the window were not written"
    rows = torch.tensor(sorted({0, 1, 63, 64, 95, 96, 127, 128, 191, 192, 255, 256, M // 2 - 1, M // 2, M - 257, M - 256, M - 193, M - 192, M - 129,
                                M - 128, M - 97, M - 96, M - 65, M - 64, M - 2, M - 1}), device=DEV)
    ref = (a[rows].double().cpu() @ b.double().cpu().t() + bias.double().cpu()).float()
    close(Cm.view[rows], ref, "C (sampled rows)", **OUT16)
    return None


@case("egk_colsum", "egk_split_bf16", "egk_cast_rows", variants=[
    dict(M=300, N=1024, pad=8, dt=bf16), dict(M=37, N=250, pad=3, dt=f32), dict(M=2100, N=72, pad=4, dt=f32), dict(M=9, N=3, pad=1, dt=bf16),
    dict(M=0, N=64, pad=0, dt=f32)])
def colsum_split_cast_rows(lib, ops, G, M, N, pad, dt):
    g = gen(M + N)
    x = r16(torch.randn(M, N, generator=g))
    X = G.m("x", M, N, dt, pad=pad, init=x)
    # ---- column sums: ws = float [egk_colsum_ws_len(M, N)], out stored and accumulated
    n_ws = lib.egk_colsum_ws_len(M, N)
    o0 = torch.randn(N, generator=g)
    WS, O, OA = G.v("ws", n_ws, f32, guard=max(GUARD_ELEMS, 2 * N)), G.v("out", N, f32), G.v("out (accumulate)", N, f32, init=o0)
    ok(lib.egk_colsum(S(), P(X), X.ld, M, N, P(O), 0, P(WS), edt(dt)), "egk_colsum")
    ok(lib.egk_colsum(S(), P(X), X.ld, M, N, P(OA), 1, P(WS), edt(dt)), "egk_colsum")
    G.check()
    ref = x.double().sum(0)
    # test_linear_relu_and_fused_grad_slot / test_multi_linear_matches_concatenation compare bias gradients at rtol 1e-4 / atol 1e-4
    close(O.view, ref.float(), "out", rtol=1e-4, atol=1e-4), close(OA.view, (o0.double() + ref).float(), "out (accumulate)", rtol=1e-4, atol=1e-4)
    out = dict(colsum=O, colsum_acc=OA)
    # ---- x = hi + lo (f32 source), leading dimensions of its own; hi may be NULL
    if dt == f32:
        xs = torch.randn(M, N, generator=g)
        XS = G.m("split src", M, N, f32, pad=pad, init=xs)
        HI, LO, LO2 = G.m("hi", M, N, bf16, pad=2 * pad), G.m("lo", M, N, bf16, pad=2 * pad), G.m("lo (hi = NULL)", M, N, bf16, pad=2 * pad)
        ok(lib.egk_split_bf16(S(), P(XS), XS.ld, P(HI), P(LO), HI.ld, M, N), "egk_split_bf16")
        ok(lib.egk_split_bf16(S(), P(XS), XS.ld, None, P(LO2), LO2.ld, M, N), "egk_split_bf16")
        G.check()
        same(HI.view.view(torch.int16), xs.to(bf16).view(torch.int16), "hi")                 # tests/test_gpu_precise.py: exact
        same(LO.view.view(torch.int16), (xs - xs.to(bf16).float()).to(bf16).view(torch.int16), "lo")
        same(_bits(LO2), _bits(LO), "lo with hi = NULL")
        refused(lib.egk_split_bf16(S(), P(XS), N - 1, P(HI), P(LO), HI.ld, M, N), "leading dimension")
        out.update(hi=HI, lo=LO)
    # ---- row-strided conversion, all four type pairs; columns [cols, zero_cols) cleared, [zero_cols, ld_dst) untouched
    for ddt in (f32, bf16):
        Dm = G.m(f"cast_rows dst {ddt}", M, N, ddt, pad=9)
        zero_cols = min(N + 5, Dm.ld)
        ok(lib.egk_cast_rows(S(), P(X), edt(dt), X.ld, P(Dm), edt(ddt), Dm.ld, M, N, zero_cols), "egk_cast_rows")
        torch.cuda.synchronize()
        same(Dm.view.float(), x.to(ddt).float(), f"cast_rows {dt} -> {ddt}")                  # test_cast_roundtrip: exact
        wide = Dm.buf.as_strided((M, Dm.ld), (Dm.ld, 1), Dm._start)
        if M and N:
            assert not wide[:, N:zero_cols].float().ne(0).any(), "columns [cols, zero_cols) are not zero"
            tail = Dm._raw.as_strided((M, Dm.ld - zero_cols), (Dm.ld, 1), Dm._start + zero_cols)
            assert bool((tail == Dm._bits).all()), "columns from zero_cols on were written"
            wide[:, N:zero_cols] = float("nan")                        # (back to a NaN, then the sentinel bits, for the guard check)
            Dm._raw.as_strided((M, zero_cols - N), (Dm.ld, 1), Dm._start + N).fill_(Dm._bits)
        G.check()
        out[f"cast_rows_{_fmt(ddt)}"] = Dm
    refused(lib.egk_cast_rows(S(), P(X), edt(dt), X.ld, P(Dm), edt(ddt), Dm.ld, M, N, Dm.ld + 1), "zero_cols")
    return out


# =====================================================================================================================
# the driver
# =====================================================================================================================
def _bits(x):
    if x is None:
        return None
    if isinstance(x, Guarded2D):
        return x.bits().cpu()
    return x.detach().cpu().contiguous().view(torch.int16 if x.element_size() == 2 else torch.int32 if x.element_size() == 4 else
                                             torch.int64 if x.element_size() == 8 else u8)


@pytest.mark.gpu
@pytest.mark.parametrize("name,fn,variant,covers,plain", CASES, ids=[c[0] for c in CASES])
def test_bounds(name, fn, variant, covers, plain):
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from egopack_amd import _lib, ops
    lib = _lib.load()
    knobs = (lib.egk_gemm_set_pipeline(1), lib.egk_gather_max_tune(-1))
    lib.egk_gemm_set_pipeline(knobs[0])
    try:
        G = Guards()
        out = fn(lib, ops, G, **variant)
        G.check()
        if plain and out:
            got = {k: _bits(v) for k, v in out.items()}
            H = Guards(plain=True)
            base = fn(lib, ops, H, **variant)
            torch.cuda.synchronize()
            for k, v in base.items():
                if k not in got:
                    continue
                b = _bits(v)
                assert got[k].shape == b.shape and torch.equal(got[k], b), f"{k}: the guarded / strided call and the contiguous call differ in bits"
    finally:
        lib.egk_gemm_set_pipeline(knobs[0])
        lib.egk_gather_max_tune(knobs[1])
        lib.egk_tee_split_next(None, None, 0)
        lib.egk_slab_input_next(None, None, None)
        lib.egk_gemm_defer_reduce_next(0)
        torch.cuda.synchronize()
