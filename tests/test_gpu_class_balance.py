"""Class-balanced cross entropy on the GPU (include/egopack_ce_balanced.h, ops.cross_entropy(weight=, offset=)): parity with the
float64 host model of tests/class_balance_common.py, the fused launch on the classifier bank's logits, logits layouts, "off is
the old path" and "on" in the multi-task step (eager and captured), the task / wrapper plumbing and main_temporal.py with
``class_balance.mode=weight`` (checkpoint entry, resume).

Tolerances are the project's cross-entropy tolerances (loss rtol 1e-5 / atol 1e-5, gradient rtol 1e-4 / atol 1e-6): the f32
arithmetic of the formulas stays within 0.03 / 0.25 of them against float64 over C in {2, 115, 478}, Zipf weights 0.009 .. 14 and
logits ~ 3 N(0, 1)."""
import ctypes as C
import subprocess
import sys
from pathlib import Path

import pytest
import torch

from tests import class_balance_common as CB

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF = torch.bfloat16
REPO = Path(__file__).resolve().parents[1]
ROWS = 77  # ragged for 4 waves per workgroup; y[::3] = -1


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


@pytest.fixture
def compute_restored():
    from egopack_amd import ops
    prev = ops.get_compute()
    yield
    ops.set_compute(prev)


def gen(seed):
    return torch.Generator().manual_seed(seed)


def _vectors(heads, presence):
    """(weights, offsets) as ops.cross_entropy takes them (host tensors) for the four presence patterns."""
    w = [CB.zipf_weights(c) for c in heads]
    a = [CB.zipf_offsets(c) for c in heads]
    if presence == "weight":
        return tuple(w), None
    if presence == "offset":
        return None, tuple(a)
    if presence == "both":
        return tuple(w), tuple(a)
    # "mixed": the first head has both vectors, the others none
    return tuple([w[0]] + [None] * (len(heads) - 1)), tuple([a[0]] + [None] * (len(heads) - 1))


def _problem(heads, seed):
    g = gen(seed)
    logits = [3 * torch.randn(ROWS, c, generator=g) for c in heads]
    y = torch.stack([torch.randint(0, c, (ROWS,), generator=g) for c in heads], 1)
    y[::3] = -1
    gloss = torch.randn(ROWS, generator=g)
    return logits, y, gloss


def _dev(vs):
    return None if vs is None else tuple(None if v is None else v.to(DEV) for v in vs)


def _model(logits, y, ws, offs, eps, gloss):
    total, grads = torch.zeros(y.shape[0], dtype=torch.float64), []
    for h, l in enumerate(logits):
        loss, _, d = CB.model(l, y[:, h], None if ws is None else ws[h], None if offs is None else offs[h], eps, gloss)
        total += loss
        grads.append(d)
    return total, grads


# ---- 1. parity against the host model ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("presence", ["weight", "offset", "both", "mixed"])
@pytest.mark.parametrize("eps", [0.0, 0.1])
@pytest.mark.parametrize("heads", [(115, 478), (2,), (65,)], ids=["115x478", "2", "65"])
def test_loss_and_gradient_match_the_host_model(heads, eps, presence):
    """(Fails without the feature: ``cross_entropy() got an unexpected keyword argument 'weight'``.)"""
    from egopack_amd import ops
    logits, y, gloss = _problem(heads, 7 * sum(heads) + int(10 * eps))
    ws, offs = _vectors(heads, presence)
    dl = [l.to(DEV).requires_grad_(True) for l in logits]
    with ops.compute_mode("f32"):
        loss = ops.cross_entropy(tuple(dl), y.to(DEV), eps, weight=_dev(ws), offset=_dev(offs))
        loss.backward(gloss.to(DEV))
    want, grads = _model(logits, y, ws, offs, eps, gloss)
    torch.testing.assert_close(loss.detach().cpu(), want.float(), **CB.LOSS_TOL)
    for h, (l, d) in enumerate(zip(dl, grads)):
        torch.testing.assert_close(l.grad.cpu(), d.float(), msg=lambda s: f"head {h}: {s}", **CB.GRAD_TOL)
        assert not l.grad[::3].ne(0).any(), f"head {h}: ignored rows have a gradient"
    assert not loss[::3].ne(0).any(), "ignored rows have a loss"
    if len(heads) == 1:  # a single head also takes one tensor per argument
        one = ops.cross_entropy(dl[0].detach(), y[:, 0].to(DEV), eps, weight=None if ws is None else ws[0].to(DEV),
                                offset=None if offs is None else offs[0].to(DEV))
        assert torch.equal(one, loss.detach())


def test_all_none_issues_the_plain_launches():
    from egopack_amd import _lib, ops
    from tests.test_gpu_bounds import _counted
    logits, y, gloss = _problem((115, 478), 3)
    dl = [l.to(DEV).requires_grad_(True) for l in logits]
    with _counted(_lib.load()) as c:
        loss = ops.cross_entropy(tuple(dl), y.to(DEV), 0.1, weight=(None, None), offset=None)
        loss.backward(gloss.to(DEV))
    assert c.names.get("ce_fwd") == 2 and c.names.get("ce_bwd") == 2 and "ce_balanced" not in c.names, c.names
    plain = ops.cross_entropy(tuple(l.detach() for l in dl), y.to(DEV), 0.1)
    assert torch.equal(plain, loss.detach())
    with _counted(_lib.load()) as c:
        loss = ops.cross_entropy(tuple(dl), y.to(DEV), 0.1, weight=(CB.zipf_weights(115).to(DEV), None))
        loss.backward(gloss.to(DEV))
    assert c.names == {"ce_balanced": 4}, c.names


def test_bad_vectors_raise_naming_the_head():
    from egopack_amd import ops
    logits, y, _ = _problem((115, 478), 4)
    dl, yd = tuple(l.to(DEV) for l in logits), y.to(DEV)
    w = [CB.zipf_weights(115).to(DEV), CB.zipf_weights(478).to(DEV)]
    with pytest.raises(ValueError, match="head 1"):
        ops.cross_entropy(dl, yd, weight=(w[0], w[1][:-1]))                     # wrong length
    with pytest.raises(ValueError, match="head 0"):
        ops.cross_entropy(dl, yd, offset=(w[0].double(), None))                # not f32
    with pytest.raises(ValueError, match="head 1"):
        ops.cross_entropy(dl, yd, weight=(None, w[1].cpu()))                   # another device
    with pytest.raises(ValueError, match="2 heads"):
        ops.cross_entropy(dl, yd, weight=w[0])                                 # one tensor for two heads
    with pytest.raises(ValueError, match="1 entries"):
        ops.cross_entropy(dl, yd, offset=(w[0],))


# ---- 2. the fused launch ------------------------------------------------------------------------------------------------------------------
def _bank_task(H=64, heads=(115, 478)):
    """An AR head whose classifiers are one bank of a materialised flat optimizer (pads 115 -> 128, 478 -> 512)."""
    from egopack_amd.models.tasks import RecognitionTask
    from egopack_amd.optim import FlatAdam
    torch.manual_seed(5)
    task = RecognitionTask(H, H, heads).to(DEV)
    opt = FlatAdam(task.parameters(), lr=1e-2)
    for p in task.parameters():
        p.grad = torch.zeros_like(p)
    opt._materialise()
    v = task.classifiers[0][1].weight._egk_bank_views
    assert v["rows"] == [(0, 115), (128, 478)] and v["n"] == 640
    return task, opt


@pytest.mark.parametrize("mode", ["f32", "bf16"])
@pytest.mark.parametrize("eps", [0.0, 0.1])
def test_fused_launch_on_the_bank_logits_equals_the_unfused_pair(mode, eps, compute_restored):
    from egopack_amd import _lib, ops
    from tests.test_gpu_bounds import _counted
    heads, coef = (115, 478), 0.37 / ROWS
    ws, offs = _vectors(heads, "both")
    ws, offs = (ws[0], None), (None, offs[1])          # weights on the verbs, offsets on the nouns
    _, y, _ = _problem(heads, 17)
    with ops.compute_mode(mode):
        task, _ = _bank_task()
        x = torch.randn(ROWS, 64, generator=gen(2)).to(DEV).to(ops.act_dtype()).requires_grad_(True)
        with _counted(_lib.load()) as c, ops.bank_grad_handoff(), ops.loss_seed(coef):
            logits = task.forward_logits(x)
            gbuf = logits[0]._egk_grad_dst[0]
            loss = ops.cross_entropy(logits, y.to(DEV), eps, weight=_dev(ws), offset=_dev(offs))
            operand = gbuf.detach().clone()
        assert c.names.get("ce_balanced") == 1 and "ce_fwd" not in c.names and "ce_bwd" not in c.names, c.names
        assert operand.shape == (ROWS, 640) and operand.dtype == (BF if mode == "bf16" else torch.float32)
        plain = [l.detach().clone().requires_grad_(True) for l in logits]
        ref = ops.cross_entropy(tuple(plain), y.to(DEV), eps, weight=_dev(ws), offset=_dev(offs))
        ref.backward(torch.full_like(ref, coef))
    torch.testing.assert_close(loss.detach(), ref.detach(), **CB.LOSS_TOL)
    want, grads = _model([l.detach().cpu() for l in logits], y, ws, offs, eps, torch.full((ROWS,), coef))
    torch.testing.assert_close(loss.detach().cpu(), want.float(), **CB.LOSS_TOL)
    for (c0, Cn), pad_end, p in zip([(0, 115), (128, 478)], (128, 640), plain):
        block = operand[:, c0:c0 + Cn].float()
        if mode == "f32":
            torch.testing.assert_close(block, p.grad, **CB.GRAD_TOL)
        else:
            # NOT the gradient tolerance: a bf16 element carries 8 significand bits, so the operand can only agree with an f32
            # gradient to one rounding, 2^-8 relative.  This is a plausibility bound for the element type and nothing to copy: the
            # exact statement -- the bf16 operand is RNE(f32 operand), bit for bit, and the f32 operand meets GRAD_TOL against
            # the host model -- is made in the two tests below.
            torch.testing.assert_close(block, p.grad, rtol=2.0 ** -8, atol=1e-6)
        assert not operand[:, c0 + Cn:pad_end].float().ne(0).any(), "pad columns are not exactly 0"
        assert not operand[::3, c0:pad_end].float().ne(0).any(), "ignored rows have a gradient"


def _plain_bank_logits(rows, seed):
    """(logits, gradient operand) of a fresh ``_bank_task`` on seeded features; call under ``bank_grad_handoff``."""
    from egopack_amd import ops
    task, _ = _bank_task()
    x = torch.randn(rows, 64, generator=gen(seed)).to(DEV).to(ops.act_dtype()).requires_grad_(True)
    logits = task.forward_logits(x)
    return logits, logits[0]._egk_grad_dst[0]


@pytest.mark.parametrize("mode", ["f32", "bf16"])
@pytest.mark.parametrize("eps", [0.0, 0.1])
def test_single_task_fused_launch_has_the_bits_of_the_multi_task_launch(mode, eps, compute_restored):
    """No vectors.  ``ops.cross_entropy`` on bank logits under an announced seed (``_CE._fused``: one fused launch) gives the loss
    and the operand buffer, pad columns included, of ``ops.cross_entropy_multi`` on the same task beside a second one -- both
    plan the task with the same rules and fill the same launch argument."""
    from egopack_amd import _lib, ops
    from tests.test_gpu_bounds import _counted
    rows, coefs = (ROWS, 40), (0.37 / ROWS, 0.11 / 40)
    _, y, _ = _problem((115, 478), 17)
    y2 = y[:40].clone()
    with ops.compute_mode(mode):
        with _counted(_lib.load()) as c, ops.bank_grad_handoff(), ops.loss_seed(coefs[0]):
            logits, gbuf = _plain_bank_logits(rows[0], 2)
            one = ops.cross_entropy(logits, y.to(DEV), eps)
        assert c.names.get("ce_fwd") == 1 and "ce_bwd" not in c.names and "ce_balanced" not in c.names, c.names
        with _counted(_lib.load()) as c, ops.bank_grad_handoff():
            pair = [_plain_bank_logits(rows[0], 2), _plain_bank_logits(rows[1], 3)]
            losses = ops.cross_entropy_multi([(pair[0][0], y.to(DEV)), (pair[1][0], y2.to(DEV))], coefs, eps)
        assert losses is not None and len(losses) == 2, "the two bank tasks did not qualify for the one-launch form"
        assert c.names.get("ce_fwd") == 1 and "ce_bwd" not in c.names and "ce_balanced" not in c.names, c.names
    for a, b in zip(logits, pair[0][0]):
        assert torch.equal(a.detach(), b.detach()), "the two runs did not see the same logits"
    assert gbuf.shape == (ROWS, 640) and gbuf.dtype == (BF if mode == "bf16" else torch.float32)
    assert torch.equal(one.detach(), losses[0].detach()), "loss bits"
    assert torch.equal(gbuf.view(torch.int16 if mode == "bf16" else torch.int32),
                       pair[0][1].view(torch.int16 if mode == "bf16" else torch.int32)), "operand bits"
    assert not gbuf[:, 115:128].float().ne(0).any() and not gbuf[:, 128 + 478:].float().ne(0).any(), "pad columns are not exactly 0"
    assert one.detach()[::3].eq(0).all() and not gbuf[::3].float().ne(0).any(), "ignored rows"


@pytest.mark.parametrize("mode", ["f32", "bf16"])
def test_a_first_block_behind_column_0_takes_the_single_task_fused_launch_only(mode, compute_restored):
    """The nouns alone: their block starts at column 128 of the bank's operand.  ``cross_entropy_multi`` does not take such a task
    (None: its launch argument has no way to clear the columns in front); ``ops.cross_entropy`` still issues the single-task
    fused launch -- the bits the block has when both heads go through it -- and zero-fills the leading columns itself."""
    from egopack_amd import _lib, ops
    from tests.test_gpu_bounds import _counted
    eps, coef = 0.1, 0.37 / ROWS
    _, y, _ = _problem((115, 478), 17)
    yn = y[:, 1:2].contiguous()
    with ops.compute_mode(mode):
        with ops.bank_grad_handoff(), ops.loss_seed(coef):
            both, gboth = _plain_bank_logits(ROWS, 2)
            ops.cross_entropy(both, y.to(DEV), eps)
        with ops.bank_grad_handoff():
            pair = [_plain_bank_logits(ROWS, 2), _plain_bank_logits(40, 3)]
            assert ops.cross_entropy_multi([((pair[0][0][1],), yn.to(DEV)), (pair[1][0], y[:40].to(DEV))], (coef, coef), eps) is None
        with _counted(_lib.load()) as c, ops.bank_grad_handoff(), ops.loss_seed(coef):
            logits, gbuf = _plain_bank_logits(ROWS, 2)
            gbuf.fill_(float("nan"))
            loss = ops.cross_entropy((logits[1],), yn.to(DEV), eps)
        assert c.names.get("ce_fwd") == 1 and "ce_bwd" not in c.names and "ce_balanced" not in c.names, c.names
        ref = ops.cross_entropy((logits[1].detach().clone(),), yn.to(DEV), eps)
    assert not gbuf[:, :128].float().ne(0).any(), "the columns in front of the first block are not exactly 0"
    bits = torch.int16 if mode == "bf16" else torch.int32
    assert torch.equal(gbuf[:, 128:].contiguous().view(bits), gboth[:, 128:].contiguous().view(bits)), "the nouns' block and its pad columns"
    torch.testing.assert_close(loss.detach(), ref.detach(), **CB.LOSS_TOL)
    assert loss.detach()[::3].eq(0).all()


def _fused_call(lib, tasks, eps, dt):
    """egk_ce_w_fused_multi over ``tasks`` = [(logits list, y, weights, offsets, pads, gscale)] on plain device tensors; returns
    [(loss, operand)] per task.  The operand has two spare columns behind the last block (they must keep their fill)."""
    from egopack_amd import _lib
    arr = (_lib.CEWTask * len(tasks))()
    keep, out = [], []
    for a, (logits, y, ws, offs, pads, gs) in zip(arr, tasks):
        rows, width = logits[0].shape[0], sum(pads) + 2
        loss = torch.full((rows,), 7.0, device=DEV)
        D = torch.full((rows, width), 3.0, device=DEV, dtype=dt)
        b, col = a.base, 0
        for h, l in enumerate(logits):
            b.logits[h], b.ld[h], b.C[h], b.pad[h], b.dcol[h] = l.data_ptr(), l.stride(0), l.shape[1], pads[h], col
            a.weight[h] = None if ws[h] is None else ws[h].data_ptr()
            a.offset[h] = None if offs[h] is None else offs[h].data_ptr()
            col += pads[h]
        b.n_heads, b.y, b.y_stride, b.loss, b.dlogits, b.ldd, b.rows, b.gscale = len(logits), y.data_ptr(), y.shape[1], \
            loss.data_ptr(), D.data_ptr(), D.stride(0), rows, gs
        keep.append((logits, y, ws, offs))
        out.append((loss, D))
    rc = lib.egk_ce_w_fused_multi(C.c_void_p(torch.cuda.current_stream().cuda_stream), arr, len(tasks), eps, 1 if dt == BF else 0)
    assert rc == 0, _lib.last_error()
    torch.cuda.synchronize()
    return out


def _fused_tasks():
    specs = [((115, 478), (128, 512), 0.5 / ROWS, "mixed", ROWS), ((65,), (128,), 0.25, "both", 33), ((2, 115), (8, 128), 1.0, "offset", ROWS)]
    tasks = []
    for i, (heads, pads, gs, presence, rows) in enumerate(specs):
        g = gen(50 + i)
        logits = [(3 * torch.randn(rows, c, generator=g)).to(DEV) for c in heads]
        y = torch.stack([torch.randint(0, c, (rows,), generator=g) for c in heads], 1)
        y[::3] = -1
        ws, offs = _vectors(heads, presence)
        ws, offs = ws or (None,) * len(heads), offs or (None,) * len(heads)
        tasks.append((logits, y.to(DEV), _dev(ws), _dev(offs), pads, gs))
    return tasks


@pytest.mark.parametrize("eps", [0.0, 0.1])
def test_several_tasks_in_one_launch_have_the_bits_of_their_own_launch_and_bf16_is_the_rounded_f32(eps):
    from egopack_amd import _lib
    lib = _lib.load()
    tasks = _fused_tasks()
    single = {dt: [_fused_call(lib, [t], eps, dt)[0] for t in tasks] for dt in (torch.float32, BF)}
    for dt in (torch.float32, BF):
        for count in (2, 3):
            got = _fused_call(lib, tasks[:count], eps, dt)
            for i, ((loss, D), (loss1, D1)) in enumerate(zip(got, single[dt])):
                assert torch.equal(loss, loss1), f"count {count}, task {i}: loss bits"
                assert torch.equal(D.view(torch.int16 if dt == BF else torch.int32), D1.view(torch.int16 if dt == BF else torch.int32)), \
                    f"count {count}, task {i}: operand bits"
    for i, ((loss32, D32), (loss16, D16)) in enumerate(zip(single[torch.float32], single[BF])):
        assert torch.equal(loss32, loss16)
        assert torch.equal(D32.to(BF).view(torch.int16), D16.view(torch.int16)), f"task {i}: bf16 operand != RNE(f32 operand)"
        assert bool((D32[:, -2:] == 3.0).all()) and bool((D16[:, -2:].float() == 3.0).all()), "columns behind the blocks were written"
        logits, y, ws, offs, pads, gs = tasks[i]
        want, grads = _model([l.cpu() for l in logits], y.cpu(), [None if w is None else w.cpu() for w in ws],
                             [None if a is None else a.cpu() for a in offs], eps, torch.full((y.shape[0],), gs))
        torch.testing.assert_close(loss32.cpu(), want.float(), **CB.LOSS_TOL)
        col = 0
        for h, d in enumerate(grads):
            Cn = d.shape[1]
            torch.testing.assert_close(D32[:, col:col + Cn].cpu(), d.float(), **CB.GRAD_TOL)
            assert not D32[:, col + Cn:col + pads[h]].ne(0).any()
            col += pads[h]


def _spec_vectors():
    """Asymmetric on purpose -- task 0 (AR): weights on both heads, no offset; task 1 (LTA): no weight, offsets on the nouns only,
    as the second part of ONE concatenated vector (a contiguous slice at byte offset 460: 4-byte aligned, not 16) -- so a launch
    that hands a task the other's vectors, swaps weights and offsets or shifts a head misses the model."""
    a_all = torch.cat([CB.zipf_offsets(115), CB.zipf_offsets(478)])
    return [((CB.zipf_weights(115), CB.zipf_weights(478)), None), (None, (None, a_all[115:]))], a_all


@pytest.mark.parametrize("mode", ["f32", "bf16"])
def test_cross_entropy_multi_on_bank_logits_matches_the_host_model_per_task(mode, compute_restored):
    """``ops.cross_entropy_multi(weights=, offsets=)`` -- the call of the engine's banked chain, through ``_CEMulti`` and its task
    marshalling -- on the logits of two classifier banks under an announced seed: per task, the loss vector and the operand
    buffer against the host model on the logits the launch consumed, with that task's own vectors.  The bf16 operand is
    compared bit for bit with RNE of the f32 operand of the same task (a one-task launch on the same logits, itself within
    GRAD_TOL of the model)."""
    from egopack_amd import _lib, ops
    from tests.test_gpu_bounds import _counted
    heads, eps = (115, 478), 0.1
    rows, coefs = (ROWS, 40), (0.37 / ROWS, 0.11 / 40)
    spec, a_all = _spec_vectors()
    a_dev = a_all.to(DEV)
    dev_vec = [(_dev(spec[0][0]), None), (None, (None, a_dev[115:]))]
    assert a_dev[115:].data_ptr() % 16 != 0 and a_dev[115:].is_contiguous()
    ys = []
    for i, r in enumerate(rows):
        g = gen(70 + i)
        y = torch.stack([torch.randint(0, c, (r,), generator=g) for c in heads], 1)
        y[i::3] = -1
        ys.append(y)
    with ops.compute_mode(mode):
        banks = [_bank_task() for _ in rows]
        with _counted(_lib.load()) as c, ops.bank_grad_handoff():
            logits = []
            for i, r in enumerate(rows):
                x = torch.randn(r, 64, generator=gen(80 + i)).to(DEV).to(ops.act_dtype()).requires_grad_(True)
                with ops.loss_seed(coefs[i]):
                    logits.append(banks[i][0].forward_logits(x))
            losses = ops.cross_entropy_multi([(l, y.to(DEV)) for l, y in zip(logits, ys)], coefs, eps,
                                             weights=[w for w, _ in dev_vec], offsets=[a for _, a in dev_vec])
        assert losses is not None and len(losses) == 2, "the two bank tasks did not qualify for the one-launch form"
        assert c.names.get("ce_balanced") == 1 and "ce_fwd" not in c.names and "ce_bwd" not in c.names, c.names
        torch.cuda.synchronize()
        for i, r in enumerate(rows):
            ws, offs = spec[i]
            operand = logits[i][0]._egk_grad_dst[0].detach()
            assert operand.shape == (r, 640) and operand.dtype == (BF if mode == "bf16" else torch.float32)
            seen = [l.detach().clone() for l in logits[i]]  # the logits the launch consumed (f32, blocks of the bank's output)
            want, grads = _model([l.cpu() for l in seen], ys[i], ws, offs, eps, torch.full((r,), coefs[i]))
            torch.testing.assert_close(losses[i].detach().cpu(), want.float(), msg=lambda s: f"task {i} loss: {s}", **CB.LOSS_TOL)
            assert not losses[i].detach()[i::3].ne(0).any()
            op32 = operand
            if mode == "bf16":
                dv = tuple(None if v is None else v.contiguous() for v in (dev_vec[i][0] or (None, None))), \
                    tuple(None if v is None else v.contiguous() for v in (dev_vec[i][1] or (None, None)))
                loss32, op32 = _fused_call(_lib.load(), [(seen, ys[i].to(DEV), dv[0], dv[1], (128, 512), coefs[i])], eps, torch.float32)[0]
                op32 = op32[:, :640]
                assert torch.equal(loss32, losses[i].detach()), f"task {i}: loss bits"
                assert torch.equal(op32.to(BF).view(torch.int16), operand.view(torch.int16)), f"task {i}: bf16 operand != RNE(f32 operand)"
            for (c0, Cn), pad_end, d in zip([(0, 115), (128, 478)], (128, 640), grads):
                torch.testing.assert_close(op32[:, c0:c0 + Cn].cpu(), d.float(), msg=lambda s: f"task {i} operand: {s}", **CB.GRAD_TOL)
                assert not operand[:, c0 + Cn:pad_end].float().ne(0).any(), "pad columns are not exactly 0"
                assert not operand[i::3, c0:pad_end].float().ne(0).any(), "ignored rows have a gradient"


def test_a_sliced_vector_gives_the_bits_of_its_copy():
    """A contiguous slice of a longer vector (the noun part of verbs ++ nouns: byte offset 460) is read where it lies."""
    from egopack_amd import ops
    heads, eps = (115, 478), 0.1
    logits, y, gloss = _problem(heads, 29)
    w_all = torch.cat([CB.zipf_weights(c) for c in heads]).to(DEV)
    a_all = torch.cat([CB.zipf_offsets(c) for c in heads]).to(DEV)
    sliced = ((w_all[:115], w_all[115:]), (a_all[:115], a_all[115:]))
    assert w_all[115:].data_ptr() % 16 == 12
    copies = tuple(tuple(v.clone() for v in vs) for vs in sliced)
    out = []
    with ops.compute_mode("f32"):
        for ws, offs in (sliced, copies):
            dl = [l.to(DEV).requires_grad_(True) for l in logits]
            loss = ops.cross_entropy(tuple(dl), y.to(DEV), eps, weight=ws, offset=offs)
            loss.backward(gloss.to(DEV))
            out.append((loss.detach(), [l.grad for l in dl]))
    assert torch.equal(out[0][0], out[1][0]) and all(torch.equal(a, b) for a, b in zip(out[0][1], out[1][1]))
    want, grads = _model(logits, y, [v.cpu() for v in sliced[0]], [v.cpu() for v in sliced[1]], eps, gloss)
    torch.testing.assert_close(out[0][0].cpu(), want.float(), **CB.LOSS_TOL)
    for g, d in zip(out[0][1], grads):
        torch.testing.assert_close(g.cpu(), d.float(), **CB.GRAD_TOL)


# ---- 3. layouts -----------------------------------------------------------------------------------------------------------------------------
def _layout(name, t):
    """``t`` [rows, C] in another memory layout (same values), detached: a leaf that keeps the strides."""
    if name == "padded":
        base = torch.full((t.shape[0], t.shape[1] + 5), float("nan"), device=t.device)
        base[:, :t.shape[1]] = t
        v = base[:, :t.shape[1]]
    elif name == "cat":
        v = torch.cat([torch.full((t.shape[0], 3), float("nan"), device=t.device), t], dim=1)[:, 3:]
    else:  # transposed
        v = t.t().contiguous().t()
    assert not v.is_contiguous() and torch.equal(v, t)
    return v.detach().requires_grad_(True)


@pytest.mark.parametrize("layout", ["padded", "cat", "transposed", "sum"])
def test_logits_layouts_give_the_bits_of_contiguous_copies(layout):
    from egopack_amd import ops
    heads, eps = (115, 478), 0.1
    logits, y, gloss = _problem(heads, 23)
    ws, offs = _vectors(heads, "both")
    ws, offs, yd, gd = _dev(ws), _dev(offs), y.to(DEV), gloss.to(DEV)

    def run(ls, by_sum):
        loss = ops.cross_entropy(tuple(ls), yd, eps, weight=ws, offset=offs)
        if by_sum:
            loss.sum().backward()  # (the gradient of sum(): an expanded, stride-0 vector of ones)
        else:
            loss.backward(gd)
        return loss.detach(), [l.grad for l in ls]

    with ops.compute_mode("f32"):
        base = [l.to(DEV).requires_grad_(True) for l in logits]
        want, wgrads = run(base, layout == "sum")
        other = [l.to(DEV).requires_grad_(True) for l in logits] if layout == "sum" else [_layout(layout, l.to(DEV)) for l in logits]
        got, ggrads = run(other, layout == "sum")
    assert torch.equal(got, want)
    for a, b in zip(ggrads, wgrads):
        assert torch.equal(a, b)
    if layout == "sum":  # ... and equals the explicit vector of ones
        with ops.compute_mode("f32"):
            ls = [l.to(DEV).requires_grad_(True) for l in logits]
            loss = ops.cross_entropy(tuple(ls), yd, eps, weight=ws, offset=offs)
            loss.backward(torch.ones_like(loss))
        for a, l in zip(wgrads, ls):
            assert torch.equal(a, l.grad)


# ---- 4. the multi-task step: off is the old path, on matches the model, captured == eager ---------------------------------------------------
SIZES = [("f32", 2), ("bf16", 2), ("bf16", 8)]
SIZE_IDS = ["f32-B2", "bf16-B2", "bf16-B8-banked"]


def _build_step(compute, balance, batch=2, seed=11):
    """AR + LTA + PNR, B = ``batch`` per task, T = 8, H = 64, dropout off, Adam.  ``balance``: None (the criteria bench.py builds,
    without the new arguments), "none" (the new arguments, every vector None) or "on" (weights on AR, offsets on LTA).
    B = 2 is 16 rows per task: every head takes the per-task path (one fused cross entropy per task).  B = 8 is 64 rows, the
    smallest batch the grouped chains take (whole 64-row tiles, bf16): AR and LTA share the banked chain and ONE cross-entropy
    launch."""
    import bench
    from egopack_amd import engine, ops
    from egopack_amd import train as T
    from egopack_amd.criterion import CrossEntropyNone, MetricSelectorWrapper
    args = bench.parse_args(["--workload", "mtl", "--batch", str(batch), "--T", "8", "--hidden", "64", "--trn-hidden", "64", "--dropout", "0.0",
                             "--compute", compute])
    ops.set_compute(compute)
    ops.manual_seed(seed)
    model, tasks, crit, weights, dev, merged = bench.build_workload(args, 0, torch.device(DEV))
    model.to(DEV).train()
    for t in tasks.values():
        t.to(DEV).train()
    vec = {}
    if balance is not None:
        class DS:
            has_joint_label, num_labels = False, 2
        if balance == "on":
            vec = {"ar": dict(class_weights=[CB.zipf_weights(115).to(DEV), CB.zipf_weights(478).to(DEV)]),
                   "lta": dict(class_offsets=[CB.zipf_offsets(115).to(DEV), CB.zipf_offsets(478).to(DEV)])}
        else:
            vec = {"ar": dict(class_weights=[None, None], class_offsets=None), "lta": dict(class_weights=None, class_offsets=[None, None])}
        crit = dict(crit)
        for t in ("ar", "lta"):
            crit[t] = MetricSelectorWrapper(CrossEntropyNone(weight=None, offset=None), DS(), **vec[t])
    cfg = T.load_config(["optimizer.lr=1e-2"])
    flat = [*model.configure_optimizers(0), *(p for t in ("ar", "oscc", "lta", "pnr") for p in tasks[t].configure_optimizers(0))]
    opt = T.build_optimizer(cfg, T.build_param_groups(cfg, model, tasks), layout_order=flat)
    step = engine.MTLStep(model, tasks, crit, weights, opt, fused_backbone=True)
    return step, opt, dev, merged, vec


def _run_eager(compute, balance, steps=3, batch=2):
    from egopack_amd import _lib
    from tests.test_gpu_bounds import _counted
    step, opt, dev, merged, _ = _build_step(compute, balance, batch)
    names, vectors = [], []
    for _ in range(steps):
        with _counted(_lib.load()) as c:
            total, vs = step.step(dev, merged)
        names.append(dict(c.names))
        vectors.append((total.clone().cpu(), {t: v.clone().cpu() for t, v in vs.items()}))
    torch.cuda.synchronize()
    return names, vectors, opt.flat_p.clone().cpu(), step.loss_sums()


@pytest.mark.parametrize("compute,batch", SIZES, ids=SIZE_IDS)
def test_off_is_the_old_path_in_the_step(compute, batch, compute_restored):
    names0, vec0, p0, sums0 = _run_eager(compute, None, batch=batch)
    names1, vec1, p1, sums1 = _run_eager(compute, "none", batch=batch)
    assert all("ce_balanced" not in n for n in names0 + names1), names1
    assert names0 == names1
    assert torch.equal(p0, p1) and sums0 == sums1
    for (tot0, v0), (tot1, v1) in zip(vec0, vec1):
        assert torch.equal(tot0, tot1) and v0.keys() == v1.keys() and all(torch.equal(v0[t], v1[t]) for t in v0)
    assert bool(torch.isfinite(p0).all())


@pytest.mark.parametrize("compute,batch", SIZES, ids=SIZE_IDS)
def test_on_in_the_step_matches_the_host_model_and_counts_one_launch(compute, batch, compute_restored):
    """The loss vectors of the eager step against the host model, f32 and bf16, on the step's OWN logits -- the ones its criteria's
    ``select`` received in that very step (with the labels it received: a compacted head hands it the labelled rows), keyed by
    task, evaluated with that task's vectors: AR's vectors on LTA, weights as offsets or a shifted head miss the model.  Then the
    objective sum_t w_t mean(loss_t) with ignored nodes counting in the mean, and the launches: no plain cross-entropy launch is
    left for AR / LTA and no launch is added -- one fused launch per task on the per-task path (16 rows), ONE ce_balanced launch
    per step for both tasks on the banked path (64 rows, bf16)."""
    from egopack_amd import _lib
    from tests.test_gpu_bounds import _counted
    step, opt, dev, merged, vec = _build_step(compute, "on", batch)
    for _ in range(2):  # (the optimizer's flat buffers and with them the classifier banks exist after the first step)
        step.step(dev, merged)
    seen = {}
    for t in ("ar", "lta"):
        def spy(logits, gt, t=t, inner=step.criteria[t].select):
            seen[t] = ([l.detach().clone() for l in logits], gt.detach().clone())
            return inner(logits, gt)
        step.criteria[t].select = spy
    with _counted(_lib.load()) as c:
        total, vs = step.step(dev, merged)
    names = dict(c.names)
    for t in ("ar", "lta"):
        del step.criteria[t].select
    torch.cuda.synchronize()
    print("launches of the step with the vectors:", names)
    assert names.get("ce_balanced", 0) >= 1 and "ce_fwd" not in names and "ce_bwd" not in names, names
    off_names, off_vec, _, _ = _run_eager(compute, None, steps=3, batch=batch)
    off_names, off_vec = off_names[2:], off_vec[2:]
    print("launches of the step without:", off_names[0])
    assert "ce_balanced" not in off_names[0]
    assert names["ce_balanced"] == off_names[0]["ce_fwd"] == (1 if batch == 8 else 2), (names, off_names[0])
    # the vectors add no launch: every other kernel runs as often as in the step without them
    assert {k: v for k, v in names.items() if k != "ce_balanced"} == {k: v for k, v in off_names[0].items() if k not in ("ce_fwd", "ce_bwd")}
    objective = 0.0
    for t, kind in (("ar", "class_weights"), ("lta", "class_offsets")):
        y = dev[t].y.cpu()
        ls, gt = [l.float().cpu() for l in seen[t][0]], seen[t][1].cpu()
        assert all(l.dtype == torch.float32 for l in seen[t][0]) and [l.shape[1] for l in ls] == [115, 478]
        v = [x.cpu() for x in vec[t][kind]]
        want, _ = _model(ls, gt, v if kind == "class_weights" else None, v if kind == "class_offsets" else None, 0.0, None)
        if gt.shape != y.shape or not torch.equal(gt, y):
            # a compacted head: the launch ran on the labelled rows (padded to whole 64-row tiles), node n is its row live_inv[n];
            # the other nodes have loss 0
            inv = dev[t].live_inv.cpu()
            assert torch.equal(gt[inv[inv >= 0]], y[inv >= 0]) and bool((y[inv < 0] < 0).all())
            want = torch.where(inv >= 0, want[inv.clamp(min=0)], torch.zeros((), dtype=want.dtype))
        assert vs[t].numel() == y.shape[0] and bool((y >= 0).any())
        assert not vs[t].cpu()[(y < 0).all(1)].ne(0).any()
        print(f"{compute} B={batch} {t}: max |loss - model| = {float((vs[t].cpu().double() - want).abs().max()):.3e}")
        torch.testing.assert_close(vs[t].cpu(), want.float(), msg=lambda s: f"{t}: {s}", **CB.LOSS_TOL)
        assert not torch.equal(vs[t].cpu(), off_vec[0][1][t]), "the vectors changed nothing"
        objective = objective + step.weights[t] * vs[t].double().cpu().mean()
    objective = objective + step.weights["pnr"] * vs["pnr"].double().cpu().mean()
    torch.testing.assert_close(total.double().cpu(), objective, rtol=1e-5, atol=1e-6)


@pytest.mark.parametrize("compute,batch", SIZES, ids=SIZE_IDS)
def test_captured_step_replayed_twice_equals_two_eager_steps(compute, batch, compute_restored):
    def run(use_graph):
        step, opt, dev, merged, _ = _build_step(compute, "on", batch)
        if use_graph:
            step.capture(dev, merged, warmup=2)
            for _ in range(2):
                step.replay()
        else:
            for _ in range(4):
                step.step(dev, merged)
        torch.cuda.synchronize()
        return opt.flat_p.clone().cpu(), step.loss_sums(), int(opt._t_dev)
    p_e, sums_e, t_e = run(False)
    p_g, sums_g, t_g = run(True)
    assert t_e == t_g == 4
    assert torch.equal(p_e, p_g), "captured and eager parameters differ"
    assert sums_e == sums_g and all(n > 0 for _, n in sums_e.values()), (sums_e, sums_g)


# ---- 5. tasks and wrapper -----------------------------------------------------------------------------------------------------------------
def test_wrapper_with_a_joint_label_dataset_uses_the_vectors_of_the_selected_heads():
    from egopack_amd import ops
    from egopack_amd.criterion import CrossEntropyNone, MetricSelectorWrapper

    class Joint:
        has_joint_label, num_labels = True, 3

    heads = (4, 6, 24)
    g = gen(5)
    logits = tuple((3 * torch.randn(ROWS, c, generator=g)).to(DEV) for c in heads)
    y = torch.stack([torch.randint(0, c, (ROWS,), generator=g) for c in heads], 1)
    y[::3] = -1
    w = [(torch.rand(c, generator=g) + 0.5) for c in heads]
    a = [torch.randn(c, generator=g) for c in heads]
    with ops.compute_mode("f32"):
        sep = MetricSelectorWrapper(CrossEntropyNone(label_smoothing=0.1), Joint(), class_weights=w, class_offsets=a).to(DEV)
        got = sep(logits, y.to(DEV))
        want, _ = _model([l.cpu() for l in logits[:2]], y[:, :2], w[:2], a[:2], 0.1, None)
        torch.testing.assert_close(got.cpu(), want.float(), **CB.LOSS_TOL)
        joint = MetricSelectorWrapper(CrossEntropyNone(), Joint(), True, class_weights=w, class_offsets=[None, None, a[2]]).to(DEV)
        got = joint(logits, y.to(DEV))
        want, _ = _model([logits[2].cpu()], y[:, 2:], [w[2]], [a[2]], 0.0, None)
        torch.testing.assert_close(got.cpu(), want.float(), **CB.LOSS_TOL)
        assert torch.equal(joint.eval()(logits, y.to(DEV)), ops.cross_entropy(logits[2:], y[:, 2:].contiguous().to(DEV)))
        single = CrossEntropyNone(label_smoothing=0.1, weight=w[1], offset=a[1]).to(DEV)
        want, _, _ = CB.model(logits[1].cpu(), y[:, 1], w[1], a[1], 0.1)
        torch.testing.assert_close(single(logits[1], y[:, 1].contiguous().to(DEV)).cpu(), want.float(), **CB.LOSS_TOL)


def test_task_compute_loss_uses_the_vectors_only_while_training():
    from egopack_amd import ops
    from egopack_amd.models.tasks import LTATask, RecognitionTask
    heads = (115, 478)
    logits, y, _ = _problem(heads, 31)
    ws, offs = _vectors(heads, "both")
    dl, yd = tuple(l.to(DEV) for l in logits), y.to(DEV)
    with ops.compute_mode("f32"):
        task = RecognitionTask(64, 64, heads).to(DEV)
        plain = ops.cross_entropy(dl, yd)
        lta = LTATask(64, 64, heads).to(DEV)  # (its compute_loss takes no ``return_separate_losses``)
        lta.set_class_balance(ws, None)
        want_lta, _ = _model(logits, y, ws, None, 0.0, None)
        torch.testing.assert_close(lta.train().compute_loss(dl, yd).cpu(), want_lta.float(), **CB.LOSS_TOL)
        assert torch.equal(lta.eval().compute_loss(dl, yd), plain)
        assert torch.equal(task.train().compute_loss(dl, yd), plain)
        task.set_class_balance(ws, [offs[0], None])
        assert task.class_weight_0.device.type == "cuda" and "class_weight_0" not in task.state_dict()
        got, parts = task.train().compute_loss(dl, yd, return_separate_losses=True)
        want, _ = _model(logits, y, ws, [offs[0], None], 0.0, None)
        torch.testing.assert_close(got.cpu(), want.float(), **CB.LOSS_TOL)
        torch.testing.assert_close((parts[0] + parts[1]).cpu(), want.float(), **CB.LOSS_TOL)
        assert torch.equal(task.eval().compute_loss(dl, yd), plain), "a validation loss is the plain cross entropy, bit for bit"
        with pytest.raises(ValueError, match="head 1"):
            task.set_class_balance([ws[0], ws[1][:-1]], None)
        task.class_weight_1 = ws[1][:-1].to(DEV)  # (a vector of the wrong length that reached the op anyway)
        with pytest.raises(ValueError, match="head 1"):
            task.train().compute_loss(dl, yd)


# ---- 6. main_temporal.py: log lines, the checkpoint entry, resume ---------------------------------------------------------------------------
CHILD = r"""
import sys
from pathlib import Path
sys.path.insert(0, sys.argv[1])
tmp = Path(sys.argv[2])
import main_temporal

BASE = ["k=1", "batch_size=4", "synthetic_samples=8", "model.hidden_size=64", "model.temporal_pooling.hidden_size=64",
        "oscc_feat_size=64", "save_model=True", "compute=f32", "optimizer.lr=1e-3", "enabled_tasks=[ar,lta,pnr]",
        "dataset_recognition.T=8", "dataset_lta.T=8", "dataset_pnr.T=8", "dataset_oscc.T=8",
        "class_balance.mode=weight", "lr_scheduler.T_max=2", "use_graph=false", "save_every=1"]
main_temporal.main(BASE + ["num_epochs=2", f"checkpoint_dir={tmp / 'full'}"])
main_temporal.main(BASE + ["num_epochs=1", f"checkpoint_dir={tmp / 'part'}"])
part = tmp / "part" / "MTL_ar-lta-pnr" / "checkpoint.pth"
main_temporal.main(BASE + ["num_epochs=2", f"checkpoint_dir={tmp / 'resumed'}", f"resume_from={part}"])
print("RESUMED-WITH-OTHER-VECTORS", file=sys.stderr, flush=True)
main_temporal.main([a for a in BASE if not a.startswith("class_balance")] + ["class_balance.mode=logit_adjust", "num_epochs=1",
                   "save_model=False", f"checkpoint_dir={tmp / 'other'}", f"resume_from={part}"])
print("CHILD-OK")
"""


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("class_balance_runs")
    script = tmp / "child.py"
    script.write_text(CHILD)
    r = subprocess.run([sys.executable, str(script), str(REPO), str(tmp)], capture_output=True, text=True, cwd=str(tmp), timeout=600)
    assert r.returncode == 0 and "CHILD-OK" in r.stdout, (r.returncode, r.stdout[-3000:], r.stderr[-6000:])
    load = lambda *parts: torch.load(tmp.joinpath(*parts), weights_only=False)
    return dict(log=r.stderr + r.stdout, full=load("full", "MTL_ar-lta-pnr", "checkpoint.pth"),
                part=load("part", "MTL_ar-lta-pnr", "checkpoint.pth"), resumed=load("resumed", "MTL_ar-lta-pnr", "checkpoint.pth"))


@pytest.mark.timeout(600)
def test_main_temporal_logs_stores_and_resumes_bit_for_bit(runs):
    from egopack_amd import train as T
    log, full, part, res = runs["log"], runs["full"], runs["part"], runs["resumed"]
    for t in ("ar", "lta"):
        for h, Cn in enumerate((115, 478)):
            assert log.count(f"class balance {t} head {h} ({Cn} classes): mode weight/effective_number, weight in [") == 3
    assert "class balance lta head 0 (115 classes): mode logit_adjust, offset in [" in log
    cb = full["class_balance"]
    assert cb["config"]["mode"] == "weight" and cb["config"]["scheme"] == "effective_number" and set(cb["vectors"]) == {"ar", "lta"}
    cfg = T.load_config(["synthetic_samples=8", "dataset_recognition.T=8", "dataset_lta.T=8", "class_balance.mode=weight"])
    want = T.build_class_balance(cfg, T.build_datasets(cfg, "train"))
    for t in ("ar", "lta"):
        assert cb["vectors"][t]["offsets"] is None
        for h, Cn in enumerate((115, 478)):
            v = cb["vectors"][t]["weights"][h]
            assert v.dtype == torch.float32 and v.shape == (Cn,) and v.device.type == "cpu" and torch.equal(v, want[t]["weights"][h])
    assert all(k not in key for ckpt in (full, part) for key in ckpt["task/lta"] for k in ("class_weight", "class_offset"))
    # the resumed run: no warning while the vectors agree, one line when they do not; the same bits as the uninterrupted run
    head, tail = log.split("RESUMED-WITH-OTHER-VECTORS")
    assert "differ from the checkpoint's" not in head and tail.count("differ from the checkpoint's") == 1
    assert part["epoch"] == 1 and res["epoch"] == full["epoch"] == 2
    moved = 0.0
    for key in ("temporal_graph", "task/recognition", "task/lta", "task/pnr"):
        for k, v in full[key].items():
            torch.testing.assert_close(res[key][k], v, rtol=0, atol=0, msg=lambda s: f"{key}.{k}: {s}")
            if v.is_floating_point():
                moved = max(moved, float((v - part[key][k]).abs().max()))
    assert moved > 0
    for i, st in full["optimizer"]["state"].items():
        for k in ("exp_avg", "exp_avg_sq"):
            assert torch.equal(st[k], res["optimizer"]["state"][i][k]), (i, k)
    assert all(torch.equal(a, b) for t in ("ar", "lta") for a, b in zip(res["class_balance"]["vectors"][t]["weights"],
                                                                       cb["vectors"][t]["weights"]))
