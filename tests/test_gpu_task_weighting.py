"""Task weights in device memory (include/egopack_task_scale.h) on the GPU.

1. Scale equals seed: every _s entry point, f32 and bf16, with the scales 1.0, 0.5, 0.3 and 1.7, against its sibling with
   fl32(c * scale) by value -- every output and workspace bit for bit.
2. egk_task_scale_prepare: within one f32 ulp of float32(exp(-float64(s))), exactly 1 for s = 0.
3. egk_task_scale_grad against the float64 model of tests/task_weighting_common.py at rtol 1e-6; the same bits over two runs.
4. - 7. the step: ``uncertainty`` and ``manual`` modes, ``none`` is the old path, resume (further down).

Inputs of a family are built once per shape and shared by the scales (``functools.lru_cache``); nothing modifies them."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from tests import task_weighting_common as TW

pytestmark = pytest.mark.gpu
f32, bf16, i64, f64 = torch.float32, torch.bfloat16, torch.int64, torch.float64
DEV = "cuda"


@pytest.fixture(scope="module")
def lib():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from egopack_amd import _lib
    return _lib.load()


def S():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def P(t, off=0):
    return None if t is None else C.c_void_p(t.data_ptr() + off)


def ok(rc, what):
    from egopack_amd import _lib
    assert rc == 0, f"{what} returned {rc}: {_lib.last_error()}"


def edt(dt):
    return 1 if dt == bf16 else 0


def bits(t):
    return t.view(torch.int16 if t.dtype == bf16 else (torch.int64 if t.dtype == f64 else torch.int32))


def same(a, b, what):
    assert a.shape == b.shape and torch.equal(bits(a), bits(b)), f"{what}: {(bits(a) != bits(b)).sum().item()} of {a.numel()} elements differ in bits"


def word(v):
    return torch.tensor([v], dtype=f32, device=DEV)


# ---- 1. scale equals seed --------------------------------------------------------------------------------------------------------
CE_TASKS = [(70, (115, 478), (128, 512)), (13, (3,), (8,)), (13, (115, 478), (128, 512)), (70, (3,), (8,))]  # rows, heads, pads


@functools.lru_cache(maxsize=None)
def _ce_inputs(i, bal):
    rows, Cs, pads = CE_TASKS[i]
    g = torch.Generator().manual_seed(100 + i)
    logits = [(torch.randn(rows, c, generator=g) * 3).to(DEV) for c in Cs]
    y = torch.stack([torch.randint(0, c, (rows,), generator=g) for c in Cs], 1)
    y[1::4, 0] = -1                                                                      # some labels -1
    y[2::5, len(Cs) - 1] = -1
    w = [(torch.rand(c, generator=g) + 0.1).to(DEV) if bal else None for c in Cs]
    a = [(torch.randn(c, generator=g) * 0.5).to(DEV) if bal else None for c in Cs]
    return logits, y.to(DEV), w, a


def _ce_launch(lib, count, dt, bal, gscales, scales):
    """One fused launch over the first ``count`` tasks; ``scales`` None: the sibling.  Returns [(loss, dlogits)]."""
    from egopack_amd import _lib
    arr = ((_lib.CEWTask if bal else _lib.CETask) * count)()
    outs, keep = [], []
    for i in range(count):
        rows, Cs, pads = CE_TASKS[i]
        logits, y, w, a = _ce_inputs(i, bal)
        loss = torch.full((rows,), float("nan"), device=DEV)
        D = torch.full((rows, sum(pads)), float("nan"), device=DEV).to(dt)
        t = arr[i].base if bal else arr[i]
        col = 0
        for h, l in enumerate(logits):
            t.logits[h], t.ld[h], t.C[h], t.pad[h], t.dcol[h] = l.data_ptr(), l.stride(0), Cs[h], pads[h], col
            col += pads[h]
            if bal:
                arr[i].weight[h], arr[i].offset[h] = w[h].data_ptr(), a[h].data_ptr()
        t.n_heads, t.y, t.y_stride, t.loss, t.dlogits, t.ldd, t.rows, t.gscale = len(Cs), y.data_ptr(), len(Cs), loss.data_ptr(), D.data_ptr(), \
            D.stride(0), rows, gscales[i]
        outs.append((loss, D))
    if scales is None:
        fn, name = (lib.egk_ce_w_fused_multi, "egk_ce_w_fused_multi") if bal else (lib.egk_ce_fused_multi, "egk_ce_fused_multi")
        ok(fn(S(), arr, count, 0.1, edt(dt)), name)
    else:
        vec = torch.tensor(scales, dtype=f32, device=DEV)
        keep.append(vec)
        ptrs = (C.c_void_p * count)(*[vec.data_ptr() + 4 * i for i in range(count)])
        fn, name = (lib.egk_ce_w_fused_multi_s, "egk_ce_w_fused_multi_s") if bal else (lib.egk_ce_fused_multi_s, "egk_ce_fused_multi_s")
        ok(fn(S(), arr, ptrs, count, 0.1, edt(dt)), name)
    torch.cuda.synchronize()
    return outs


@pytest.mark.parametrize("bal", [False, True], ids=["plain", "balanced"])
@pytest.mark.parametrize("dt", [f32, bf16], ids=["f32", "bf16"])
@pytest.mark.parametrize("count", [1, 2, 4])
def test_fused_cross_entropy_with_a_scale_equals_its_sibling_with_the_product(lib, count, dt, bal):
    base = [0.37 / 70, 0.5 / 13, 1.0 / 13, 2.0 / 70]
    for rot in range(4):                                                                 # every task meets every scale
        scales = [TW.SCALES[(i + rot) % 4] for i in range(count)]
        got = _ce_launch(lib, count, dt, bal, base, scales)
        ref = _ce_launch(lib, count, dt, bal, [TW.scaled_seed(base[i], scales[i]) for i in range(count)], None)
        for i, ((gl, gd), (rl, rd)) in enumerate(zip(got, ref)):
            same(gl, rl, f"loss of task {i} (scale {scales[i]})")
            same(gd, rd, f"dlogits of task {i} (scale {scales[i]})")
            assert bool(torch.isfinite(gd.float()).all()), "an element of the gradient block was not written"


@functools.lru_cache(maxsize=None)
def _bce_inputs(rows, cols, dt):
    g = torch.Generator().manual_seed(rows * 31 + cols)
    f = torch.randn(rows, cols, generator=g).to(dt).to(DEV)
    w = (torch.randn(cols, generator=g) * 0.05).to(dt).to(DEV)
    return f, w, torch.randn(1, generator=g).to(DEV), torch.randint(0, 2, (rows,), generator=g).to(DEV)


def _bce_launch(lib, rows, cols, dt, shape, seed, scale):
    f, w, bias, y = _bce_inputs(rows, cols, dt)
    logits, loss = torch.full((rows,), float("nan"), device=DEV), torch.full((rows,), float("nan"), device=DEV)
    df = torch.full((rows, cols), float("nan"), device=DEV).to(dt)
    ws = torch.full((lib.egk_rowdot_ws_rows(rows) * (cols + 4),), float("nan"), device=DEV)
    flat = torch.zeros(cols + 8, device=DEV)                                             # dw | db
    sc = None if scale is None else word(scale)
    head = (S(), P(f), P(w), P(bias), P(y), P(logits), P(loss), P(df), P(ws), rows, cols, seed)
    if shape is None:
        rc = lib.egk_rowdot_bce(*head, edt(dt)) if sc is None else lib.egk_rowdot_bce_s(*head, P(sc), edt(dt))
    else:
        rc = lib.egk_rowdot_bce_w(*head, *shape, edt(dt)) if sc is None else lib.egk_rowdot_bce_w_s(*head, P(sc), *shape, edt(dt))
    ok(rc, "egk_rowdot_bce*")
    ok(lib.egk_rowdot_reduce(S(), P(ws), P(flat), P(flat, cols * 4), rows, cols), "egk_rowdot_reduce")
    torch.cuda.synchronize()
    return dict(logits=logits, loss=loss, df=df, ws=ws, flat=flat)


@pytest.mark.parametrize("shape", [None, (3.0, 0.5, 2.0)], ids=["plain", "shaped"])
@pytest.mark.parametrize("dt", [f32, bf16], ids=["f32", "bf16"])
@pytest.mark.parametrize("cols", [64, 256, 1024])
def test_one_logit_head_with_a_scale_equals_its_sibling_with_the_product(lib, cols, dt, shape):
    for rows in (1, 13, 70):
        c = 2.0 / rows
        for scale in TW.SCALES:
            got = _bce_launch(lib, rows, cols, dt, shape, c, scale)
            ref = _bce_launch(lib, rows, cols, dt, shape, TW.scaled_seed(c, scale), None)
            for k in ("logits", "loss", "df", "ws", "flat"):                             # (ws: the words no launch writes keep one NaN pattern)
                same(got[k], ref[k], f"{k} (rows {rows}, scale {scale})")
            assert bool(torch.isfinite(got["df"].float()).all())


@functools.lru_cache(maxsize=None)
def _ce2_inputs(n_src, rows, cols, dt):
    g = torch.Generator().manual_seed(n_src * 7 + rows + cols)
    fs = [torch.randn(rows, cols, generator=g).to(dt).to(DEV) for _ in range(n_src)]
    Ws = [(torch.randn(2, cols, generator=g) * 0.05).to(dt).to(DEV) for _ in range(n_src)]
    bs = [torch.randn(2, generator=g).to(DEV) for _ in range(n_src)]
    y = torch.randint(0, 2, (rows,), generator=g)
    y[3::7] = -1
    return fs, Ws, bs, y.to(DEV)


def _ce2_launch(lib, n_src, rows, cols, dt, average, phases, single, seed, scale):
    fs, Ws, bs, y = _ce2_inputs(n_src, rows, cols, dt)
    logits, loss = torch.full((rows, 2), float("nan"), device=DEV), torch.full((rows,), float("nan"), device=DEV)
    gws = torch.full((rows, 2), float("nan"), device=DEV)
    dfs = [torch.full((rows, cols), float("nan"), device=DEV).to(dt) for _ in range(n_src)]
    dws, dbs = [torch.zeros(2, cols, device=DEV) for _ in range(n_src)], [torch.zeros(2, device=DEV) for _ in range(n_src)]
    sc = None if scale is None else word(scale)
    arr = lambda ts: (C.c_void_p * n_src)(*[t.data_ptr() for t in ts])
    if single:
        head = (S(), P(fs[0]), P(Ws[0]), P(bs[0]), P(y), P(logits), P(loss), P(dfs[0]), P(dws[0]), P(dbs[0]), P(gws), rows, cols, 0.1, seed)
        ok(lib.egk_rowdot_ce2(*head, edt(dt)) if sc is None else lib.egk_rowdot_ce2_s(*head, P(sc), edt(dt)), "egk_rowdot_ce2*")
    else:
        for phase in phases:
            head = (S(), n_src, arr(fs), arr(Ws), arr(bs), P(y), P(logits), P(loss), arr(dfs), arr(dws), arr(dbs), P(gws), rows, cols,
                    average | (phase << 1), 0.1, seed)
            ok(lib.egk_rowdot_ce2_multi(*head, edt(dt)) if sc is None else lib.egk_rowdot_ce2_multi_s(*head, P(sc), edt(dt)),
               "egk_rowdot_ce2_multi*")
    torch.cuda.synchronize()
    return dict(logits=logits, loss=loss, gws=gws, **{f"df{k}": t for k, t in enumerate(dfs)}, **{f"dw{k}": t for k, t in enumerate(dws)},
                **{f"db{k}": t for k, t in enumerate(dbs)})


@pytest.mark.parametrize("dt", [f32, bf16], ids=["f32", "bf16"])
@pytest.mark.parametrize("n_src,single", [(1, True), (1, False), (3, False)], ids=["ce2", "multi-1", "multi-3"])
def test_two_logit_head_with_a_scale_equals_its_sibling_with_the_product(lib, n_src, single, dt):
    for rows in (1, 9):
        for cols in (256, 1024):
            for average in ((0,) if single else (0, 1)):
                for phases in (((0,),) if single else ((0,), (1, 2))):
                    c = 1.3 / rows
                    for scale in TW.SCALES:
                        got = _ce2_launch(lib, n_src, rows, cols, dt, average, phases, single, c, scale)
                        ref = _ce2_launch(lib, n_src, rows, cols, dt, average, phases, single, TW.scaled_seed(c, scale), None)
                        for k in got:
                            same(got[k], ref[k], f"{k} (rows {rows}, cols {cols}, average {average}, phases {phases}, scale {scale})")


def test_fill_scaled_from_is_the_rounded_product(lib):
    for n in (1, 70, 2048):
        for scale in TW.SCALES:
            out = torch.full((n,), float("nan"), device=DEV)
            ok(lib.egk_fill_scaled_from(S(), P(out), n, 2.0 / 70, P(word(scale))), "egk_fill_scaled_from")
            same(out.cpu(), torch.full((n,), TW.scaled_seed(2.0 / 70, scale), dtype=f32), f"out (n {n}, scale {scale})")


# ---- 2. prepare --------------------------------------------------------------------------------------------------------------------
def test_prepare_is_exp_of_minus_s_within_one_ulp_and_exactly_one_at_zero(lib):
    s = torch.tensor(TW.LOG_VARS, dtype=f32, device=DEV)
    scale = torch.full_like(s, float("nan"))
    ok(lib.egk_task_scale_prepare(S(), P(s), P(scale), s.numel()), "egk_task_scale_prepare")
    got = scale.cpu().numpy()
    for v, g in zip(TW.LOG_VARS, got):
        ref = TW.prepared_scale(v)
        print(f"s = {v}: scale {float(g)!r}, float32(exp(-float64(s))) {ref!r}")
        assert abs(float(g) - ref) <= TW.ulp32(ref), (v, float(g), ref)
    assert got[0] == np.float32(1.0) and TW.LOG_VARS[0] == 0.0


# ---- 3. grad -----------------------------------------------------------------------------------------------------------------------
def _grad_case(lib, learned):
    g = torch.Generator().manual_seed(5)
    vecs = [torch.rand(1, generator=g) * 3, None, torch.rand(70, generator=g) * 3, torch.rand(2048, generator=g) * 3]  # one absent slot
    counts = [None, None, 140, None]                                                     # vector 2 is compacted: its mean divides by 140
    w = [1.0, 0.5, 2.0, 1.0]
    s = torch.tensor([0.0, 0.4, 0.3, -0.7], dtype=f32)
    scale = torch.tensor([TW.prepared_scale(v) for v in s.tolist()], dtype=f32)
    n = len(vecs)
    dev = [None if v is None else v.to(DEV) for v in vecs]
    s_d, sc_d = s.to(DEV), scale.to(DEV)
    acc0 = torch.tensor([0.5, 1.5, 2.5, 3.5], dtype=f64)
    runs = []
    for _ in range(2):
        ds, obj, acc = torch.full((n,), float("nan"), device=DEV), torch.full((1,), float("nan"), device=DEV), acc0.to(DEV)
        xs = (C.c_void_p * n)(*[None if v is None else v.data_ptr() for v in dev])
        ns = (C.c_int64 * n)(*[0 if v is None else v.numel() for v in dev])
        cn = (C.c_int64 * n)(*[c or 0 for c in counts])
        ok(lib.egk_task_scale_grad(S(), xs, ns, cn, (C.c_float * n)(*w), P(s_d) if learned else None, P(sc_d), P(ds) if learned else None,
                                   P(obj), P(acc), n), "egk_task_scale_grad")
        torch.cuda.synchronize()
        runs.append((ds.cpu(), obj.cpu(), acc.cpu()))
    J, dref, sums = TW.objective(vecs, w, scale.tolist(), s.tolist() if learned else None, counts)
    return runs, J, dref, sums, acc0


@pytest.mark.parametrize("learned", [True, False], ids=["uncertainty", "manual"])
def test_grad_matches_the_float64_model_and_repeats_its_bits(lib, learned):
    runs, J, dref, sums, acc0 = _grad_case(lib, learned)
    ds, obj, acc = runs[0]
    print(f"objective {float(obj):.9g} (model {J:.12g}); ds {ds.tolist()} (model {dref}); sums {(acc - acc0).tolist()} (model {sums})")
    torch.testing.assert_close(obj.double(), torch.tensor([J], dtype=f64), rtol=1e-6, atol=0)
    torch.testing.assert_close(acc - acc0, torch.tensor(sums, dtype=f64), rtol=1e-6, atol=0)
    if learned:
        torch.testing.assert_close(ds.double(), torch.tensor(dref, dtype=f64), rtol=1e-6, atol=0)
        assert float(ds[1]) == 0.0                                                      # the absent task
        same(runs[0][0], runs[1][0], "ds over two runs")
    same(runs[0][1], runs[1][1], "objective over two runs")
    same(runs[0][2], runs[1][2], "accumulated sums over two runs")


# ---- 4. - 7. the step ----------------------------------------------------------------------------------------------------------------
@pytest.fixture
def compute_restored():
    from egopack_amd import ops
    prev = ops.get_compute()
    yield
    ops.set_compute(prev)


def _build_step(mode, compute="bf16", batch=8, clip=0.0, weights=None, key=True, seed=11):
    """The smallest three-task configuration tests/test_gpu_class_balance.py steps: AR + LTA + PNR, B = ``batch`` per task, T = 8,
    H = 64, dropout off, Adam, lr 1e-2.  B = 8 (bf16): AR and LTA share the banked chain and ONE cross-entropy launch, PNR is the
    one-pass head; B = 2: one fused cross entropy per task.  ``key``: False builds without the ``task_weighting`` config key and
    without the step's arguments (the call every caller made before the feature).  ``weights``: overrides of the task weights."""
    import bench
    from egopack_amd import engine, ops
    from egopack_amd import train as T
    args = bench.parse_args(["--workload", "mtl", "--batch", str(batch), "--T", "8", "--hidden", "64", "--trn-hidden", "64", "--dropout", "0.0",
                             "--compute", compute])
    ops.set_compute(compute)
    ops.manual_seed(seed)
    model, tasks, crit, w, dev, merged = bench.build_workload(args, 0, torch.device(DEV))
    w = {**w, **(weights or {})}
    model.to(DEV).train()
    for t in tasks.values():
        t.to(DEV).train()
    over = ["optimizer.lr=1e-2"] + ([f"task_weighting.mode={mode}"] if key else []) + ([f"grad_clip_norm={clip}"] if clip else [])
    cfg = T.load_config(over)
    flat = [*model.configure_optimizers(0), *(p for t in ("ar", "oscc", "lta", "pnr") for p in tasks[t].configure_optimizers(0))]
    if not key:
        opt = T.build_optimizer(cfg, T.build_param_groups(cfg, model, tasks), layout_order=flat)
        return engine.MTLStep(model, tasks, crit, w, opt, fused_backbone=True), opt, dev, merged, cfg
    enabled = [t for t in engine.MTLStep.order if w.get(t, 0) > 0 and t in tasks]
    log_var = T.build_task_weighting(cfg, enabled, DEV)
    opt = T.build_optimizer(cfg, T.build_param_groups(cfg, model, tasks), layout_order=flat, log_var=log_var)
    step = engine.MTLStep(model, tasks, crit, w, opt, fused_backbone=True, task_weighting=T.task_weighting_config(cfg)["mode"], log_var=log_var)
    return step, opt, dev, merged, cfg


def _others(step, opt):
    """The flat parameters without the log-variances' slot (the whole buffer when there is none), on the host."""
    p = opt.flat_p.detach().clone().cpu()
    if step.task_log_var is None:
        return p
    lo, n = opt._slot_of[id(step.task_log_var.log_var)]
    assert lo + n == p.numel(), "the log-variances' slot is the last one"
    return p[:lo]


SIZES = [("f32", 2), ("bf16", 2), ("bf16", 8)]
SIZE_IDS = ["f32-B2", "bf16-B2", "bf16-B8-banked"]


@pytest.mark.parametrize("compute,batch", SIZES, ids=SIZE_IDS)
def test_uncertainty_first_step_is_the_fixed_weight_step_and_log_var_follows_the_model(lib, compute, batch, compute_restored):
    step0, opt0, dev0, merged0, _ = _build_step("none", compute, batch)
    step0.step(dev0, merged0)
    step1, opt1, dev1, merged1, _ = _build_step("uncertainty", compute, batch)
    total, vs = step1.step(dev1, merged1)
    torch.cuda.synchronize()
    same(_others(step1, opt1), _others(step0, opt0), "every parameter other than log_var after step 1")
    assert opt1.param_groups[-1]["name"] == "task_weighting" and opt1.param_groups[-1]["weight_decay"] == 0.0
    # d J / d s and J from THIS step's loss vectors (one element per node, ignored nodes 0), s = 0, scale = 1
    w = [step1.weights[t] for t in step1.enabled]
    vecs = [vs[t].detach().float().cpu() for t in step1.enabled]
    J, ds, _ = TW.objective(vecs, w, [1.0] * len(w), [0.0] * len(w))
    p = step1.task_log_var.log_var
    got_ds, got_s = p.grad.detach().double().cpu(), p.detach().double().cpu()
    print(f"J {float(total):.9g} (model {J:.12g}); ds {got_ds.tolist()} (model {ds}); log_var {got_s.tolist()}")
    torch.testing.assert_close(got_ds, torch.tensor(ds, dtype=f64), rtol=1e-6, atol=1e-9)
    torch.testing.assert_close(total.detach().double().cpu().reshape(()), torch.tensor(J, dtype=f64), rtol=1e-6, atol=0)
    # log_var after the step: the optimizer's Adam rule on s = 0 with the model's gradient, in float64 (TW.adam_first_step: the
    # rule's f32 hyperparameters are its inputs)
    grp = opt1.param_groups[-1]
    want = torch.tensor([TW.adam_first_step(g, grp["lr"], *grp["betas"], grp["eps"]) for g in ds], dtype=f64)
    print(f"log_var model {want.tolist()}")
    torch.testing.assert_close(got_s, want, rtol=1e-6, atol=0)
    assert bool((got_s != 0).all())


@pytest.mark.parametrize("compute,batch", SIZES[1:], ids=SIZE_IDS[1:])
def test_uncertainty_three_eager_steps_equal_three_replays(lib, compute, batch, compute_restored):
    def run(use_graph):
        step, opt, dev, merged, _ = _build_step("uncertainty", compute, batch)
        if use_graph:
            step.capture(dev, merged, warmup=2)
            for _ in range(3):
                step.replay()
        else:
            for _ in range(5):
                step.step(dev, merged)
        torch.cuda.synchronize()
        lv = step.task_log_var.log_var.detach().clone().cpu()
        return opt.flat_p.clone().cpu(), [b.clone().cpu() for b in opt._state_bufs], lv, step.loss_sums(), step.captures
    pe, me, lve, sums_e, cap_e = run(False)
    pg, mg, lvg, sums_g, cap_g = run(True)
    print("log_var after five steps:", lve.tolist())
    same(pg, pe, "parameters, replayed against eager")
    for i, (a, b) in enumerate(zip(mg, me)):
        same(a, b, f"optimizer state buffer {i}, replayed against eager")
    same(lvg, lve, "log_var")
    assert sums_e == sums_g and (cap_e, cap_g) == (0, 1)
    assert bool(torch.isfinite(pe).all()) and bool((lve != 0).all())


def test_uncertainty_with_clipping_skips_a_non_finite_step_and_leaves_log_var(lib, compute_restored):
    step, opt, dev, merged, _ = _build_step("uncertainty", "bf16", 8, clip=1.0)
    for _ in range(2):
        step.step(dev, merged)
    torch.cuda.synchronize()
    before = (opt.flat_p.clone(), [b.clone() for b in opt._state_bufs], step.task_log_var.log_var.detach().clone())
    keep = merged.x[5, 1, 9].clone()
    merged.x[5, 1, 9] = float("inf")
    step.step(dev, merged)
    torch.cuda.synchronize()
    same(opt.flat_p, before[0], "parameters over a skipped step")
    same(step.task_log_var.log_var.detach(), before[2], "log_var over a skipped step")
    for i, (a, b) in enumerate(zip(opt._state_bufs, before[1])):
        same(a, b, f"optimizer state buffer {i} over a skipped step")
    merged.x[5, 1, 9] = keep
    step.step(dev, merged)
    torch.cuda.synchronize()
    assert step.grad_norm_stats()["skipped"] == 1
    assert not torch.equal(step.task_log_var.log_var.detach(), before[2]) and bool(torch.isfinite(opt.flat_p).all())


@pytest.mark.parametrize("compute,batch", SIZES[1:], ids=SIZE_IDS[1:])
def test_manual_scales_change_a_replay_without_a_new_capture(lib, compute, batch, compute_restored):
    """Powers of two keep both seeds exact: scale 0.5 on LTA and 2 on PNR is the step with weight_lta halved and weight_pnr
    doubled, bit for bit."""
    step, opt, dev, merged, _ = _build_step("manual", compute, batch)
    step.capture(dev, merged, warmup=2)              # two eager steps with every scale 1
    assert step.captures == 1
    step.set_task_scale({"lta": 0.5, "pnr": 2.0})
    step.replay()
    torch.cuda.synchronize()
    assert step.captures == 1 and step.task_scales() == {"ar": 1.0, "lta": 0.5, "pnr": 2.0}
    ref, ropt, rdev, rmerged, _ = _build_step("none", compute, batch)
    for _ in range(2):
        ref.step(rdev, rmerged)
    ref.weights["lta"] *= 0.5
    ref.weights["pnr"] *= 2.0
    ref.step(rdev, rmerged)
    torch.cuda.synchronize()
    same(opt.flat_p.cpu(), ropt.flat_p.cpu(), "parameters: a replay with scales (1, 0.5, 2) against an eager step with the weights changed")
    plain, popt, pdev, pmerged, _ = _build_step("none", compute, batch)
    for _ in range(3):
        plain.step(pdev, pmerged)
    torch.cuda.synchronize()
    assert not torch.equal(popt.flat_p.cpu(), opt.flat_p.cpu()), "the scales changed nothing"
    with pytest.raises(ValueError, match="not among the enabled tasks"):
        step.set_task_scale({"oscc": 2.0})
    with pytest.raises(ValueError, match="finite and >= 0"):
        step.set_task_scale({"ar": float("nan")})


@pytest.mark.parametrize("compute,batch", SIZES, ids=SIZE_IDS)
def test_off_is_the_old_path(lib, compute, batch, compute_restored):
    from tests.test_gpu_bounds import _counted

    def run(key):
        step, opt, dev, merged, _ = _build_step("none", compute, batch, key=key)
        names, outs = [], []
        for _ in range(2):
            with _counted(lib) as c:
                total, vs = step.step(dev, merged)
            names.append(dict(c.names))
            outs.append((total.clone().cpu(), {t: v.clone().cpu() for t, v in vs.items()}))
        torch.cuda.synchronize()
        return names, outs, opt.flat_p.clone().cpu(), step.loss_sums()
    n0, o0, p0, s0 = run(False)
    n1, o1, p1, s1 = run(True)
    assert all("task_scale" not in n for n in n0 + n1), n1
    assert n0 == n1 and s0 == s1
    same(p1, p0, "parameters after two steps")
    for (t0, v0), (t1, v1) in zip(o0, o1):
        same(t1, t0, "objective")
        assert v0.keys() == v1.keys()
        for t in v0:
            same(v1[t], v0[t], f"loss vector of {t}")
    # ... and the feature does run its own launches when it is on
    step, opt, dev, merged, _ = _build_step("uncertainty", compute, batch)
    step.step(dev, merged)
    with _counted(lib) as c:
        step.step(dev, merged)
    print("launches of a step with learned task weights:", dict(c.names))
    # prepare, grad, the scaled PNR row pass and the scaled cross entropy -- ONE launch for AR and LTA on the banked chain (B = 8),
    # one per task otherwise -- and nothing else; grad REPLACES the objective's rider (a one-workgroup sum_scale launch)
    assert c.names.get("task_scale", 0) == (4 if batch == 8 else 5), dict(c.names)
    assert c.names.get("sum_scale", 0) == n1[1].get("sum_scale", 0) - 1, (dict(c.names), n1[1])
    upd = ("adam", "optim", "optim_groups")  # (the update: one launch either way, the grouped entry point with the extra group)
    assert sum(c.names.get(k, 0) for k in upd) == sum(n1[1].get(k, 0) for k in upd) == 1
    assert {k: v for k, v in c.names.items() if k not in ("task_scale", "sum_scale", *upd)} == \
        {k: v for k, v in n1[1].items() if k not in ("ce_fwd", "ce_balanced", "bce_fwd", "sum_scale", *upd)}, (dict(c.names), n1[1])


def test_uncertainty_resumes_bit_for_bit(lib, tmp_path, compute_restored):
    import logging
    from egopack_amd import train as T
    full, fopt, fdev, fmerged, _ = _build_step("uncertainty", "f32", 2)
    for _ in range(3):
        full.step(fdev, fmerged)
    a, aopt, adev, amerged, cfg = _build_step("uncertainty", "f32", 2)
    for _ in range(2):
        a.step(adev, amerged)
    torch.cuda.synchronize()
    path = tmp_path / "checkpoint.pth"
    T.save_checkpoint(path, a.model, a.tasks, 1, optimizer=aopt, task_weighting=T.task_weighting_state(cfg, a))
    ck = torch.load(path, weights_only=False)
    assert ck["task_weighting"]["tasks"] == ["ar", "lta", "pnr"] and ck["task_weighting"]["config"]["mode"] == "uncertainty"
    same(ck["task_weighting"]["log_var"], a.task_log_var.log_var.detach().cpu(), "the stored log_var")
    assert not any("log_var" in k for key in ("temporal_graph", "task/recognition", "task/lta", "task/pnr") for k in ck[key])
    assert max(ck["optimizer"]["state"]) == len(aopt._all_params()) - 1  # (the log-variances' moments: the indices run on)
    b, bopt, bdev, bmerged, _ = _build_step("uncertainty", "f32", 2)
    ck = T.load_checkpoint(path, b.model, b.tasks, device=DEV, optimizer=bopt)
    assert T.load_task_weighting(logging.getLogger("test"), ck, b)
    b.step(bdev, bmerged)
    torch.cuda.synchronize()
    same(bopt.flat_p.cpu(), fopt.flat_p.cpu(), "parameters (log_var included): two steps + resume + one step against three steps")
    for i, (x, y) in enumerate(zip(bopt._state_bufs, fopt._state_bufs)):
        same(x.cpu(), y.cpu(), f"optimizer state buffer {i}")
    same(b.task_log_var.log_var.detach().cpu(), full.task_log_var.log_var.detach().cpu(), "log_var")


def test_a_head_off_the_announced_seed_paths_starts_from_the_filled_scaled_seed(lib, compute_restored):
    """PNR with the one-pass head switched off runs classifier + BCE on the criterion path: its backward starts from the cached
    ``_coef_grads`` tensor, which egk_fill_scaled_from fills in every step -- eager and inside the captured graph.  Scale 0.5 on
    PNR (a power of two) is the step with weight_pnr halved, bit for bit; one fill launch per step, the cross entropies stay on
    their scaled fused launches."""
    from tests.test_gpu_bounds import _counted

    def build(mode):
        step, opt, dev, merged, _ = _build_step(mode, "bf16", 2)
        step.one_pass_heads = False
        return step, opt, dev, merged
    step, opt, dev, merged = build("manual")
    step.capture(dev, merged, warmup=2)
    step.set_task_scale({"pnr": 0.5})
    step.replay()
    step.replay()
    torch.cuda.synchronize()
    assert step.captures == 1
    ref, ropt, rdev, rmerged = build("none")
    for _ in range(2):
        ref.step(rdev, rmerged)
    ref.weights["pnr"] *= 0.5
    for _ in range(2):
        ref.step(rdev, rmerged)
    torch.cuda.synchronize()
    same(opt.flat_p.cpu(), ropt.flat_p.cpu(), "parameters: two replays with the PNR scale 0.5 against two eager steps with weight_pnr halved")
    with _counted(lib) as c:
        step.step(dev, merged)
    with _counted(lib) as c0:
        ref.step(rdev, rmerged)
    torch.cuda.synchronize()
    print("launches, PNR on the criterion path with a scale:", dict(c.names), "without:", dict(c0.names))
    # two scaled cross entropies, ONE fill, grad; the BCE pair of the criterion path as in the step without scales
    assert c.names.get("task_scale", 0) == 4 and c.names.get("bce_fwd") == c0.names.get("bce_fwd") and c.names.get("bce_bwd") == c0.names.get("bce_bwd") == 1
    same(opt.flat_p.cpu(), ropt.flat_p.cpu(), "parameters after one more eager step each")


def test_uncertainty_warm_starts_from_a_fixed_weight_checkpoint_with_its_optimizer_state(lib, tmp_path, caplog, compute_restored):
    """A checkpoint a ``mode: none`` run wrote -- optimizer state included, no "task_weighting" entry, one parameter group fewer --
    resumes in ``uncertainty`` mode through train.load_checkpoint: s = 0 with fresh moments and ONE log line, every other
    parameter continues the fixed-weight run bit for bit (s = 0 is scale 1 exactly)."""
    import logging
    from egopack_amd import train as T
    full, fopt, fdev, fmerged, _ = _build_step("none", "f32", 2)
    for _ in range(3):
        full.step(fdev, fmerged)
    a, aopt, adev, amerged, cfg = _build_step("none", "f32", 2)
    for _ in range(2):
        a.step(adev, amerged)
    torch.cuda.synchronize()
    path = tmp_path / "checkpoint.pth"
    T.save_checkpoint(path, a.model, a.tasks, 1, optimizer=aopt, task_weighting=T.task_weighting_state(cfg, a))
    saved = torch.load(path, weights_only=False)
    assert "task_weighting" not in saved and len(saved["optimizer"]["param_groups"]) == 1
    b, bopt, bdev, bmerged, _ = _build_step("uncertainty", "f32", 2)
    assert len(bopt.param_groups) == 2
    ck = T.load_checkpoint(path, b.model, b.tasks, device=DEV, optimizer=bopt)
    with caplog.at_level(logging.INFO):
        caplog.clear()
        assert not T.load_task_weighting(logging.getLogger("test"), ck, b)
    assert sum("starting from s = 0" in r.getMessage() for r in caplog.records) == 1
    lv = b.task_log_var.log_var
    assert lv.detach().tolist() == [0.0, 0.0, 0.0] and bopt.materialised and id(lv) in bopt._slot_of
    assert all(float(v.abs().max()) == 0.0 for v in bopt._moment_views[id(lv)])        # fresh moments
    b.step(bdev, bmerged)
    torch.cuda.synchronize()
    same(_others(b, bopt), fopt.flat_p.cpu(), "every parameter other than log_var: two steps + warm start + one step against three steps")
    got = lv.detach().cpu()
    assert bool(torch.isfinite(got).all()) and bool((got != 0).all()) and float(got.abs().max()) < 0.1
    # any other difference in the groups is still refused
    c, copt, _, _, _ = _build_step("uncertainty", "f32", 2)
    bad = {**saved["optimizer"], "param_groups": []}
    with pytest.raises(ValueError, match="different number of parameter groups"):
        copt.load_state_dict(bad)
