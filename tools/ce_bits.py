#!/usr/bin/env python3
"""The bits of the cross-entropy family, for an A/B of two builds of the library (profiles/ce_family_ab.txt).

``dump OUT`` drives every entry point of the family through ``egopack_amd._lib`` on seeded, CPU-generated inputs and saves the raw
bit patterns of every output to ``OUT`` (.npz): egk_ce_fwd / _bwd and their _w forms (null and non-null vectors), the fused forms
(egk_ce_fused, egk_ce_fused_multi, egk_ce_w_fused_multi, their _s forms, a shaped task with margin, gamma and row seeds, and its
forward-only form), egk_ce_mix_fused_multi (lam 0, 1, 0.3, random; with and without a scale), and egk_class_report /
egk_topk_softmax for the shared log-sum-exp.  Rows 1, 5, 67; heads (2, 115) and (478, 513); smoothing 0 and 0.1; f32 and bf16
gradients; pad = C + 3 behind a spare column (a non-zero dcol); ignored labels present.  ``EGK_LIB_PATH`` names the build.
``compare A B`` reports every tensor of two dumps as identical or not; exit status 1 when one differs.
Usage: python tools/ce_bits.py dump OUT | compare A B"""
import ctypes as C
import os
import sys

sys.path.insert(0, os.getcwd())
import numpy as np
import torch

ROWS, HEADS, SMOOTH = (1, 5, 67), ((2, 115), (478, 513)), (0.0, 0.1)


def compare(a, b):
    A, B = np.load(a), np.load(b)
    bad = sorted(set(A.files) ^ set(B.files))
    for k in bad:
        print(f"only in one dump: {k}")
    same = 0
    for k in sorted(set(A.files) & set(B.files)):
        if A[k].shape == B[k].shape and A[k].dtype == B[k].dtype and np.array_equal(A[k], B[k]):
            same += 1
        else:
            bad.append(k)
            print(f"DIFFERENT: {k}")
    groups = sorted({k.split("/")[0] for k in A.files})
    print(f"{same} tensors identical, {len(bad)} different or missing ({len(groups)} entry points: {', '.join(groups)})")
    return 1 if bad else 0


def dump(out_path):
    from egopack_amd import _lib
    lib = _lib.load()
    dev = "cuda"
    out = {}
    S = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)
    P = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    vp = lambda ts: (C.c_void_p * len(ts))(*[None if t is None else t.data_ptr() for t in ts])

    def ok(rc, what):
        if rc != 0:
            raise RuntimeError(f"{what} failed (code {rc}): {_lib.last_error()}")
        torch.cuda.synchronize()

    def keep(name, t):
        t = t.detach().cpu().contiguous()
        out[name] = t.view({1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()]).numpy()

    def labels(rows, Cs, g):
        """[rows, heads + 1] int64 (the last column a poison): random labels, some ignored (-1, and C itself)."""
        y = torch.stack([torch.randint(0, c, (rows,), generator=g) for c in Cs] + [torch.zeros(rows, dtype=torch.int64)], 1)
        for h, c in enumerate(Cs):
            y[h::7, h] = -1
            y[2::7, h] = -1
        if rows > 5:
            y[5, 0] = Cs[0]
        return y

    def task_buffers(rows, Cs, g, dt):
        """One task as tests/test_gpu_mixup.py::run_ce lays it out: logits rows 5 elements apart from the next (NaN between), pad =
        C + 3, the heads' blocks side by side behind a spare column, a gradient buffer filled with 7."""
        z = [torch.randn(rows, c, generator=g) * 3 for c in Cs]
        L = []
        for l in z:
            buf = torch.full((rows, l.shape[1] + 5), float("nan"), device=dev)
            buf[:, :l.shape[1]] = l.to(dev)
            L.append(buf)
        pads = [c + 3 for c in Cs]
        dcol = [1 + sum(pads[:h]) for h in range(len(Cs))]
        y, yb = labels(rows, Cs, g).to(dev), labels(rows, Cs, g).to(dev)
        vec = lambda lo, hi: [(torch.rand(c, generator=g) * (hi - lo) + lo).to(dev) for c in Cs]
        return dict(L=L, Cs=Cs, pads=pads, dcol=dcol, y=y, yb=yb, rows=rows, w=vec(0.2, 2.0), a=vec(-1.0, 1.0), m=vec(0.0, 0.5),
                    gloss=(torch.randn(rows, generator=g)).to(dev),
                    loss=torch.full((rows,), float("nan"), device=dev),
                    D=torch.full((rows, 1 + sum(pads) + 2), 7.0, dtype=dt, device=dev))

    def fill(t, b, gscale, vecs=False, shaped=False, loss_only=False):
        """One egk_ce_task (``t`` the task, or the base of an egk_ce_w_task ``w``)."""
        base = t.base if hasattr(t, "base") else t
        for h, l in enumerate(b["L"]):
            base.logits[h], base.ld[h], base.C[h], base.pad[h], base.dcol[h] = l.data_ptr(), l.stride(0), b["Cs"][h], b["pads"][h], b["dcol"][h]
            if vecs:
                t.weight[h], t.offset[h] = b["w"][h].data_ptr(), (b["a"][h].data_ptr() if h == 0 else None)
            if shaped:
                base.margin[h] = b["m"][h].data_ptr() if h == 0 else None
        base.n_heads, base.y, base.y_stride, base.loss = len(b["L"]), b["y"].data_ptr(), b["y"].shape[1], b["loss"].data_ptr()
        base.dlogits, base.ldd, base.rows, base.gscale = (None if loss_only else b["D"].data_ptr()), b["D"].stride(0), b["rows"], gscale
        if shaped:
            base.focal_gamma, base.loss_only = 1.5, int(loss_only)
            base.gloss = None if loss_only else b["gloss"].data_ptr()

    edt = lambda dt: 0 if dt == torch.float32 else 1
    for rows in ROWS:
        for Cs in HEADS:
            for sm in SMOOTH:
                for dt in (torch.float32, torch.bfloat16):
                    tag = f"rows{rows}_C{Cs[0]}x{Cs[1]}_sm{sm}_{'f32' if dt == torch.float32 else 'bf16'}"
                    g = torch.Generator().manual_seed(1000 * rows + Cs[1])
                    fresh = lambda: (task_buffers(rows, Cs, g, dt), task_buffers(5, (20,), g, dt))
                    sc = [torch.tensor([0.7], device=dev), torch.tensor([-1.3], device=dev)]

                    # the two-pass launches, per head, accumulating over the heads
                    for name, vecs in (("egk_ce_fwd", None), ("egk_ce_w_fwd_null", False), ("egk_ce_w_fwd", True)):
                        b, _ = fresh()
                        for h, l in enumerate(b["L"]):
                            lse = torch.empty(rows, device=dev)
                            yh = b["y"][:, h]
                            d = torch.full((rows, Cs[h] + 2), 7.0, dtype=dt, device=dev)
                            w, a = (b["w"][h], b["a"][h]) if vecs else (None, None)
                            if vecs is None:
                                ok(lib.egk_ce_fwd(S(), P(l), l.stride(0), P(yh), b["y"].shape[1], P(b["loss"]), P(lse), rows, Cs[h], sm, int(h > 0)), name)
                                ok(lib.egk_ce_bwd(S(), P(l), l.stride(0), P(yh), b["y"].shape[1], P(lse), P(b["gloss"]), P(d), d.stride(0), rows, Cs[h],
                                                  sm, edt(dt)), name)
                            else:
                                ok(lib.egk_ce_w_fwd(S(), P(l), l.stride(0), P(yh), b["y"].shape[1], P(w), P(a), P(b["loss"]), P(lse), rows, Cs[h], sm,
                                                    int(h > 0)), name)
                                ok(lib.egk_ce_w_bwd(S(), P(l), l.stride(0), P(yh), b["y"].shape[1], P(w), P(a), P(lse), P(b["gloss"]), P(d), d.stride(0),
                                                    rows, Cs[h], sm, edt(dt)), name)
                            keep(f"{name}/{tag}/lse{h}", lse)
                            keep(f"{name.replace('fwd', 'bwd')}/{tag}/d{h}", d)
                        keep(f"{name}/{tag}/loss", b["loss"])

                    # the fused launches: two tasks each (the second one small, one head)
                    def fused(name, entry, struct, scaled, **kw):
                        bs = fresh()
                        arr = (struct * 2)()
                        for i, b in enumerate(bs):
                            fill(arr[i], b, 0.37 if i == 0 else -0.01, **kw)
                        args = (S(), arr, vp(sc), 2, sm, edt(dt)) if scaled else (S(), arr, 2, sm, edt(dt))
                        ok(getattr(lib, entry)(*args), entry)
                        for i, b in enumerate(bs):
                            keep(f"{name}/{tag}/loss{i}", b["loss"])
                            if not kw.get("loss_only"):
                                keep(f"{name}/{tag}/D{i}", b["D"])

                    fused("egk_ce_fused_multi", "egk_ce_fused_multi", _lib.CETask, False)
                    fused("egk_ce_fused_multi_s", "egk_ce_fused_multi_s", _lib.CETask, True)
                    fused("egk_ce_w_fused_multi_null", "egk_ce_w_fused_multi", _lib.CEWTask, False)
                    fused("egk_ce_w_fused_multi", "egk_ce_w_fused_multi", _lib.CEWTask, False, vecs=True)
                    fused("egk_ce_w_fused_multi_s", "egk_ce_w_fused_multi_s", _lib.CEWTask, True, vecs=True)
                    fused("egk_ce_fused_multi_shaped", "egk_ce_fused_multi", _lib.CETask, False, shaped=True)
                    fused("egk_ce_w_fused_multi_s_shaped", "egk_ce_w_fused_multi_s", _lib.CEWTask, True, vecs=True, shaped=True)
                    fused("egk_ce_w_fused_multi_loss_only", "egk_ce_w_fused_multi", _lib.CEWTask, False, vecs=True, shaped=True, loss_only=True)

                    b, _ = fresh()
                    n = len(Cs)
                    ok(lib.egk_ce_fused(S(), vp(b["L"]), (C.c_int64 * n)(*[l.stride(0) for l in b["L"]]), (C.c_int32 * n)(*Cs), (C.c_int32 * n)(*b["pads"]),
                                        (C.c_int64 * n)(*b["dcol"]), n, P(b["y"]), b["y"].shape[1], P(b["loss"]), P(b["D"]), b["D"].stride(0), rows, sm,
                                        0.37, edt(dt)), "egk_ce_fused")
                    keep(f"egk_ce_fused/{tag}/loss", b["loss"])
                    keep(f"egk_ce_fused/{tag}/D", b["D"])

                    # the two-target launch, the array form: entry [4 * task + head]
                    for kind in (0.0, 1.0, 0.3, "random"):
                        for scaled in (False, True):
                            bs = fresh()
                            lams = [(torch.rand(b["rows"], generator=g) if kind == "random" else torch.full((b["rows"],), kind)).to(dev) for b in bs]
                            lg, ld, Cn = (C.c_void_p * 8)(), (C.c_int64 * 8)(), (C.c_int32 * 8)()
                            pad, dcol = (C.c_int32 * 8)(), (C.c_int64 * 8)()
                            for i, b in enumerate(bs):
                                for h, l in enumerate(b["L"]):
                                    k = 4 * i + h
                                    lg[k], ld[k], Cn[k], pad[k], dcol[k] = l.data_ptr(), l.stride(0), b["Cs"][h], b["pads"][h], b["dcol"][h]
                            ok(lib.egk_ce_mix_fused_multi(
                                S(), 2, lg, ld, Cn, pad, dcol, (C.c_int32 * 2)(*[len(b["L"]) for b in bs]), vp([b["y"] for b in bs]),
                                vp([b["yb"] for b in bs]), (C.c_int64 * 2)(*[b["y"].shape[1] for b in bs]), vp(lams), vp([b["loss"] for b in bs]),
                                vp([b["D"] for b in bs]), (C.c_int64 * 2)(*[b["D"].stride(0) for b in bs]), (C.c_int32 * 2)(*[b["rows"] for b in bs]),
                                (C.c_float * 2)(0.37, -0.01), vp([sc[0], None]) if scaled else None, sm, edt(dt)), "egk_ce_mix_fused_multi")
                            for i, b in enumerate(bs):
                                keep(f"egk_ce_mix_fused_multi/{tag}/lam{kind}_scaled{int(scaled)}/loss{i}", b["loss"])
                                keep(f"egk_ce_mix_fused_multi/{tag}/lam{kind}_scaled{int(scaled)}/D{i}", b["D"])

                    # the shared log-sum-exp: the validation report's loss and the export's lse / probabilities (dtype: the logits')
                    b, _ = fresh()
                    rep = (_lib.ClassReportTask * len(Cs))()
                    bufs = []
                    for h, l in enumerate(b["L"]):
                        c = Cs[h]
                        conf, top2 = torch.zeros(c, c, dtype=torch.int64, device=dev), torch.zeros(c, c, dtype=torch.int64, device=dev)
                        q24, counts = torch.zeros(c, dtype=torch.int64, device=dev), torch.zeros(4, dtype=torch.int64, device=dev)
                        t = rep[h]
                        t.logits, t.ld, t.labels, t.label_stride, t.rows, t.C = l.data_ptr(), l.stride(0), b["y"][:, h].data_ptr(), b["y"].shape[1], rows, c
                        t.confusion, t.top2, t.loss_q24, t.counts = conf.data_ptr(), top2.data_ptr(), q24.data_ptr(), counts.data_ptr()
                        bufs.append((conf, top2, q24, counts))
                    if dt == torch.float32:
                        ok(lib.egk_class_report(S(), rep, len(Cs)), "egk_class_report")
                        for h, ts in enumerate(bufs):
                            for nm, t in zip(("confusion", "top2", "loss_q24", "counts"), ts):
                                keep(f"egk_class_report/{tag}/{nm}{h}", t)
                    top = (_lib.TopkTask * len(Cs))()
                    k = 2
                    tb = []
                    for h, l in enumerate(b["L"]):
                        x = torch.nan_to_num(l, nan=0.0).to(dt)
                        idx, prob = torch.zeros(rows, k, dtype=torch.int64, device=dev), torch.zeros(rows, k, device=dev)
                        lse = torch.zeros(rows, device=dev)
                        t = top[h]
                        t.logits, t.ld, t.C, t.idx, t.idx_row_stride, t.prob, t.prob_row_stride, t.lse = \
                            x.data_ptr(), x.stride(0), Cs[h], idx.data_ptr(), k, prob.data_ptr(), k, lse.data_ptr()
                        tb.append((x, idx, prob, lse))
                    ok(lib.egk_topk_softmax(S(), top, len(Cs), rows, k, edt(dt)), "egk_topk_softmax")
                    for h, (_, idx, prob, lse) in enumerate(tb):
                        keep(f"egk_topk_softmax/{tag}/idx{h}", idx)
                        keep(f"egk_topk_softmax/{tag}/prob{h}", prob)
                        keep(f"egk_topk_softmax/{tag}/lse{h}", lse)
    np.savez_compressed(out_path, **out)
    print(f"{len(out)} tensors -> {out_path} (library {_lib.LIB_PATH})")
    return 0


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "dump":
        sys.exit(dump(sys.argv[2]))
    if len(sys.argv) == 4 and sys.argv[1] == "compare":
        sys.exit(compare(sys.argv[2], sys.argv[3]))
    sys.exit(__doc__)
