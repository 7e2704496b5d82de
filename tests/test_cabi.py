"""The C-ABI library loads on a CPU-only box and exports every symbol include/egopack_hip.h declares
(no compute calls without a GPU)."""
import ctypes

from egopack_amd import _lib


def test_library_is_built_and_loads():
    lib = _lib.load()
    assert lib.egk_version() >= 100
    assert isinstance(_lib.last_error(), str)


def test_every_header_symbol_is_exported_and_bound():
    lib = _lib.load()
    declared = _lib.header_symbols()
    assert len(declared) >= 35
    for name in declared:
        assert hasattr(lib, name), f"{name} declared in include/egopack_hip.h but not exported"
    assert set(declared) == set(_lib.SIGNATURES), set(declared) ^ set(_lib.SIGNATURES)


def test_gemm_descriptor_layout_matches_header():
    # field order / count of struct egk_gemm_desc as declared in the header
    import re
    text = _lib.HEADER.read_text()
    body = re.search(r"typedef struct egk_gemm_desc \{(.*?)\} egk_gemm_desc;", text, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = []
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        for part in decl.split(","):
            names.append(re.findall(r"[A-Za-z_][A-Za-z0-9_]*", part)[-1])
    assert names == [f[0] for f in _lib.GemmDesc._fields_]


def test_argument_errors_are_reported_without_a_gpu():
    lib = _lib.load()
    assert lib.egk_gemm(None, None) == -1  # EGK_EINVAL: null descriptor
    assert "null descriptor" in _lib.last_error()
    assert lib.egk_prof_count() > 30
    assert lib.egk_gemm_splitk(128, 256, 8192, 1) > 1 and lib.egk_gemm_splitk(6144, 1024, 1024, 1) == 1
    assert lib.egk_rowln_bwd_ws_rows(6144) >= 1 and lib.egk_graphln_ws_bytes(6144, 1024, 3) > 0
    name = ctypes.create_string_buffer(64)
    n, ms, fl, by = ctypes.c_int64(), ctypes.c_double(), ctypes.c_double(), ctypes.c_double()
    assert lib.egk_prof_get(0, name, 64, ctypes.byref(n), ctypes.byref(ms), ctypes.byref(fl), ctypes.byref(by)) == 0
    assert name.value.decode().startswith("gemm")
    # the grouped max aggregation: null pointers and a group count outside 1 .. 4
    buf = (ctypes.c_void_p * 4)(1, 1, 1, 1)
    assert lib.egk_gather_max_group_fwd(None, None, buf, buf, 2, None, None, 8, 256, 4, 1) == -1 and "null pointer" in _lib.last_error()
    one = ctypes.c_void_p(1)
    assert lib.egk_gather_max_group_fwd(None, one, buf, buf, 5, one, one, 8, 256, 4, 1) == -1 and "1 .. 4 groups" in _lib.last_error()
    assert lib.egk_gather_max_group_fwd(None, one, buf, buf, 3, one, one, 0, 256, 4, 1) == 0  # (no rows: nothing launched)
    prev = lib.egk_gather_max_tune(-1)
    assert prev in (0, 1) and lib.egk_gather_max_tune(0) == prev and lib.egk_gather_max_tune(prev) == 0


def test_heavy_row_threshold_is_shared_by_the_csr_builder_and_the_kernel():
    """data.build_csr lists EXACTLY the rows the gather kernel leaves to its split launches."""
    from egopack_amd import _lib, data
    assert _lib.load().egk_csr_heavy_threshold() == data.HEAVY_DEGREE
    import torch
    ei = torch.stack([torch.zeros(100, dtype=torch.long), torch.arange(1, 101)])  # node 0 -> 100 targets
    g = data.build_csr(ei, 101)
    assert g.t_heavy.tolist() == [0] and g.heavy.numel() == 0 and g.t_heavy.dtype == torch.int32
    ei = torch.stack([torch.zeros(data.HEAVY_DEGREE, dtype=torch.long), torch.arange(1, data.HEAVY_DEGREE + 1)])
    assert data.build_csr(ei, data.HEAVY_DEGREE + 1).t_heavy.numel() == 0  # exactly the threshold: not listed


# ---- the guard-band ledger: every entry point of the header has a bounds case, or writes no device memory ---------------------------
# The ONLY admissible reason for an exemption is "writes no device memory" (queries, knobs, the one-shot arming calls -- whose effect
# is covered by the launch they arm, listed in that case's ``covers`` -- and the egk_host_* helpers, which run on the CPU).
EXEMPT = {
    "egk_version": "query: writes no device memory",
    "egk_last_error": "query: writes no device memory",
    "egk_prof_enable": "host-side switch of the launch counters: writes no device memory",
    "egk_prof_reset": "host-side counters: writes no device memory",
    "egk_prof_count": "query: writes no device memory",
    "egk_prof_get": "query (synchronises recorded events): writes no device memory",
    "egk_gemm_ws_bytes": "query: writes no device memory",
    "egk_gemm_splitk": "query: writes no device memory",
    "egk_gemm_set_pipeline": "knob: writes no device memory",
    "egk_tune": "knob: writes no device memory",
    "egk_gather_max_tune": "knob: writes no device memory",
    "egk_colsum_ws_len": "query: writes no device memory",
    "egk_rowln_bwd_ws_rows": "query: writes no device memory",
    "egk_graphln_ws_bytes": "query: writes no device memory",
    "egk_graphln_stats_blocks": "query: writes no device memory",
    "egk_rowdot_ws_rows": "query: writes no device memory",
    "egk_rowdot_ce2_max_rows": "query: writes no device memory",
    "egk_csr_heavy_ws_bytes": "query: writes no device memory",
    "egk_csr_heavy_threshold": "query: writes no device memory",
    "egk_grad_sumsq_slots": "query: writes no device memory",
    "egk_host_bounded_draws": "runs on the CPU: writes no device memory",
    "egk_host_window_rows": "runs on the CPU: writes no device memory",
    "egk_host_build_batch": "runs on the CPU: writes no device memory",
    "egk_host_batch_sizes": "runs on the CPU: writes no device memory",
    "egk_host_merge_batches": "runs on the CPU: writes no device memory",
}
# covered by a case (they launch nothing themselves, the launch they arm writes device memory): must NOT be exempt
ARMING = {"egk_tee_split_next", "egk_gemm_defer_reduce_next", "egk_slab_input_next"}
# egk_gemm_stats_blocks is a query too, but the statistics case declares it: it sizes the guarded st_ws


def test_every_entry_point_has_a_bounds_case_or_writes_no_device_memory():
    """A kernel added to the header later fails here until it gets a case in tests/test_gpu_bounds.py."""
    from tests import test_gpu_bounds as B  # (importable without a GPU)
    declared, covered = set(_lib.header_symbols()), set(B.covered())
    assert covered <= declared, f"cases name entry points the header does not declare: {sorted(covered - declared)}"
    assert set(EXEMPT) <= declared, f"exemptions of entry points the header does not declare: {sorted(set(EXEMPT) - declared)}"
    both = covered & set(EXEMPT)
    assert not both, f"in exactly one of the two places: {sorted(both)}"
    missing = declared - covered - set(EXEMPT)
    assert not missing, f"entry points with neither a bounds case nor an exemption: {sorted(missing)}"
    assert all("writes no device memory" in why for why in EXEMPT.values())
    assert ARMING <= covered
    for name, fn, variant, covers, plain in B.CASES:
        assert covers and all(c.startswith("egk_") for c in covers), name
    assert len({c[0] for c in B.CASES}) == len(B.CASES), "case ids must be unique"


def test_unaligned_and_undersized_arguments_are_refused_before_any_launch():
    """Host-side refusals (tests/test_gpu_bounds.py runs the same entry points on the GPU): small fake non-null pointers are safe
    because every check below precedes the first dereference and the first launch -- each call must return EGK_EINVAL with its
    message.  Row kernels access rows of a multiple of 4 columns four elements at a time and take that from the width alone, so
    their launchers refuse base pointers that are not aligned to such a group."""
    lib = _lib.load()
    vp = ctypes.c_void_p
    A, U4, U8 = vp(0x1000), vp(0x1004), vp(0x1008)      # 16-byte aligned / 4 bytes past / 8 bytes past
    arr = lambda *ps: (ctypes.c_void_p * len(ps))(*[p.value for p in ps])
    i32s = lambda *v: (ctypes.c_int32 * len(v))(*v)
    F32, BF16 = 0, 1

    def refused(rc, needle="unaligned pointer"):
        assert rc == -1 and needle in _lib.last_error(), (rc, _lib.last_error())

    # ---- the one-wave row kernels: vec = (cols % 4 == 0) alone
    refused(lib.egk_rowln_fwd(None, U4, A, A, A, A, A, None, 8, 64, 1e-5, 0, 0.0, 0, 0, None, F32))          # x
    refused(lib.egk_rowln_fwd(None, A, U4, A, A, A, A, None, 8, 64, 1e-5, 0, 0.0, 0, 0, None, F32))          # w
    refused(lib.egk_rowln_fwd(None, A, A, A, U4, A, A, None, 8, 64, 1e-5, 0, 0.0, 0, 0, None, BF16))         # y, bf16: 8 bytes
    refused(lib.egk_rowln_fwd(None, A, A, A, A, A, A, vp(0x1002), 8, 64, 1e-5, 0, 0.5, 0, 0, None, F32))     # mask: 4 bytes
    refused(lib.egk_rowln_bwd(None, A, U4, A, A, A, A, None, A, A, A, A, 8, 64, 0, 0.0, F32))
    refused(lib.egk_rowln_group_fwd(None, U4, arr(A), arr(A), i32s(0, 8), 1, A, A, A, 64, 1e-5, 0, F32))
    refused(lib.egk_rowln_group_fwd(None, A, arr(U4), arr(A), i32s(0, 8), 1, A, A, A, 64, 1e-5, 0, F32))
    refused(lib.egk_rowln_group_bwd(None, A, A, arr(A), arr(A), i32s(0, 8), 1, A, A, U8, A, 64, 0, F32))
    refused(lib.egk_graphln_fwd(None, A, A, A, U4, A, A, 1, 8, 64, 1e-5, 0.2, A, F32))
    refused(lib.egk_graphln_bwd(None, U8, A, A, A, A, A, A, A, A, 1, 8, 64, 1e-5, 0.2, A, F32))
    refused(lib.egk_graphln_stats(None, U4, A, 1, 8, 64, A, F32))
    refused(lib.egk_graphln_fwd_apply(None, A, A, U4, A, A, A, 1, 8, 64, 1e-5, 0.2, A, 1, F32))
    refused(lib.egk_graphln_bwd_stats(None, A, U4, A, A, A, A, 1, 8, 64, 0.2, A, F32))
    refused(lib.egk_graphln_bwd_apply(None, A, A, A, A, A, U4, A, 1, 8, 64, 1e-5, 0.2, A, 1, A, F32))
    refused(lib.egk_graphln_bwd_finish(None, A, A, A, A, A, U4, A, A, A, 1, 8, 64, 1e-5, 0.2, A, 1, A, F32))
    refused(lib.egk_rowdot_bce(None, U4, A, A, A, A, A, None, None, 8, 64, 1.0, F32))
    refused(lib.egk_rowdot_ce2(None, A, vp(0x1004), A, A, A, A, None, None, None, None, 8, 64, 0.0, 1.0, BF16))
    refused(lib.egk_colsum(None, A, 64, 8, 64, A, 0, U4, F32))                                                # ws
    refused(lib.egk_pe_add(None, U4, A, A, A, 8, 64, F32))
    refused(lib.egk_pe_add_table(None, A, A, A, U4, 0, 4, A, 8, 64, F32))                                     # table
    refused(lib.egk_csr_gather(None, A, A, A, None, None, U8, 8, 64, F32, None, 0, None, 0))                  # out
    refused(lib.egk_csr_gather_banded(None, vp(0x1004), A, A, A, A, 8, 64, BF16, None, 0, None, 0))           # x, bf16
    refused(lib.egk_gather_max_fwd(None, A, U4, A, A, A, 8, 64, 3, F32))                                      # bank
    refused(lib.egk_gather_max_fwd(None, A, A, A, A, vp(0x1001), 8, 64, 3, F32))                              # arg
    refused(lib.egk_gather_max_bwd(None, U4, A, A, 8, 64, 3, 0, F32))
    refused(lib.egk_gather_max_bwd(None, A, vp(0x1002), A, 8, 63, 3, 0, F32))                                 # (a flat walk: any width)
    refused(lib.egk_gather_max_bank_grad(None, U4, A, A, A, A, 8, 64, 3, F32))
    refused(lib.egk_row_inv_norm(None, U4, A, 8, 64, F32))
    refused(lib.egk_row_sq_norm(None, vp(0x1004), A, 8, 64, BF16))
    refused(lib.egk_segment_sum_rows_f64(None, U4, A, A, A, A, A, 2, 64, 4, F32))
    refused(lib.egk_gather_rows(None, U4, F32, 64, 4, A, A, F32, 8, 64))
    refused(lib.egk_gather_rows(None, A, BF16, 64, 4, A, U8, BF16, 8, 64))
    # ---- entry points that already checked on the host: the refusals get their test here
    refused(lib.egk_row_inv_norm_cast(None, U4, A, A, A, 8, 64), "16-byte aligned input")
    refused(lib.egk_row_inv_norm_cast(None, A, A, A, A, 8, 62), "multiple of 4")
    refused(lib.egk_cast_f16(None, U4, A, 64), "unaligned buffers")
    refused(lib.egk_zero_fill(None, U4, 64), "16-byte aligned")
    refused(lib.egk_zero_fill(None, A, 24), "whole 16-byte groups")
    one = (ctypes.c_int64 * 1)
    refused(lib.egk_zero_fill_ranges(None, U8, one(0), one(16), 1), "16-byte aligned")
    refused(lib.egk_zero_fill_ranges(None, A, one(4), one(16), 1), "whole 16-byte groups")
    refused(lib.egk_adam_step(None, A, U4, F32, A, A, 64, A, 0.9, 0.999, 1e-8, 0.0, None), "16-byte aligned")
    refused(lib.egk_adam_step_bump(None, A, A, F32, A, A, 64, A, 0.9, 0.999, 1e-8, 0.0, vp(0x1004), None, None, 0), "8-byte aligned")
    refused(lib.egk_adam_step_gated(None, A, A, F32, A, A, 64, A, 0.9, 0.999, 1e-8, 0.0, A, vp(0x1002), None, 0, A), "8-byte aligned")
    refused(lib.egk_tee_split_next(vp(0x1004), A, 64), "8-byte aligned")
    refused(lib.egk_slab_input_next(U4, None, A), "16-byte aligned")
    banks = arr(A)
    refused(lib.egk_topk_window_group16(None, A, 64, U4, 64, banks, 64, A, banks, banks, A, None, 1, 8, 64, 64, 4, 1), "16-byte aligned")
    refused(lib.egk_topk_window_group(None, A, 64, A, 64, arr(U4), 64, A, banks, banks, A, None, 1, 8, 64, 64, 4), "16-byte aligned")
    refused(lib.egk_topk_window(None, A, 63, A, 64, A, 64, A, A, A, A, None, 8, 64, 64, 4), "leading dimension")
    # ---- sizes: an entry point that takes a size refuses one byte (one slot) less than the launch needs
    d = _lib.GemmDesc()
    d.M, d.N, d.K1, d.A1, d.B1, d.lda1, d.ldb1, d.C, d.ldc = 128, 128, 1024, 0x1000, 0x1000, 1024, 1024, 0x1000, 128
    d.a_dtype = d.b_dtype = d.compute = BF16
    d.alpha, d.splitk, d.ws = 1.0, 4, 0x1000
    need = lib.egk_gemm_ws_bytes(ctypes.byref(d))
    assert need == 4 * 128 * 128 * 4
    d.ws_bytes = need - 1
    refused(lib.egk_gemm(None, ctypes.byref(d)), "workspace too small")
    # the bias gradient of a dW launch by the column-sum route (f32 operands, K not a multiple of 32: the generic kernel)
    d.splitk, d.transA, d.transB, d.lda1, d.ldb1, d.dbias, d.K1 = 1, 1, 1, 128, 128, 0x1000, 1000
    d.a_dtype = d.b_dtype = d.compute = F32
    need = lib.egk_gemm_ws_bytes(ctypes.byref(d))
    assert need == lib.egk_colsum_ws_len(1000, 128) * 4 > 0
    d.ws_bytes = need - 1
    refused(lib.egk_gemm(None, ctypes.byref(d)), "workspace too small")
    refused(lib.egk_grad_sumsq(None, A, F32, 40000, A, lib.egk_grad_sumsq_slots(40000) - 1), "partial sums")
    refused(lib.egk_rowdot_ce2(None, A, A, A, A, A, A, None, None, None, None, lib.egk_rowdot_ce2_max_rows() + 1, 64, 0.0, 1.0, F32), "at most")
    refused(lib.egk_cast_rows(None, A, F32, 64, A, F32, 64, 8, 60, 65), "zero_cols")
    # disarm whatever a refused call may have left armed
    assert lib.egk_tee_split_next(None, None, 0) == 0 and lib.egk_slab_input_next(None, None, None) == 0
