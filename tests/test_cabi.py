"""The C-ABI library loads on a CPU-only box, exports every symbol the headers of include/ declare and is bound with the types they
declare (no compute calls without a GPU): the one ledger of all headers, the struct layouts, and the prototype parser itself."""
import ctypes

import pytest

from egopack_amd import _lib
from tests import cabi_common as CC


def test_library_is_built_and_loads():
    lib = _lib.load()
    assert lib.egk_version() >= 100
    assert isinstance(_lib.last_error(), str)


# ---- the one ledger of the C ABI: every header of _lib.HEADERS, in one form (tests/cabi_common.py holds what is pinned per header) ---
KEYS = list(_lib.HEADERS)


def test_every_header_has_its_ledger_entries():
    assert KEYS == list(CC.NAMES) == list(CC.EXEMPT) == list(CC.BOUNDS)


@pytest.mark.parametrize("key", KEYS)
def test_every_header_symbol_is_exported_and_bound(key):
    """The names of a header are the pinned ones, and each is exported and bound with the types its prototype declares."""
    lib, header = _lib.load(), _lib.HEADERS[key].name
    declared, sigs = _lib.declared(key), _lib.signatures()[key]
    assert declared == CC.NAMES[key] == sorted(sigs), sorted(set(declared) ^ set(CC.NAMES[key]))
    for name in declared:
        assert hasattr(lib, name), f"{name} declared in include/{header} but not exported"
        fn, (restype, argtypes) = getattr(lib, name), sigs[name]
        assert fn.restype == restype and list(fn.argtypes) == argtypes, name
    if key != "hip":
        assert f'#include "{header}"' in _lib.HEADERS["hip"].read_text()  # (a C user includes one file)


def test_no_entry_point_is_declared_by_two_headers():
    for i, a in enumerate(KEYS):
        for b in KEYS[i + 1:]:
            both = set(_lib.declared(a)) & set(_lib.declared(b))
            assert not both, f"{sorted(both)} declared in {a} and in {b}"
    assert len(_lib.declared()) == len(set(_lib.declared())) == sum(len(v) for v in CC.NAMES.values())


def test_struct_layouts_match_the_headers():
    """Every struct typedef of every header is registered in _lib.STRUCTS, and its Structure has the header's field names, types
    and array lengths in the header's order."""
    seen = {}
    for key in KEYS:
        for typedef in CC.struct_typedefs(key):
            assert typedef not in seen, f"{typedef} declared in {seen[typedef]} and in {key}"
            seen[typedef] = key
    assert set(seen) == set(_lib.STRUCTS), set(seen) ^ set(_lib.STRUCTS)
    for typedef, cls in _lib.STRUCTS.items():
        want, have = CC.struct_fields(seen[typedef], typedef), [(f[0], f[1]) for f in cls._fields_]
        assert [n for n, _ in have] == [n for n, _ in want], typedef
        assert have == want, (typedef, [(h, w) for h, w in zip(have, want) if h != w])


# ---- the prototype parser itself: fixed points written out by hand, and what it must refuse ---------------------------------------
vp, i32, i64, u64, f32, f64 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64, ctypes.c_uint64, ctypes.c_float, ctypes.c_double
P = ctypes.POINTER
PINNED = {  # key, name: the prototype as the header spells it, (restype, argtypes) by hand
    ("hip", "egk_last_error"): ("const char* egk_last_error(void);", (ctypes.c_char_p, [])),
    ("hip", "egk_prof_get"): ("""int egk_prof_get(int id, char* name, int name_len, int64_t* launches, double* total_ms,
                 double* alg_flops, double* alg_bytes);""", (ctypes.c_int, [ctypes.c_int, ctypes.c_char_p, ctypes.c_int, vp, vp, vp, vp])),
    ("hip", "egk_gemm"): ("int egk_gemm(egk_stream_t s, const egk_gemm_desc* d);", (ctypes.c_int, [vp, P(_lib.GemmDesc)])),
    ("hip", "egk_gemm_ws_bytes"): ("int64_t egk_gemm_ws_bytes(const egk_gemm_desc* d);", (i64, [P(_lib.GemmDesc)])),
    ("hip", "egk_rowln_fwd"): ("""int egk_rowln_fwd(egk_stream_t s, const void* x, const float* w, const float* b, void* y, float* mean,
                  float* rstd, uint8_t* mask, int32_t rows, int32_t cols, float eps, int32_t relu, float p,
                  uint64_t seed, uint64_t offset, const uint64_t* dev_offset, int32_t dtype);""",
                                (ctypes.c_int, [vp, vp, vp, vp, vp, vp, vp, vp, i32, i32, f32, i32, f32, u64, u64, vp, i32])),
    ("hip", "egk_host_build_batch"): ("""int64_t egk_host_build_batch(const egk_host_dataset* ds, uint32_t* mt_key, int32_t* mt_pos, const int64_t* idx, int64_t B,
                             egk_host_batch* out);""", (i64, [P(_lib.HostDataset), vp, vp, vp, i64, P(_lib.HostBatch)])),
    ("hip", "egk_ln_bwd_reduce_multi"): ("""int egk_ln_bwd_reduce_multi(egk_stream_t s, const void* const* ws, float* const* dw, float* const* db, const int32_t* rows,
                            const int32_t* cols, const int32_t* n_seg, int32_t count);""", (ctypes.c_int, [vp, vp, vp, vp, vp, vp, vp, i32])),
    ("hip", "egk_adam_hyper"): ("int egk_adam_hyper(egk_stream_t s, const float* src, int64_t* t_dev, double beta1, double beta2, float* hyper);",
                                 (ctypes.c_int, [vp, vp, vp, f64, f64, vp])),
    ("hip", "egk_ce_fused_multi"): ("int egk_ce_fused_multi(egk_stream_t s, const egk_ce_task* tasks, int32_t count, float smoothing, int32_t dtype);",
                                     (ctypes.c_int, [vp, P(_lib.CETask), i32, f32, i32])),
    ("hip", "egk_rowdot_ws_rows"): ("int32_t egk_rowdot_ws_rows(int32_t rows);", (i32, [i32])),
    ("sample", "egk_categorical_sample"): ("""int egk_categorical_sample(egk_stream_t s, const egk_sample_task* tasks, int32_t count, int32_t rows, int32_t K, uint64_t seed,
                           int64_t ordinal, int64_t row0, int32_t dtype);""", (ctypes.c_int, [vp, P(_lib.SampleTask), i32, i32, i32, u64, i64, i64, i32])),
    ("ema", "egk_optim_step_ema"): ("int egk_optim_step_ema(egk_stream_t s, const egk_optim_desc* d, const egk_optim_groups* g, const egk_ema_desc* e);",
                                     (ctypes.c_int, [vp, P(_lib.OptimDesc), P(_lib.OptimGroups), P(_lib.EmaDesc)])),
    ("task_scale", "egk_rowdot_bce_w_s"): ("""int egk_rowdot_bce_w_s(egk_stream_t s, const void* f, const void* w, const float* bias, const int64_t* y, float* logits, float* loss,
                       void* df, float* ws, int32_t rows, int32_t cols, float seed, const float* scale, float pos, float neg,
                       float gamma, int32_t dtype);""", (ctypes.c_int, [vp, vp, vp, vp, vp, vp, vp, vp, vp, i32, i32, f32, vp, f32, f32, f32, i32])),
}


def test_hand_pinned_signatures_are_what_the_parser_reads():
    """The fixed points that keep the parser honest: from the prototype's text alone, and from the header it was copied from."""
    text = "/* a comment with egk_not_a_function(int) in it */\n#include <stdint.h>\n" + "\n// another\n".join(t for t, _ in PINNED.values())
    parsed = _lib.parse_prototypes(text)
    assert sorted(parsed) == sorted(name for _, name in PINNED)
    for (key, name), (_, want) in PINNED.items():
        assert parsed[name] == want, name
        assert _lib.signatures()[key][name] == want, name
    # struct and enum bodies, typedefs and the extern "C" braces declare no entry point; parameter names are optional
    text = 'extern "C" {\ntypedef void* egk_stream_t;\nenum { EGK_A = 0 };\ntypedef struct egk_t { int32_t a, b; } egk_t;\nint egk_f(egk_stream_t, const float* const*, int32_t);\n}\n'
    assert _lib.parse_prototypes(text) == {"egk_f": (ctypes.c_int, [vp, vp, i32])}


@pytest.mark.parametrize("what, text, needle", [
    ("an unknown base type", "int egk_f(egk_stream_t s, size_t n);", "size_t n"),
    ("a pointer to an unknown base type", "int egk_f(const egk_unlisted_desc* d);", "egk_unlisted_desc"),
    ("an unknown return type", "unsigned egk_f(void);", "unsigned"),
    ("a function-pointer parameter", "int egk_f(egk_stream_t s, void (*done)(int32_t, void*), void* arg);", "(*done)"),
    ("a by-value struct", "int egk_f(egk_stream_t s, egk_gemm_desc d);", "egk_gemm_desc d"),
    ("a pointer to a pointer to a struct", "int egk_f(const egk_gemm_desc* const* d);", "egk_gemm_desc"),
    ("a name declared twice", "int egk_f(int32_t a);\nint egk_f(int64_t a);", "declared twice"),
    ("a prototype without the prefix", "int other_f(int32_t a);", "other_f"),
])
def test_the_parser_refuses(what, text, needle):
    """A type the parser does not know never becomes c_void_p silently: it raises, naming the header, the function and the text."""
    with pytest.raises(TypeError) as e:
        _lib.parse_prototypes(text, "some_header.h")
    assert "some_header.h" in str(e.value) and needle in str(e.value), (what, str(e.value))
    if "egk_f" in text:
        assert "egk_f" in str(e.value)


def test_a_missing_header_and_a_name_in_two_headers_are_refused_by_the_loader(tmp_path, monkeypatch):
    monkeypatch.setattr(_lib, "HEADERS", {**_lib.HEADERS, "absent": tmp_path / "egopack_absent.h"})
    _lib.signatures.cache_clear()
    try:
        with pytest.raises(RuntimeError, match="egopack_absent.h is missing.*'absent'"):
            _lib.signatures()
        (tmp_path / "egopack_absent.h").write_text("int egk_version(void);\n")
        with pytest.raises(RuntimeError, match="egk_version is declared in egopack_hip.h and again in egopack_absent.h"):
            _lib.signatures()
    finally:
        monkeypatch.undo()
        _lib.signatures.cache_clear()
    assert list(_lib.signatures()) == KEYS


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


# ---- the guard-band ledger: every entry point of a header has a bounds case, or writes no device memory (tests/cabi_common.py) -------
@pytest.mark.parametrize("key", KEYS)
def test_every_entry_point_has_a_bounds_case_or_writes_no_device_memory(key):
    """A kernel added to a header later fails here until it gets a case in the header's bounds module (cabi_common.BOUNDS)."""
    B, exempt = CC.bounds(key), CC.EXEMPT[key]  # (importable without a GPU)
    declared, covered = set(_lib.declared(key)), set(B.covered())
    assert covered <= declared, f"cases name entry points the header does not declare: {sorted(covered - declared)}"
    assert set(exempt) <= declared, f"exemptions of entry points the header does not declare: {sorted(set(exempt) - declared)}"
    both = covered & set(exempt)
    assert not both, f"in exactly one of the two places: {sorted(both)}"
    missing = CC.uncovered(key)
    assert not missing, f"entry points with neither a bounds case nor an exemption: {sorted(missing)}"
    assert all("writes no device memory" in why for why in exempt.values())
    assert CC.ARMING.get(key, set()) <= covered
    for name, fn, variant, covers, plain in B.CASES:
        assert covers and all(c.startswith("egk_") for c in covers), name
    assert len({c[0] for c in B.CASES}) == len(B.CASES), "case ids must be unique"


def test_the_bounds_modules_hold_their_own_cases():
    """The cases of a header live in their own list, and no entry point is covered from two modules."""
    mods = [CC.bounds(key) for key in KEYS]
    for i, a in enumerate(mods):
        for b in mods[i + 1:]:
            assert a.CASES is not b.CASES and not set(a.covered()) & set(b.covered()), (a.__name__, b.__name__)


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
