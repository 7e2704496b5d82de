"""What the ledger of ``_lib.ADDON_HEADERS`` (tests/test_cabi_addons.py) pins for the key "mixup", include/egopack_mixup.h."""
import ctypes

vp, i32, i64, f32 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64, ctypes.c_float

NAMES = ["egk_ce_mix_fused_multi", "egk_mix_rows_multi"]  # sorted
EXEMPT = {}  # (the only admissible reason: "writes no device memory" -- both launches write)
BOUNDS = "tests.test_gpu_bounds_mixup"
PINNED = {  # name: (the prototype as the header spells it, (restype, argtypes) by hand)
    "egk_mix_rows_multi": ("""int egk_mix_rows_multi(egk_stream_t s, int32_t n_seg, const void* const* x_in, void* const* x_out, const int64_t* ld_in,
                       const int64_t* ld_out, const int32_t* rows, const int32_t* const* src, const float* const* lam, int32_t cols,
                       int32_t dtype);""",
                           (ctypes.c_int, [vp, i32, vp, vp, vp, vp, vp, vp, vp, i32, i32])),
    "egk_ce_mix_fused_multi": ("""int egk_ce_mix_fused_multi(egk_stream_t s, int32_t count, const float* const* logits, const int64_t* ld, const int32_t* C,
                           const int32_t* pad, const int64_t* dcol, const int32_t* n_heads, const int64_t* const* y,
                           const int64_t* const* y_b, const int64_t* y_stride, const float* const* lam, float* const* loss,
                           void* const* dlogits, const int64_t* ldd, const int32_t* rows, const float* gscale,
                           const float* const* scales, float smoothing, int32_t dtype);""",
                               (ctypes.c_int, [vp, i32, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, f32, i32])),
}
