"""What the ledger of ``_lib.ADDON_HEADERS`` (tests/test_cabi_addons.py) pins for the key "calibrate", include/egopack_calibrate.h."""
import ctypes

vp, i32, i64, f32 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64, ctypes.c_float

NAMES = ["egk_temp_newton", "egk_temp_scale_rows", "egk_temp_stats", "egk_temp_topk_prob"]  # sorted
EXEMPT = {}  # (the only admissible reason: "writes no device memory" -- all four launches write)
BOUNDS = "tests.test_gpu_bounds_calibration"
PINNED = {  # name: (the prototype as the header spells it, (restype, argtypes) by hand)
    "egk_temp_stats": ("""int egk_temp_stats(egk_stream_t s, const void* logits, int64_t ld, const int64_t* labels, int64_t label_stride,
                   int32_t rows, int32_t C, const float* beta, int64_t* acc, int32_t dtype);""",
                       (ctypes.c_int, [vp, vp, i64, vp, i64, i32, i32, vp, vp, i32])),
}
