"""What the ledger of ``_lib.ADDON_HEADERS`` (tests/test_cabi_addons.py) pins for the key "bootstrap", include/egopack_bootstrap.h."""
import ctypes

vp, i32, i64, u64 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64, ctypes.c_uint64

NAMES = ["egk_bootstrap_accumulate", "egk_bootstrap_weights"]  # sorted
EXEMPT = {}  # (the only admissible reason: "writes no device memory" -- both launches write)
BOUNDS = "tests.test_gpu_bounds_bootstrap"
PINNED = {  # name: (the prototype as the header spells it, (restype, argtypes) by hand)
    "egk_bootstrap_accumulate": ("""int egk_bootstrap_accumulate(egk_stream_t s, const int64_t* cluster, const int64_t* num, const int64_t* den, int64_t ld,
                             int32_t rows, int32_t M, const int64_t* label, int64_t label_stride, int32_t class_col, int32_t C,
                             int64_t* acc_num, int64_t* acc_den, int64_t* cls_num, int64_t* cls_den, int32_t R, uint64_t key);""",
                                 (ctypes.c_int, [vp, vp, vp, vp, i64, i32, i32, vp, i64, i32, i32, vp, vp, vp, vp, i32, u64])),
    "egk_bootstrap_weights": ("""int egk_bootstrap_weights(egk_stream_t s, const int64_t* cluster, int32_t rows, int32_t R, uint64_t key, uint8_t* w /* [rows, R] */);""",
                              (ctypes.c_int, [vp, vp, i32, i32, u64, vp])),
}
