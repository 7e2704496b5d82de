"""What the ledger of ``_lib.ADDON_HEADERS`` (tests/test_cabi_addons.py) pins for the key "edge_drop", include/egopack_edge_drop.h."""
import ctypes

vp, i32, u64, f32 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_uint64, ctypes.c_float

NAMES = ["egk_csr_mean_drop_bwd", "egk_csr_mean_drop_fwd"]  # sorted
EXEMPT = {}  # (the only admissible reason: "writes no device memory" -- both launches write)
BOUNDS = "tests.test_gpu_bounds_edge_drop"
PINNED = {  # name: (the prototype as the header spells it, (restype, argtypes) by hand)
    "egk_csr_mean_drop_fwd": ("""int egk_csr_mean_drop_fwd(egk_stream_t s, const void* x, const int32_t* rowptr, const int32_t* col, void* out, float* inv_deg,
                          uint8_t* keep_out, int32_t rows, int32_t cols, int32_t dtype, float p, int32_t flags, uint64_t seed,
                          uint64_t offset, const uint64_t* word);""",
                              (ctypes.c_int, [vp, vp, vp, vp, vp, vp, vp, i32, i32, i32, f32, i32, u64, u64, vp])),
    "egk_csr_mean_drop_bwd": ("""int egk_csr_mean_drop_bwd(egk_stream_t s, const void* dout, const int32_t* t_rowptr, const int32_t* t_col, const float* inv_deg,
                          const void* gate, void* dx, uint8_t* keep_out, int32_t rows, int32_t cols, int32_t dtype, float p,
                          int32_t flags, uint64_t seed, uint64_t offset, const uint64_t* word);""",
                              (ctypes.c_int, [vp, vp, vp, vp, vp, vp, vp, vp, i32, i32, i32, f32, i32, u64, u64, vp])),
}
