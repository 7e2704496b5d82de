"""What the ledger of ``_lib.ADDON_HEADERS`` (tests/test_cabi_addons.py) pins for the key "action", include/egopack_action.h."""
import ctypes

vp, i32, i64 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64

NAMES = ["egk_action_topk", "egk_edit_distance_pairs"]  # sorted
EXEMPT = {}  # (the only admissible reason: "writes no device memory" -- both launches write)
BOUNDS = "tests.test_gpu_bounds_action"
PINNED = {  # name: (the prototype as the header spells it, (restype, argtypes) by hand)
    "egk_action_topk": ("""int egk_action_topk(egk_stream_t s, const void* verb_logits, int64_t ld_v, int32_t Cv, const void* noun_logits, int64_t ld_n,
                    int32_t Cn, const float* beta, const int64_t* verb_labels, int64_t verb_label_stride,
                    const int64_t* noun_labels, int64_t noun_label_stride, int32_t rows, int32_t k, int64_t* pair,
                    int64_t pair_row_stride, float* logp, float* prob, int64_t out_row_stride, float* lse, int32_t* rank,
                    int32_t dtype);""",
                        (ctypes.c_int, [vp, vp, i64, i32, vp, i64, i32, vp, vp, i64, vp, i64, i32, i32, vp, i64, vp, vp, i64, vp, vp, i32])),
    "egk_edit_distance_pairs": ("""int egk_edit_distance_pairs(egk_stream_t s, const int64_t* pred_v, const int64_t* pred_n, int64_t p_sn, int64_t p_sz, int64_t p_sk,
                            const int64_t* label_v, const int64_t* label_n, int64_t l_sn, int64_t l_sz, int32_t* out, int32_t N,
                            int32_t Z, int32_t K);""",
                                (ctypes.c_int, [vp, vp, vp, i64, i64, i64, vp, vp, i64, i64, vp, i32, i32, i32])),
}
