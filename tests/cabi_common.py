"""What the one ledger of the C ABI (tests/test_cabi.py) holds per header key of ``_lib.HEADERS``: the pinned entry-point names, the
exemptions from the guard-band cases, the module that holds those cases -- and the struct bodies of the headers parsed into ctypes
fields.  A new header adds one entry to each of NAMES, EXEMPT and BOUNDS."""
import importlib
import re

from egopack_amd import _lib

# ---- the entry points of every header, sorted: an entry point added to (or lost from) a header fails the ledger until it is listed here
NAMES = {
    "hip": [
        "egk_adam_hyper", "egk_adam_step", "egk_adam_step_bump", "egk_adam_step_gated", "egk_axpby", "egk_bce_bwd",
        "egk_bce_fwd", "egk_bf16_residual_ratio", "egk_cast", "egk_cast_f16", "egk_cast_rows", "egk_ce_bwd", "egk_ce_fused",
        "egk_ce_fused_multi", "egk_ce_fwd", "egk_colsum", "egk_colsum_ws_len", "egk_copy_blocks", "egk_cos_dist",
        "egk_csr_gather", "egk_csr_gather_banded", "egk_csr_heavy_threshold", "egk_csr_heavy_ws_bytes", "egk_dropout_bwd",
        "egk_dropout_fwd", "egk_edit_distance", "egk_fill_scaled", "egk_fill_scaled_multi", "egk_gather_lerp_rows",
        "egk_gather_max_bank_grad", "egk_gather_max_bwd", "egk_gather_max_fwd", "egk_gather_max_group_fwd",
        "egk_gather_max_tune", "egk_gather_rows", "egk_gemm", "egk_gemm_defer_reduce_next", "egk_gemm_grouped",
        "egk_gemm_reduce_slabs", "egk_gemm_set_pipeline", "egk_gemm_splitk", "egk_gemm_stats_blocks", "egk_gemm_ws_bytes",
        "egk_grad_norm_finalize", "egk_grad_sumsq", "egk_grad_sumsq_slots", "egk_graphln_bwd", "egk_graphln_bwd_apply",
        "egk_graphln_bwd_finish", "egk_graphln_bwd_stats", "egk_graphln_fwd", "egk_graphln_fwd_apply", "egk_graphln_stats",
        "egk_graphln_stats_blocks", "egk_graphln_ws_bytes", "egk_host_batch_sizes", "egk_host_bounded_draws",
        "egk_host_build_batch", "egk_host_merge_batches", "egk_host_window_rows", "egk_label_rank", "egk_last_error",
        "egk_ln_bwd_reduce", "egk_ln_bwd_reduce_multi", "egk_onehot_sigmoid_loss_bwd", "egk_onehot_sigmoid_loss_fwd",
        "egk_pe_add", "egk_pe_add_table", "egk_pe_table", "egk_prof_count", "egk_prof_enable", "egk_prof_get", "egk_prof_reset",
        "egk_relu_gate", "egk_residual_ratio16", "egk_row_inv_norm", "egk_row_inv_norm_cast", "egk_row_sq_norm",
        "egk_rowdot_bce", "egk_rowdot_ce2", "egk_rowdot_ce2_max_rows", "egk_rowdot_ce2_multi", "egk_rowdot_reduce",
        "egk_rowdot_ws_rows", "egk_rowln_bwd", "egk_rowln_bwd_ws_rows", "egk_rowln_fwd", "egk_rowln_group_bwd",
        "egk_rowln_group_fwd", "egk_segment_max_bwd", "egk_segment_max_fwd", "egk_segment_max_multi_bwd",
        "egk_segment_max_multi_fwd", "egk_segment_sum_rows_f64", "egk_slab_input_next", "egk_split_bf16", "egk_stamp",
        "egk_sum_scale", "egk_tee_split_next", "egk_topk_smallest", "egk_topk_smallest_l2", "egk_topk_window",
        "egk_topk_window_group", "egk_topk_window_group16", "egk_tune", "egk_version", "egk_weighted_sums",
        "egk_weighted_sums_acc", "egk_zero_fill", "egk_zero_fill_ranges"],
    "optim": ["egk_optim_step"],
    "optim_groups": ["egk_optim_step_groups"],
    "ema": ["egk_ema_swap", "egk_optim_step_ema"],
    "ce_balanced": ["egk_ce_w_bwd", "egk_ce_w_fused_multi", "egk_ce_w_fwd"],
    "bce_balanced": ["egk_bce_w_bwd", "egk_bce_w_fwd", "egk_rowdot_bce_w"],
    "task_scale": ["egk_ce_fused_multi_s", "egk_ce_w_fused_multi_s", "egk_fill_scaled_from", "egk_rowdot_bce_s", "egk_rowdot_bce_w_s",
                   "egk_rowdot_ce2_multi_s", "egk_rowdot_ce2_s", "egk_task_scale_grad", "egk_task_scale_prepare"],
    "sample": ["egk_categorical_sample"],
    "class_report": ["egk_class_report"],
    "topk": ["egk_topk_softmax"],
    "retrieval": ["egk_retrieval_report"],
}

# ---- the guard-band ledger: every entry point of a header has a bounds case, or writes no device memory -------------------------------
# The ONLY admissible reason for an exemption is "writes no device memory" (queries, knobs, the one-shot arming calls -- whose effect
# is covered by the launch they arm, listed in that case's ``covers`` -- and the egk_host_* helpers, which run on the CPU).
EXEMPT = {key: {} for key in NAMES}
EXEMPT["hip"] = {
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
ARMING = {"hip": {"egk_tee_split_next", "egk_gemm_defer_reduce_next", "egk_slab_input_next"}}
# egk_gemm_stats_blocks is a query too, but the statistics case declares it: it sizes the guarded st_ws

# the module that holds the guard-band cases of each header (CASES, covered(); importable without a GPU)
BOUNDS = {
    "hip": "tests.test_gpu_bounds", "optim": "tests.test_gpu_bounds_optim", "optim_groups": "tests.test_gpu_bounds_param_groups",
    "ema": "tests.test_gpu_bounds_ema", "ce_balanced": "tests.test_gpu_bounds_class_balance",
    "bce_balanced": "tests.test_gpu_bounds_pnr_balance", "task_scale": "tests.test_gpu_bounds_task_weighting",
    "sample": "tests.test_gpu_bounds_lta_sampling", "class_report": "tests.test_gpu_bounds_class_report",
    "topk": "tests.test_gpu_bounds_topk", "retrieval": "tests.test_gpu_bounds_retrieval",
}


def bounds(key):
    return importlib.import_module(BOUNDS[key])


def uncovered(key, extra=()):
    """The entry points of a header (and ``extra``) with neither a bounds case nor an exemption: empty, says the ledger."""
    return (set(_lib.declared(key)) | set(extra)) - set(bounds(key).covered()) - set(EXEMPT[key])


# ---- the struct bodies of the headers --------------------------------------------------------------------------------------------
_STRUCT = r"typedef\s+struct\s*\w*\s*\{([^{}]*)\}\s*(\w+)\s*;"  # both forms: ``typedef struct egk_x { } egk_x;`` and ``typedef struct { } egk_x;``


def struct_typedefs(key):
    """typedef name -> body text of every struct the header declares."""
    return {name: body for body, name in re.findall(_STRUCT, _lib.strip_c(_lib.HEADERS[key].read_text()))}


def struct_fields(key, typedef):
    """[(name, ctype), ...] of ``typedef`` as the header of ``key`` declares it: multi-declarator lines (``int32_t M, N;``,
    ``const void *A1, *A2;``), ``[n]`` arrays and nested registered structs; pointer and scalar types by the rules of
    ``_lib.ctype_of``."""
    where, fields = f"{_lib.HEADERS[key].name}: {typedef}", []
    for decl in filter(None, (" ".join(d.split()) for d in struct_typedefs(key)[typedef].split(";"))):
        first, *more = decl.split(",")
        base, stars, name, dim = re.fullmatch(r"(.+?)\s*((?:\*\s*)*)(\w+)\s*(?:\[(\d+)\])?", first.strip()).groups()
        declarators = [(stars, name, dim)] + [re.fullmatch(r"((?:\*\s*)*)(\w+)\s*(?:\[(\d+)\])?", m.strip()).groups() for m in more]
        for stars, name, dim in declarators:
            nested = _lib.STRUCTS.get(base.replace("const", "").strip()) if not stars else None
            ctype = nested or _lib.ctype_of(base + " " + stars, where)
            fields.append((name, ctype * int(dim) if dim else ctype))
    return fields

