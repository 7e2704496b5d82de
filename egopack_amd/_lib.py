"""ctypes binding of libegopack_hip.so -- the reference-side stub a maintainer adds.

The library is the product: if it is missing this module raises, there is no fallback of any
kind (the CPU oracle under oracle/ is test infrastructure and is never imported from here).
"""
from __future__ import annotations

import ctypes as C
import os
import re
from pathlib import Path

# torch must be imported BEFORE the library is dlopen'ed: the PyTorch-ROCm wheel bundles its own HIP /
# HSA runtime; loading ours first would pull the system copies into the process and the second runtime
# then fails with "no ROCm-capable device is detected".  With torch first, the library's
# libamdhip64 dependency resolves to the runtime torch already loaded (one runtime, shared streams).
import torch  # noqa: F401

HERE = Path(__file__).resolve().parent
LIB_PATH = Path(os.environ["EGK_LIB_PATH"]) if os.environ.get("EGK_LIB_PATH") else HERE / "libegopack_hip.so"  # (env: development A/B of two builds)
HEADER = HERE.parent / "include" / "egopack_hip.h"
OPTIM_HEADER = HERE.parent / "include" / "egopack_optim.h"  # included by egopack_hip.h; its symbols: OPTIM_SIGNATURES
OPTIM_GROUPS_HEADER = HERE.parent / "include" / "egopack_optim_groups.h"  # likewise; its symbols: OPTIM_GROUPS_SIGNATURES

EMA_HEADER = HERE.parent / "include" / "egopack_ema.h"  # likewise; its symbols: EMA_SIGNATURES
CE_BALANCED_HEADER = HERE.parent / "include" / "egopack_ce_balanced.h"  # likewise; its symbols: CE_BALANCED_SIGNATURES
BCE_BALANCED_HEADER = HERE.parent / "include" / "egopack_bce_balanced.h"  # likewise; its symbols: BCE_BALANCED_SIGNATURES
TASK_SCALE_HEADER = HERE.parent / "include" / "egopack_task_scale.h"  # likewise; its symbols: TASK_SCALE_SIGNATURES
SAMPLE_HEADER = HERE.parent / "include" / "egopack_sample.h"  # likewise; its symbols: SAMPLE_SIGNATURES
CLASS_REPORT_HEADER = HERE.parent / "include" / "egopack_class_report.h"  # likewise; its symbols: CLASS_REPORT_SIGNATURES
TOPK_HEADER = HERE.parent / "include" / "egopack_topk.h"  # likewise; its symbols: TOPK_SIGNATURES
RETRIEVAL_HEADER = HERE.parent / "include" / "egopack_retrieval.h"  # likewise; its symbols: RETRIEVAL_SIGNATURES

vp, i32, i64, u64, f32 = C.c_void_p, C.c_int32, C.c_int64, C.c_uint64, C.c_float


class GemmDesc(C.Structure):
    """struct egk_gemm_desc (include/egopack_hip.h)."""
    _fields_ = [
        ("M", i32), ("N", i32), ("K1", i32), ("K2", i32),
        ("A1", vp), ("A2", vp), ("B1", vp), ("B2", vp),
        ("lda1", i64), ("lda2", i64), ("ldb1", i64), ("ldb2", i64),
        ("transA", i32), ("transB", i32), ("a_dtype", i32), ("b_dtype", i32),
        ("compute", i32),
        ("C", vp), ("ldc", i64), ("c_dtype", i32),
        ("accumulate", i32), ("act", i32), ("alpha", f32),
        ("bias", vp), ("residual", vp), ("ldr", i64), ("r_dtype", i32),
        ("splitk", i32), ("ws", vp), ("ws_bytes", i64), ("dbias", vp),
        ("st_mode", i32), ("st_nseg", i32), ("st_min_seg_rows", i32), ("st_seg_ptr", vp), ("st_ws", vp), ("st_x", vp),
        ("st_ldx", i64), ("st_stats", vp), ("st_w", vp), ("st_b", vp), ("st_slope", f32),
        ("n_extra", i32), ("xK", i32 * 4), ("xA", vp * 4), ("xB", vp * 4), ("xlda", i64 * 4), ("xldb", i64 * 4),
        ("op_f16", i32),
    ]


class HostDataset(C.Structure):
    """struct egk_host_dataset (include/egopack_hip.h): the per-sample tables of a resident dataset."""
    _fields_ = [("T", i32), ("S", i32), ("train", i32), ("y_heads", i32), ("L", i64), ("y_elems", i64), ("heavy_in_launch", i64),
                ("live_share", C.c_double),
                ("y", vp), ("pos", vp), ("tau", vp), ("first", vp), ("vlen", vp), ("starts", vp), ("ends", vp),
                ("n_tmpl", i64), ("e_max", i64), ("h_max", i64), ("th_max", i64),
                ("t_e", vp), ("t_ei", vp), ("t_col", vp), ("t_tcol", vp), ("t_tw", vp), ("t_rp", vp), ("t_trp", vp), ("t_band", vp),
                ("t_nh", vp), ("t_nth", vp), ("t_hv", vp), ("t_thv", vp), ("t_dmax", vp), ("t_tdmax", vp)]


class HostBatch(C.Structure):
    """struct egk_host_batch (include/egopack_hip.h): the caller-allocated arrays of one batch + what the call reports."""
    _fields_ = [("E", i64), ("heavy_cap", i64), ("t_heavy_cap", i64), ("live_cap", i64),
                ("y", vp), ("pos", vp), ("batch", vp), ("ptr", vp), ("ptr32", vp), ("x_idx", vp), ("edge_index", vp),
                ("rowptr", vp), ("col", vp), ("t_rowptr", vp), ("t_col", vp), ("t_wgt", vp), ("band", vp), ("heavy", vp), ("t_heavy", vp),
                ("live_idx", vp), ("live_inv", vp), ("live_y", vp),
                ("n_heavy", i64), ("n_t_heavy", i64), ("n_live", i64), ("pos_min", i64), ("pos_max", i64),
                ("heavy_mode", i32), ("t_heavy_mode", i32), ("edge_cap", i64), ("live_ap_first", i64), ("live_ap_step", i64)]


class HostPart(C.Structure):
    """struct egk_host_part (include/egopack_hip.h): one task batch as the merged batch's builder reads it."""
    _fields_ = [("n_nodes", i64), ("E", i64), ("n_heavy", i64), ("n_t_heavy", i64), ("edge_stride", i64), ("pos_min", i64), ("pos_max", i64),
                ("pos", vp), ("edge_index", vp), ("rowptr", vp), ("col", vp), ("t_rowptr", vp), ("t_col", vp), ("t_wgt", vp), ("band", vp),
                ("heavy", vp), ("t_heavy", vp), ("heavy_mode", i32), ("t_heavy_mode", i32)]


class HostMerged(C.Structure):
    """struct egk_host_merged (include/egopack_hip.h)."""
    _fields_ = [("edge_cap", i64), ("pos", vp), ("edge_index", vp), ("rowptr", vp), ("col", vp), ("t_rowptr", vp), ("t_col", vp),
                ("t_wgt", vp), ("band", vp), ("heavy", vp), ("t_heavy", vp), ("seg_ptr", vp),
                ("n_nodes", i64), ("E", i64), ("min_seg_rows", i64), ("pos_min", i64), ("pos_max", i64),
                ("heavy_mode", i32), ("t_heavy_mode", i32)]


class CETask(C.Structure):
    """struct egk_ce_task (include/egopack_hip.h)."""
    _fields_ = [("logits", vp * 4), ("ld", i64 * 4), ("C", i32 * 4), ("pad", i32 * 4), ("dcol", i64 * 4), ("n_heads", i32),
                ("y", vp), ("y_stride", i64), ("loss", vp), ("dlogits", vp), ("ldd", i64), ("rows", i32), ("gscale", f32)]


class CEWTask(C.Structure):
    """struct egk_ce_w_task (include/egopack_ce_balanced.h): a task of the fused cross entropy + its per-class vectors."""
    _fields_ = [("base", CETask), ("weight", vp * 4), ("offset", vp * 4)]


class OptimDesc(C.Structure):
    """struct egk_optim_desc (include/egopack_optim.h)."""
    _fields_ = [("rule", i32), ("g_dtype", i32), ("n", i64), ("p", vp), ("g", vp), ("state0", vp), ("state1", vp), ("hyper", vp),
                ("t_dev", vp), ("beta1", C.c_double), ("beta2", C.c_double), ("eps", f32), ("weight_decay", f32), ("momentum", f32), ("dampening", f32),
                ("nesterov", i32), ("bf16_shadow", vp), ("bf16_lo_shadow", vp), ("bump_word", vp), ("bump", i64), ("gate", vp)]


class OptimGroups(C.Structure):
    """struct egk_optim_groups (include/egopack_optim_groups.h)."""
    _fields_ = [("base", i64), ("n_seg", i32), ("n_groups", i32), ("seg_begin", vp), ("seg_group", vp), ("group_hyper", vp)]


class EmaDesc(C.Structure):
    """struct egk_ema_desc (include/egopack_ema.h)."""
    _fields_ = [("ema", vp), ("decay", C.c_double), ("warmup", i32)]


class SampleTask(C.Structure):
    """struct egk_sample_task (include/egopack_sample.h): one head of a categorical-sampling launch."""
    _fields_ = [("logits", vp), ("ld", i64), ("C", i32), ("head", i32), ("out", vp), ("out_row_stride", i64), ("out_k_stride", i64),
                ("lo", vp), ("hi", vp), ("total", vp)]


class ClassReportTask(C.Structure):
    """struct egk_class_report_task (include/egopack_class_report.h): one head of a per-class report launch."""
    _fields_ = [("logits", vp), ("ld", i64), ("labels", vp), ("label_stride", i64), ("rows", i32), ("C", i32),
                ("confusion", vp), ("top2", vp), ("loss_q24", vp), ("counts", vp)]


class TopkTask(C.Structure):
    """struct egk_topk_task (include/egopack_topk.h): one head of a top-k softmax launch."""
    _fields_ = [("logits", vp), ("ld", i64), ("C", i32), ("reserved", i32), ("idx", vp), ("idx_row_stride", i64),
                ("prob", vp), ("prob_row_stride", i64), ("lse", vp)]


class RetrievalTask(C.Structure):
    """struct egk_retrieval_task (include/egopack_retrieval.h): one auxiliary task of a retrieval report launch."""
    _fields_ = [("f", vp), ("f_ld", i64), ("f_act", vp), ("f_act_ld", i64), ("bank", vp), ("bank_ld", i64), ("K", i32), ("reserved", i32),
                ("nn", vp), ("nn_row_stride", i64), ("dist", vp), ("dist_row_stride", i64), ("wins", vp), ("wins_row_stride", i64)]


RETRIEVAL_MAX_TASKS, RETRIEVAL_MAX_K = 8, 32  # EGK_RETRIEVAL_MAX_* (include/egopack_retrieval.h)
TOPK_MAX_TASKS, TOPK_MAX_K = 8, 64  # EGK_TOPK_MAX_* (include/egopack_topk.h)
CLASS_REPORT_MAX_TASKS = 8  # EGK_CLASS_REPORT_MAX_TASKS (include/egopack_class_report.h)
SAMPLE_MAX_TASKS, SAMPLE_MAX_K = 8, 1024  # EGK_SAMPLE_MAX_* (include/egopack_sample.h)
OPT_ADAM, OPT_ADAMW, OPT_SGD = 0, 1, 2  # EGK_OPT_* (include/egopack_optim.h)

# name -> (restype, argtypes); mirrors include/egopack_hip.h one to one
SIGNATURES = {
    "egk_version": (C.c_int, []),
    "egk_last_error": (C.c_char_p, []),
    "egk_prof_enable": (C.c_int, [C.c_int]),
    "egk_prof_reset": (C.c_int, []),
    "egk_prof_count": (C.c_int, []),
    "egk_prof_get": (C.c_int, [C.c_int, C.c_char_p, C.c_int, C.POINTER(i64), C.POINTER(C.c_double),
                               C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    "egk_stamp": (C.c_int, [vp, vp, i32]),
    "egk_tee_split_next": (C.c_int, [vp, vp, i64]),
    "egk_gemm": (C.c_int, [vp, C.POINTER(GemmDesc)]),
    "egk_gemm_stats_blocks": (C.c_int, [C.POINTER(GemmDesc)]),
    "egk_gemm_grouped": (C.c_int, [vp, C.POINTER(GemmDesc), i32]),
    "egk_gemm_ws_bytes": (i64, [C.POINTER(GemmDesc)]),
    "egk_gemm_splitk": (C.c_int, [i32, i32, i32, i32]),
    "egk_gemm_set_pipeline": (C.c_int, [i32]),
    "egk_colsum_ws_len": (C.c_int, [i32, i32]),
    "egk_colsum": (C.c_int, [vp, vp, i64, i32, i32, vp, i32, vp, i32]),
    "egk_rowln_fwd": (C.c_int, [vp, vp, vp, vp, vp, vp, vp, vp, i32, i32, f32, i32, f32, u64, u64, vp, i32]),
    "egk_rowln_bwd_ws_rows": (C.c_int, [i32]),
    "egk_rowln_bwd": (C.c_int, [vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, i32, i32, i32, f32, i32]),
    "egk_ln_bwd_reduce": (C.c_int, [vp, vp, vp, vp, i32, i32, i32]),
    "egk_ln_bwd_reduce_multi": (C.c_int, [vp, vp, vp, vp, vp, vp, vp, i32]),
    "egk_rowln_group_fwd": (C.c_int, [vp, vp, vp, vp, vp, i32, vp, vp, vp, i32, f32, i32, i32]),
    "egk_rowln_group_bwd": (C.c_int, [vp, vp, vp, vp, vp, vp, i32, vp, vp, vp, vp, i32, i32, i32]),
    "egk_graphln_ws_bytes": (i64, [i32, i32, i32]),
    "egk_graphln_fwd": (C.c_int, [vp, vp, vp, vp, vp, vp, vp, i32, i32, i32, f32, f32, vp, i32]),
    "egk_graphln_bwd": (C.c_int, [vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, i32, i32, i32, f32, f32, vp, i32]),
    "egk_rowdot_ws_rows": (i32, [i32]),
    "egk_rowdot_bce": (C.c_int, [vp, vp, vp, vp, vp, vp, vp, vp, vp, i32, i32, f32, i32]),
    "egk_rowdot_reduce": (C.c_int, [vp, vp, vp, vp, i32, i32]),
    "egk_rowdot_ce2_max_rows": (i32, []),
    "egk_rowdot_ce2": (C.c_int, [vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, i32, i32, f32, f32, i32]),
    "egk_rowdot_ce2_multi": (C.c_int, [vp, i32, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, i32, i32, i32, f32, f32, i32]),
    "egk_graphln_stats_blocks": (i32, [i32]),
    "egk_graphln_stats": (C.c_int, [vp, vp, vp, i32, i32, i32, vp, i32]),
    "egk_graphln_bwd_stats": (C.c_int, [vp, vp, vp, vp, vp, vp, vp, i32, i32, i32, f32, vp, i32]),
    "egk_graphln_bwd_finish": (C.c_int, [vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, i32, i32, i32, f32, f32, vp, i32, vp, i32]),
    "egk_graphln_fwd_apply": (C.c_int, [vp, vp, vp, vp, vp, vp, vp, i32, i32, i32, f32, f32, vp, i32, i32]),
    "egk_graphln_bwd_apply": (C.c_int, [vp, vp, vp, vp, vp, vp, vp, vp, i32, i32, i32, f32, f32, vp, i32, vp, i32]),
    "egk_pe_table": (C.c_int, [vp, vp, i64, i32, i32, vp]),
    "egk_pe_add_table": (C.c_int, [vp, vp, vp, vp, vp, i64, i32, vp, i32, i32, i32]),
    "egk_pe_add": (C.c_int, [vp, vp, vp, vp, vp, i32, i32, i32]),
    "egk_csr_gather": (C.c_int, [vp, vp, vp, vp, vp, vp, vp, i32, i32, i32, vp, i32, vp, i32]),
    "egk_csr_gather_banded": (C.c_int, [vp, vp, vp, vp, vp, vp, i32, i32, i32, vp, i32, vp, i32]),
    "egk_csr_heavy_ws_bytes": (i64, [i32, i32]),
    "egk_csr_heavy_threshold": (i32, []),
    "egk_gather_max_fwd": (C.c_int, [vp, vp, vp, vp, vp, vp, i32, i32, i32, i32]),
    "egk_gather_max_group_fwd": (C.c_int, [vp, vp, vp, vp, i32, vp, vp, i32, i32, i32, i32]),
    "egk_gather_max_tune": (C.c_int, [i32]),
    "egk_gather_max_bwd": (C.c_int, [vp, vp, vp, vp, i32, i32, i32, i32, i32]),
    "egk_segment_max_fwd": (C.c_int, [vp, vp, vp, vp, vp, i32, i32, i32]),
    "egk_segment_max_bwd": (C.c_int, [vp, vp, vp, vp, vp, i32, i32, i32, i32]),
    "egk_segment_max_multi_fwd": (C.c_int, [vp, vp, vp, vp, vp, i32, i32, i32, i32]),
    "egk_segment_max_multi_bwd": (C.c_int, [vp, vp, vp, vp, vp, i32, i32, i32, i32, i32]),
    "egk_row_inv_norm": (C.c_int, [vp, vp, vp, i32, i32, i32]),
    "egk_cos_dist": (C.c_int, [vp, vp, i64, vp, vp, vp, i32, i32]),
    "egk_topk_smallest": (C.c_int, [vp, vp, i64, vp, vp, vp, i32, i32, i32]),
    "egk_row_sq_norm": (C.c_int, [vp, vp, vp, i32, i32, i32]),
    "egk_topk_smallest_l2": (C.c_int, [vp, vp, i64, vp, vp, vp, i32, i32, i32]),
    "egk_topk_window": (C.c_int, [vp, vp, i64, vp, i64, vp, i64, vp, vp, vp, vp, vp, i32, i32, i32, i32]),
    "egk_gemm_defer_reduce_next": (C.c_int, [i32]),
    "egk_slab_input_next": (C.c_int, [vp, vp, vp]),
    "egk_gemm_reduce_slabs": (C.c_int, [vp, vp, i32, i32, i32, vp, vp, i64]),
    "egk_topk_window_group": (C.c_int, [vp, vp, i64, vp, i64, vp, i64, vp, vp, vp, vp, vp, i32, i32, i32, i32, i32]),
    "egk_topk_window_group16": (C.c_int, [vp, vp, i64, vp, i64, vp, i64, vp, vp, vp, vp, vp, i32, i32, i32, i32, i32, i32]),
    "egk_residual_ratio16": (C.c_int, [vp, vp, i64, vp, vp, i32, i32, i32]),
    "egk_cast_f16": (C.c_int, [vp, vp, vp, i64]),
    "egk_row_inv_norm_cast": (C.c_int, [vp, vp, vp, vp, vp, i32, i32]),
    "egk_bf16_residual_ratio": (C.c_int, [vp, vp, i64, vp, vp, i32, i32]),
    "egk_gather_max_bank_grad": (C.c_int, [vp, vp, vp, vp, vp, vp, i32, i32, i32, i32]),
    "egk_segment_sum_rows_f64": (C.c_int, [vp, vp, vp, vp, vp, vp, vp, i32, i32, i64, i32]),
    "egk_onehot_sigmoid_loss_fwd": (C.c_int, [vp, vp, vp, vp, i32, i32, i32, f32, f32]),
    "egk_onehot_sigmoid_loss_bwd": (C.c_int, [vp, vp, vp, vp, vp, i32, i32, i32, f32, f32, i32]),
    "egk_ce_fwd": (C.c_int, [vp, vp, i64, vp, i64, vp, vp, i32, i32, f32, i32]),
    "egk_ce_bwd": (C.c_int, [vp, vp, i64, vp, i64, vp, vp, vp, i64, i32, i32, f32, i32]),
    "egk_ce_fused_multi": (C.c_int, [vp, vp, i32, f32, i32]),
    "egk_ce_fused": (C.c_int, [vp, vp, vp, vp, vp, vp, i32, vp, i64, vp, vp, i64, i32, f32, f32, i32]),
    "egk_bce_fwd": (C.c_int, [vp, vp, vp, vp, i32]),
    "egk_bce_bwd": (C.c_int, [vp, vp, vp, vp, vp, i32, i32]),
    "egk_dropout_fwd": (C.c_int, [vp, vp, vp, vp, i64, f32, u64, u64, vp, i32]),
    "egk_dropout_bwd": (C.c_int, [vp, vp, vp, vp, i64, f32, i32]),
    "egk_relu_gate": (C.c_int, [vp, vp, vp, vp, i64, i32]),
    "egk_cast": (C.c_int, [vp, vp, i32, vp, i32, i64]),
    "egk_split_bf16": (C.c_int, [vp, vp, i64, vp, vp, i64, i64, i64]),
    "egk_host_bounded_draws": (i64, [vp, vp, vp, i64, i32, vp]),
    "egk_host_window_rows": (i64, [vp, vp, vp, vp, vp, vp, i64, i32, i32, vp]),
    "egk_host_build_batch": (i64, [C.POINTER(HostDataset), vp, vp, vp, i64, C.POINTER(HostBatch)]),
    "egk_host_batch_sizes": (i64, [C.POINTER(HostDataset), vp, i64, vp]),
    "egk_host_merge_batches": (i64, [C.POINTER(HostPart), i32, C.POINTER(HostMerged)]),
    "egk_tune": (C.c_int, [i32, i32]),
    "egk_weighted_sums": (C.c_int, [vp, vp, vp, vp, i32, vp]),
    "egk_weighted_sums_acc": (C.c_int, [vp, vp, vp, vp, i32, vp, vp]),
    "egk_fill_scaled_multi": (C.c_int, [vp, vp, vp, vp, vp, i32]),
    "egk_copy_blocks": (C.c_int, [vp, vp, vp, vp, i32]),
    "egk_gather_rows": (C.c_int, [vp, vp, i32, i64, i64, vp, vp, i32, i64, i32]),
    "egk_gather_lerp_rows": (C.c_int, [vp, vp, i32, i64, i64, vp, vp, vp, vp, i32, i64, i32]),
    "egk_label_rank": (C.c_int, [vp, vp, i64, vp, i64, vp, i32, i32]),
    "egk_edit_distance": (C.c_int, [vp, vp, i64, i64, i64, vp, i64, i64, vp, i32, i32, i32]),
    "egk_cast_rows": (C.c_int, [vp, vp, i32, i64, vp, i32, i64, i32, i32, i32]),
    "egk_axpby": (C.c_int, [vp, vp, vp, vp, i64, f32, f32]),
    "egk_fill_scaled": (C.c_int, [vp, vp, f32, vp, i64]),
    "egk_sum_scale": (C.c_int, [vp, vp, vp, i64, f32, i32]),
    "egk_adam_step": (C.c_int, [vp, vp, vp, i32, vp, vp, i64, vp, f32, f32, f32, f32, vp]),
    "egk_zero_fill": (C.c_int, [vp, vp, i64]),
    "egk_zero_fill_ranges": (C.c_int, [vp, vp, vp, vp, i32]),
    "egk_adam_step_bump": (C.c_int, [vp, vp, vp, i32, vp, vp, i64, vp, f32, f32, f32, f32, vp, vp, vp, i64]),
    "egk_adam_hyper": (C.c_int, [vp, vp, vp, C.c_double, C.c_double, vp]),
    "egk_grad_sumsq_slots": (C.c_int, [i64]),
    "egk_grad_sumsq": (C.c_int, [vp, vp, i32, i64, vp, i32]),
    "egk_grad_norm_finalize": (C.c_int, [vp, vp, i32, vp, f32, vp, vp, vp, vp]),
    "egk_adam_step_gated": (C.c_int, [vp, vp, vp, i32, vp, vp, i64, vp, f32, f32, f32, f32, vp, vp, vp, i64, vp]),
}


# ... and include/egopack_optim.h, the header egopack_hip.h includes (its own table: the ledgers of the two headers are separate)
OPTIM_SIGNATURES = {
    "egk_optim_step": (C.c_int, [vp, C.POINTER(OptimDesc)]),
}


# ... and include/egopack_optim_groups.h (the third ledger: tests/test_param_groups_cpu.py over tests/test_gpu_bounds_param_groups.py)
OPTIM_GROUPS_SIGNATURES = {
    "egk_optim_step_groups": (C.c_int, [vp, C.POINTER(OptimDesc), C.POINTER(OptimGroups)]),
}


# ... and include/egopack_ema.h (the fourth ledger: tests/test_ema_cpu.py over tests/test_gpu_bounds_ema.py)
EMA_SIGNATURES = {
    "egk_optim_step_ema": (C.c_int, [vp, C.POINTER(OptimDesc), C.POINTER(OptimGroups), C.POINTER(EmaDesc)]),
    "egk_ema_swap": (C.c_int, [vp, vp, vp, i64]),
}


# ... and include/egopack_ce_balanced.h (the fifth ledger: tests/test_class_balance_cpu.py over tests/test_gpu_bounds_class_balance.py)
CE_BALANCED_SIGNATURES = {
    "egk_ce_w_fwd": (C.c_int, [vp, vp, i64, vp, i64, vp, vp, vp, vp, i32, i32, f32, i32]),
    "egk_ce_w_bwd": (C.c_int, [vp, vp, i64, vp, i64, vp, vp, vp, vp, vp, i64, i32, i32, f32, i32]),
    "egk_ce_w_fused_multi": (C.c_int, [vp, C.POINTER(CEWTask), i32, f32, i32]),
}


# ... and include/egopack_bce_balanced.h (the sixth ledger: tests/test_pnr_balance_cpu.py over tests/test_gpu_bounds_pnr_balance.py)
BCE_BALANCED_SIGNATURES = {
    "egk_bce_w_fwd": (C.c_int, [vp, vp, vp, vp, i32, f32, f32, f32]),
    "egk_bce_w_bwd": (C.c_int, [vp, vp, vp, vp, vp, i32, f32, f32, f32, i32]),
    "egk_rowdot_bce_w": (C.c_int, [vp, vp, vp, vp, vp, vp, vp, vp, vp, i32, i32, f32, f32, f32, f32, i32]),
}


# ... and include/egopack_task_scale.h (the seventh ledger: tests/test_task_weighting_cpu.py over tests/test_gpu_bounds_task_weighting.py)
TASK_SCALE_SIGNATURES = {
    "egk_ce_fused_multi_s": (C.c_int, [vp, vp, vp, i32, f32, i32]),
    "egk_ce_w_fused_multi_s": (C.c_int, [vp, C.POINTER(CEWTask), vp, i32, f32, i32]),
    "egk_rowdot_bce_s": (C.c_int, [vp, vp, vp, vp, vp, vp, vp, vp, vp, i32, i32, f32, vp, i32]),
    "egk_rowdot_bce_w_s": (C.c_int, [vp, vp, vp, vp, vp, vp, vp, vp, vp, i32, i32, f32, vp, f32, f32, f32, i32]),
    "egk_rowdot_ce2_s": (C.c_int, [vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, i32, i32, f32, f32, vp, i32]),
    "egk_rowdot_ce2_multi_s": (C.c_int, [vp, i32, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, i32, i32, i32, f32, f32, vp, i32]),
    "egk_task_scale_prepare": (C.c_int, [vp, vp, vp, i32]),
    "egk_task_scale_grad": (C.c_int, [vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, i32]),
    "egk_fill_scaled_from": (C.c_int, [vp, vp, i64, f32, vp]),
}


# ... and include/egopack_sample.h (the eighth ledger: tests/test_lta_sampling_cpu.py over tests/test_gpu_bounds_lta_sampling.py)
SAMPLE_SIGNATURES = {
    "egk_categorical_sample": (C.c_int, [vp, C.POINTER(SampleTask), i32, i32, i32, u64, i64, i64, i32]),
}


# ... and include/egopack_class_report.h (the ninth ledger: tests/test_class_report_cpu.py over tests/test_gpu_bounds_class_report.py)
CLASS_REPORT_SIGNATURES = {
    "egk_class_report": (C.c_int, [vp, C.POINTER(ClassReportTask), i32]),
}


# ... and include/egopack_topk.h (the tenth ledger: tests/test_topk_cpu.py over tests/test_gpu_bounds_topk.py)
TOPK_SIGNATURES = {
    "egk_topk_softmax": (C.c_int, [vp, C.POINTER(TopkTask), i32, i32, i32, i32]),
}


# ... and include/egopack_retrieval.h (the eleventh ledger: tests/test_retrieval_cpu.py over tests/test_gpu_bounds_retrieval.py)
RETRIEVAL_SIGNATURES = {
    "egk_retrieval_report": (C.c_int, [vp, C.POINTER(RetrievalTask), i32, i32, i32, i32, i32, i32]),
}


def _declared(header: Path) -> list:
    text = header.read_text()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(egk_[a-z0-9_]+)\s*\(", text)))


def header_symbols() -> list:
    """Every function name declared in include/egopack_hip.h."""
    return _declared(HEADER)


def optim_header_symbols() -> list:
    """Every function name declared in include/egopack_optim.h."""
    return _declared(OPTIM_HEADER)


def optim_groups_header_symbols() -> list:
    """Every function name declared in include/egopack_optim_groups.h."""
    return _declared(OPTIM_GROUPS_HEADER)


def ema_header_symbols() -> list:
    """Every function name declared in include/egopack_ema.h."""
    return _declared(EMA_HEADER)


def ce_balanced_header_symbols() -> list:
    """Every function name declared in include/egopack_ce_balanced.h."""
    return _declared(CE_BALANCED_HEADER)


def bce_balanced_header_symbols() -> list:
    """Every function name declared in include/egopack_bce_balanced.h."""
    return _declared(BCE_BALANCED_HEADER)


def task_scale_header_symbols() -> list:
    """Every function name declared in include/egopack_task_scale.h."""
    return _declared(TASK_SCALE_HEADER)


def sample_header_symbols() -> list:
    """Every function name declared in include/egopack_sample.h."""
    return _declared(SAMPLE_HEADER)


def class_report_header_symbols() -> list:
    """Every function name declared in include/egopack_class_report.h."""
    return _declared(CLASS_REPORT_HEADER)


def topk_header_symbols() -> list:
    """Every function name declared in include/egopack_topk.h."""
    return _declared(TOPK_HEADER)


def retrieval_header_symbols() -> list:
    """Every function name declared in include/egopack_retrieval.h."""
    return _declared(RETRIEVAL_HEADER)


_lib = None


def load() -> C.CDLL:
    """Load the library (once).  Raises if it has not been built: there is no fallback."""
    global _lib
    if _lib is not None:
        return _lib
    if not LIB_PATH.exists():
        raise RuntimeError(
            f"{LIB_PATH} is missing: build it with `python -m egopack_amd.build` "
            "(or __graft_entry__.build()).  egopack_amd has no CPU / eager fallback.")
    lib = C.CDLL(str(LIB_PATH))
    for name, (res, args) in [*SIGNATURES.items(), *OPTIM_SIGNATURES.items(), *OPTIM_GROUPS_SIGNATURES.items(),
                              *EMA_SIGNATURES.items(), *CE_BALANCED_SIGNATURES.items(), *BCE_BALANCED_SIGNATURES.items(),
                              *TASK_SCALE_SIGNATURES.items(), *SAMPLE_SIGNATURES.items(), *CLASS_REPORT_SIGNATURES.items(),
                              *TOPK_SIGNATURES.items(), *RETRIEVAL_SIGNATURES.items()]:
        fn = getattr(lib, name)  # AttributeError if the symbol is not exported
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def last_error() -> str:
    return load().egk_last_error().decode(errors="replace")
