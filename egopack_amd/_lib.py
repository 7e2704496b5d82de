"""ctypes binding of libegopack_hip.so -- the reference-side stub a maintainer adds.

The library is the product: if it is missing this module raises, there is no fallback of any
kind (the CPU oracle under oracle/ is test infrastructure and is never imported from here).
"""
from __future__ import annotations

import ctypes as C
import functools
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
# The headers ARE the table of the C ABI: load() binds every prototype they declare (signatures() below).  A C user includes
# the first, which includes the others; a new header is one more key here.
HEADERS = {key: HERE.parent / "include" / f"egopack_{key}.h" for key in (
    "hip", "optim", "optim_groups", "ema", "ce_balanced", "bce_balanced", "task_scale", "sample", "class_report", "topk", "retrieval")}

# Headers bound from a SECOND table: the same parser, the same rules, their own ledger (tests/test_cabi_lamb.py).  Their prototypes take
# scalars and pointers only, so STRUCTS stays the set the first ledger pins.  HEADERS, signatures() and declared() do not see them.
EXTRA_HEADERS = {"lamb": HERE.parent / "include" / "egopack_lamb.h"}
LAMB_PIECE = 4096  # EGK_LAMB_PIECE (include/egopack_lamb.h)

# The OPEN third table: every later header goes here.  The same parser, the same rules, and one ledger for the whole
# table, tests/test_cabi_addons.py, which reads what it pins per key from tests/cabi_addon_<key>.py -- a new header adds a key here and
# files there.  Scalars and pointers only (STRUCTS stays as ledgered); a name another header of any table declares is refused.
ADDON_HEADERS = {"calibrate": HERE.parent / "include" / "egopack_calibrate.h", "action": HERE.parent / "include" / "egopack_action.h",
                 "mixup": HERE.parent / "include" / "egopack_mixup.h", "edge_drop": HERE.parent / "include" / "egopack_edge_drop.h",
                 "bootstrap": HERE.parent / "include" / "egopack_bootstrap.h"}
BOOT_MAX_R, BOOT_MAX_M, BOOT_MAX_C = 65536, 8, 1024  # EGK_BOOT_MAX_* (include/egopack_bootstrap.h)
EDGE_DROP_SYMMETRIC, EDGE_DROP_KEEP_SELF = 1, 2  # EGK_EDGE_DROP_* (include/egopack_edge_drop.h)
MIX_MAX_SEGMENTS, CE_MIX_MAX_TASKS, CE_MIX_MAX_HEADS = 4, 4, 4  # EGK_MIX_MAX_SEGMENTS, EGK_CE_MIX_MAX_* (include/egopack_mixup.h)
TEMP_MAX_HEADS, TEMP_MAX_K = 8, 64  # EGK_TEMP_MAX_* (include/egopack_calibrate.h)
ACTION_MAX_K, ACTION_MAX_C = 32, 1024  # EGK_ACTION_MAX_* (include/egopack_action.h)

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
                ("y", vp), ("y_stride", i64), ("loss", vp), ("dlogits", vp), ("ldd", i64), ("rows", i32), ("gscale", f32),
                ("margin", vp * 4), ("gloss", vp), ("focal_gamma", f32), ("loss_only", i32), ("reserved", i64)]


class CEWTask(C.Structure):
    """struct egk_ce_w_task (include/egopack_ce_balanced.h): a task of the fused cross entropy + its per-class vectors."""
    _fields_ = [("base", CETask), ("weight", vp * 4), ("offset", vp * 4)]


class OptimDesc(C.Structure):
    """struct egk_optim_desc (include/egopack_optim.h)."""
    _fields_ = [("rule", i32), ("g_dtype", i32), ("n", i64), ("p", vp), ("g", vp), ("state0", vp), ("state1", vp), ("hyper", vp),
                ("t_dev", vp), ("beta1", C.c_double), ("beta2", C.c_double), ("eps", f32), ("weight_decay", f32), ("momentum", f32), ("dampening", f32),
                ("nesterov", i32), ("bf16_shadow", vp), ("bf16_lo_shadow", vp), ("bump_word", vp), ("bump", i64), ("gate", vp),
                ("state_dtype", i32), ("state_round", i32), ("state_seed", u64), ("elem0", i64)]


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

# C typedef name -> Structure: what a ``const egk_x*`` parameter binds to, and what tests/test_cabi.py compares with the header field by field
STRUCTS = {"egk_gemm_desc": GemmDesc, "egk_host_dataset": HostDataset, "egk_host_batch": HostBatch, "egk_host_part": HostPart,
           "egk_host_merged": HostMerged, "egk_ce_task": CETask, "egk_ce_w_task": CEWTask, "egk_optim_desc": OptimDesc,
           "egk_optim_groups": OptimGroups, "egk_ema_desc": EmaDesc, "egk_sample_task": SampleTask,
           "egk_class_report_task": ClassReportTask, "egk_topk_task": TopkTask, "egk_retrieval_task": RetrievalTask}

# ---- the prototypes of the headers as ctypes signatures ---------------------------------------------------------------------------
SCALARS = {"int": C.c_int, "int32_t": i32, "int64_t": i64, "uint64_t": u64, "float": f32, "double": C.c_double, "egk_stream_t": vp}
POINTEES = {"void", "float", "double", "int32_t", "int64_t", "uint8_t", "uint32_t", "uint64_t"}  # T*, T* const*, ... -> c_void_p


def strip_c(text: str) -> str:
    """C text without its comments and preprocessor lines."""
    text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", text, flags=re.S)
    return re.sub(r"^[ \t]*#.*$", "", text, flags=re.M)


def ctype_of(decl: str, where: str):
    """The ctypes type of one C parameter (its name dropped), return type or struct field type.  The rules are fixed: a scalar of
    SCALARS; one pointer to a struct of STRUCTS -> POINTER(Structure); char* -> c_char_p; any other pointer, of any depth, to a
    type of POINTEES -> c_void_p.  Everything else raises: a type nobody listed never becomes c_void_p silently."""
    tokens = [t for t in re.findall(r"\w+|\S", decl) if t != "const"]
    if len(tokens) > 1 and re.fullmatch(r"\w+", tokens[-1]):
        tokens.pop()  # the parameter's name
    base, depth = [t for t in tokens if t != "*"], tokens.count("*")
    if len(base) == 1 and re.fullmatch(r"\w+", base[0]):
        if depth == 0 and base[0] in SCALARS:
            return SCALARS[base[0]]
        if depth == 1 and base[0] in STRUCTS:
            return C.POINTER(STRUCTS[base[0]])
        if depth == 1 and base[0] == "char":
            return C.c_char_p
        if depth >= 1 and base[0] in POINTEES:
            return vp
    raise TypeError(f"{where}: no ctypes rule for '{decl.strip()}'")


def parse_prototypes(text: str, where: str = "<text>") -> dict:
    """name -> (restype, argtypes) of every ``ret egk_name(args);`` of a header's text.  A statement with a parenthesis that is not
    such a prototype, a type ctype_of() refuses and a name declared twice raise, naming ``where``, the function and the text."""
    text = re.sub(r'extern\s*"C"\s*\{', " ", strip_c(text))
    text = re.sub(r"\{[^{}]*\}", " ", text).replace("}", " ")  # struct and enum bodies; the closing brace of extern "C"
    out = {}
    for stmt in text.split(";"):
        stmt = " ".join(stmt.split())
        if "(" not in stmt or stmt.startswith("typedef "):
            continue
        m = re.fullmatch(r"(.+?)\b(egk_\w+) ?\((.*)\)", stmt)
        if m is None:
            raise TypeError(f"{where}: not a prototype of an egk_ entry point: '{stmt}'")
        ret, name, args = m.groups()
        if name in out:
            raise TypeError(f"{where}: {name} is declared twice")
        args = [] if args.strip() in ("", "void") else args.split(",")
        out[name] = (ctype_of(ret + " ", f"{where}: return type of {name}"), [ctype_of(a, f"{where}: {name}") for a in args])
    return out


@functools.lru_cache(maxsize=None)
def signatures() -> dict:
    """header key -> {name: (restype, argtypes)}, parsed from the files of HEADERS (once)."""
    out, owner = {}, {}
    for key, path in HEADERS.items():
        if not path.exists():
            raise RuntimeError(f"{path} is missing: it is header '{key}' of the C ABI, and the binding of libegopack_hip.so is "
                               "read from the headers (there is no second table).")
        out[key] = parse_prototypes(path.read_text(), path.name)
        for name in out[key]:
            if name in owner:
                raise RuntimeError(f"{name} is declared in {HEADERS[owner[name]].name} and again in {path.name}")
            owner[name] = key
    return out


def declared(key: str | None = None) -> list:
    """The sorted entry-point names of one header, or those of all headers in the order of HEADERS."""
    sigs = signatures()
    return sorted(sigs[key]) if key is not None else [name for k in sigs for name in sorted(sigs[k])]


@functools.lru_cache(maxsize=None)
def extra_signatures() -> dict:
    """header key -> {name: (restype, argtypes)} of the files of EXTRA_HEADERS (once); a name a header of HEADERS declares too is
    refused."""
    owner = {name: key for key, table in signatures().items() for name in table}
    out = {}
    for key, path in EXTRA_HEADERS.items():
        if not path.exists():
            raise RuntimeError(f"{path} is missing: it is header '{key}' of the C ABI (EXTRA_HEADERS)")
        out[key] = parse_prototypes(path.read_text(), path.name)
        for name in out[key]:
            if name in owner:
                raise RuntimeError(f"{name} is declared in {path.name} and again under the key '{owner[name]}'")
            owner[name] = key
    return out


@functools.lru_cache(maxsize=None)
def addon_signatures() -> dict:
    """header key -> {name: (restype, argtypes)} of the files of ADDON_HEADERS (once); a name that a header of HEADERS, of
    EXTRA_HEADERS or another add-on declares too is refused."""
    owner = {name: key for tables in (signatures(), extra_signatures()) for key, table in tables.items() for name in table}
    out = {}
    for key, path in ADDON_HEADERS.items():
        if not path.exists():
            raise RuntimeError(f"{path} is missing: it is header '{key}' of the C ABI (ADDON_HEADERS)")
        out[key] = parse_prototypes(path.read_text(), path.name)
        for name in out[key]:
            if name in owner:
                raise RuntimeError(f"{name} is declared in {path.name} and again under the key '{owner[name]}'")
            owner[name] = key
    return out


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
    for table in (*signatures().values(), *extra_signatures().values(), *addon_signatures().values()):  # (raises for a missing header and for a name two headers declare)
        for name, (res, args) in table.items():
            fn = getattr(lib, name)  # AttributeError if the symbol is not exported
            fn.restype = res
            fn.argtypes = args
    _lib = lib
    return lib


def last_error() -> str:
    return load().egk_last_error().decode(errors="replace")
