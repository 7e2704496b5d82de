"""Every development switch of the package in ONE place: name -> (default, one-line meaning).

A switch is a boolean with a default; the environment overrides it by EXACT name (comma lists):

    EGK_DISABLE=grad_store,x3_tee             turns the named switches off
    EGK_ENABLE=sharded_update                 turns the named switches on
    EGK_DBG=window_cand                       debug prints (``debug()``)

The code asks ``switches.enabled("name")``; a name that is not registered here is a programming error (KeyError), and a name
in the environment that is not registered is reported once (``check_env``) instead of being silently ignored -- the former
``"name" in os.environ.get("EGK_DISABLE", "")`` tests matched SUBSTRINGS (``oscc_one_pass`` also switched ``one_pass`` off).
A switch stays only where its off path is a reference that tests compare against, or a mode of its own (the N-rank modes, the
prototype search's precise pass); settled alternatives are retired and their measurements kept in HISTORY.md.
Default-off entries are the N-rank modes that a caller (or bench.py's probe) opts into.  Knobs with a variable of their own are listed in ``KNOBS``.
``python -m egopack_amd.switches`` prints the table.
"""
from __future__ import annotations

import os
import warnings

# name: (default, meaning)
REGISTRY = {
    # ---- the training step's structure (engine.py) --------------------------------------------------------------------------
    "wgrad_grouping": (True, "H x H weight gradients parked and issued six at a time as one grouped launch"),
    "deferred_forks": (True, "forked launches are issued one launch late so that the dX chain keeps its hardware queue under capture"),
    "oscc_one_pass": (True, "the OSCC head (max pool, 2-logit classifier, cross entropy) as pool + one launch"),
    "graphone_adam": (True, "EgoPack step: Adam over GraphONE's slice beside the backbone's backward"),
    "grad_store": (True, "gradient slots with one writer per step are stored, not cleared and accumulated (every capture)"),
    # ---- EgoPack's precise pass / prototype search ------------------------------------------------------------------------------
    "precise_search": (True, "bf16 modes: the features behind the nearest-prototype search come from a forward-only 'bf16x3' pass"),
    "one_pass": (True, "ONE backbone pass: the bf16 training graph is built from the precise pass's taped results"),
    "x3_tee": (True, "row kernels of the precise pass also store the bf16 halves of their f32 result (split tee)"),
    "x3_lazy_input": (True, "the bf16 input of the precise pass is not widened in memory"),
    "graphone_grouped": (True, "GraphONE's stages of all auxiliary tasks as one chain of grouped launches"),
    # ---- several ranks ----------------------------------------------------------------------------------------------------------
    "one_graph_exchange": (False, "N ranks: ONE hipGraph incl. the RCCL collectives (bench.py's probe decides; the attribute also sets it)"),
    "sharded_update": (False, "N ranks: reduce-scatter -> Adam on 1 / world of the buffers -> all-gather instead of all-reduce + full Adam"),
}

DEBUG = {
    "window_cand": "print the candidate statistics of eager window searches",
    "group_shapes": "print the problems of every grouped contraction launch issued outside a capture",
    "stage_profile": "print a cProfile of the staging thread (engine.StagedBatches) when a training loop's epoch ends",
}

# knobs with a variable of their own
KNOBS = {
    "EGK_LIB_PATH": "another build of libegopack_hip.so (A/B of two builds in one tree)",
}

_seen_env = {}


def _names(var: str) -> list:
    raw = os.environ.get(var, "")
    hit = _seen_env.get(var)
    if hit is not None and hit[0] == raw:
        return hit[1]
    out = [item.strip() for item in raw.split(",") if item.strip()]
    _seen_env[var] = (raw, out)
    unknown = [k for k in out if k not in (DEBUG if var == "EGK_DBG" else REGISTRY)]
    if unknown:
        warnings.warn(f"{var}: unknown switch name(s) {unknown} (see egopack_amd/switches.py)")
    return out


def enabled(name: str) -> bool:
    """The switch's value: its default unless EGK_DISABLE / EGK_ENABLE name it (EGK_DISABLE wins)."""
    default = REGISTRY[name][0]
    if name in _names("EGK_DISABLE"):
        return False
    if name in _names("EGK_ENABLE"):
        return True
    return default


def override(name: str):
    """True / False when the environment names the switch, None when it does not (per-object defaults: engine attributes)."""
    REGISTRY[name]
    if name in _names("EGK_DISABLE"):
        return False
    if name in _names("EGK_ENABLE"):
        return True
    return None


def debug(name: str) -> bool:
    DEBUG[name]
    return name in _names("EGK_DBG")


def table() -> str:
    rows = [f"{'switch':26s} default  meaning"]
    for k, (d, m) in REGISTRY.items():
        rows.append(f"{k:26s} {'on ' if d else 'off'}      {m}")
    rows.append("")
    rows += [f"EGK_DBG={k:18s}          {m}" for k, m in DEBUG.items()]
    rows += [f"{k:26s}          {m}" for k, m in KNOBS.items()]
    return "\n".join(rows)


if __name__ == "__main__":
    print(table())
