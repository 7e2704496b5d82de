"""LAMB without a GPU: the config target and the refusals, the piece table, the C-side refusals of include/egopack_lamb.h with fake
pointers (every check precedes the first dereference and the first launch), and the float64 model of tests/lamb_common.py held
against its f32 restatement and its mutants on the inputs the GPU tests use."""
import ctypes

import numpy as np
import pytest
import torch

from egopack_amd import _lib, optim, train
from tests import lamb_common as L


# ---- the public interface -------------------------------------------------------------------------------------------------------------
def test_the_config_target_resolves_to_flat_lamb():
    assert train.OPTIMIZERS["egopack_amd.optim.FlatLAMB"] is optim.FlatLAMB
    assert issubclass(optim.FlatLAMB, optim.FlatAdam)
    cfg = train.load_config(["optimizer._target_=egopack_amd.optim.FlatLAMB", "optimizer.lr=2e-3", "optimizer.weight_decay=0.01",
                             "+optimizer.trust_clip=true", "+optimizer.eps=1e-6"])
    w = torch.nn.Parameter(torch.zeros(4, 4))
    opt = train.build_optimizer(cfg, [w])
    assert type(opt) is optim.FlatLAMB and opt.trust_clip and not opt.always_adapt
    g = opt.param_groups[0]
    assert g["lr"] == 2e-3 and g["weight_decay"] == 0.01 and g["trust_clip"] is True and g["always_adapt"] is False
    assert opt._state_keys == ("exp_avg", "exp_avg_sq") and set(optim.FlatLAMB._fixed_keys) >= {"trust_clip", "always_adapt"}
    assert opt.trust_ratios() == {}  # (before the flat buffers exist)


@pytest.mark.parametrize("kw, needle", [
    (dict(amsgrad=True), "amsgrad=True is not built"),
    (dict(maximize=True), "maximize=True is not built"),
    (dict(state_dtype=torch.bfloat16), "state_dtype=torch.bfloat16"),
    (dict(state_dtype="bf16"), "state_dtype=torch.bfloat16"),
    (dict(decoupled_weight_decay=True), "decoupled_weight_decay=True is not built"),
    (dict(eps=0.0), "eps must be positive"),
])
def test_what_flat_lamb_refuses_by_name(kw, needle):
    with pytest.raises(ValueError) as e:
        optim.FlatLAMB([torch.nn.Parameter(torch.zeros(8))], **kw)
    assert "FlatLAMB" in str(e.value) and needle in str(e.value)


def _state(lamb: bool):
    groups = [{"lr": 1e-3, "betas": (0.9, 0.999), "eps": 1e-8, "weight_decay": 0.0, "params": [0]}]
    if lamb:
        groups[0].update(trust_clip=False, always_adapt=False)
    return {"state": {0: {"step": torch.tensor(3.0), "exp_avg": torch.zeros(8), "exp_avg_sq": torch.zeros(8)}}, "param_groups": groups}


def test_a_state_of_the_other_rule_is_refused_by_name_in_both_directions():
    w = torch.nn.Parameter(torch.zeros(8))
    with pytest.raises(RuntimeError, match="FlatLAMB.load_state_dict.*holds Adam / AdamW state.*configured optimizer is FlatLAMB"):
        optim.FlatLAMB([w]).load_state_dict(_state(False))
    with pytest.raises(RuntimeError, match="FlatAdam.load_state_dict.*holds LAMB state.*configured optimizer is FlatAdam"):
        optim.FlatAdam([w]).load_state_dict(_state(True))
    with pytest.raises(RuntimeError, match="SGD state with momentum"):
        optim.FlatLAMB([w]).load_state_dict({"state": {0: {"momentum_buffer": torch.zeros(8)}}, "param_groups": _state(True)["param_groups"]})
    opt = optim.FlatLAMB([w], trust_clip=True)
    opt.load_state_dict(_state(True))  # (its own rule loads; the fixed keys stay the constructor's)
    assert opt.step_count == 3 and opt.param_groups[0]["trust_clip"] is True
    optim.FlatAdam([w]).load_state_dict(_state(False))


def test_the_sharded_update_refuses_lamb_by_name():
    from egopack_amd import dist

    class Opt:
        trust_ratios = None
    with pytest.raises(ValueError, match="Opt does not combine with the sharded update.*whole parameter slot"):
        dist.GradSync._refuse_lamb(None, Opt())
    dist.GradSync._refuse_lamb(None, object())


# ---- the piece table ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sizes", [L.SIZES, [8], [4096], [4104, 8], [8, 8, 8, 12288, 24, 4608 * 3 + 16]])
def test_the_piece_table_covers_the_buffers_inside_slots(sizes):
    begin, piece0, pieces = optim.FlatLAMB.piece_table(sizes)
    assert (begin, piece0, pieces) == L.piece_table(sizes)  # (the optimizer's builder and the tests' own)
    assert begin[0] == 0 and begin[-1] == sum(sizes) == pieces[-1] and pieces[0] == 0 and piece0[-1] == len(pieces) - 1
    assert all(b > a for a, b in zip(pieces, pieces[1:])) and all(0 < b - a <= L.PIECE for a, b in zip(pieces, pieces[1:]))
    assert all(x % 8 == 0 for x in pieces) and L.PIECE == _lib.LAMB_PIECE
    for s in range(len(sizes)):  # the pieces of a slot tile exactly that slot; all but its last are whole
        mine = pieces[piece0[s]:piece0[s + 1] + 1]
        assert mine[0] == begin[s] and mine[-1] == begin[s + 1]
        assert all(b - a == L.PIECE for a, b in zip(mine[:-2], mine[1:-1]))
    with pytest.raises(ValueError, match="multiples of 8"):
        optim.FlatLAMB.piece_table([12])


def test_the_header_states_the_piece_length():
    assert f"#define EGK_LAMB_PIECE {L.PIECE}" in _lib.EXTRA_HEADERS["lamb"].read_text()


# ---- the C side refuses what it can see -----------------------------------------------------------------------------------------------
def test_the_entry_points_refuse_bad_arguments_before_any_launch():
    lib = _lib.load()
    vp = ctypes.c_void_p
    A, U4, U8 = 0x1000, 0x1004, 0x1008
    base = dict(p=A, g=A, m=A, v=A, hyper=A, part=A, slot_begin=A, slot_piece0=A, slot_group=A, group_hyper=A, trust=A, norms=A, w16=A)

    def mom(lo=0, hi=8192, piece0=0, n_pieces=2, on=0, g_dtype=0, n_slots=1, n_groups=1, b1=L.B1, b2=L.B2, eps=L.EPS, **over):
        q = {**base, **over}
        return lib.egk_lamb_moments(None, vp(q["p"]), vp(q["g"]), g_dtype, vp(q["m"]), vp(q["v"]), lo, hi, piece0, n_pieces, on,
                                    vp(q["slot_begin"]), vp(q["slot_piece0"]), vp(q["slot_group"]), n_slots, vp(q["group_hyper"]), n_groups,
                                    vp(q["hyper"]), b1, b2, eps, vp(q["part"]), None, None, 0)

    def refused(rc, needle):
        assert rc == -1 and needle in _lib.last_error() and "egk_lamb_" in _lib.last_error(), (rc, _lib.last_error())

    for name in ("p", "g", "m", "v", "hyper", "part"):
        refused(mom(**{name: None}), "null pointer")
    for name in ("slot_begin", "slot_piece0", "slot_group", "group_hyper"):
        refused(mom(**{name: None}), "null table pointer")
    for name in ("p", "g", "m", "v"):
        refused(mom(**{name: U4}), "16-byte aligned")
    refused(mom(g=U4, g_dtype=1), "16-byte aligned")
    refused(mom(part=U4), "misaligned part")
    refused(mom(slot_begin=U4), "misaligned table pointer")
    refused(mom(group_hyper=U8), "misaligned table pointer")
    refused(mom(g_dtype=2), "unknown gradient dtype")
    refused(mom(lo=8192, hi=8192), "empty or negative range")
    refused(mom(lo=-8, hi=8192), "empty or negative range")
    refused(mom(lo=4, hi=8196), "multiples of 8")
    refused(mom(lo=0, hi=8196), "multiples of 8")
    refused(mom(lo=0, hi=4088), "shorter than a piece")
    refused(mom(lo=0, hi=8192, n_pieces=0), "n_pieces >= 1")
    refused(mom(piece0=-1), "piece0 >= 0")
    refused(mom(n_slots=0), "n_slots >= 1")
    refused(mom(n_groups=65), "n_groups in 1..64")
    refused(mom(eps=0.0), "eps > 0")
    refused(mom(b1=1.0), "betas in [0, 1)")

    def tr(n_slots=1, n_groups=1, **over):
        q = {**base, **over}
        return lib.egk_lamb_trust(None, vp(q["part"]), vp(q["slot_piece0"]), vp(q["slot_group"]), n_slots, vp(q["group_hyper"]), n_groups, 0, 0,
                                  vp(q["trust"]), vp(q["norms"]), None)
    for name in ("part", "trust", "norms"):
        refused(tr(**{name: None}), "null pointer")
    refused(tr(slot_piece0=None), "null table pointer")
    refused(tr(norms=U4), "misaligned part, norms")
    refused(tr(n_slots=0), "n_slots >= 1")
    refused(tr(n_groups=0), "n_groups in 1..64")

    def ap(n=8192, n_pieces=2, n_slots=1, n_groups=1, eps=L.EPS, lo16=None, ema=None, decay=0.0, warmup=0, t_dev=None, **over):
        q = {**base, **over}
        return lib.egk_lamb_apply(None, vp(q["p"]), vp(q["m"]), vp(q["v"]), n, n_pieces, vp(q["slot_begin"]), vp(q["slot_piece0"]),
                                  vp(q["slot_group"]), n_slots, vp(q["group_hyper"]), n_groups, vp(q["hyper"]), eps, vp(q["trust"]),
                                  vp(q["w16"]), vp(lo16), vp(ema), decay, warmup, vp(t_dev), None)
    for name in ("p", "m", "v", "hyper", "trust", "w16"):
        refused(ap(**{name: None}), "null pointer")
    refused(ap(p=U8), "16-byte aligned")
    refused(ap(ema=U8), "16-byte aligned")
    refused(ap(w16=U4), "8-byte aligned")
    refused(ap(lo16=0x1002), "8-byte aligned")
    refused(ap(slot_group=None), "null table pointer")
    refused(ap(n=0), "n >= 1")
    refused(ap(n_pieces=0), "n_pieces >= 1")
    refused(ap(eps=-1.0), "eps > 0")
    refused(ap(ema=A, decay=1.0), "ema_decay in [0, 1)")
    refused(ap(ema=A, decay=0.9, warmup=1), "ema_warmup needs t_dev")
    # the knob: key 0 alone, the value kept
    prev = lib.egk_lamb_tune(0, -1)
    assert prev in (0, 1) and lib.egk_lamb_tune(0, 1 - prev) == prev and lib.egk_lamb_tune(0, prev) == 1 - prev and lib.egk_lamb_tune(1, 0) == -1


def test_the_three_launches_have_profile_ids():
    lib = _lib.load()
    name, names = ctypes.create_string_buffer(64), []
    n, ms, fl, by = ctypes.c_int64(), ctypes.c_double(), ctypes.c_double(), ctypes.c_double()
    for i in range(lib.egk_prof_count()):
        assert lib.egk_prof_get(i, name, 64, ctypes.byref(n), ctypes.byref(ms), ctypes.byref(fl), ctypes.byref(by)) == 0
        names.append(name.value.decode())
    assert names[-3:] == ["lamb_moments", "lamb_trust", "lamb_apply"] and len(set(names)) == len(names)


# ---- the model, its f32 restatement and its mutants on the inputs the GPU tests use ---------------------------------------------------
def _steps(dtype, mutant=None, **kw):
    """Three steps from the problem; every step starts from the f32-rounded result of the model's previous step."""
    pr = L.problem()
    p, m, v, out = pr["p"], pr["m"], pr["v"], []
    for t in (1, 2, 3):
        ref = L.lamb_model(p, pr["g"][t - 1], m, v, pr["begin"], L.SLOT_GROUP, L.GROUPS, L.hyper(t), **kw)
        got = ref if dtype is np.float64 and mutant is None else L.lamb_model(p, pr["g"][t - 1], m, v, pr["begin"], L.SLOT_GROUP, L.GROUPS,
                                                                            L.hyper(t), dtype=dtype, mutant=mutant, **kw)
        out.append((ref, got))
        p, m, v = (x.astype(np.float32) for x in ref[:3])
    return pr, out


def test_the_f32_restatement_of_the_model_stays_inside_every_tolerance():
    """What the kernels compute, restated in numpy f32 (every operation rounded separately, the sums in f64): the tolerances of
    tests/test_gpu_lamb.py hold for it on the chosen inputs with room to spare -- else another SEED is to be taken."""
    pr, steps = _steps(np.float32)
    for t, (ref, got) in enumerate(steps, 1):
        for k, name in enumerate(("p", "m", "v")):
            assert L.excess(got[k], ref[k], **L.TOL) < 0.5, (t, name, L.excess(got[k], ref[k], **L.TOL))
        assert np.max(np.abs(got[3] - ref[3]) / ref[3]) < 0.5 * L.TRUST_RTOL, (t, got[3], ref[3])
        assert not np.any(ref[0][~pr["mask"]]) and not np.any(ref[1][~pr["mask"]]) and not np.any(ref[2][~pr["mask"]])  # the padding stays zero
    tr = steps[0][0][3]
    assert tr[1] == 1.0 and tr[4] == 1.0 and all(x != 1.0 for x in tr[[0, 2, 3, 5]])  # (group 1 decays nothing: trust 1)


@pytest.mark.parametrize("mutant", L.MUTANTS)
def test_every_mutant_is_ten_tolerances_away_on_the_tensor_it_moves(mutant):
    _, steps = _steps(np.float64, mutant=mutant)
    worst = {}
    for ref, got in steps:
        for k, name in enumerate(("p", "m", "v")):
            worst[name] = max(worst.get(name, 0.0), L.excess(got[k], ref[k], **L.TOL))
        worst["trust"] = max(worst.get("trust", 0.0), float(np.max(np.abs(got[3] - ref[3]) / ref[3])) / L.TRUST_RTOL)
    moved = {"trust_from_g": "trust", "global_norms": "trust", "no_wd_in_norm": "trust", "adapt_at_wd0": "trust",
             "no_bias_correction": "p", "scale_after_moments": "m"}[mutant]
    assert worst[moved] >= 10.0, (mutant, worst)
