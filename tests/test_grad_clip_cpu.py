"""Host-side logic of global-norm gradient clipping (no GPU): the constructor argument, the configuration key, the argument checks
of the new C-ABI entry points, the refusal of the sharded update."""
import ctypes

import pytest
import torch


def test_max_grad_norm_off_and_refused_values():
    from egopack_amd.optim import FlatAdam
    p = [torch.zeros(8, requires_grad=True)]
    assert not FlatAdam(p).clipping and not FlatAdam(p, max_grad_norm=0).clipping and not FlatAdam(p, max_grad_norm=None).clipping
    assert FlatAdam(p, max_grad_norm=0.5).clipping and FlatAdam(p, max_grad_norm=0.5).max_grad_norm == 0.5
    for bad in (-1.0, float("nan")):
        with pytest.raises(ValueError, match="max_grad_norm"):
            FlatAdam(p, max_grad_norm=bad)
    with pytest.raises(RuntimeError, match="max_grad_norm"):
        FlatAdam(p).grad_norm_stats()
    with pytest.raises(RuntimeError, match="max_grad_norm"):
        FlatAdam(p).norm_partials()
    assert FlatAdam(p, max_grad_norm=0.5).grad_norm_stats() == {"steps": 0, "mean_norm": 0.0, "max_norm": 0.0, "clipped": 0,
                                                                 "skipped": 0, "last_norm": 0.0}
    assert "max_grad_norm" not in FlatAdam(p, max_grad_norm=0.5).state_dict()["param_groups"][0]  # (torch.optim.Adam's layout)


def test_grad_clip_norm_key_reaches_the_optimizer():
    from egopack_amd import train as T
    cfg = T.load_config([])
    assert cfg.grad_clip_norm == 0 and "grad_clip_norm" not in cfg.optimizer  # (beside the block Hydra instantiates, not inside it)
    p = [torch.zeros(8, requires_grad=True)]
    assert not T.build_optimizer(cfg, p).clipping
    opt = T.build_optimizer(T.load_config(["grad_clip_norm=2.5"]), p)
    assert opt.clipping and opt.max_grad_norm == 2.5


def test_norm_entry_points_check_their_arguments():
    from egopack_amd import _lib
    lib = _lib.load()
    assert [lib.egk_grad_sumsq_slots(n) for n in (-1, 0, 1, 16384, 16385, 1 << 40)] == [0, 0, 1, 1, 2, 1024]
    one, odd = ctypes.c_void_p(1 << 20), ctypes.c_void_p((1 << 20) + 4)
    assert lib.egk_grad_sumsq(None, None, 0, 32, one, 1) == -1 and "null pointer" in _lib.last_error()
    assert lib.egk_grad_sumsq(None, odd, 0, 32, one, 1) == -1 and "16-byte aligned" in _lib.last_error()
    assert lib.egk_grad_sumsq(None, one, 0, 0, one, 0) == -1 and "n >= 1" in _lib.last_error()
    assert lib.egk_grad_sumsq(None, one, 0, 32, one, 2) == -1 and "partial sums" in _lib.last_error()
    assert lib.egk_grad_norm_finalize(None, one, 1, one, 1.0, one, one, None, one) == -1 and "null pointer" in _lib.last_error()
    assert lib.egk_grad_norm_finalize(None, one, 0, one, 1.0, one, one, one, one) == -1 and "at least one" in _lib.last_error()
    assert lib.egk_grad_norm_finalize(None, one, 1, one, 0.0, one, one, one, one) == -1 and "max_norm > 0" in _lib.last_error()


def test_sharded_update_refuses_a_clipping_optimizer():
    from egopack_amd.dist import GradSync

    class Opt:
        clipping = True
        flat_g = torch.zeros(64)
    sync = GradSync(2, shard_update=True)
    with pytest.raises(RuntimeError, match="sharded update"):
        sync.reduce_and_step(Opt())
    with pytest.raises(RuntimeError, match="sharded update"):
        sync.start(Opt(), 0, 64)
