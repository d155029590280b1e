"""CPU: the host side of activation recomputation -- the new entries and flag bits in the library and the header,
their refusals that need no device, and the argument checks of FusedStep / BSGMP / DataParallel / Trainer / input_gradient.  No kernel
is launched (tests/test_hip_recompute.py runs them)."""
import inspect
import os
import re
from types import SimpleNamespace

import pytest
import torch

OK, E_INVALID_ARG = 0, -1
LEAN, RECOMPUTE = 4, 2
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "bsms_hip.h")


def _sim(depth=2):
    import bsms_gnn_amd as eng
    from oracle import bsms_oracle as ro
    return eng, eng.BSMS_Simulator(ro.make_cfg(2, 32, 2, depth, 2))


def test_entries_and_flags_are_declared():
    from bsms_gnn_amd import _abi
    L = _abi.lib()
    text = open(HEADER).read()
    for name in ("bsms_bsgmp_saved_bytes_ex", "bsms_bsgmp_work_bytes_ex"):
        assert name in _abi.SIGNATURES and getattr(L, name) is not None
        assert re.search(r"size_t\s+" + name + r"\s*\(", text), name
    assert re.search(r"BSMS_FWD_LEAN\s*=\s*4\b", text) and re.search(r"BSMS_BWD_RECOMPUTE\s*=\s*2\b", text)
    assert re.search(r"BSMS_BWD_DEFER_JOIN\s*=\s*1\b", text)          # the bit next to it keeps its value
    from bsms_gnn_amd import ops
    assert (ops.FWD_LEAN, ops.BWD_RECOMPUTE) == (LEAN, RECOMPUTE)
    assert L.bsms_abi_version() == 4                                   # no signature changed


def test_refusals_without_a_device():
    from bsms_gnn_amd import _abi
    L = _abi.lib()
    one = 0x1000                                                       # a non-null address that must never be dereferenced
    err = lambda: L.bsms_last_error()
    # the size queries: 0 for null plans, unknown flag bits, a bad depth
    for query in (L.bsms_bsgmp_saved_bytes_ex, L.bsms_bsgmp_work_bytes_ex):
        assert query(None, 2, 2, 32, 2, 3, 0, RECOMPUTE) == 0
        assert query(None, 2, 2, 32, 2, 3, 0, 0) == 0
        assert query(None, 0, 2, 32, 2, 3, 0, 8) == 0
    none_pl, _keep = _abi.ptr_array([None])
    for query in (L.bsms_bsgmp_saved_bytes_ex, L.bsms_bsgmp_work_bytes_ex):
        assert query(none_pl, 0, 2, 32, 2, 3, 0, RECOMPUTE) == 0       # a null plan in the table
        assert query(none_pl, -1, 2, 32, 2, 3, 0, RECOMPUTE) == 0 and query(none_pl, 17, 2, 32, 2, 3, 0, RECOMPUTE) == 0
    # the forward: unknown bits of `reuse`, the lean bit without `saved`, null plans -- in that order, before anything is looked at
    fwd = lambda plans, saved, reuse: L.bsms_bsgmp_fwd_p(plans, None, 0, one, one, 2, 32, 2, 0, 3, None, one, saved, one, reuse, 0, None)
    assert fwd(None, one, 8) == E_INVALID_ARG and b"unknown bits" in err()
    assert fwd(None, one, LEAN | 32) == E_INVALID_ARG and b"unknown bits" in err()
    assert fwd(None, None, LEAN) == E_INVALID_ARG and b"BSMS_FWD_LEAN" in err()
    assert fwd(None, one, LEAN) == E_INVALID_ARG and b"unknown bits" not in err()          # null plans
    # the three backwards that take flags
    a = (None, None, 0, one, one, one, 2, 32, 2, 0, 3, None)
    calls = {
        "ex": lambda saved, flags: L.bsms_bsgmp_bwd_ex(*a, saved, one, one, None, 0, flags, None),
        "ev": lambda saved, flags: L.bsms_bsgmp_bwd_ev(*a, saved, one, one, None, 0, flags, None, None),
        "pos_ev": lambda saved, flags: L.bsms_bsgmp_bwd_pos_ev(*a, saved, one, one, None, 0, flags, None, None, None, None),
    }
    for name, call in calls.items():
        assert call(one, 4) == E_INVALID_ARG and b"unknown bits" in err(), name
        assert call(one, RECOMPUTE | 1 | 16) == E_INVALID_ARG and b"unknown bits" in err(), name
        assert call(None, RECOMPUTE) == E_INVALID_ARG and b"BSMS_BWD_RECOMPUTE" in err(), name
        assert call(one, RECOMPUTE | 1) == E_INVALID_ARG and b"unknown bits" not in err(), name       # null plans


def test_fused_step_validates_recompute():
    eng, sim = _sim()
    grads = eng.GradBuckets(list(sim.parameters()))
    for bad in (1, 0, None, "yes"):
        with pytest.raises(TypeError, match="recompute"):
            eng.FusedStep(sim, grads, recompute=bad)
    assert eng.FusedStep(sim, grads).recompute is False and eng.FusedStep(sim, grads, recompute=True).recompute is True
    assert inspect.signature(eng.FusedStep.__init__).parameters["recompute"].default is False
    with pytest.raises(RuntimeError, match="has not run"):
        eng.FusedStep(sim, grads, recompute=True).held_bytes()
    assert inspect.signature(eng.DataParallel.__init__).parameters["recompute"].default is False
    with pytest.raises(ValueError, match="recompute needs the fused step"):          # a CPU model has no fused step
        eng.DataParallel(sim, recompute=True)
    with pytest.raises(TypeError, match="recompute"):
        eng.DataParallel(sim, recompute=1)


def test_bsgmp_recompute_is_the_one_call_path_only():
    eng, sim = _sim()
    net = sim.process
    assert net.recompute is False
    net.recompute = True
    assert net.recompute is True
    with pytest.raises(TypeError):
        net.recompute = 1
    net.recompute = False
    net.per_block = True
    with pytest.raises(ValueError, match="per_block"):
        net.recompute = True
    assert net.recompute is False
    net.per_block = False
    net.recompute = True
    net.per_block = True                                               # ... switched afterwards: refused by the forward
    z = torch.zeros(1, 10, 32)
    with pytest.raises(ValueError, match="per_block"):
        net(z, [torch.zeros(3, dtype=torch.int64)] * 2, [torch.zeros(2, 4, dtype=torch.int64)] * 3, z[..., :2])


def test_cfg_key():
    from bsms_gnn_amd.trainer import recompute_from_cfg
    assert recompute_from_cfg(SimpleNamespace()) is False              # a cfg without the key: the route as it was
    assert recompute_from_cfg(SimpleNamespace(recompute_activations=None)) is False
    assert recompute_from_cfg(SimpleNamespace(recompute_activations=False)) is False
    assert recompute_from_cfg(SimpleNamespace(recompute_activations=True)) is True
    for bad in (1, "true", 0.0):
        with pytest.raises(TypeError, match="recompute_activations"):
            recompute_from_cfg(SimpleNamespace(recompute_activations=bad))


def test_input_gradient_cache_key_separates_recompute():
    eng, sim = _sim()
    from bsms_gnn_amd.step import _input_gradient_key
    obj = eng.Objective()
    a, b = _input_gradient_key(2, None, False, obj, True, False), _input_gradient_key(2, None, False, obj, True, True)
    assert a != b and sum(x != y for x, y in zip(a, b)) == 1 and len(a) == len(b)
    assert _input_gradient_key(2, None, False, obj, True) == a        # the default is the step without the flag
    assert inspect.signature(eng.input_gradient).parameters["recompute"].default is False
    z = torch.zeros(1, 10, 5)
    data = (z, z[..., :2], z[..., :1], [torch.zeros(1, 2, 4, dtype=torch.int64)] * 3, [torch.zeros(1, 3, dtype=torch.int64)] * 2)
    with pytest.raises(TypeError, match="recompute"):
        eng.input_gradient(sim, data, recompute=1)
    with pytest.raises(eng._abi.BsmsError, match="GPU only"):           # refused like every CPU batch; the flagged step was built and cached
        eng.input_gradient(sim, data, recompute=True)
    steps = [v for k, v in sim._bsms_input_grad_steps.items() if k != "grads"]
    assert len(steps) == 1 and steps[0].recompute is True
