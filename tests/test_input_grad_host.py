"""CPU: the host side of the input gradient through the fused step -- bsms_sim_input_grad and
bsms_bsgmp_bwd_pos_ev are declared, exported and bound, bsms_sim_input_grad refuses in the documented order before any device
call, and FusedStep / DataParallel / input_gradient validate their arguments before any device work.  No kernel is launched
(tests/test_hip_input_grad.py runs them)."""
import ctypes as C
import os
import re

import pytest
import torch

from conftest import ROOT

NEW = {"bsms_sim_input_grad": 14, "bsms_bsgmp_bwd_pos_ev": 22}      # name -> number of arguments
OK, E_INVALID_ARG, E_SHAPE, E_UNSUPPORTED = 0, -1, -2, -3


@pytest.fixture(scope="module")
def L():
    from bsms_gnn_amd import _abi
    return _abi.lib()


def test_new_entries_are_declared_exported_and_bound(L):
    from bsms_gnn_amd import _abi
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "bsms_hip.h")).read(), flags=re.S)
    lib = C.CDLL(_abi.LIB_PATH)
    for name, nargs in NEW.items():
        m = re.search(rf"\bint {name}\s*\((.*?)\)\s*;", text, flags=re.S)
        assert m, f"{name} is not declared in include/bsms_hip.h"
        assert hasattr(lib, name), f"{name} is not exported"
        assert len(m.group(1).split(",")) == len(_abi.SIGNATURES[name][1]) == nargs       # header and binding in step
    assert L.bsms_abi_version() == 4                                                       # no existing signature changed
    # the pair differs from the entries it combines by exactly the arguments it adds
    ev, pos, both = (_abi.SIGNATURES[n][1] for n in ("bsms_bsgmp_bwd_ev", "bsms_bsgmp_bwd_pos", "bsms_bsgmp_bwd_pos_ev"))
    assert both[:-1] == ev[:-1] + pos[-3:-1] and both[-1] == ev[-1]


def test_sim_input_grad_refuses_in_the_stated_order(L):
    one = 0x1000                                             # a non-null address that must never be dereferenced

    def call(R=300, Cc=2, p=2, ptr=one, first=1, over=1, **null):
        a = {k: (None if null.get(k) else ptr) for k in ("g_pred", "g_nin", "g_pos", "mask", "mean", "meansq", "eps", "grad_in")}
        return L.bsms_sim_input_grad(a["g_pred"], a["g_nin"], a["g_pos"], a["mask"], R, Cc, p, a["mean"], a["meansq"], a["eps"],
                                     first, over, a["grad_in"], None)

    # the envelope, before any pointer is looked at
    assert call(R=0, ptr=None) == E_UNSUPPORTED and call(R=-1) == E_UNSUPPORTED
    assert call(Cc=0, ptr=None) == E_UNSUPPORTED and call(Cc=9, ptr=None) == E_UNSUPPORTED
    assert b"C=9" in L.bsms_last_error()
    assert call(p=0, ptr=None) == E_UNSUPPORTED and call(p=8, ptr=None) == E_UNSUPPORTED
    assert b"p=8" in L.bsms_last_error()
    assert call(Cc=9, g_nin=True) == E_UNSUPPORTED and call(p=8, first=1, g_pred=True) == E_UNSUPPORTED
    # then the pointers
    for Cc, p in ((1, 1), (8, 7)):
        assert call(Cc=Cc, p=p, ptr=None) == E_INVALID_ARG
    for name in ("g_nin", "g_pos", "mask", "mean", "meansq", "eps", "grad_in"):
        for first in (0, 1):
            assert call(first=first, **{name: True}) == E_INVALID_ARG, name
    assert call(first=1, g_pred=True) == E_INVALID_ARG and b"g_pred" in L.bsms_last_error()
    assert call(first=1, over=0, g_pred=True) == E_INVALID_ARG


def test_bsgmp_bwd_pos_ev_checks_like_its_parts(L):
    one = 0x1000
    PP = C.POINTER(C.c_void_p)
    null_pp = PP()

    def call(p, grad_pos, pos_work):
        return L.bsms_bsgmp_bwd_pos_ev(null_pp, null_pp, 2, None, None, None, 1, 128, p, 0, 3, null_pp, None, None, None, null_pp, 0, 0,
                                       null_pp, grad_pos, pos_work, None)

    assert call(0, one, one) == E_INVALID_ARG and b"pos_dim=0" in L.bsms_last_error()
    assert call(8, one, one) == E_INVALID_ARG
    assert call(2, one, None) == E_INVALID_ARG and b"pos_work" in L.bsms_last_error()
    ev = L.bsms_bsgmp_bwd_ev(null_pp, null_pp, 2, None, None, None, 1, 128, 2, 0, 3, null_pp, None, None, None, null_pp, 0, 0, null_pp, None)
    msg = L.bsms_last_error()
    assert ev != OK and call(2, None, None) == ev and L.bsms_last_error() == msg     # grad_pos = NULL: the checks of bsms_bsgmp_bwd_ev
    assert call(2, one, one) == ev                                                     # null plans: refused before any device call


def _sim():
    import bsms_gnn_amd as eng
    from oracle import bsms_oracle as ro
    sim = eng.BSMS_Simulator(ro.make_cfg(2, 32, 2, 2, 2))
    return eng, sim, eng.GradBuckets(list(sim.parameters()))


def test_fused_step_validates_the_flag_before_any_device_work():
    eng, sim, grads = _sim()
    off = eng.FusedStep(sim, grads)
    assert off._input_grad is False
    with pytest.raises(ValueError, match="input_grad=True"):
        off.input_grad()
    for bad in (1, "yes", None):
        with pytest.raises(TypeError, match="input_grad"):
            eng.FusedStep(sim, grads, input_grad=bad)
    with pytest.raises(ValueError, match="graph"):
        eng.FusedStep(sim, grads, use_graph=True, unroll=2, input_grad=True)       # capture of the unrolled step: still not here
    with pytest.raises(ValueError, match="step_weights"):
        eng.FusedStep(sim, grads, unroll=3, step_weights=[0.5, 0.5], input_grad=True)
    for kw in (dict(), dict(unroll=3, detach=True), dict(use_graph=True), dict(objective=eng.Objective("normalized", "mse", [1, 4]))):
        on = eng.FusedStep(sim, grads, input_grad=True, **kw)
        with pytest.raises(RuntimeError, match="not run"):
            on.input_grad()
    z = torch.zeros(1, 10, 5)
    with pytest.raises(_abi_error(eng), match="GPU only"):                        # a CPU batch is refused as without the flag
        eng.FusedStep(sim, grads, input_grad=True)((z, z[..., :2], z[..., :1], [torch.zeros(1, 2, 4, dtype=torch.int64)] * 3,
                                                    [torch.zeros(1, 3, dtype=torch.int64)] * 2), True)


def _abi_error(eng):
    return eng._abi.BsmsError


def test_data_parallel_and_input_gradient_validate():
    eng, sim, _ = _sim()
    with pytest.raises(ValueError, match="input_grad needs the fused step"):       # a CPU model has no fused step
        eng.DataParallel(sim, input_grad=True)
    with pytest.raises(TypeError, match="input_grad"):
        eng.DataParallel(sim, input_grad="yes")
    assert eng.DataParallel(sim).fused is None
    assert callable(eng.input_gradient)
    z = torch.zeros(1, 10, 5)
    data = (z, z[..., :2], z[..., :1], [torch.zeros(1, 2, 4, dtype=torch.int64)] * 3, [torch.zeros(1, 3, dtype=torch.int64)] * 2)
    with pytest.raises(ValueError, match="step_weights"):
        eng.input_gradient(sim, data, later_targets=torch.zeros(2, 1, 10, 2), step_weights=[0.5, 0.5])      # K = 3 from later_targets
    with pytest.raises(_abi_error(eng), match="GPU only"):
        eng.input_gradient(sim, data)
