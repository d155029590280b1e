"""CPU: the host side of gradient accumulation -- bsms_accum_coef and bsms_grad_fold are declared, exported, bound
and validate their arguments before any device call; FusedStep, DataParallel and the Trainer's configuration refuse, by name and at
construction, what accumulation does not implement.  No kernel is launched (tests/test_hip_accumulate.py runs them)."""
import ctypes as C
import os
import re

import pytest

from conftest import ROOT

NEW = {"bsms_accum_coef": 17, "bsms_grad_fold": 5}          # entry -> number of arguments
OK, E_INVALID_ARG, E_SHAPE, E_UNSUPPORTED = 0, -1, -2, -3


@pytest.fixture(scope="module")
def eng():
    import __graft_entry__
    __graft_entry__.build()
    import bsms_gnn_amd as eng
    return eng


def test_new_entries_are_declared_exported_and_bound(eng):
    from bsms_gnn_amd import _abi
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "bsms_hip.h")).read(), flags=re.S)
    lib = C.CDLL(_abi.LIB_PATH)
    for name, nargs in NEW.items():
        m = re.search(rf"\bint {name}\s*\((.*?)\)\s*;", text, flags=re.S)
        assert m, f"{name} is not declared in include/bsms_hip.h"
        assert hasattr(lib, name), f"{name} is not exported"
        assert len(m.group(1).split(",")) == len(_abi.SIGNATURES[name][1]) == nargs      # header and binding in step
    for const in ("BSMS_ACCUM_SUMS_PAIR = 0", "BSMS_ACCUM_SUMS_ROW = 1", "BSMS_ACCUM_BATCH = 0", "BSMS_ACCUM_MEAN = 1"):
        assert const in text
    from bsms_gnn_amd.step import REDUCTIONS
    assert REDUCTIONS == {"batch": 0, "mean": 1}
    assert _abi.lib().bsms_abi_version() == 4               # no existing signature changed


def test_grad_fold_validates_before_any_device_call(eng):
    L = eng._abi.lib()
    one = 0x1000                                             # a non-null address that must never be dereferenced
    assert L.bsms_grad_fold(None, None, 0, None, None) == OK
    assert L.bsms_grad_fold(one, one + 64, -1, one + 128, None) == E_SHAPE
    assert L.bsms_grad_fold(None, one, 8, one + 128, None) == E_INVALID_ARG
    assert L.bsms_grad_fold(one, None, 8, one + 128, None) == E_INVALID_ARG
    assert L.bsms_grad_fold(one, one + 64, 8, None, None) == E_INVALID_ARG
    assert L.bsms_grad_fold(one, one, 8, one + 128, None) == E_INVALID_ARG
    assert b"same buffer" in L.bsms_last_error()


def test_accum_coef_validates_before_any_device_call(eng):
    L = eng._abi.lib()
    one = 0x1000

    def call(sums=one, layout=0, stride=2, Cc=2, stats=one, weights=None, space=0, kind=0, reduction=0, t=0, K=1, running=one, coef=one,
             loss=one):
        return L.bsms_accum_coef(sums, layout, stride, Cc, stats, stats, stats, weights, space, kind, reduction, t, K, running, coef, loss, None)

    assert call(K=0) == E_UNSUPPORTED and call(K=4097) == E_UNSUPPORTED
    assert call(Cc=0) == E_UNSUPPORTED and call(Cc=9) == E_UNSUPPORTED
    assert b"C=9" in L.bsms_last_error()
    assert call(t=-1) == E_UNSUPPORTED
    for bad in (dict(layout=2), dict(space=2), dict(kind=-1), dict(reduction=2)):
        assert call(**bad) == E_UNSUPPORTED, bad
    assert call(Cc=9, sums=None) == E_UNSUPPORTED           # the envelope is checked before the pointers
    assert call(stride=1) == E_SHAPE                         # a pair is two floats
    assert call(layout=1, stride=2, Cc=2) == E_SHAPE         # a row is at least 1 + C doubles
    for missing in ("sums", "running", "coef", "loss"):
        assert call(**{missing: None}) == E_INVALID_ARG, missing
    assert call(layout=1, stride=7, space=1, stats=None) == E_INVALID_ARG        # the normalized space reads the statistics
    assert b"normalized" in L.bsms_last_error()


def _cpu_model(eng):
    from oracle import bsms_oracle as ro
    sim = eng.BSMS_Simulator(ro.make_cfg(2, 32, 2, 2, 2))
    return sim, eng.GradBuckets(list(sim.parameters()))


def test_fused_step_refuses_by_name_at_construction(eng):
    sim, grads = _cpu_model(eng)
    for bad in (0, -1, 1.5, True):
        with pytest.raises(ValueError, match="accumulate"):
            eng.FusedStep(sim, grads, accumulate=bad)
    with pytest.raises(ValueError, match="reduction"):
        eng.FusedStep(sim, grads, accumulate=2, reduction="sum")
    with pytest.raises(ValueError, match="reduction"):
        eng.FusedStep(sim, grads, reduction="sum")           # unknown whatever `accumulate` is
    with pytest.raises(ValueError, match="graph"):
        eng.FusedStep(sim, grads, accumulate=2, use_graph=True)
    with pytest.raises(ValueError, match="input_grad"):
        eng.FusedStep(sim, grads, accumulate=2, input_grad=True)
    # unroll > 1 with an rmse loss under "batch": no scalar factor -- the message names both ways out
    with pytest.raises(ValueError, match=r'reduction="mean".*loss_kind="mse"'):
        eng.FusedStep(sim, grads, accumulate=2, unroll=2)
    with pytest.raises(ValueError, match=r'reduction="mean".*loss_kind="mse"'):
        eng.FusedStep(sim, grads, accumulate=2, unroll=2, objective=eng.Objective("normalized", "rmse", [1.0, 2.0]))
    for ok in (dict(unroll=2, reduction="mean"), dict(unroll=2, objective=eng.Objective(kind="mse")), dict(),
               dict(objective=eng.Objective("normalized", "rmse", [1.0, 2.0]))):
        step = eng.FusedStep(sim, grads, accumulate=3, **ok)
        assert step.accumulate == 3 and step.micro_index == 0 and step.ready is False
        step.reset_accumulation()
        assert step.micro_index == 0
        with pytest.raises(RuntimeError):
            step.accumulated_loss()                          # nothing has run
    one = eng.FusedStep(sim, grads)                          # today's constructor
    assert one.accumulate == 1 and one.reduction == "batch" and one.ready is True and one.micro_index == 0
    assert one._acc is None and one._gscratch is None and one._gsum is None          # no new buffer
    with pytest.raises(ValueError, match="accumulate = 1"):
        one.accumulated_loss()
    with pytest.raises(ValueError, match="accumulate = 1"):
        one.accumulation_coefficients()


def test_data_parallel_needs_the_fused_step(eng):
    sim, _ = _cpu_model(eng)                                 # a CPU model: DataParallel takes the autograd route
    with pytest.raises(ValueError, match="accumulate > 1 needs the fused step"):
        eng.DataParallel(sim, accumulate=2)
    with pytest.raises(ValueError, match="accumulate"):
        eng.DataParallel(sim, accumulate=0)
    dp = eng.DataParallel(sim)
    assert dp.fused is None
