"""CPU: the host side of the unrolled (K-step) training loss -- the three C-ABI entries are declared, bound and validate their
arguments before any device call, the trajectory bank's epoch order respects the horizon, and FusedStep refuses what it does
not implement.  No kernel is launched (tests/test_hip_unroll.py runs them)."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT

NEW = ("bsms_sim_unroll_bwd", "bsms_grad_accumulate", "bsms_batch_targets")
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
    for name in NEW:
        assert re.search(rf"\bint {name}\s*\(", text), f"{name} is not declared in include/bsms_hip.h"
        assert hasattr(lib, name), f"{name} is not exported"
        assert name in _abi.SIGNATURES
    assert _abi.lib().bsms_abi_version() == 4               # no existing signature changed


def test_sim_unroll_bwd_validates_before_any_device_call(eng):
    L = eng._abi.lib()
    one = 0x1000                                             # a non-null address that must never be dereferenced
    call = lambda R, Cc, pred=one, nxt=None, nin=None, in_stats=one, gnp=one: L.bsms_sim_unroll_bwd(
        pred, one, one, R, Cc, one, one, one, in_stats, in_stats, in_stats, one, 1.0, nxt, nin, None, None, gnp, None)
    assert call(300, 0) == E_UNSUPPORTED and call(300, 9) == E_UNSUPPORTED
    assert b"C=9" in L.bsms_last_error()
    assert call(0, 2) == E_UNSUPPORTED and call(-1, 2) == E_UNSUPPORTED      # like bsms_sim_loss_bwd: R >= 1
    assert call(300, 2, pred=None) == E_INVALID_ARG and call(300, 2, gnp=None) == E_INVALID_ARG
    assert call(300, 2, nxt=one) == E_INVALID_ARG and call(300, 2, nin=one) == E_INVALID_ARG     # half a carried pair
    assert b"together" in L.bsms_last_error()
    assert call(300, 2, nxt=one, nin=one, in_stats=None) == E_INVALID_ARG    # a carry needs the input normaliser
    assert call(300, 9, pred=None) == E_UNSUPPORTED          # the envelope is checked before the pointers


def test_grad_accumulate_and_batch_targets_validate_before_any_device_call(eng):
    L = eng._abi.lib()
    one = 0x1000
    assert L.bsms_grad_accumulate(None, None, 0, 0, None) == OK
    assert L.bsms_grad_accumulate(one, one + 64, -1, 0, None) == E_SHAPE
    assert L.bsms_grad_accumulate(None, one, 8, 0, None) == E_INVALID_ARG and L.bsms_grad_accumulate(one, None, 8, 1, None) == E_INVALID_ARG
    assert L.bsms_grad_accumulate(one, one, 8, 0, None) == E_INVALID_ARG

    from bsms_gnn_amd.databank import _Sample
    table = (_Sample * 2)()
    for s in table:
        s.state_in = s.state_tar = s.pos = s.type = one
        s.n = 100
    t = C.addressof(table)
    assert L.bsms_batch_targets(t, 2, 0, 2, one, None) == E_UNSUPPORTED and L.bsms_batch_targets(t, 2, 9, 2, one, None) == E_UNSUPPORTED
    assert L.bsms_batch_targets(t, 2, 3, 0, None, None) == OK            # K - 1 = 0: nothing to write, nothing is touched
    assert L.bsms_batch_targets(None, 0, 3, 2, None, None) == OK         # n_samples = 0 likewise
    assert L.bsms_batch_targets(t, 2, 3, 2, None, None) == E_INVALID_ARG and L.bsms_batch_targets(None, 2, 3, 2, one, None) == E_INVALID_ARG
    assert L.bsms_batch_targets(t, -1, 3, 2, one, None) == E_INVALID_ARG and L.bsms_batch_targets(t, 2, 3, -1, one, None) == E_INVALID_ARG
    table[1].state_tar = None
    assert L.bsms_batch_targets(t, 2, 3, 2, one, None) == E_INVALID_ARG
    table[1].state_tar, table[1].n = one, 1 << 40
    assert L.bsms_batch_targets(t, 2, 3, 2, one, None) == E_UNSUPPORTED


def test_epoch_picks_respect_the_horizon(eng):
    from bsms_gnn_amd.databank import epoch_picks, pick_lengths
    frames = [6, 9, 4]
    assert pick_lengths(frames) == [5, 8, 3] and pick_lengths(frames, 3) == [3, 6, 1]
    for order in ("trajectory", "global"):
        # horizon = 1 replays today's order draw for draw: the same generator state gives the same picks as the T - 1 lengths
        a = epoch_picks(np.random.default_rng(7), pick_lengths(frames, 1), order)
        b = epoch_picks(np.random.default_rng(7), [T - 1 for T in frames], order)
        assert a == b and len(a) == 16
        rng = np.random.default_rng(7)
        for _ in range(3):                                   # a few epochs on one generator
            picks = epoch_picks(rng, pick_lengths(frames, 3), order)
            assert sorted(picks) == [(si, ti) for si, T in enumerate(frames) for ti in range(T - 3)]
            assert all(ti + 3 <= frames[si] - 1 for si, ti in picks)       # frame t + horizon exists


def test_fused_step_refuses_what_it_does_not_implement(eng):
    from oracle import bsms_oracle as ro
    sim = eng.BSMS_Simulator(ro.make_cfg(2, 32, 2, 2, 2))
    grads = eng.GradBuckets(list(sim.parameters()))
    with pytest.raises(ValueError, match="graph"):
        eng.FusedStep(sim, grads, use_graph=True, unroll=2)
    with pytest.raises(ValueError):
        eng.FusedStep(sim, grads, unroll=0)
    with pytest.raises(ValueError, match="step_weights"):
        eng.FusedStep(sim, grads, unroll=3, step_weights=[0.5, 0.5])
    step = eng.FusedStep(sim, grads, unroll=3)
    assert step.unroll == 3 and step.step_weights == [1 / 3] * 3 and step.detach is False
    one = eng.FusedStep(sim, grads)                          # today's constructor: the single-step loss
    assert one.unroll == 1 and one.step_weights == [1.0]
