"""CPU: the host side of the robust training objectives -- `masked_loss` with kind "mae" / "huber" against
torch.nn.functional's l1_loss / huber_loss, the limiting cases of the Huber loss, `Objective`'s validation of `delta`, the two new
C-ABI entries declared, exported, bound and refusing in the documented order, and the constructors that take a robust objective.  No
kernel is launched (tests/test_hip_robust.py runs them)."""
import ctypes as C
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import ROOT

OK, E_INVALID_ARG, E_SHAPE, E_UNSUPPORTED = 0, -1, -2, -3
PAIRS = [("physical", "mae"), ("physical", "huber"), ("normalized", "mae"), ("normalized", "huber")]


@pytest.fixture(scope="module")
def L():
    from bsms_gnn_amd import _abi
    return _abi.lib()


# ------------------------------------------------------------------------------------------------ the definition in torch
def _case():
    """Six rows, three channels, every entry a multiple of 1/8 (the fp32 difference is exact, so fp64 copies of the inputs give the
    same d).  Row 2 is masked out; d == 0 exactly at [0, 2] and [4, 0]; |d| == 0.5 exactly at [0, 0], [1, 1], [3, 2]."""
    pred = np.array([[1.0, 2.0, 0.5], [0.0, -1.0, 0.25], [9.0, 9.0, 9.0], [2.0, 0.5, -0.5], [-1.0, 1.0, 0.75], [0.125, -3.0, 2.0]])
    tar = np.array([[0.5, 2.5, 0.5], [1.0, -1.5, 0.5], [0.0, 0.0, 0.0], [1.0, 1.0, -1.0], [-1.0, 0.0, 0.5], [0.0, 1.0, -0.25]])
    mask = np.array([1, 1, 0, 1, 1, 1], dtype=np.float64)
    return pred, tar, mask


def _third_party(pred, tar, mask, omega, s, w, delta, kind):
    """The loss from torch.nn.functional alone, fp64: rho on pred / s and tar / s, weighted by mu * w_c, summed, over M C."""
    p, t = pred / s, tar / s
    if kind == "mae":
        rho = F.l1_loss(p, t, reduction="none")
    else:                                                    # huber_loss takes one delta: channel by channel
        rho = torch.stack([F.huber_loss(p[..., c], t[..., c], reduction="none", delta=float(delta[c])) for c in range(p.shape[-1])], -1)
    mu = (mask * omega).unsqueeze(-1)
    return (mu * w * rho).sum() / (mu.sum() * p.shape[-1])


@pytest.mark.parametrize("node_weighted", [False, True])
@pytest.mark.parametrize("space,kind,delta", [(s, k, d) for s, k in PAIRS for d in ((0.5, (0.5, 2.0, 0.125)) if k == "huber" else (0.5,))])
def test_masked_loss_is_torch_functional_l1_and_huber(space, kind, delta, node_weighted):
    """Value and pred.grad against torch.nn.functional at 1e-12, in fp64: `pred` is an fp64 leaf holding fp32 values, so autograd's
    gradient is not rounded to fp32 on the way out; `masked_loss` itself returns its fp64 value rounded ONCE to fp32 (as every kind
    does), so the value is compared before that rounding (the terms of `finish_loss` on `robust_sums`) and `masked_loss` must be that
    number's fp32 rounding, bit for bit.  delta = 0.5 in the physical space puts three elements exactly on |u| == delta."""
    from bsms_gnn_amd import Objective, masked_loss
    from bsms_gnn_amd.objective import finish_loss, robust_sums
    pred, tar, mask = (torch.tensor(a, dtype=torch.float64) for a in _case())
    std = torch.tensor([2.0, 0.5, 0.25], dtype=torch.float64)          # powers of two: u is exact in the normalized space too
    s = std if space == "normalized" else torch.ones(3, dtype=torch.float64)
    w = torch.tensor([1.0, 0.5, 4.0], dtype=torch.float64)
    omega = torch.tensor([0.5, 2.0, 7.0, 1.0, 0.25, 3.0], dtype=torch.float64) if node_weighted else torch.ones(6, dtype=torch.float64)
    dl = torch.tensor([delta] * 3 if isinstance(delta, float) else delta, dtype=torch.float64)
    obj = Objective(space, kind, [1.0, 0.5, 4.0], node_weighted, delta=delta if kind == "huber" else None)
    nw = omega.float() if node_weighted else None

    p_ref = pred.clone().requires_grad_(True)
    want = _third_party(p_ref, tar, mask, omega, s, w, dl, kind)
    want.backward()

    p = pred.clone().requires_grad_(True)
    M, S = robust_sums(p.reshape(1, 6, 3), tar.reshape(1, 6, 3), mask.reshape(1, 6, 1), obj, std, nw)
    loss32, terms = finish_loss(M, S, obj, std)
    got = terms.sum()
    got_f, want_f = float(got.detach()), float(want.detach())
    assert got.dtype == torch.float64 and abs(got_f - want_f) <= 1e-12 * abs(want_f), (got_f, want_f)
    p2 = pred.clone().requires_grad_(True)
    loss = masked_loss(p2.reshape(1, 6, 3), tar.reshape(1, 6, 3), mask.reshape(1, 6, 1), obj, std, node_weights=nw)
    assert loss.dtype == torch.float32 and torch.equal(loss.detach(), got.detach().float()) and torch.equal(loss32.detach(), loss.detach())
    loss.backward()
    scale = float(p_ref.grad.abs().max())
    assert float((p2.grad - p_ref.grad).abs().max()) <= 1e-12 * scale
    assert bool((p2.grad[2] == 0).all())                                               # the masked-out row
    assert float(p2.grad[0, 2]) == 0.0 and float(p2.grad[4, 0]) == 0.0                 # d == 0 exactly: sign(0) = 0
    assert float(p2.grad[0, 0]) != 0.0
    # fp32 inputs, what the step sees: the same loss bits, the same gradient rounded once
    p3 = pred.float().requires_grad_(True)
    l3 = masked_loss(p3.reshape(1, 6, 3), tar.float().reshape(1, 6, 3), mask.float().reshape(1, 6, 1), obj, std, node_weights=nw)
    l3.backward()
    assert torch.equal(l3.detach(), loss.detach()) and torch.equal(p3.grad, p2.grad.float())


def test_an_element_on_the_threshold_takes_either_branch_to_the_same_value():
    """d = 0.5 with delta = 0.5 in the physical space: u^2 / 2 = delta (|u| - delta / 2) = 0.125 and psi = 0.5 from both sides."""
    from bsms_gnn_amd import Objective, masked_loss
    p = torch.tensor([[[1.0]]], requires_grad=True)
    loss = masked_loss(p, torch.tensor([[[0.5]]]), torch.ones(1, 1, 1), Objective(kind="huber", delta=0.5))
    loss.backward()
    assert float(loss) == 0.125 and float(p.grad) == 0.5


@pytest.mark.parametrize("space", ["physical", "normalized"])
def test_huber_limits_are_half_the_mse_and_a_shifted_mae(space):
    """delta = 1e30: every element is in the quadratic branch, the loss is half the "mse" objective of the same space and weights.
    delta below every |u|: every element is in the linear branch, S_c = delta_c (AE_c - M delta_c / 2) -- per channel, the terms are
    delta_c (mae_c - w_c delta_c / (2 C)).  Both to 1e-12 relative, on the fp64 terms (before the one rounding to fp32)."""
    from bsms_gnn_amd import Objective
    from bsms_gnn_amd.objective import channel_sums, finish_loss, robust_sums
    gen = torch.Generator().manual_seed(11)
    pred, tar = torch.randn(2, 41, 3, generator=gen), torch.randn(2, 41, 3, generator=gen)
    mask = (torch.rand(2, 41, 1, generator=gen) < 0.8).float()
    nw = torch.exp(torch.randn(2, 41, generator=gen))
    std = torch.tensor([2.0, 0.3, 0.05], dtype=torch.float64)
    cw = [1.0, 0.5, 3.0]
    terms = lambda o: finish_loss(*(robust_sums(pred, tar, mask, o, std, nw) if o.is_robust else channel_sums(pred, tar, mask, nw)), o, std)[1]
    big = terms(Objective(space, "huber", cw, True, delta=1e30))
    mse = terms(Objective(space, "mse", cw, True))
    assert float(((big - 0.5 * mse).abs() / (0.5 * mse)).max()) <= 1e-12
    s = std if space == "normalized" else torch.ones(3, dtype=torch.float64)
    u_min = ((pred - tar).double() / s).abs()[mask[..., 0] > 0].min(0).values
    delta = tuple(float(x) for x in 0.5 * u_min)
    assert all(d > 0 for d in delta)
    small = terms(Objective(space, "huber", cw, True, delta=delta))
    mae = terms(Objective(space, "mae", cw, True))
    dl = torch.tensor(delta, dtype=torch.float64)
    want = dl * (mae - torch.tensor(cw, dtype=torch.float64) * 0.5 * dl / 3)
    assert float(((small - want).abs() / want).max()) <= 1e-12


# ------------------------------------------------------------------------------------------------ Objective
def test_objective_validates_delta_and_keeps_every_old_objective():
    from bsms_gnn_amd import Objective
    from bsms_gnn_amd import objective as om
    assert om.KINDS == {"rmse": 0, "mse": 1} and om.SPACES == {"physical": 0, "normalized": 1} and om.ROBUST_KINDS == {"mae": 0, "huber": 1}
    with pytest.raises(ValueError, match="delta"):
        Objective(kind="huber")                              # missing
    for kind in ("mae", "mse", "rmse"):
        with pytest.raises(ValueError, match="delta"):
            Objective(kind=kind, delta=1.0)                  # refused by every other kind
    for bad in (0.0, -1.0, float("inf"), float("nan"), [], [1.0, 0.0], [1.0, float("nan")], "1", True, [[1.0]]):
        with pytest.raises(ValueError):
            Objective(kind="huber", delta=bad)
    with pytest.raises(ValueError):
        Objective(kind="l1")
    with pytest.raises(TypeError):
        Objective("physical", "huber", None, False, 1.0)     # keyword only: the positional order is unchanged
    h = Objective("normalized", "huber", delta=1)
    assert h.delta == 1.0 and isinstance(h.delta, float) and h.is_robust and not h.is_default and h.bind(3) is h
    hc = Objective(kind="huber", delta=[1, 2, 0.5])
    assert hc.delta == (1.0, 2.0, 0.5) and hc.bind(3) is hc
    assert Objective(kind="huber", delta=torch.tensor([1.0, 2.0])).delta == (1.0, 2.0)
    with pytest.raises(ValueError, match="out_dim"):
        hc.bind(2)
    with pytest.raises(AttributeError):
        h.delta = 2.0
    assert Objective(kind="mae").is_robust and not Objective(kind="mae").is_default and Objective(kind="mae").delta is None
    # equality and hash tell deltas apart (input_gradient's step cache keys on the objective)
    a, b = Objective(kind="huber", delta=1.0), Objective(kind="huber", delta=2.0)
    assert a != b and hash(a) != hash(b) and a == Objective(kind="huber", delta=1.0) and hash(a) == hash(Objective(kind="huber", delta=1))
    assert Objective(kind="huber", delta=(1.0, 1.0)) != Objective(kind="huber", delta=1.0)
    assert len({a, b, Objective(kind="huber", delta=1.0), Objective(kind="mae"), Objective(kind="mse")}) == 4
    assert "delta=1.0" in repr(a) and "delta" not in repr(Objective(kind="mae"))
    # from_cfg
    o = Objective.from_cfg(SimpleNamespace(loss_space="normalized", loss_kind="huber", loss_delta=1.5))
    assert (o.space, o.kind, o.delta) == ("normalized", "huber", 1.5)
    assert Objective.from_cfg(SimpleNamespace(loss_kind="huber", loss_delta=[1, 2])).delta == (1.0, 2.0)
    assert Objective.from_cfg(SimpleNamespace(loss_kind="mae")) == Objective(kind="mae")
    with pytest.raises(ValueError, match="delta"):
        Objective.from_cfg(SimpleNamespace(loss_kind="huber"))
    with pytest.raises(ValueError, match="delta"):
        Objective.from_cfg(SimpleNamespace(loss_kind="mse", loss_delta=1.0))
    # every objective that existed before: the same repr, equality, default flag
    assert repr(Objective()) == "Objective(space='physical', kind='rmse', channel_weights=None)"
    assert repr(Objective("normalized", "mse", [1, 2], True)) == \
        "Objective(space='normalized', kind='mse', channel_weights=(1.0, 2.0), node_weighted=True)"
    assert Objective().is_default and not Objective().is_robust and Objective() == Objective("physical", "rmse", None, False)
    assert not Objective(kind="mse").is_default and not Objective("normalized", "mse", [1, 2]).is_robust
    assert Objective.from_cfg(SimpleNamespace()).is_default and Objective.from_cfg(None).is_default


# ------------------------------------------------------------------------------------------------ the header contract
ENTRIES = {"bsms_robust_sums": 21, "bsms_sim_robust_bwd": 26}


def test_entries_are_declared_exported_and_bound(L):
    from bsms_gnn_amd import _abi
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "bsms_hip.h")).read(), flags=re.S)
    raw = C.CDLL(_abi.LIB_PATH)
    for name, nargs in ENTRIES.items():
        m = re.search(rf"\bint {name}\s*\((.*?)\)\s*;", text, flags=re.S)
        assert m, f"{name} is not declared in include/bsms_hip.h"
        assert hasattr(raw, name), f"{name} is not exported"
        assert len(m.group(1).split(",")) == len(_abi.SIGNATURES[name][1]) == nargs
        assert getattr(L, name).argtypes == _abi.SIGNATURES[name][1]
        assert "delta" in m.group(1) and "rkind" in m.group(1)
    assert re.search(r"BSMS_ROBUST_MAE\s*=\s*0\s*,\s*BSMS_ROBUST_HUBER\s*=\s*1", text)
    # the twin is bsms_sim_objective_bwd_w plus `delta`; nothing that existed moved
    assert len(_abi.SIGNATURES["bsms_sim_objective_bwd_w"][1]) == 25 and len(_abi.SIGNATURES["bsms_sim_objective_bwd"][1]) == 23
    assert len(_abi.SIGNATURES["bsms_error_sums"][1]) == 12 and len(_abi.SIGNATURES["bsms_error_sums_w"][1]) == 14
    assert len(_abi.SIGNATURES["bsms_accum_coef"][1]) == 17
    assert L.bsms_abi_version() == 4


def test_robust_sums_refuses_in_the_stated_order(L):
    one = 0x1000                                             # a non-null address that must never be dereferenced

    def call(S=2, rows=10, Cc=3, space=0, rkind=0, ptr=one, weights=None, strides=(10, 10, 10, 10), stats="same", delta="same",
             stride=None, sums="same"):
        pick = lambda v: ptr if v == "same" else v
        return L.bsms_robust_sums(ptr, ptr, ptr, weights, S, rows, Cc, *strides, pick(stats), pick(stats), pick(stats), pick(delta), space,
                                  rkind, pick(sums), 1 + Cc if stride is None else stride, ptr, None)

    assert call(Cc=0, ptr=None) == E_UNSUPPORTED and call(Cc=9, ptr=None) == E_UNSUPPORTED      # 1: before any pointer is looked at
    assert b"C=9" in L.bsms_last_error()
    for space, rkind in ((2, 0), (-1, 0), (0, 2), (0, -1)):
        assert call(space=space, rkind=rkind, ptr=None) == E_UNSUPPORTED
    assert b"rkind=-1" in L.bsms_last_error()
    assert call(Cc=9, rkind=2) == E_UNSUPPORTED and b"C=9" in L.bsms_last_error()              # C comes first
    assert call(rkind=2, rows=-1, ptr=None) == E_UNSUPPORTED                                    # ... and both before the envelope
    assert call(rows=-1) == E_INVALID_ARG and call(S=-1) == E_INVALID_ARG and call(rows=1 << 31) == E_INVALID_ARG      # 2
    for k in range(4):
        assert call(strides=tuple(-1 if j == k else 10 for j in range(4))) == E_INVALID_ARG and b"stride" in L.bsms_last_error()
    assert call(stride=3) == E_INVALID_ARG and b"sums_stride" in L.bsms_last_error()           # 1 + C = 4 doubles at least
    assert call(stride=3, ptr=None) == E_INVALID_ARG and b"sums_stride" in L.bsms_last_error()  # the envelope before the pointers
    assert call(S=0, ptr=None) == OK and call(S=0, stride=3, ptr=None) == E_INVALID_ARG
    assert call(ptr=None) == E_INVALID_ARG and b"null" in L.bsms_last_error()                  # 3
    assert call(sums=None) == E_INVALID_ARG
    assert call(space=1, stats=None) == E_INVALID_ARG and b"null" in L.bsms_last_error()       # the statistics, normalized space only
    assert call(rkind=1, delta=None) == E_INVALID_ARG and b"null" in L.bsms_last_error()       # delta, Huber only
    assert call(rows=0, ptr=None) == E_INVALID_ARG                                              # seg_rows = 0 still writes zeros


def test_robust_bwd_refuses_in_the_stated_order(L):
    one = 0x1000

    def call(R=300, Cc=3, space=1, rkind=1, ptr=one, weights=None, period=300, delta="same", nxt=None, nin=None, in_stats="same",
             gnp="same"):
        pick = lambda v: ptr if v == "same" else v
        return L.bsms_sim_robust_bwd(ptr, ptr, ptr, weights, period, R, Cc, ptr, ptr, ptr, pick(in_stats), pick(in_stats), pick(in_stats),
                                     ptr, None, pick(delta), space, rkind, 1.0, nxt, nin, None, None, None, pick(gnp), None)

    assert call(Cc=0, ptr=None) == E_UNSUPPORTED and call(Cc=9, ptr=None) == E_UNSUPPORTED     # before any pointer is looked at
    assert b"C=9" in L.bsms_last_error()
    assert call(R=0, ptr=None) == E_UNSUPPORTED and call(R=-1) == E_UNSUPPORTED
    assert call(space=2, ptr=None) == E_UNSUPPORTED and call(rkind=-1, ptr=None) == E_UNSUPPORTED
    assert b"rkind=-1" in L.bsms_last_error()
    assert call(rkind=2) == E_UNSUPPORTED and call(Cc=9, space=2) == E_UNSUPPORTED and b"C=9" in L.bsms_last_error()
    assert call(Cc=9, weights=one, period=7) == E_UNSUPPORTED                                   # the envelope before the weights
    for space in (0, 1):
        for rkind in (0, 1):
            assert call(space=space, rkind=rkind, ptr=None) == E_INVALID_ARG and b"null" in L.bsms_last_error()
    assert call(rkind=1, delta=None) == E_INVALID_ARG and b"null" in L.bsms_last_error()       # delta is required under Huber only
    assert call(rkind=0, delta=None, nxt=one) == E_INVALID_ARG and b"together" in L.bsms_last_error()
    for period in (0, -300, 7, 299, 301, 600):
        assert call(weights=one, period=period) == E_INVALID_ARG and b"weight_period" in L.bsms_last_error(), period
        assert call(period=period, nxt=one) == E_INVALID_ARG and b"together" in L.bsms_last_error()    # ignored without weights
    assert call(weights=one, period=7, gnp=None) == E_INVALID_ARG and b"null" in L.bsms_last_error()    # null pointers before the period
    assert call(weights=one, period=7, nxt=one) == E_INVALID_ARG and b"weight_period" in L.bsms_last_error()   # the period before the pair
    assert call(nin=one) == E_INVALID_ARG and b"together" in L.bsms_last_error()
    assert call(nxt=one, nin=one, in_stats=None) == E_INVALID_ARG                               # a carry needs the input normaliser


def test_the_closed_entries_stay_closed(L):
    """bsms_sim_objective_bwd(_w), bsms_error_sums(_w) and bsms_accum_coef accept and refuse what they did: the robust kinds came as
    new entries and a new enum, not as kind = 2."""
    one = 0x1000
    assert L.bsms_sim_objective_bwd(one, one, one, 300, 3, one, one, one, one, one, one, one, None, 1, 2, 1.0, None, None, None, None, None,
                                    one, None) == E_UNSUPPORTED
    assert b"kind=2" in L.bsms_last_error()
    assert L.bsms_sim_objective_bwd_w(one, one, one, one, 300, 300, 3, one, one, one, one, one, one, one, None, 1, 2, 1.0, None, None, None,
                                      None, None, one, None) == E_UNSUPPORTED
    assert L.bsms_accum_coef(one, 1, 10, 3, one, one, one, None, 0, 2, 0, 0, 1, one, one, one, None) == E_UNSUPPORTED
    assert L.bsms_accum_coef(one, 1, 3, 3, one, one, one, None, 0, 1, 0, 0, 1, one, one, one, None) == E_SHAPE     # a row shorter than 1 + C
    assert L.bsms_abi_version() == 4


# ------------------------------------------------------------------------------------------------ constructors
def _cpu_model():
    import bsms_gnn_amd as eng
    from oracle import bsms_oracle as ro
    sim = eng.BSMS_Simulator(ro.make_cfg(2, 32, 2, 2, 2))
    return eng, sim, eng.GradBuckets(list(sim.parameters()))


def test_fused_step_and_data_parallel_take_a_robust_objective():
    eng, sim, grads = _cpu_model()
    for o in (eng.Objective(kind="mae"), eng.Objective("normalized", "huber", delta=1.0),
              eng.Objective("normalized", "huber", [1.0, 2.0], True, delta=[0.5, 2.0])):
        step = eng.FusedStep(sim, grads, objective=o)
        assert step.objective == o and step._obj is o and step.objective.is_robust
        assert eng.DataParallel(sim, objective=o).objective == o
    # no square root: the exact batch gradient of an unrolled loss exists for the robust kinds, as for "mse"
    step = eng.FusedStep(sim, grads, accumulate=2, unroll=2, reduction="batch", objective=eng.Objective("normalized", "huber", delta=1.0))
    assert step.accumulate == 2 and step.unroll == 2
    eng.FusedStep(sim, grads, accumulate=2, unroll=2, reduction="batch", objective=eng.Objective(kind="mae"))
    with pytest.raises(ValueError, match=r'reduction="mean".*loss_kind="mse"'):
        eng.FusedStep(sim, grads, accumulate=2, unroll=2, reduction="batch", objective=eng.Objective("normalized", "rmse"))
    for make in (lambda o: eng.FusedStep(sim, grads, objective=o), lambda o: eng.DataParallel(sim, objective=o)):
        with pytest.raises(ValueError, match="out_dim"):
            make(eng.Objective(kind="huber", delta=[1.0, 1.0, 1.0]))
    # the keys a Trainer reads from its model config (the Trainer itself needs a device: tests/test_hip_robust.py)
    sim.cfg.loss_kind, sim.cfg.loss_delta, sim.cfg.loss_space = "huber", [1.0, 0.5], "normalized"
    assert eng.DataParallel(sim).objective == eng.Objective("normalized", "huber", delta=(1.0, 0.5))
    sim.cfg.loss_delta = [1.0, 0.5, 2.0]
    with pytest.raises(ValueError, match="out_dim"):
        eng.DataParallel(sim)


# ------------------------------------------------------------------------------------------------ two gloo ranks
def _global_case():
    gen = torch.Generator().manual_seed(3)
    pred, tar = torch.randn(6, 11, 3, generator=gen), torch.randn(6, 11, 3, generator=gen)
    mask = (torch.rand(6, 11, 1, generator=gen) < 0.7).float()
    return pred, tar, mask, torch.tensor([2.0, 0.5, 0.01], dtype=torch.float64)


def _gloo_worker(rank, world, port, out_path):
    import sys
    sys.path.insert(0, ROOT)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    import torch.distributed as dist
    dist.init_process_group("gloo", rank=rank, world_size=world)
    torch.set_num_threads(1)
    import bsms_gnn_amd.dp as dp                          # imports without touching the GPU
    from bsms_gnn_amd.objective import Objective
    pred, tar, mask, std = _global_case()
    sl = slice(rank * 3, rank * 3 + 3)
    p = pred[sl].clone().requires_grad_(True)
    loss = dp.global_masked_loss(p, tar[sl], mask[sl], Objective("normalized", "huber", [1, 1, 4], delta=(1.0, 2.0, 50.0)), std)
    loss.backward()
    torch.save({"loss": loss.detach(), "grad": p.grad}, f"{out_path}.{rank}")
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.timeout(300)
def test_global_huber_loss_over_two_gloo_ranks_is_the_whole_batch_loss(tmp_path):
    """The 1 + C fp64 sums (M, S_c) are all-reduced: both ranks hold the same bits, equal to the single-process loss on the
    concatenated batch to the fp32 rounding of the result (2e-7: fp64 sums of 2 x 33 rows differ by their order at 1e-15), and the
    local gradients are the whole batch's, slice by slice."""
    import torch.multiprocessing as mp
    import bsms_gnn_amd as eng
    port = 31500 + os.getpid() % 2000
    out = str(tmp_path / "res")
    mp.start_processes(_gloo_worker, args=(2, port, out), nprocs=2, join=True, start_method="spawn")
    r0, r1 = torch.load(out + ".0"), torch.load(out + ".1")
    pred, tar, mask, std = _global_case()
    p = pred.clone().requires_grad_(True)
    want = eng.masked_loss(p, tar, mask, eng.Objective("normalized", "huber", [1, 1, 4], delta=(1.0, 2.0, 50.0)), std)
    want.backward()
    assert torch.equal(r0["loss"], r1["loss"])
    torch.testing.assert_close(r0["loss"], want.detach(), rtol=2e-7, atol=0)
    torch.testing.assert_close(torch.cat([r0["grad"], r1["grad"]]), p.grad, rtol=1e-6, atol=1e-9 * float(p.grad.abs().max()))
