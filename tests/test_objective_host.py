"""CPU: the host side of the training objectives -- bsms_sim_objective_bwd is declared, exported, bound and
refuses in the documented order before any device call; `Objective` validates; `masked_loss` is the definition in torch.  No
kernel is launched (tests/test_hip_objective.py runs them)."""
import ctypes as C
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from conftest import ROOT

OK, E_INVALID_ARG, E_SHAPE, E_UNSUPPORTED = 0, -1, -2, -3


@pytest.fixture(scope="module")
def L():
    from bsms_gnn_amd import _abi
    return _abi.lib()


def test_entry_is_declared_exported_and_bound(L):
    from bsms_gnn_amd import _abi
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "bsms_hip.h")).read(), flags=re.S)
    m = re.search(r"\bint bsms_sim_objective_bwd\s*\((.*?)\)\s*;", text, flags=re.S)
    assert m, "bsms_sim_objective_bwd is not declared in include/bsms_hip.h"
    assert hasattr(C.CDLL(_abi.LIB_PATH), "bsms_sim_objective_bwd"), "bsms_sim_objective_bwd is not exported"
    assert len(m.group(1).split(",")) == len(_abi.SIGNATURES["bsms_sim_objective_bwd"][1]) == 23     # header and binding in step
    assert L.bsms_abi_version() == 4                         # no existing signature changed


def test_refusals_come_in_the_stated_order(L):
    one = 0x1000                                             # a non-null address that must never be dereferenced

    def call(R=300, Cc=3, space=1, kind=1, ptr=one, pred=None, nxt=None, nin=None, in_stats=None, gnp=None, sums=None, w=None):
        pick = lambda v: ptr if v is None else (None if v == "null" else v)
        return L.bsms_sim_objective_bwd(pick(pred), ptr, ptr, R, Cc, ptr, ptr, ptr, pick(in_stats), pick(in_stats), pick(in_stats),
                                        pick(sums), None if w is None else w, space, kind, 1.0, nxt, nin, None, None, None, pick(gnp), None)

    assert call(Cc=0, ptr=None) == E_UNSUPPORTED and call(Cc=9, ptr=None) == E_UNSUPPORTED     # before any pointer is looked at
    assert b"C=9" in L.bsms_last_error()
    assert call(space=2, ptr=None) == E_UNSUPPORTED and call(kind=-1, ptr=None) == E_UNSUPPORTED
    assert b"kind=-1" in L.bsms_last_error()
    assert call(space=-1) == E_UNSUPPORTED and call(kind=2) == E_UNSUPPORTED
    assert call(R=0, ptr=None) == E_UNSUPPORTED and call(R=-1) == E_UNSUPPORTED
    assert call(Cc=9, space=2) == E_UNSUPPORTED and b"C=9" in L.bsms_last_error()            # the envelope of R and C comes first
    for space in (0, 1):
        for kind in (0, 1):
            assert call(space=space, kind=kind, ptr=None) == E_INVALID_ARG                   # valid envelope, null pointers
            assert call(space=space, kind=kind, pred="null") == E_INVALID_ARG
    assert call(gnp="null") == E_INVALID_ARG and call(sums="null") == E_INVALID_ARG
    assert call(nxt=one) == E_INVALID_ARG                    # g_pred_next without g_norm_in_next
    assert b"together" in L.bsms_last_error()
    assert call(nin=one) == E_INVALID_ARG
    assert call(nxt=one, nin=one, in_stats="null") == E_INVALID_ARG                          # a carry needs the input normaliser


def test_objective_validates_and_knows_its_default():
    from bsms_gnn_amd import Objective
    assert Objective().is_default and Objective("physical", "rmse", None).is_default
    for o in (Objective(space="normalized"), Objective(kind="mse"), Objective(channel_weights=[1, 1, 1]), Objective("normalized", "mse", [1, 2])):
        assert not o.is_default
    assert Objective(channel_weights=[1, 2]).channel_weights == (1.0, 2.0)
    assert Objective("normalized", "mse", [1, 2]) == Objective("normalized", "mse", (1.0, 2.0)) != Objective("normalized", "mse")
    for bad in (dict(space="normalised"), dict(space=1), dict(kind="l1"), dict(kind=None), dict(channel_weights=[]),
                dict(channel_weights=[1.0, -1.0]), dict(channel_weights=[0.0, 0.0]), dict(channel_weights=[1.0, float("nan")]),
                dict(channel_weights=3.0), dict(channel_weights=["a"])):
        with pytest.raises(ValueError):
            Objective(**bad)
    with pytest.raises(AttributeError):
        Objective().kind = "mse"
    assert Objective(channel_weights=[1, 1, 4]).bind(3).channel_weights == (1.0, 1.0, 4.0)
    with pytest.raises(ValueError, match="out_dim"):
        Objective(channel_weights=[1, 1, 4]).bind(2)
    assert Objective.from_cfg(SimpleNamespace()).is_default and Objective.from_cfg(None).is_default
    o = Objective.from_cfg(SimpleNamespace(loss_space="normalized", loss_kind="mse", loss_channel_weights=[1, 2, 3]))
    assert (o.space, o.kind, o.channel_weights) == ("normalized", "mse", (1.0, 2.0, 3.0))


def test_wrong_number_of_weights_is_refused_when_bound_to_a_model():
    import bsms_gnn_amd as eng
    from oracle import bsms_oracle as ro
    sim = eng.BSMS_Simulator(ro.make_cfg(2, 32, 2, 2, 2))
    grads = eng.GradBuckets(list(sim.parameters()))
    with pytest.raises(ValueError, match="out_dim"):
        eng.FusedStep(sim, grads, objective=eng.Objective(channel_weights=[1, 1, 4]))
    with pytest.raises(ValueError, match="out_dim"):
        eng.DataParallel(sim, objective=eng.Objective(channel_weights=[1, 1, 4]))
    step = eng.FusedStep(sim, grads, objective=eng.Objective("normalized", "mse", [1, 4]))
    assert step.objective == eng.Objective("normalized", "mse", [1, 4]) and eng.FusedStep(sim, grads).objective.is_default


def _case():
    """Five rows, three channels, written out by hand; row 2 is masked out."""
    pred = np.array([[1.0, 2.0, 0.5], [0.0, -1.0, 0.25], [9.0, 9.0, 9.0], [2.0, 0.5, -0.5], [-1.0, 1.0, 0.75]], dtype=np.float32)
    tar = np.array([[0.5, 2.5, 0.25], [1.0, -1.5, 0.5], [0.0, 0.0, 0.0], [1.0, 1.0, -0.25], [-0.5, 0.0, 0.5]], dtype=np.float32)
    mask = np.array([1, 1, 0, 1, 1], dtype=np.float32)
    std = np.array([2.0, 0.5, 0.01], dtype=np.float64)
    return pred, tar, mask, std


def test_default_objective_is_masked_rmse_bit_for_bit():
    import bsms_gnn_amd as eng
    gen = torch.Generator().manual_seed(0)
    pred, tar = torch.randn(2, 37, 3, generator=gen), torch.randn(2, 37, 3, generator=gen)
    mask = (torch.rand(2, 37, 1, generator=gen) < 0.8).float()
    want = eng.masked_rmse(pred, tar, mask)
    assert torch.equal(eng.masked_loss(pred, tar, mask, eng.Objective(), None), want)
    assert torch.equal(eng.masked_loss(pred, tar, mask), want)
    p2 = pred.clone().requires_grad_(True)
    eng.masked_loss(p2, tar, mask, eng.Objective()).backward()
    p3 = pred.clone().requires_grad_(True)
    eng.masked_rmse(p3, tar, mask).backward()
    assert torch.equal(p2.grad, p3.grad)


@pytest.mark.parametrize("space", ["physical", "normalized"])
@pytest.mark.parametrize("kind", ["mse", "rmse"])
def test_masked_loss_against_numpy_fp64(space, kind):
    import bsms_gnn_amd as eng
    pred, tar, mask, std = _case()
    w = np.array([1.0, 1.0, 4.0])
    d = (pred - tar).astype(np.float64)                      # every entry is a multiple of 0.25: the fp32 difference is exact
    M, SE = mask.astype(np.float64).sum(), (mask[:, None].astype(np.float64) * d * d).sum(0)
    assert M == 4.0 and np.array_equal(SE, [0.25 + 1.0 + 1.0 + 0.25, 0.25 + 0.25 + 0.25 + 1.0, 4 * 0.0625])
    a = w / std ** 2 if space == "normalized" else w
    Q = (a * SE).sum() / (M * 3)
    want = Q if kind == "mse" else np.sqrt(Q)
    G = 2.0 / (M * 3) if kind == "mse" else 1.0 / (want * M * 3)
    want_grad = G * a[None, :] * mask[:, None] * d
    p = torch.tensor(pred).reshape(1, 5, 3).requires_grad_(True)
    loss = eng.masked_loss(p, torch.tensor(tar).reshape(1, 5, 3), torch.tensor(mask).reshape(1, 5, 1),
                           eng.Objective(space, kind, [1, 1, 4]), torch.tensor(std))
    assert loss.dtype == torch.float32 and abs(float(loss.detach()) - want) <= 6e-8 * want       # one rounding to fp32
    loss.backward()
    got = p.grad[0].double().numpy()
    assert np.abs(got - want_grad).max() <= 2e-7 * np.abs(want_grad).max() and bool((got[2] == 0).all())
    if space == "normalized":
        with pytest.raises(ValueError, match="std"):
            eng.masked_loss(p, torch.tensor(tar).reshape(1, 5, 3), torch.tensor(mask).reshape(1, 5, 1), eng.Objective(space, kind))
    with pytest.raises(ValueError, match="out_dim"):
        eng.masked_loss(p, torch.tensor(tar).reshape(1, 5, 3), torch.tensor(mask).reshape(1, 5, 1), eng.Objective(space, kind, [1, 4]),
                        torch.tensor(std))


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
    loss = dp.global_masked_loss(p, tar[sl], mask[sl], Objective("normalized", "rmse", [1, 1, 4]), std)
    loss.backward()
    torch.save({"loss": loss.detach(), "grad": p.grad}, f"{out_path}.{rank}")
    dist.barrier()
    dist.destroy_process_group()


def _global_case():
    gen = torch.Generator().manual_seed(3)
    pred, tar = torch.randn(6, 11, 3, generator=gen), torch.randn(6, 11, 3, generator=gen)
    mask = (torch.rand(6, 11, 1, generator=gen) < 0.7).float()
    return pred, tar, mask, torch.tensor([2.0, 0.5, 0.01], dtype=torch.float64)


@pytest.mark.timeout(300)
def test_global_masked_loss_over_two_gloo_ranks_is_the_whole_batch_loss(tmp_path):
    """The autograd route under data parallelism: the 1 + C fp64 sums are all-reduced, every rank holds the loss of the whole batch
    and the local gradients are the whole batch's, slice by slice (fp64 sums of 2 x 33 rows: the order of summation shows at 1e-15)."""
    import torch.multiprocessing as mp
    import bsms_gnn_amd as eng
    port = 29500 + os.getpid() % 2000
    out = str(tmp_path / "res")
    mp.start_processes(_gloo_worker, args=(2, port, out), nprocs=2, join=True, start_method="spawn")
    r0, r1 = torch.load(out + ".0"), torch.load(out + ".1")
    pred, tar, mask, std = _global_case()
    p = pred.clone().requires_grad_(True)
    want = eng.masked_loss(p, tar, mask, eng.Objective("normalized", "rmse", [1, 1, 4]), std)
    want.backward()
    assert torch.equal(r0["loss"], r1["loss"])
    torch.testing.assert_close(r0["loss"], want.detach(), rtol=2e-7, atol=0)
    torch.testing.assert_close(torch.cat([r0["grad"], r1["grad"]]), p.grad, rtol=1e-6, atol=1e-9 * float(p.grad.abs().max()))
