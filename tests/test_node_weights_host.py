"""CPU: the host side of node-weighted objectives -- `lumped_node_measure` against closed forms, `Objective`'s
`node_weighted` flag, `masked_loss(node_weights=)` against NumPy fp64 and its autograd gradient against the closed form, every
refusal before a device is needed, and the two new C-ABI entries declared, exported, bound and refusing in the documented order.  No
kernel is launched (tests/test_hip_node_weights.py runs them)."""
import ctypes as C
import math
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


# ------------------------------------------------------------------------------------------------ 10: the lumped measure
SQUARE = np.array([[0.0, 0.0], [1.0, 0.0], [1.0, 1.0], [0.0, 1.0]])
TWO_TRIANGLES = np.array([[0, 1, 2], [0, 2, 3]])
TETRA = np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]])


def test_lumped_measure_closed_forms():
    from bsms_gnn_amd import lumped_node_measure
    from bsms_gnn_amd.hierarchy import lumped_node_measure64
    m = lumped_node_measure(SQUARE, TWO_TRIANGLES, "tri")
    assert m.dtype == np.float32 and m.shape == (4,)
    third, sixth = np.float32(1.0 / 3.0), np.float32(1.0 / 6.0)
    assert m.tolist() == [third, sixth, third, sixth]                  # the diagonal nodes 0 and 2 belong to both triangles
    m64 = lumped_node_measure64(SQUARE, TWO_TRIANGLES, "tri")
    assert m64.dtype == np.float64 and m64.tolist() == [2 * (0.5 / 3), 0.5 / 3, 2 * (0.5 / 3), 0.5 / 3]
    assert math.fsum(m64) == 1.0                                       # the fp64 sum, rounded once, is the area exactly
    q = lumped_node_measure64(SQUARE, np.array([[0, 1, 2, 3]]), "quad")
    assert q.tolist() == [0.25] * 4 and q.sum() == 1.0
    assert lumped_node_measure(SQUARE, np.array([[0, 1, 2, 3]]), "quad").tolist() == [0.25] * 4
    t = lumped_node_measure64(TETRA, np.array([[0, 1, 2, 3]]), "tetra")
    assert np.abs(t - 1.0 / 24.0).max() <= 1e-16 and lumped_node_measure(TETRA, np.array([[0, 1, 2, 3]]), "tetra").tolist() == [np.float32(1 / 24)] * 4
    # orientation does not matter, an unused node gets 0, a triangle in 3-D has its area
    assert lumped_node_measure64(SQUARE, TWO_TRIANGLES[:, ::-1], "tri").tolist() == m64.tolist()
    pos5 = np.concatenate([SQUARE, [[5.0, 5.0]]])
    assert lumped_node_measure64(pos5, TWO_TRIANGLES, "tri").tolist() == [*m64.tolist(), 0.0]
    lifted = np.concatenate([SQUARE, np.zeros((4, 1))], 1) @ np.array([[0.6, 0.0, 0.8], [0.0, 1.0, 0.0], [-0.8, 0.0, 0.6]])
    assert np.abs(lumped_node_measure64(lifted, TWO_TRIANGLES, "tri") - m64).max() <= 1e-15
    # line segments ([2, E], as to_flat_edge reads them): half a length per end
    assert lumped_node_measure64(SQUARE, np.array([[0, 1], [1, 2]]), "line").tolist() == [0.5, 1.0, 0.5, 0.0]


@pytest.mark.parametrize("mesh_type,pos,cells,power", [("tri", SQUARE, TWO_TRIANGLES, 2), ("quad", SQUARE, np.array([[0, 1, 2, 3]]), 2),
                                                       ("tetra", TETRA, np.array([[0, 1, 2, 3]]), 3), ("line", SQUARE, np.array([[0, 1], [1, 2]]), 1)])
def test_lumped_measure_scales_with_the_mesh(mesh_type, pos, cells, power):
    """A translated mesh scaled by s = 4 (a power of two: exact) has s^p times the measure."""
    from bsms_gnn_amd.hierarchy import lumped_node_measure64
    base = lumped_node_measure64(pos, cells, mesh_type)
    moved = lumped_node_measure64(4.0 * pos + 3.0, cells, mesh_type)
    assert np.abs(moved - 4.0 ** power * base).max() <= 1e-13 * 4.0 ** power and base.sum() > 0


def test_lumped_measure_on_a_delaunay_mesh_sums_to_the_hull_area():
    from scipy.spatial import ConvexHull, Delaunay
    from bsms_gnn_amd.hierarchy import lumped_node_measure64
    pts = np.random.default_rng(3).random((200, 2))
    m = lumped_node_measure64(pts, Delaunay(pts).simplices, "tri")
    assert m.min() > 0 and abs(m.sum() - ConvexHull(pts).volume) <= 1e-12


def test_lumped_measure_refusals():
    from bsms_gnn_amd import lumped_node_measure, to_flat_edge
    for bad in ("hexa", "triangle", None):
        with pytest.raises(ValueError):
            lumped_node_measure(SQUARE, TWO_TRIANGLES, bad)
        with pytest.raises(ValueError):
            to_flat_edge(TWO_TRIANGLES, bad)                           # the same types are refused by both
    with pytest.raises(ValueError):
        lumped_node_measure(SQUARE, TWO_TRIANGLES, "quad")             # three nodes per cell
    with pytest.raises(ValueError):
        lumped_node_measure(SQUARE, np.array([[0, 1, 4]]), "tri")      # node 4 of 4
    with pytest.raises(ValueError):
        lumped_node_measure(SQUARE, np.array([[0, 1, 2, 3]]), "tetra")  # 2-D positions


# ------------------------------------------------------------------------------------------------ 11: Objective
def test_objective_flag():
    from bsms_gnn_amd import Objective
    o = Objective(node_weighted=True)
    assert o.node_weighted and not o.is_default and Objective().node_weighted is False and Objective().is_default
    assert o == Objective("physical", "rmse", None, True) and o != Objective() and hash(o) != hash(Objective())
    assert Objective("normalized", "mse", [1, 2], node_weighted=True) != Objective("normalized", "mse", [1, 2])
    assert len({o, Objective(node_weighted=True), Objective()}) == 2
    assert "node_weighted=True" in repr(o) and "node_weighted" not in repr(Objective())
    for bad in (1, "yes", None):
        with pytest.raises(ValueError):
            Objective(node_weighted=bad)
    with pytest.raises(AttributeError):
        o.node_weighted = False
    cfg = SimpleNamespace(loss_space="normalized", loss_node_weights=True)
    assert Objective.from_cfg(cfg) == Objective("normalized", node_weighted=True)
    assert Objective.from_cfg(SimpleNamespace(loss_node_weights=False)).is_default and Objective.from_cfg(SimpleNamespace()).is_default
    with pytest.raises(ValueError):
        Objective.from_cfg(SimpleNamespace(loss_node_weights="measure"))   # a flag, not the bank's option


def test_weight_refusals_need_no_device():
    from bsms_gnn_amd import Objective, masked_loss
    from bsms_gnn_amd.objective import channel_sums
    pred, tar, mask, w = torch.zeros(2, 5, 3), torch.ones(2, 5, 3), torch.ones(2, 5, 1), torch.ones(5)
    on, off = Objective(node_weighted=True), Objective(kind="mse")
    with pytest.raises(ValueError, match="no node_weights"):
        masked_loss(pred, tar, mask, on)
    for objective in (off, Objective(), None):
        with pytest.raises(ValueError):
            masked_loss(pred, tar, mask, objective, node_weights=w)    # weights without the flag, the default objective included
    for bad in (w.double(), w.int(), [1.0] * 5, -w, torch.tensor([1.0, 1.0, float("nan"), 1.0, 1.0]), torch.tensor([1.0, 1.0, float("inf"), 1.0, 1.0])):
        with pytest.raises(ValueError):
            masked_loss(pred, tar, mask, on, node_weights=bad)
    assert float(masked_loss(pred, tar, mask, on, node_weights=torch.zeros(5).index_fill_(0, torch.tensor([2]), 1.0))) == 1.0   # zeros are weights
    assert channel_sums(pred, tar, mask)[0] == 10.0 and channel_sums(pred, tar, mask, 2 * w)[0] == 20.0


def np_loss(pred, tar, mask, w, space, kind, cw, std):
    d = (pred - tar).astype(np.float32).astype(np.float64)
    mu = (mask.astype(np.float64) * w.astype(np.float64))[..., None]
    C = pred.shape[-1]
    M, SE = mu.sum(), (mu * d * d).reshape(-1, C).sum(0)
    a = np.ones(C) if cw is None else np.asarray(cw, np.float64)
    if space == "normalized":
        a = a / std.astype(np.float64) ** 2
    Q = (a * SE).sum() / (M * C)
    return M, SE, a, (Q if kind == "mse" else np.sqrt(Q))


@pytest.mark.parametrize("space,kind", [("physical", "rmse"), ("physical", "mse"), ("normalized", "rmse"), ("normalized", "mse")])
def test_masked_loss_with_weights_against_numpy_and_its_gradient(space, kind):
    """The sums 1e-12 from NumPy fp64, the loss to fp32 round-off (it is rounded once: 6e-8, asserted at 2e-7), for [N], [B, N] and
    [B, N, 1] weights; autograd's gradient against the closed form g = G a_c mu d with G = 2 / (M C) (mse) or 1 / (loss M C) (rmse),
    at 1e-6 (fp32 products of fp64-formed factors)."""
    from bsms_gnn_amd import Objective, masked_loss
    from bsms_gnn_amd.objective import channel_sums
    gen = torch.Generator().manual_seed(5)
    B, N, Cc = 3, 70, 3
    pred, tar = torch.randn(B, N, Cc, generator=gen), torch.randn(B, N, Cc, generator=gen)
    mask = (torch.rand(B, N, 1, generator=gen) < 0.8).float()
    std = torch.tensor([0.5, 2.0, 1e-2])
    cw = [1.0, 0.5, 3.0]
    obj = Objective(space, kind, cw, node_weighted=True)
    for shape in ((N,), (B, N), (B, N, 1)):
        w = torch.exp(2.0 * torch.randn(*shape, generator=gen))
        full = np.broadcast_to(w.numpy().reshape((1, N) if len(shape) == 1 else (B, N)), (B, N))
        M, SE, a, loss = np_loss(pred.numpy(), tar.numpy(), mask.numpy()[..., 0], full, space, kind, cw, std.numpy())
        gM, gSE = channel_sums(pred, tar, mask, w)
        assert gM.dtype == torch.float64 and abs(float(gM) - M) <= 1e-12 * M and np.abs(gSE.numpy() - SE).max() <= 1e-12 * SE.max()
        p = pred.clone().requires_grad_(True)
        got = masked_loss(p, tar, mask, obj, std, node_weights=w)
        assert got.dtype == torch.float32 and abs(float(got.detach()) - loss) <= 2e-7 * loss, (shape, float(got.detach()), loss)
        got.backward()
        G = 2.0 / (M * Cc) if kind == "mse" else 1.0 / (loss * M * Cc)
        d = (pred - tar).numpy().astype(np.float64)
        want = G * a[None, None, :] * (mask.numpy().astype(np.float64) * full[..., None]) * d
        assert np.abs(p.grad.numpy() - want).max() <= 1e-6 * np.abs(want).max(), shape
        assert bool((p.grad[mask[..., 0] == 0] == 0).all())
    unit = masked_loss(pred, tar, mask, obj, std, node_weights=torch.ones(N))
    assert torch.equal(unit, masked_loss(pred, tar, mask, Objective(space, kind, cw), std))     # unit weights: the unweighted objective


# ------------------------------------------------------------------------------------------------ 12: the header contract
ENTRIES = {"bsms_error_sums_w": 14, "bsms_sim_objective_bwd_w": 25}


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
        assert "row_weights" in m.group(1)
    # the unweighted entries keep their signatures: the new arguments came as new entries
    assert len(_abi.SIGNATURES["bsms_error_sums"][1]) == 12 and len(_abi.SIGNATURES["bsms_sim_objective_bwd"][1]) == 23
    assert L.bsms_abi_version() == 4


def test_error_sums_w_refuses_like_error_sums(L):
    one = 0x1000                                             # a non-null address that must never be dereferenced
    f = L.bsms_error_sums_w
    assert f(None, None, None, None, 2, 10, 9, 10, 10, 10, 10, None, None, None) == E_UNSUPPORTED          # C = 9, before any pointer
    assert b"C=9" in L.bsms_last_error()
    assert f(None, None, None, None, 2, 10, 0, 10, 10, 10, 10, None, None, None) == E_UNSUPPORTED
    assert f(one, one, one, one, 2, -1, 3, 10, 10, 10, 10, one, one, None) == E_INVALID_ARG
    assert f(one, one, one, one, 2, 10, 3, 10, 10, 10, -1, one, one, None) == E_INVALID_ARG               # a negative weight stride
    assert b"stride" in L.bsms_last_error()
    assert f(one, one, one, None, 2, 10, 3, 10, 10, 10, 0, one, one, None) == E_INVALID_ARG               # null weights with work to do
    assert b"null" in L.bsms_last_error()
    assert f(None, None, None, None, 2, 0, 3, 0, 0, 0, 0, None, None, None) == E_INVALID_ARG               # seg_rows = 0 still writes zeros
    assert f(None, None, None, None, 0, 10, 3, 10, 10, 10, 10, None, None, None) == OK                     # S = 0: nothing to touch


def test_objective_bwd_w_refuses_in_the_stated_order(L):
    one = 0x1000

    def call(R=300, Cc=3, space=1, kind=1, ptr=one, weights=one, period=300, nxt=None, nin=None, in_stats=None, gnp=None):
        pick = lambda v: ptr if v is None else (None if v == "null" else v)
        wp = None if (weights == "null" or ptr is None) else weights
        return L.bsms_sim_objective_bwd_w(ptr, ptr, ptr, wp, period, R, Cc, ptr, ptr, ptr, pick(in_stats), pick(in_stats), pick(in_stats),
                                          ptr, None, space, kind, 1.0, nxt, nin, None, None, None, pick(gnp), None)

    assert call(Cc=0, ptr=None) == E_UNSUPPORTED and call(Cc=9, ptr=None) == E_UNSUPPORTED     # before any pointer is looked at
    assert b"C=9" in L.bsms_last_error()
    assert call(space=2, ptr=None) == E_UNSUPPORTED and call(kind=-1, ptr=None) == E_UNSUPPORTED
    assert b"kind=-1" in L.bsms_last_error()
    assert call(R=0, ptr=None) == E_UNSUPPORTED and call(Cc=9, space=2) == E_UNSUPPORTED and b"C=9" in L.bsms_last_error()
    assert call(Cc=9, period=7, weights="null") == E_UNSUPPORTED                               # the envelope before the weights
    assert call(ptr=None) == E_INVALID_ARG and call(weights="null") == E_INVALID_ARG
    assert b"null" in L.bsms_last_error()
    for period in (0, -300, 7, 299, 301, 600):
        assert call(period=period) == E_INVALID_ARG, period
        assert b"weight_period" in L.bsms_last_error()
    assert call(period=7, weights="null") == E_INVALID_ARG and b"null" in L.bsms_last_error()   # null pointers before the period
    assert call(gnp="null") == E_INVALID_ARG
    assert call(nxt=one) == E_INVALID_ARG and b"together" in L.bsms_last_error()                # then half a carried pair
    assert call(period=7, nxt=one) == E_INVALID_ARG and b"weight_period" in L.bsms_last_error()
    assert call(nxt=one, nin=one, in_stats="null") == E_INVALID_ARG
