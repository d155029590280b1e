"""CPU: the host side of the objective with an edge-difference term, J = L + lambda T -- `Objective(edge_weight=,
edge_weighting=)`, `masked_loss(.., g=, pos=)` in fp64 against a plain NumPy loop over the graphs of tests/test_edge_diff_host.py,
and the C ABI of bsms_edge_diff_fold / bsms_sim_edge_objective_bwd (declared, exported, bound, the order of the argument checks;
nothing is launched).  tests/test_hip_edge_objective.py runs the kernels."""
import ctypes as C
import math
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from conftest import ROOT
from test_edge_diff_host import NEW as EDGE_DIFF_ENTRIES
from test_edge_diff_host import OLDER as BEFORE_EDGE_DIFF
from test_edge_diff_host import np_edge_sums, small_case

PAIRS = [("physical", "rmse"), ("physical", "mse"), ("normalized", "rmse"), ("normalized", "mse")]
WEIGHTINGS = ["difference", "quotient"]


@pytest.fixture(scope="module")
def eng():
    import __graft_entry__
    __graft_entry__.build()
    import bsms_gnn_amd as eng
    return eng


# ------------------------------------------------------------------------------------------------ the value
def test_edge_weight_and_weighting_are_validated(eng):
    O = eng.Objective
    assert not O().has_edge_term and O().edge_weight is None and O().edge_weighting == "difference"
    assert O(edge_weight=None, edge_weighting="quotient").has_edge_term is False
    o = O("normalized", "mse", [1.0, 2.0], edge_weight=0.5, edge_weighting="quotient")
    assert o.has_edge_term and o.edge_weight == 0.5 and o.edge_weighting == "quotient" and isinstance(O(edge_weight=2).edge_weight, float)
    for bad in (0, 0.0, -1.0, float("inf"), float("nan"), "0.1", True, [0.1]):
        with pytest.raises(ValueError):
            O(edge_weight=bad)
    for bad in ("gradient", None, 1):
        with pytest.raises(ValueError):
            O(edge_weight=0.1, edge_weighting=bad)
    with pytest.raises(ValueError):
        O(edge_weighting="gradient")                                   # checked with or without a weight
    with pytest.raises(AttributeError):
        o.edge_weight = 1.0


def test_the_three_refusals(eng):
    O = eng.Objective
    with pytest.raises(ValueError, match="robust"):
        O(kind="mae", edge_weight=0.1)
    with pytest.raises(ValueError, match="robust"):
        O("normalized", "huber", delta=1.0, edge_weight=0.1)
    with pytest.raises(ValueError, match="node_weighted"):
        O("physical", "mse", None, True, edge_weight=0.1)
    O(kind="mae", edge_weighting="quotient")                           # the weighting alone refuses nothing
    O("physical", "mse", None, True)


def test_from_cfg_eq_hash_repr_and_is_default(eng):
    O = eng.Objective
    cfg = SimpleNamespace(loss_space="normalized", loss_kind="mse", loss_edge_weight=0.25, loss_edge_weighting="quotient")
    o = O.from_cfg(cfg)
    assert o == O("normalized", "mse", edge_weight=0.25, edge_weighting="quotient") and hash(o) == hash(O("normalized", "mse", edge_weight=0.25, edge_weighting="quotient"))
    assert o != O("normalized", "mse") and o != O("normalized", "mse", edge_weight=0.25) and o != O("normalized", "mse", edge_weight=0.5, edge_weighting="quotient")
    assert O.from_cfg(SimpleNamespace(loss_edge_weight=0.1)) == O(edge_weight=0.1)
    assert O.from_cfg(SimpleNamespace()) == O() and O.from_cfg(SimpleNamespace(loss_edge_weight=None, loss_edge_weighting=None)) == O()
    assert "edge_weight=0.25" in repr(o) and "edge_weighting='quotient'" in repr(o) and "edge" not in repr(O())
    assert O().is_default and not O(edge_weight=0.1).is_default          # physical / rmse / no weights, but never the default route
    assert len({O(), O(edge_weight=0.1), O(edge_weight=0.1, edge_weighting="quotient"), O(edge_weighting="quotient")}) == 4


# ------------------------------------------------------------------------------------------------ masked_loss against a NumPy loop
def np_objective(pred, tar, mask, g, pos, space, kind, weights, std, lam, weighting):
    """J = L + lam T in plain NumPy fp64 (no fp32 rounding of d: the inputs are fp64)."""
    S, N, Cn = pred.shape
    d = pred - tar
    m = mask.reshape(1, N, 1)
    a = np.ones(Cn) if weights is None else np.asarray(weights, np.float64)
    if space == "normalized":
        a = a / std ** 2
    M, SE = S * mask.sum(), (m * d * d).reshape(-1, Cn).sum(0)
    es = np_edge_sums(pred, tar, mask, g, pos, weighting, exact_d=True)
    ME, DE = es[:, 0].sum(), es[:, 1:1 + Cn].sum(0)
    Q, H = (a * SE).sum() / (M * Cn), (a * DE).sum() / (ME * Cn)
    rt = math.sqrt if kind == "rmse" else (lambda x: x)
    return rt(Q) + lam * rt(H), rt(Q), rt(H)


@pytest.mark.parametrize("weighting", WEIGHTINGS)
@pytest.mark.parametrize("space,kind", PAIRS)
def test_masked_loss_against_a_numpy_loop(eng, space, kind, weighting):
    """The graph of `small_case`: a self-loop, a duplicated edge, one-directional edges, a degree-0 node, coincident nodes joined by
    an edge, a zero of the mask on one end of four edges."""
    pred, tar, mask, g, pos = small_case(7, 21)
    pred, tar = pred.astype(np.float64), tar.astype(np.float64)
    std = np.array([0.1, 3.0, 1.5])
    for weights in (None, [0.5, 2.0, 1.0]):
        obj = eng.Objective(space, kind, weights, edge_weight=0.3, edge_weighting=weighting)
        got = eng.masked_loss(torch.tensor(pred), torch.tensor(tar), torch.tensor(mask).reshape(1, 7, 1).expand(2, 7, 1), obj,
                              torch.tensor(std), g=torch.tensor(g), pos=torch.tensor(pos))
        want, L, T = np_objective(pred, tar, mask.astype(np.float64), g, pos, space, kind, weights, std, 0.3, weighting)
        assert got.dtype == torch.float32 and got.dim() == 0 and T > 0 and L > 0
        assert float(got) == float(np.float32(want)) or abs(float(got) - want) <= 2.0 ** -23 * want      # rounded once
        # ... and the fp64 value behind the rounding, at 1e-12: L and T apart through the library's own pieces
        sums = eng.edge_difference_sums(torch.tensor(pred), torch.tensor(tar), torch.tensor(mask), torch.tensor(g), torch.tensor(pos), weighting)
        from bsms_gnn_amd.objective import edge_term
        assert abs(float(edge_term(sums, obj, torch.tensor(std))) - T) <= 1e-12 * T
        plain = eng.Objective(space, kind, weights)
        M, SE = eng.objective.channel_sums(torch.tensor(pred), torch.tensor(tar), torch.tensor(mask).reshape(1, 7, 1).expand(2, 7, 1))
        Q = (plain.coefficients(torch.tensor(std), 3, "cpu") * SE / (M * 3)).sum()
        L64 = float(torch.sqrt(Q) if kind == "rmse" else Q)
        assert abs(L64 - L) <= 1e-12 * L and abs((L64 + 0.3 * float(edge_term(sums, obj, torch.tensor(std)))) - want) <= 1e-12 * want


def test_masked_loss_needs_the_graph_and_the_positions(eng):
    pred, tar, mask, g, pos = (torch.tensor(v) for v in small_case(7, 2))
    mask = mask.reshape(1, 7, 1).expand(2, 7, 1)
    with pytest.raises(ValueError, match="needs g"):
        eng.masked_loss(pred, tar, mask, eng.Objective(kind="mse", edge_weight=0.1))
    with pytest.raises(ValueError, match="needs pos"):
        eng.masked_loss(pred, tar, mask, eng.Objective(kind="mse", edge_weight=0.1, edge_weighting="quotient"), g=g)
    eng.masked_loss(pred, tar, mask, eng.Objective(kind="mse", edge_weight=0.1), g=g)                       # "difference" reads no positions
    flat = eng.masked_loss(pred[0], tar[0], mask[0], eng.Objective(kind="mse", edge_weight=0.1), g=g)               # [R, C]: one segment
    assert torch.equal(flat, eng.masked_loss(pred[:1], tar[:1], mask[:1], eng.Objective(kind="mse", edge_weight=0.1), g=g))


@pytest.mark.parametrize("weighting", WEIGHTINGS)
@pytest.mark.parametrize("kind", ["mse", "rmse"])
def test_gradcheck(eng, kind, weighting):
    pred, tar, mask, g, pos = small_case(7, 9)
    obj = eng.Objective("normalized", kind, [0.5, 2.0, 1.0], edge_weight=0.7, edge_weighting=weighting)
    std = torch.tensor([0.4, 3.0, 1.5], dtype=torch.float64)
    p = torch.tensor(pred, dtype=torch.float64, requires_grad=True)
    t, gt, x = torch.tensor(tar, dtype=torch.float64), torch.tensor(g), torch.tensor(pos, dtype=torch.float64)
    m = torch.tensor(mask, dtype=torch.float64).reshape(1, 7, 1).expand(2, 7, 1)

    def J(p_):                                                         # the fp64 value in front of masked_loss's one rounding
        from bsms_gnn_amd.objective import channel_sums, edge_difference_sums, edge_term
        M, SE = channel_sums(p_, t, m)
        Q = (obj.coefficients(std, 3, "cpu") * SE / (M * 3)).sum()
        return (torch.sqrt(Q) if kind == "rmse" else Q) + obj.edge_weight * edge_term(edge_difference_sums(p_, t, m, gt, x, weighting), obj, std)

    assert torch.autograd.gradcheck(J, [p])
    got = eng.masked_loss(p, t, m, obj, std, g=gt, pos=x)
    assert float(got.detach()) == float(J(p).detach().float())
    got.backward()
    assert p.grad is not None and bool(torch.isfinite(p.grad).all()) and float(p.grad.abs().max()) > 0


def parent_masked_loss(eng, pred, tar, mask, objective=None, std=None, node_weights=None):
    """`masked_loss` as the parent commit had it, restated op for op from its pieces."""
    from bsms_gnn_amd.objective import channel_sums, finish_loss, robust_sums
    if objective is not None:
        node_weights = objective.check_node_weights(node_weights)
    if objective is None or objective.is_default:
        return eng.masked_rmse(pred, tar, mask)
    objective.bind(pred.shape[-1])
    if objective.is_robust:
        M, SE = robust_sums(pred, tar, mask, objective, std, node_weights)
    else:
        M, SE = channel_sums(pred, tar, mask, node_weights)
    return finish_loss(M, SE, objective, std)[0]


def test_without_an_edge_term_the_function_is_the_parents(eng):
    pred, tar, mask, g, pos = (torch.tensor(v) for v in small_case(7, 4))
    mask = mask.reshape(1, 7, 1).expand(2, 7, 1)
    std = torch.tensor([0.1, 3.0, 1.5], dtype=torch.float64)
    nw = torch.rand(7, generator=torch.Generator().manual_seed(0))
    O = eng.Objective
    for obj, kw in ((None, {}), (O(), {}), (O("normalized", "mse", [1.0, 2.0, 0.5]), {}), (O("physical", "rmse", [1.0, 2.0, 0.5]), {}),
                    (O(kind="mae"), {}), (O("normalized", "huber", delta=0.5), {}), (O("normalized", "mse", None, True), dict(node_weights=nw))):
        want = parent_masked_loss(eng, pred, tar, mask, obj, std, **kw)
        assert torch.equal(eng.masked_loss(pred, tar, mask, obj, std, **kw), want)
        assert torch.equal(eng.masked_loss(pred, tar, mask, obj, std, g=g, pos=pos, **kw), want)            # given but not needed: not read


# ------------------------------------------------------------------------------------------------ the C ABI
# The two entries live in the companion library (include/bsms_hip_ext.h, libbsms_hip_ext.so, _abi.EXT_SIGNATURES): the surface of
# libbsms_hip.so stays the parent's, entry for entry.
NEW = {"bsms_edge_diff_fold": 5, "bsms_sim_edge_objective_bwd": 31}
OLDER = {**BEFORE_EDGE_DIFF, **{k[len("bsms_"):]: v for k, v in EDGE_DIFF_ENTRIES.items()}}       # the parent's header: 99 entries


def declared(text, name):
    decl = re.search(r"\b" + name + r"\s*\(([^;]*)\)\s*;", text)
    return None if decl is None else len([a for a in decl.group(1).split(",") if a.strip() not in ("", "void")])


def test_new_entries_are_declared_exported_and_bound(eng):
    import subprocess
    from bsms_gnn_amd import _abi
    strip = lambda path: re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", path)).read(), flags=re.S)
    text, ext_text = strip("bsms_hip.h"), strip("bsms_hip_ext.h")
    raw = C.CDLL(_abi.EXT_LIB_PATH)
    for name, nargs in NEW.items():
        assert declared(ext_text, name) == nargs and declared(text, name) is None, name
        assert hasattr(raw, name) and len(_abi.EXT_SIGNATURES[name][1]) == nargs, name
    # the companion library exports exactly what its header declares, and the binding lists exactly that
    names = set(re.findall(r"\b(bsms_[a-z0-9_]+)\s*\(", ext_text))
    out = subprocess.run(["nm", "-D", "--defined-only", _abi.EXT_LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if ln.split() and ln.split()[-1].startswith("bsms_") and ln.split()[-2] in ("T", "t", "W")}
    assert names == set(NEW) == set(_abi.EXT_SIGNATURES) == exported
    # libbsms_hip.so is the parent's: version, the set of entries, every argument count, in the binding and in the header
    assert _abi.lib().bsms_abi_version() == 4
    assert len(OLDER) == 99 and set(_abi.SIGNATURES) == {"bsms_" + k for k in OLDER}
    for name, nargs in OLDER.items():
        assert len(_abi.SIGNATURES["bsms_" + name][1]) == nargs, name
        assert declared(text, "bsms_" + name) == nargs, name
    assert _abi.EXT_SIGNATURES["bsms_sim_edge_objective_bwd"][1][21:23] == [C.c_double, C.c_float]         # edge_lambda, w
    for doc in ("INTEGRATION.md", "README.md", "DESIGN.md"):
        body = open(os.path.join(ROOT, doc)).read()
        assert "bsms_edge_diff_fold" in body and "bsms_sim_edge_objective_bwd" in body and "bsms_hip_ext" in body, doc


def test_refusal_order_without_gpu(eng):
    L, X = eng._abi.lib(), eng._abi.ext()
    one = C.c_double(0.0)
    ptr = C.addressof(one)                                             # a non-null pointer that is never dereferenced: every call below fails first

    def fold(S=3, Cn=3, sums=ptr, out=ptr):
        return X.bsms_edge_diff_fold(sums, S, Cn, out, None)

    assert fold(Cn=0) == -3 and fold(Cn=9) == -3 and fold(Cn=9, S=-1, sums=None, out=None) == -3          # C before anything else
    assert b"C in 1..8" in L.bsms_last_error()
    assert fold(S=-1) == -1 and fold(out=None) == -1 and fold(sums=None) == -1 and fold(S=0, sums=None, out=None) == -1

    def bwd(plan=None, seg_rows=10, S=2, Cn=3, p=2, weighting=0, space=0, kind=0, lam=0.5, ptrs=ptr, pos=ptr, g_next=None, g_nin=None):
        return X.bsms_sim_edge_objective_bwd(plan, seg_rows, S, ptrs, ptrs, ptrs, pos, Cn, p, weighting, ptrs, ptrs, ptrs, None, None, None,
                                             ptrs, ptrs, None, space, kind, lam, 1.0, g_next, g_nin, None, None, None, None, ptrs, None)

    # 1: what is unsupported, before any pointer (and any other argument) is looked at
    for kw in (dict(Cn=0), dict(Cn=9), dict(weighting=2), dict(weighting=-1), dict(weighting=1, p=0), dict(weighting=1, p=4), dict(space=2),
               dict(kind=2), dict(kind=-1)):
        assert bwd(S=0, seg_rows=0, lam=float("nan"), ptrs=None, **kw) == -3, kw
    assert bwd(Cn=9) == -3 and b"C in 1..8" in L.bsms_last_error()
    assert bwd(weighting=0, p=99) == -1                                # "difference" ignores p: the next failing check is the null plan
    # 2: the arguments
    for kw in (dict(S=0), dict(S=-1), dict(seg_rows=0), dict(seg_rows=-5), dict(S=1 << 20, seg_rows=1 << 20), dict(lam=-0.1), dict(lam=float("inf")),
               dict(lam=float("nan")), dict(), dict(ptrs=None), dict(weighting=1, pos=None), dict(g_next=ptr), dict(g_nin=ptr)):
        assert bwd(**kw) == -1, kw
    assert bwd() == -1 and b"plan is null" in L.bsms_last_error()
    assert bwd(lam=-0.1) == -1 and b"edge_lambda" in L.bsms_last_error()                                   # before the null plan
    assert bwd(lam=0.0) == -1 and b"plan is null" in L.bsms_last_error()                                   # 0 is allowed at this level


def test_step_and_engine_refuse_accumulation_before_any_launch(eng, monkeypatch):
    from bsms_gnn_amd import _abi
    real = _abi.lib()
    touched = []

    class Watch:
        def __getattr__(self, name):
            touched.append(name)
            return getattr(real, name)

    monkeypatch.setattr(_abi, "lib", lambda: Watch())
    monkeypatch.setattr(_abi, "ext", lambda: Watch())
    from oracle import bsms_oracle as ro
    sim = eng.BSMS_Simulator(ro.make_cfg(2, 32, 3, 3, 2))
    obj = eng.Objective("normalized", "mse", edge_weight=0.1)
    grads = eng.GradBuckets(list(sim.parameters()))
    with pytest.raises(ValueError, match="edge term"):
        eng.FusedStep(sim, grads, objective=obj, accumulate=2)
    with pytest.raises(ValueError, match="edge term"):
        eng.FusedStep(sim, grads, objective=obj, accumulate=2, reduction="mean")
    with pytest.raises(ValueError, match="accumulate"):                 # (on the GPU the fused step refuses; without it accumulate > 1 is refused as ever)
        eng.DataParallel(sim, objective=obj, accumulate=2)
    step = eng.FusedStep(sim, grads, objective=obj)                     # accumulate = 1 is fine, and nothing has run
    assert step._edge and step.objective.has_edge_term
    with pytest.raises(RuntimeError):
        step.loss_parts()
    with pytest.raises(ValueError, match="no edge term"):
        eng.FusedStep(sim, grads, objective=eng.Objective("normalized", "mse")).loss_parts()
    assert eng.DataParallel(sim, objective=obj).objective == obj
    cfg = ro.make_cfg(2, 32, 3, 3, 2)
    cfg.loss_kind, cfg.loss_edge_weight, cfg.loss_edge_weighting = "mse", 0.2, "quotient"
    assert eng.DataParallel(eng.BSMS_Simulator(cfg)).objective == eng.Objective(kind="mse", edge_weight=0.2, edge_weighting="quotient")
    assert not touched


# ------------------------------------------------------------------------------------------------ the route without the fused step
def _dp_case():
    pred, tar, mask, g, pos = (torch.tensor(v) for v in small_case(7, 13))
    std = torch.tensor([0.1, 3.0, 1.5], dtype=torch.float64)
    return pred, tar, mask.reshape(1, 7, 1).expand(2, 7, 1).contiguous(), g, pos, std


DP_OBJECTIVES = [dict(space="normalized", kind="mse", channel_weights=[0.5, 2.0, 1.0], edge_weight=0.3, edge_weighting="quotient"),
                 dict(space="physical", kind="rmse", channel_weights=None, edge_weight=0.7, edge_weighting="difference")]


def _objective(eng, kw):
    kw = dict(kw)
    return eng.Objective(kw.pop("space"), kw.pop("kind"), kw.pop("channel_weights"), **kw)


@pytest.mark.parametrize("kw", DP_OBJECTIVES)
def test_global_masked_loss_without_a_process_group_is_masked_loss(eng, kw):
    from bsms_gnn_amd.dp import global_masked_loss
    pred, tar, mask, g, pos, std = _dp_case()
    obj = _objective(eng, kw)
    p0, p1 = pred.clone().requires_grad_(True), pred.clone().requires_grad_(True)
    want = eng.masked_loss(p0, tar, mask, obj, std, g=g, pos=pos)
    got = global_masked_loss(p1, tar, mask, obj, std, g=g, pos=pos)
    assert torch.equal(got.detach(), want.detach())
    want.backward()
    got.backward()
    assert torch.equal(p1.grad, p0.grad) and float(p0.grad.abs().max()) > 0
    with pytest.raises(ValueError, match="needs g"):
        global_masked_loss(pred, tar, mask, obj, std)


def _gloo_worker(rank, world, port, out_path):
    import os as _os
    import sys as _sys
    import torch.distributed as dist
    _sys.path.insert(0, ROOT)
    _sys.path.insert(0, _os.path.join(ROOT, "tests"))
    _os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    torch.set_num_threads(1)
    import bsms_gnn_amd as eng                                          # imports without touching the GPU
    from bsms_gnn_amd.dp import global_masked_loss
    pred, tar, mask, g, pos, std = _dp_case()
    out = {}
    for k, kw in enumerate(DP_OBJECTIVES):
        sl = slice(rank, rank + 1)                                      # one sample per rank
        mine = pred[sl].clone().requires_grad_(True)
        loss = global_masked_loss(mine, tar[sl], mask[sl], _objective(eng, kw), std, g=g, pos=pos)
        loss.backward()
        out[k] = (loss.detach(), mine.grad.clone())
    torch.save(out, f"{out_path}.{rank}")
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.timeout(120)
def test_global_masked_loss_on_two_gloo_ranks_is_the_batch_loss(eng, tmp_path):
    """One sample per rank: M, SE, ME and DE travel in one all-reduced message, the value is the B = 2 loss on both ranks, and each
    rank's gradient is its sample's slice of the B = 2 gradient (the sums are all-reduced, the gradient flows through the local part)."""
    import torch.multiprocessing as mp
    port = 29500 + (os.getpid() + 11) % 2000
    out = str(tmp_path / "res")
    mp.start_processes(_gloo_worker, args=(2, port, out), nprocs=2, join=True, start_method="spawn")
    res = [torch.load(f"{out}.{r}") for r in range(2)]
    pred, tar, mask, g, pos, std = _dp_case()
    for k, kw in enumerate(DP_OBJECTIVES):
        whole = pred.clone().requires_grad_(True)
        want = eng.masked_loss(whole, tar, mask, _objective(eng, kw), std, g=g, pos=pos)
        want.backward()
        assert torch.equal(res[0][k][0], res[1][k][0])                  # the same value on both ranks
        assert abs(float(res[0][k][0]) - float(want.detach())) <= 2.0 ** -22 * float(want.detach())
        for r in range(2):
            got, ref = res[r][k][1].double(), whole.grad[r:r + 1].double()
            assert float((got - ref).abs().max()) <= 1e-6 * float(ref.abs().max()) and float(ref.abs().max()) > 0


def test_engine_without_the_fused_step_hands_the_graph_and_the_positions_over(eng, graphs):
    """DataParallel on a CPU replica (the oracle model: no fused step): step_loss_backward takes the level-0 edge list and the position
    columns of node_in itself, and its loss and gradients are those of masked_loss(model(data), .., g=, pos=).backward()."""
    from conftest import load_golden
    from oracle import bsms_oracle as ro
    from test_hip_unroll import sim_batch
    data = sim_batch(graphs, 3)
    obj = _objective(eng, dict(DP_OBJECTIVES[0], channel_weights=[1.0, 3.0]))
    models = []
    for _ in range(2):
        m = ro.BSMS_Simulator(ro.make_cfg(2, 32, 3, 3, 2))
        m.load_state_dict(load_golden("sim").state_dict())
        models.append(m)
    engine = eng.DataParallel(models[0], objective=obj)
    assert engine.fused is None
    loss = engine.step_loss_backward(data, True)
    pred = models[1](data, True, False)
    want = eng.masked_loss(pred, data[1], data[2], obj, models[1]._targetNormalizer.std_with_epsilon(), g=data[3][0][0], pos=data[0][..., 2:-1])
    want.backward()
    assert torch.equal(loss.detach(), want.detach())
    plain = eng.masked_loss(pred.detach(), data[1], data[2], eng.Objective("normalized", "mse", [1.0, 3.0]), models[1]._targetNormalizer.std_with_epsilon())
    assert float(want.detach()) > float(plain)
    for (k, a), (_, b) in zip(models[0].named_parameters(), models[1].named_parameters()):
        if b.grad is not None:
            assert float((a.grad - b.grad).abs().max()) <= 1e-5 * float(b.grad.abs().max()), k      # the same graph twice: the CPU's threaded sums differ in order
