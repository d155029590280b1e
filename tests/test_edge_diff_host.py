"""CPU: the host side of the edge-difference (discrete H1) sums -- the definition in torch
(`objective.edge_difference_sums` / `edge_difference_loss`) against an independent plain NumPy loop over the edges, its closed-form
gradient, and the C ABI of bsms_edge_diff_sums / bsms_edge_diff_bwd (declared, exported, bound, argument validation; nothing is
launched).  tests/test_hip_edge_diff.py compares the kernels with the same restatements (`np_edge_sums`, `np_edge_grad`)."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT

EPS = 2.0 ** -53


def sums_tol(n_edges):
    """Relative bound on a field of the sums: n non-negative fp64 terms added in any order, plus the few roundings inside a term."""
    return (n_edges + 16) * EPS


@pytest.fixture(scope="module")
def eng():
    import __graft_entry__
    __graft_entry__.build()
    import bsms_gnn_amd as eng
    return eng


def np_edge_sums(pred, tar, mask, g, pos=None, weighting="difference", exact_d=False):
    """[S, 1+2C] fp64 by a plain loop over the edges.  pred / tar [S, N, C] float32 (d rounded to fp32 once) or, with `exact_d`,
    float64 (no rounding); mask [N] or [S, N]; pos [N, p] or [S, N, p]."""
    S, N, Cn = pred.shape
    out = np.zeros((S, 1 + 2 * Cn), np.float64)
    for s in range(S):
        d = (pred[s] - tar[s]).astype(np.float64) if exact_d else (pred[s].astype(np.float32) - tar[s].astype(np.float32)).astype(np.float64)
        t = tar[s].astype(np.float64)
        m = (mask if mask.ndim == 1 else mask[s]).astype(np.float64)
        x = None if pos is None else (pos if pos.ndim == 2 else pos[s]).astype(np.float64)
        for e in range(g.shape[1]):
            i, j = int(g[0, e]), int(g[1, e])
            mu, w = m[i] * m[j], 1.0
            if weighting == "quotient":
                l2 = float(((x[i] - x[j]) ** 2).sum())
                if l2 == 0.0:
                    continue
                w = 1.0 / l2
            out[s, 0] += mu
            out[s, 1:1 + Cn] += mu * w * (d[i] - d[j]) ** 2
            out[s, 1 + Cn:] += mu * w * (t[i] - t[j]) ** 2
    return out


def np_edge_grad(pred, tar, mask, g, coef, pos=None, weighting="difference"):
    """(grad [S, N, C] fp64, A [S, N, C]: the sum of the absolute values of every element's terms, times |2 k_c|) -- the closed form
    of the gradient of sum_c k_c DE[c] with respect to pred: incoming and outgoing edges of every row."""
    S, N, Cn = pred.shape
    grad, A = np.zeros((S, N, Cn), np.float64), np.zeros((S, N, Cn), np.float64)
    for s in range(S):
        d = (pred[s].astype(np.float32) - tar[s].astype(np.float32)).astype(np.float64)
        m = (mask if mask.ndim == 1 else mask[s]).astype(np.float64)
        x = None if pos is None else (pos if pos.ndim == 2 else pos[s]).astype(np.float64)
        k = coef if coef.ndim == 1 else coef[s]
        for e in range(g.shape[1]):
            i, j = int(g[0, e]), int(g[1, e])
            mw = m[i] * m[j]
            if weighting == "quotient":
                l2 = float(((x[i] - x[j]) ** 2).sum())
                if l2 == 0.0:
                    continue
                mw = mw / l2
            term = mw * (d[j] - d[i])
            grad[s, j] += term                  # row j: e is one of its incoming edges
            grad[s, i] -= term                  # row i: e is one of its outgoing edges
            A[s, j] += np.abs(term)
            A[s, i] += np.abs(term)
        grad[s] *= 2.0 * k
        A[s] *= np.abs(2.0 * k)
    return grad, A


def small_case(N, seed, Cn=3, p=2, S=2):
    """A graph of N nodes holding a self-loop, a duplicated edge, a one-directional edge, a degree-0 node (the last, N >= 3) and
    two coincident nodes joined by an edge (N >= 2); a mask with a zero on one end of an edge (N >= 3)."""
    rng = np.random.default_rng(seed)
    edges = [(0, 0)]                                                    # self-loop
    if N >= 2:
        edges += [(0, 1), (1, 0), (0, 1)]                               # both directions, one of them twice
    if N >= 7:
        edges += [(1, 2), (2, 1), (2, 3), (3, 2), (3, 4), (4, 5), (5, 4), (5, 1), (1, 5), (4, 0)]     # 3 -> 4 and 4 -> 0: one direction only
    g = np.array(edges, np.int64).T
    pred = rng.standard_normal((S, N, Cn)).astype(np.float32)
    tar = (2 * rng.standard_normal((S, N, Cn))).astype(np.float32)
    pos = rng.random((N, p)).astype(np.float32)
    if N >= 7:
        pos[5] = pos[4]                                                 # coincident nodes joined by 4 <-> 5
    mask = np.ones(N, np.float32)
    if N >= 7:
        mask[2] = 0.0
    return pred, tar, mask, g, pos


def relerr(got, want):
    return float(np.max(np.abs(got - want) / np.maximum(np.abs(want), 1e-300)))


@pytest.mark.parametrize("weighting", ["difference", "quotient"])
@pytest.mark.parametrize("N", [1, 2, 7])
def test_definition_against_numpy_loop(eng, N, weighting):
    pred, tar, mask, g, pos = small_case(N, N)
    got = eng.edge_difference_sums(torch.tensor(pred), torch.tensor(tar), torch.tensor(mask), torch.tensor(g), torch.tensor(pos), weighting)
    want = np_edge_sums(pred, tar, mask, g, pos, weighting)
    assert got.dtype == torch.float64 and tuple(got.shape) == (2, 7)
    nz = want != 0
    assert np.array_equal(got.numpy() == 0, ~nz)
    assert relerr(got.numpy()[nz], want[nz]) <= sums_tol(g.shape[1]) if nz.any() else True
    # the self-loop counts under "difference" (mu = m^2, a zero difference) and has no length under "quotient"; so do the coincident nodes
    if N == 1:
        assert want[0, 0] == (1.0 if weighting == "difference" else 0.0) and not want[:, 1:].any()
    if N == 7:
        both = np_edge_sums(pred, tar, mask, g, pos, "difference")[0, 0], np_edge_sums(pred, tar, mask, g, pos, "quotient")[0, 0]
        assert both[0] - both[1] == 3.0                                 # the self-loop and 4 <-> 5
        full = np_edge_sums(pred, tar, np.ones(7, np.float32), g, pos, "difference")[0, 0]
        assert full - both[0] == 4.0                                    # the four edges with node 2 on one end
    # per-sample masks and positions give the same rows as shared ones
    rep = eng.edge_difference_sums(torch.tensor(pred), torch.tensor(tar), torch.tensor(mask).expand(2, N), torch.tensor(g),
                                   torch.tensor(pos).expand(2, N, 2), weighting)
    assert torch.equal(rep, got)
    flat = eng.edge_difference_sums(torch.tensor(pred[1]), torch.tensor(tar[1]), torch.tensor(mask).reshape(N, 1), torch.tensor(g),
                                    torch.tensor(pos), weighting)
    assert torch.equal(flat, got[1:])


def test_constant_error_field_has_no_edge_difference(eng):
    pred, tar, mask, g, pos = small_case(7, 3)
    tar = (np.round(tar * 4) / 4).astype(np.float32)                    # multiples of 1/4: the shift survives the fp32 subtraction exactly
    pred = tar + np.float32(0.75)
    for weighting in ("difference", "quotient"):
        sums = eng.edge_difference_sums(torch.tensor(pred), torch.tensor(tar), torch.tensor(mask), torch.tensor(g), torch.tensor(pos), weighting)
        assert bool((sums[:, 1:4] == 0).all()) and bool((sums[:, 0] > 0).all()) and bool((sums[:, 4:] > 0).all())


def test_linear_error_on_a_line_mesh_gives_the_squared_slope(eng):
    """d = a x on a line mesh (p = 1): every quotient (d_i - d_j)^2 / (x_i - x_j)^2 is a_c^2, so DE_c / ME = a_c^2."""
    N = 40
    x = np.cumsum(np.random.default_rng(0).integers(1, 5, N)).astype(np.float32) / 8        # exact in fp32, as are the products below
    a = np.array([0.5, -2.0, 3.0], np.float32)
    tar = np.zeros((1, N, 3), np.float32)
    pred = (x[:, None] * a[None, :])[None].astype(np.float32)
    g = np.stack([np.r_[np.arange(N - 1), np.arange(1, N)], np.r_[np.arange(1, N), np.arange(N - 1)]])
    sums = eng.edge_difference_sums(torch.tensor(pred), torch.tensor(tar), torch.ones(N), torch.tensor(g), torch.tensor(x[:, None]), "quotient")
    assert float(sums[0, 0]) == 2 * (N - 1)
    assert relerr((sums[0, 1:4] / sums[0, 0]).numpy(), a.astype(np.float64) ** 2) <= sums_tol(g.shape[1])


def f64_sums(pred, tar, mask, g, pos, weighting):
    """The definition restated for fp64 inputs, without the fp32 rounding of d (gradcheck, the adjoint checks)."""
    i, j = g[0], g[1]
    d = pred - tar
    mu = mask[i] * mask[j]
    if weighting == "quotient":
        l2 = ((pos[i] - pos[j]) ** 2).sum(-1)
        ok = l2 != 0
        mu = torch.where(ok, mu / torch.where(ok, l2, torch.ones_like(l2)), torch.zeros_like(l2))
    return (mu.unsqueeze(-1) * (d[i] - d[j]) ** 2).sum(0)


@pytest.mark.parametrize("weighting", ["difference", "quotient"])
def test_gradcheck_of_the_fp64_definition(eng, weighting):
    pred, tar, mask, g, pos = small_case(7, 5, S=1)
    pos[5] += 0.01                                                      # no edge of length 0: the quotient is smooth in pos
    args = [torch.tensor(v[0] if v.ndim == 3 else v, dtype=torch.float64, requires_grad=True) for v in (pred, tar, pos)]
    m, gt = torch.tensor(mask, dtype=torch.float64), torch.tensor(g)
    assert torch.autograd.gradcheck(lambda p_, t_, x_: f64_sums(p_, t_, m, gt, x_, weighting), args)
    # and the library's definition is that function on fp64 tensors
    lib = eng.edge_difference_sums(args[0], args[1], m, gt, args[2], weighting)
    assert torch.allclose(lib[0, 1:4], f64_sums(args[0], args[1], m, gt, args[2], weighting), rtol=1e-14, atol=0)


@pytest.mark.parametrize("weighting", ["difference", "quotient"])
def test_closed_form_gradient_against_autograd(eng, weighting):
    pred, tar, mask, g, pos = small_case(7, 6)
    mask = mask * np.float32(0.5) + np.float32(0.25) * (np.arange(7) % 2).astype(np.float32)          # soft masks too
    k = np.array([[0.3, 0.0, -1.5], [2.0, 1.0, 0.25]])
    p = torch.tensor(pred, requires_grad=True)
    sums = eng.edge_difference_sums(p, torch.tensor(tar), torch.tensor(mask), torch.tensor(g), torch.tensor(pos), weighting)
    (sums[:, 1:4] * torch.tensor(k)).sum().backward()
    want, A = np_edge_grad(pred, tar, mask, g, k, pos, weighting)
    assert np.all(np.abs(p.grad.numpy() - want) <= 2.0 ** -23 * np.abs(want) + 2.0 ** -40 * A)
    assert not want[:, :, 1][0].any() and not p.grad[0, :, 1].any()     # a zero coefficient: a zero column
    assert not want[:, 6].any()                                        # the degree-0 node


def test_loss_kinds_spaces_and_shapes(eng):
    pred, tar, mask, g, pos = small_case(7, 7)
    tp, tt, tm, tg, tx = torch.tensor(pred), torch.tensor(tar), torch.tensor(mask), torch.tensor(g), torch.tensor(pos)
    sums = eng.edge_difference_sums(tp, tt, tm, tg, tx, "quotient")
    w, std = [0.5, 2.0, 1.0], torch.tensor([0.1, 3.0, 1.5], dtype=torch.float64)
    mse = eng.edge_difference_loss(tp, tt, tm, tg, tx, weighting="quotient")
    rmse = eng.edge_difference_loss(tp, tt, tm, tg, tx, weighting="quotient", kind="rmse")
    assert mse.dtype == torch.float32 and mse.dim() == 0
    H = float(sums[:, 1:4].sum() / (sums[:, 0].sum() * 3))
    assert abs(float(mse) - H) <= 2.0 ** -23 * H and abs(float(rmse) - H ** 0.5) <= 2.0 ** -23 * H ** 0.5
    norm = eng.edge_difference_loss(tp, tt, tm, tg, tx, weighting="quotient", space="normalized", channel_weights=w, std=std)
    a = torch.tensor(w, dtype=torch.float64) / std ** 2
    assert torch.equal(a, eng.Objective("normalized", "mse", w).coefficients(std, 3, "cpu"))
    Hn = float((a * sums[:, 1:4].sum(0)).sum() / (sums[:, 0].sum() * 3))
    assert abs(float(norm) - Hn) <= 2.0 ** -23 * Hn
    flat = eng.edge_difference_loss(tp[0], tt[0], tm.reshape(7, 1), tg, tx, weighting="quotient")
    H0 = float(sums[0, 1:4].sum() / (sums[0, 0] * 3))
    assert abs(float(flat) - H0) <= 2.0 ** -23 * H0
    with pytest.raises(ValueError):
        eng.edge_difference_loss(tp, tt, tm, tg, kind="mae")
    with pytest.raises(ValueError):
        eng.edge_difference_loss(tp, tt, tm, tg, weighting="gradient")
    with pytest.raises(ValueError):
        eng.edge_difference_loss(tp, tt, tm, tg, weighting="quotient")          # no positions
    with pytest.raises(ValueError):
        eng.edge_difference_loss(tp, tt, tm, tg, space="normalized")            # no std


# ------------------------------------------------------------------------------------------------ the C ABI
# every entry of the parent's header (without the bsms_ prefix) and its argument count
OLDER = {"abi_version": 0, "last_error": 0, "plan_create": 4, "plan_set_pool": 3, "plan_bind_edge_weights": 3,
         "plan_bound_edge_weights": 1, "plan_destroy": 1, "plan_pool_trim": 0, "plan_num_nodes": 1, "plan_num_edges": 1,
         "plan_num_pooled": 1, "plan_min_out_degree": 1, "plan_max_source": 1, "plan_export": 5, "plan_export_ex": 3,
         "plan_concat": 7, "segment_sum_fwd": 7, "segment_sum_bwd": 6, "segment_sum_bf16": 6, "cal_ew": 5, "edge_conv": 9,
         "scatter_rows": 8, "gather_rows": 8, "mlp_saved_bytes": 5, "mlp_work_bytes": 5, "mlp_fwd": 12, "mlp_fwd_ex": 13,
         "pack_group_create": 1, "pack_group_destroy": 1, "pack_group_add_mlp": 10, "pack_group_add_bsgmp": 11,
         "pack_group_launch": 2, "mlp_bwd": 14, "mlp_bwd_ex": 15, "gmp_saved_bytes": 5, "gmp_work_bytes": 5, "gmp_fwd": 13,
         "gmp_bwd": 15, "gmp_pos_work_bytes": 3, "gmp_bwd_pos": 17, "bsgmp_saved_bytes": 6, "bsgmp_work_bytes": 6,
         "bsgmp_infer_work_bytes": 6, "bsgmp_fwd": 15, "bsgmp_fwd_ex": 16, "bsgmp_saved_bytes_p": 7, "bsgmp_saved_bytes_ex": 8,
         "bsgmp_work_bytes_ex": 8, "bsgmp_fwd_p": 17, "bsgmp_bwd_p": 18, "bsgmp_bwd": 17, "bsgmp_bwd_ex": 19, "bsgmp_bwd_ev": 20,
         "bsgmp_pos_work_bytes": 4, "bsgmp_bwd_pos": 20, "bsgmp_bwd_pos_ev": 22, "side_lanes_join": 1, "streams_overlap": 2,
         "sim_work_bytes": 1, "sim_prologue": 10, "sim_epilogue": 16, "sim_loss_bwd": 12, "sim_unroll_bwd": 19,
         "sim_objective_bwd": 23, "sim_objective_bwd_w": 25, "sim_robust_bwd": 26, "sim_input_grad": 14, "error_sums_work_bytes":
         2, "error_sums": 12, "error_sums_w": 14, "robust_sums": 21, "batch_assemble": 15, "batch_targets": 6,
         "batch_assemble_xf": 18, "rows_transform": 13, "hierarchy_create": 7, "hierarchy_create_f32": 7, "hierarchy_destroy": 1,
         "hierarchy_level_nodes": 2, "hierarchy_level_edges": 2, "hierarchy_copy_edges": 3, "hierarchy_copy_ids": 3,
         "adamw_work_bytes": 0, "adamw_step": 15, "optim_groups_create": 4, "optim_groups_destroy": 1, "optim_work_bytes": 0,
         "optim_step": 19, "grad_accumulate": 5, "accum_coef": 17, "grad_fold": 5, "wgrad_bound_width": 0, "wgrad_work_bytes": 2,
         "wgrad": 7, "small_wgrad_work_bytes": 1, "small_wgrad": 14}
NEW = {"bsms_edge_diff_work_bytes": 2, "bsms_edge_diff_sums": 18, "bsms_edge_diff_bwd": 20}


def test_new_entries_are_declared_exported_and_bound(eng):
    from bsms_gnn_amd import _abi
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "bsms_hip.h")).read(), flags=re.S)
    raw = C.CDLL(_abi.LIB_PATH)
    for name, nargs in NEW.items():
        decl = re.search(r"\b" + name + r"\s*\(([^;]*)\)\s*;", text)
        assert decl and len(decl.group(1).split(",")) == nargs, name
        assert hasattr(raw, name) and len(_abi.SIGNATURES[name][1]) == nargs, name
    assert _abi.lib().bsms_abi_version() == 4
    assert len(OLDER) == 96 and set(_abi.SIGNATURES) == {"bsms_" + k for k in OLDER} | set(NEW)
    for name, nargs in OLDER.items():
        assert len(_abi.SIGNATURES["bsms_" + name][1]) == nargs, name
    assert re.search(r"BSMS_EDGE_DIFFERENCE = 0, BSMS_EDGE_QUOTIENT = 1", text)


def test_argument_checks_without_gpu(eng):
    L = eng._abi.lib()

    def sums(S=2, Cn=3, p=2, weighting=0, row0=0, seg_rows=10, strides=(10, 10, 10, 10)):
        return L.bsms_edge_diff_sums(None, row0, seg_rows, None, None, None, None, S, Cn, p, weighting, *strides, None, None, None)

    def bwd(S=2, Cn=3, p=2, weighting=0, row0=0, seg_rows=10, strides=(10, 10, 10, 10)):
        return L.bsms_edge_diff_bwd(None, row0, seg_rows, None, None, None, None, S, Cn, p, weighting, *strides, None, 0, None, 10, None)

    for f in (sums, bwd):
        assert f(Cn=9) == -3 and f(Cn=0) == -3                      # unsupported before any pointer is looked at
        assert b"C in 1..8" in L.bsms_last_error()
        assert f(weighting=2) == -3 and f(weighting=-1) == -3
        assert f(weighting=1, p=4) == -3 and f(weighting=1, p=0) == -3
        assert f(weighting=0, p=0, S=0) == 0 and f(weighting=0, p=99, S=0) == 0     # "difference" ignores p
        assert f(S=-1) == -1 and f(seg_rows=-1) == -1 and f(row0=-1) == -1
        assert f(strides=(10, -1, 10, 10)) == -1 and f(strides=(10, 10, 10, -1)) == -1
        assert f(S=0) == 0                                          # nothing to touch, not even the plan
        assert f() == -1 and b"plan is null" in L.bsms_last_error()
    wb = L.bsms_edge_diff_work_bytes
    assert wb(1, 1) > 0 and wb(5, 2049) >= 5 * 3 * 17 * 8 and wb(-1, 5) == 0
    assert all(wb(s, n) <= wb(s + 1, n) and wb(s, n) <= wb(s, n + 1000) for s in (0, 1, 7) for n in (0, 1, 1024, 5000))


def test_cpu_and_mixed_inputs_are_refused_before_any_launch(eng, monkeypatch):
    from bsms_gnn_amd import _abi
    real = _abi.lib()
    touched = []

    class Watch:
        def __getattr__(self, name):
            touched.append(name)
            return getattr(real, name)

    monkeypatch.setattr(_abi, "lib", lambda: Watch())
    p, t, m = torch.zeros(2, 5, 3), torch.zeros(2, 5, 3), torch.ones(2, 5)
    with pytest.raises(_abi.BsmsError):
        eng.edge_diff_sums(p, t, m, None)
    with pytest.raises(_abi.BsmsError):
        eng.edge_diff_bwd(p, t, m, None, torch.zeros(3, dtype=torch.float64))
    g = torch.tensor([[0, 1], [1, 0]])
    with pytest.raises(RuntimeError):
        eng.edge_difference_loss(p, t.to("meta"), m, g)
    with pytest.raises(RuntimeError):
        eng.edge_difference_loss(p, t, m, g.to("meta"))
    assert not touched
    for name in ("edge_diff_sums", "edge_diff_bwd", "edge_difference_sums", "edge_difference_loss", "edge_error_mean_std"):
        assert callable(getattr(eng, name))
    assert callable(eng.Trainer.get_edge_error)


def test_edge_error_mean_std_and_the_rollout_feed(eng):
    """The arithmetic behind get_edge_error and the [ME | DE | 0 | TE] rows that rollout_bank hands to RolloutErrors.add_sums."""
    rng = np.random.default_rng(1)
    sums = np.abs(rng.standard_normal((4, 7))) + 0.1
    E = np.sqrt(sums[:, 1:4] / sums[:, :1])
    for relative, want in ((False, E), (True, E / np.sqrt(sums[:, 4:] / sums[:, :1]))):
        mean, std = eng.edge_error_mean_std(torch.tensor(sums), relative)
        assert relerr(mean.numpy(), want.mean(0)) <= 1e-14 and relerr(std.numpy(), want.std(0)) <= 1e-12
    fed = torch.cat([torch.tensor(sums[:, :4]), torch.zeros(4, 3, dtype=torch.float64), torch.tensor(sums[:, 4:])], 1)
    rmse, rmse_c, rmse_t = eng.RolloutErrors("cpu").add_sums(fed)
    assert relerr(rmse_c.double().numpy(), E) <= 2.0 ** -23 and tuple(rmse_t.shape) == (3, 4)
    assert abs(float(rmse) - np.sqrt(sums[:, 1:4].sum() / sums[:, 0].sum() / 3)) <= 2.0 ** -23 * float(rmse)
