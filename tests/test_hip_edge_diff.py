"""GPU: the edge-difference (discrete H1) sums and their adjoint (csrc/edgediff.hip) against NumPy fp64, their
determinism rules bit for bit, `edge_difference_loss` on the device against the torch fp64 definition, and the two evaluation
routes (`Trainer.get_edge_error`, `rollout_bank(edge_errors=)`).

Tolerances.  Sums: relative (n + 16) 2^-53 per field, n the number of edges of a segment -- the worst case of a sum of n
non-negative terms taken in any order plus the few roundings inside a term.  Backward, per element: 2^-23 |g_ref| + 2^-40 A with A
the sum of the absolute values of the element's terms -- one fp32 rounding with a factor 2 of headroom, plus fp64 reordering under
cancellation.  The measured worst ratios are printed by the tests and recorded in profiles/edge_diff_parity.txt."""
import numpy as np
import pytest
import torch

from conftest import load_golden
from test_datapipe import cfg as make_cfg, synthetic_traj
from test_edge_diff_host import np_edge_grad, np_edge_sums, sums_tol
from test_eval_host import REL_TOL, RMSE_TOL, rel
from test_hip_databank import OPT, model_cfg, same_mesh_trajs
from test_hip_eval import scaled, summaries_rel

pytestmark = pytest.mark.gpu

ROWS = [0, 1, 2, 255, 256, 257, 1023, 1024, 1025, 2049]       # the per-thread, per-wave and 1024-row piece edges
WEIGHTINGS = ["difference", "quotient"]


@pytest.fixture(scope="module")
def eng():
    import bsms_gnn_amd as eng
    return eng


# ------------------------------------------------------------------------------------------------ cases and references
def random_graph(n, seed):
    """(g [2, E] int64, pos [n, 3] float32): mean degree 6, both directions, in a shuffled edge order; rows without any edge (the
    last twentieth), a hub row with >= 70 incoming edges (n >= 255), self-loops, duplicates, a one-directional edge and two
    coincident nodes joined by an edge."""
    rng = np.random.default_rng(seed)
    pos = rng.random((max(n, 1), 3)).astype(np.float32)[:n]
    if n == 0:
        return np.zeros((2, 0), np.int64), pos
    if n == 1:
        return np.array([[0, 0], [0, 0]], np.int64), pos
    if n == 2:
        pos[1] = pos[0]
        return np.array([[0, 0, 1, 0], [0, 1, 0, 1]], np.int64), pos
    live = n - max(1, n // 20)
    a, b = rng.integers(0, live, 3 * n), rng.integers(0, live, 3 * n)
    edges = [np.stack([a, b]), np.stack([b, a]), np.array([[0, a[0], 1], [0, b[0], min(2, live - 1)]])]      # self-loop, duplicate, one direction
    if live >= 100:
        hub = rng.choice(live, 75, replace=False)
        edges.append(np.stack([hub, np.full(75, 3)]))                  # 75 incoming edges of row 3, none of them returned
    if live >= 6:
        pos[5] = pos[4]
        edges.append(np.array([[4, 5], [5, 4]]))
    g = np.concatenate(edges, axis=1).astype(np.int64)
    return g[:, rng.permutation(g.shape[1])], pos


def fields(S, n, C, seed, mask="random"):
    rng = np.random.default_rng(seed + 17)
    pred = rng.standard_normal((S, n, C)).astype(np.float32)
    tar = (3 * rng.standard_normal((S, n, C))).astype(np.float32)
    m = {"random": (rng.random((S, n)) < 0.8), "ones": np.ones((S, n), bool), "zeros": np.zeros((S, n), bool)}[mask].astype(np.float32)
    return pred, tar, m


def edge_weights(mask, g, pos, weighting):
    """(mu [S, E], mu * omega [S, E]) in fp64; mask [S, n], pos [n, p] or [S, n, p]."""
    i, j = g
    m = mask.astype(np.float64)
    mu = m[:, i] * m[:, j]
    if weighting == "difference":
        return mu, mu
    x = (pos if pos.ndim == 3 else pos[None]).astype(np.float64)
    l2 = ((x[:, i] - x[:, j]) ** 2).sum(-1)
    ok = l2 != 0
    mu = mu * ok
    return mu, mu * np.where(ok, 1.0 / np.where(ok, l2, 1.0), 0.0)


def ref_sums(pred, tar, mask, g, pos, weighting):
    """np_edge_sums (tests/test_edge_diff_host.py) without the Python loop: [S, 1+2C] fp64, NumPy's own summation order."""
    i, j = g
    d, t = (pred - tar).astype(np.float64), tar.astype(np.float64)
    mu, mw = edge_weights(mask, g, pos, weighting)
    return np.concatenate([mu.sum(1, keepdims=True), (mw[..., None] * (d[:, i] - d[:, j]) ** 2).sum(1),
                           (mw[..., None] * (t[:, i] - t[:, j]) ** 2).sum(1)], axis=1)


def ref_grad(pred, tar, mask, g, pos, weighting, coef):
    """np_edge_grad without the Python loop: (grad [S, n, C] fp64, A [S, n, C])."""
    i, j = g
    d = (pred - tar).astype(np.float64)
    _, mw = edge_weights(mask, g, pos, weighting)
    term = mw[..., None] * (d[:, j] - d[:, i])
    grad, A = np.zeros(pred.shape, np.float64), np.zeros(pred.shape, np.float64)
    for s in range(pred.shape[0]):
        np.add.at(grad[s], j, term[s])
        np.add.at(grad[s], i, -term[s])
        np.add.at(A[s], j, np.abs(term[s]))
        np.add.at(A[s], i, np.abs(term[s]))
    k2 = 2.0 * (coef if coef.ndim == 2 else coef[None])[:, None, :]
    return grad * k2, A * np.abs(k2)


def dev(a):
    return torch.tensor(a).cuda()


def plan_of(eng, g, n):
    from bsms_gnn_amd.graph import LevelPlan
    if n == 0:                                                          # an empty window of a one-row plan
        g, n = np.zeros((2, 1), np.int64), 1
    return LevelPlan(torch.tensor(g), n, device="cuda")


def sums_ratio(got, want, n_edges):
    """Worst |got - want| / (|want| tol); fields that are exactly 0 must be exactly 0."""
    got = got.cpu().numpy()
    zero = want == 0
    assert np.array_equal(got == 0, zero), (got, want)
    if zero.all():
        return 0.0
    return float(np.max(np.abs(got - want)[~zero] / np.abs(want)[~zero])) / sums_tol(n_edges)


def grad_ratio(got, want, A):
    got = got.double().cpu().numpy()
    tol = 2.0 ** -23 * np.abs(want) + 2.0 ** -40 * A
    assert np.array_equal(got[tol == 0] == 0, np.ones((tol == 0).sum(), bool))          # no term at all: exactly 0
    return float(np.max(np.abs(got - want)[tol > 0] / tol[tol > 0])) if (tol > 0).any() else 0.0


def raw_call(eng, plan, row0, n, pred, tar, mask, pos, C, p, weighting, coef=None, accumulate=0, base=None):
    """One raw call on guarded device buffers: sums (coef None) or the backward; pos [n, p] is shared by the segments (stride 0).
    `work` is NaN-filled and the output sits in front of
    a sentinel; returns (output, the sentinel is intact)."""
    L = eng._abi.lib()
    S = pred.shape[0]
    ptr = lambda t: None if t is None else t.data_ptr()
    stream = torch.cuda.current_stream().cuda_stream
    w = 1 if weighting == "quotient" else 0
    if coef is None:
        out = torch.full((S * (1 + 2 * C) + 64,), -7.0, dtype=torch.float64, device="cuda")
        work = torch.full((L.bsms_edge_diff_work_bytes(S, n) // 8 + 1,), float("nan"), dtype=torch.float64, device="cuda")
        rc = L.bsms_edge_diff_sums(plan.handle, row0, n, ptr(pred), ptr(tar), ptr(mask), ptr(pos), S, C, p, w, n, n, n, 0, ptr(out), ptr(work), stream)
        assert rc == 0, L.bsms_last_error()
        torch.cuda.synchronize()
        return out[:S * (1 + 2 * C)].reshape(S, -1).clone(), bool((out[S * (1 + 2 * C):] == -7.0).all()) and bool(torch.isnan(work[-1]))
    out = torch.full((S * n * C + 64,), -7.0, dtype=torch.float32, device="cuda")
    if base is not None:
        out[:S * n * C] = base.reshape(-1)
    rc = L.bsms_edge_diff_bwd(plan.handle, row0, n, ptr(pred), ptr(tar), ptr(mask), ptr(pos), S, C, p, w, n, n, n, 0, ptr(coef), accumulate, ptr(out), n, stream)
    assert rc == 0, L.bsms_last_error()
    torch.cuda.synchronize()
    return out[:S * n * C].reshape(S, n, C).clone(), bool((out[S * n * C:] == -7.0).all())


_CASES = {}


def case(eng, n, C=3, S=5, mask="random"):
    """Graph, plan, fields and device copies of one row count, built once and shared (never modified)."""
    key = (n, C, S, mask)
    if key not in _CASES:
        g, pos = random_graph(n, n)
        pred, tar, m = fields(S, n, C, n, mask)
        _CASES[key] = dict(g=g, pos=pos, pred=pred, tar=tar, mask=m, plan=plan_of(eng, g, n), dpred=dev(pred), dtar=dev(tar), dmask=dev(m),
                           dpos=[None] + [dev(np.ascontiguousarray(pos[:, :p])) for p in (1, 2, 3)])
    return _CASES[key]


# ------------------------------------------------------------------------------------------------ sums against NumPy fp64
def test_vectorised_references_are_the_loops():
    g, pos = random_graph(40, 1)
    pred, tar, m = fields(2, 40, 3, 1)
    k = np.array([[0.5, 0.0, -2.0], [1.0, 3.0, 0.25]])
    for weighting in WEIGHTINGS:
        a, b = ref_sums(pred, tar, m, g, pos[:, :2], weighting), np_edge_sums(pred, tar, m, g, pos[:, :2], weighting)
        assert np.max(np.abs(a - b) / np.abs(b)) <= sums_tol(g.shape[1])
        (ga, Aa), (gb, Ab) = ref_grad(pred, tar, m, g, pos[:, :2], weighting, k), np_edge_grad(pred, tar, m, g, k, pos[:, :2], weighting)
        assert np.all(np.abs(ga - gb) <= 2.0 ** -45 * Ab) and np.allclose(Aa, Ab, rtol=1e-12)


@pytest.mark.parametrize("weighting", WEIGHTINGS)
@pytest.mark.parametrize("k,n", list(enumerate(ROWS)))
def test_sums_against_numpy_fp64(eng, k, n, weighting):
    """Guards: every row-count edge of the pieces kernel, with C and p cycling through {1, 3, 8} x {1, 2, 3}; S = 5."""
    C, p = (1, 3, 8)[k % 3], (1, 2, 3)[(k // 3 + k) % 3]
    c = case(eng, n, C)
    got = eng.edge_diff_sums(c["dpred"], c["dtar"], c["dmask"], c["plan"], pos=c["dpos"][p], weighting=weighting, row0=0, seg_rows=n)
    assert got.dtype == torch.float64 and tuple(got.shape) == (5, 1 + 2 * C)
    ratio = sums_ratio(got, ref_sums(c["pred"], c["tar"], c["mask"], c["g"], c["pos"][:, :p], weighting), c["g"].shape[1])
    print(f"[edge_diff_sums vs NumPy fp64] rows {n} C {C} p {p} {weighting}: {ratio:.4f} of the bound")
    assert ratio <= 1.0
    if n >= 255:
        assert np.bincount(c["g"][1], minlength=n).max() >= 70 and (np.bincount(c["g"].ravel(), minlength=n) == 0).any()      # the hub, the degree-0 rows


@pytest.mark.parametrize("C", [1, 3, 8])
@pytest.mark.parametrize("p", [1, 2, 3])
def test_sums_every_channel_and_position_width(eng, C, p):
    """Guards: the vector (C = 8) and scalar row loads and every position width, across a piece edge (1025 rows); S = 1."""
    c = case(eng, 1025, C, S=1)
    for weighting in WEIGHTINGS:
        got = eng.edge_diff_sums(c["dpred"], c["dtar"], c["dmask"], c["plan"], pos=c["dpos"][p], weighting=weighting)
        ratio = sums_ratio(got, ref_sums(c["pred"], c["tar"], c["mask"], c["g"], c["pos"][:, :p], weighting), c["g"].shape[1])
        print(f"[edge_diff_sums vs NumPy fp64] rows 1025 C {C} p {p} S 1 {weighting}: {ratio:.4f} of the bound")
        assert ratio <= 1.0


def test_sums_with_four_channels_take_the_vector_loads(eng):
    c = case(eng, 257, 4)
    for weighting in WEIGHTINGS:
        got = eng.edge_diff_sums(c["dpred"], c["dtar"], c["dmask"], c["plan"], pos=c["dpos"][2], weighting=weighting)
        assert sums_ratio(got, ref_sums(c["pred"], c["tar"], c["mask"], c["g"], c["pos"][:, :2], weighting), c["g"].shape[1]) <= 1.0
        # the same rows one float further on: not 16-byte aligned, the scalar loads -- bit-equal
        shifted = torch.empty(c["dpred"].numel() + 1, device="cuda")[1:].reshape(c["dpred"].shape).copy_(c["dpred"])
        assert shifted.data_ptr() % 16 != 0
        assert torch.equal(eng.edge_diff_sums(shifted, c["dtar"], c["dmask"], c["plan"], pos=c["dpos"][2], weighting=weighting), got)


def test_zero_mask_no_segments_and_coincident_nodes(eng):
    c = case(eng, 257, 3, mask="zeros")
    for weighting in WEIGHTINGS:
        got = eng.edge_diff_sums(c["dpred"], c["dtar"], c["dmask"], c["plan"], pos=c["dpos"][2], weighting=weighting)
        assert tuple(got.shape) == (5, 7) and not bool(got.any())                       # ME = 0 and every field 0
    none = eng.edge_diff_sums(c["dpred"][:0], c["dtar"][:0], c["dmask"][:0], c["plan"], seg_rows=257)
    assert tuple(none.shape) == (0, 7)
    L = eng._abi.lib()
    assert L.bsms_edge_diff_sums(c["plan"].handle, 0, 257, None, None, None, None, 0, 3, 2, 1, 257, 257, 257, 257, None, None, None) == 0
    assert L.bsms_edge_diff_sums(c["plan"].handle, 1, 257, None, None, None, None, 1, 3, 2, 1, 257, 257, 257, 257, None, None, None) == -2      # a bad window
    assert L.bsms_edge_diff_sums(c["plan"].handle, 0, 257, None, None, None, None, 1, 3, 2, 1, 257, 257, 257, 257, None, None, None) == -1      # null pointers
    # the edge 4 <-> 5 joins coincident nodes: counted under "difference", excluded under "quotient" (with the self-loops)
    c = case(eng, 257, 3, mask="ones")
    i, j = c["g"]
    flat = int(((c["pos"][i, :2] == c["pos"][j, :2]).all(1)).sum())
    assert flat >= 3
    diff = eng.edge_diff_sums(c["dpred"], c["dtar"], c["dmask"], c["plan"])
    quot = eng.edge_diff_sums(c["dpred"], c["dtar"], c["dmask"], c["plan"], pos=c["dpos"][2], weighting="quotient")
    assert float(diff[0, 0]) == c["g"].shape[1] and float(quot[0, 0]) == c["g"].shape[1] - flat


# ------------------------------------------------------------------------------------------------ strides
def test_strided_segments(eng):
    """pred as a column block of a wider [T, B, N, C] tensor (pred_stride = B N), one mask and one position array shared by all
    segments (stride 0), and per-segment positions against shared ones."""
    T, B, n, C = 5, 3, 257, 3
    c = case(eng, n, C)
    wide = torch.randn(T, B, n, C, device="cuda")
    wide[:, 1] = c["dpred"]
    for weighting in WEIGHTINGS:
        kw = dict(pos=c["dpos"][2], weighting=weighting)
        want = eng.edge_diff_sums(c["dpred"], c["dtar"], c["dmask"], c["plan"], **kw)
        assert torch.equal(eng.edge_diff_sums(wide[:, 1], c["dtar"], c["dmask"], c["plan"], **kw), want)
        assert torch.equal(eng.edge_diff_sums(wide[:, 1], c["dtar"], c["dmask"], c["plan"], pred_stride=B * n, pos_stride=0, **kw), want)
        per = c["dpos"][2].unsqueeze(0).repeat(T, 1, 1)
        assert torch.equal(eng.edge_diff_sums(c["dpred"], c["dtar"], c["dmask"], c["plan"], pos=per, weighting=weighting), want)
        per[2] += 1.0                                                   # really read per segment
        moved = eng.edge_diff_sums(c["dpred"], c["dtar"], c["dmask"], c["plan"], pos=per, weighting=weighting)
        assert torch.equal(moved[[0, 1, 3, 4]], want[[0, 1, 3, 4]]) and (weighting == "difference") == torch.equal(moved[2], want[2])
        shared = eng.edge_diff_sums(c["dpred"], c["dtar"], c["dmask"][3], c["plan"], mask_stride=0, **kw)
        m3 = np.repeat(c["mask"][3:4], T, 0)
        assert sums_ratio(shared, ref_sums(c["pred"], c["tar"], m3, c["g"], c["pos"][:, :2], weighting), c["g"].shape[1]) <= 1.0
        assert torch.equal(shared[3], want[3])
    with pytest.raises(ValueError):
        eng.edge_diff_sums(c["dpred"], c["dtar"], c["dmask"], c["plan"], pred_stride=10 ** 6)      # reaches past the storage
    with pytest.raises(ValueError):
        eng.edge_diff_sums(c["dpred"], c["dtar"], c["dmask"], c["plan"], row0=1)                     # 258 rows of a plan of 257


# ------------------------------------------------------------------------------------------------ bit-identity
def union_case(eng):
    """Three meshes of 300 + 257 + 1025 rows as one block-diagonal plan built from the concatenated edge list; the middle one is the
    shared 257-row case."""
    c = case(eng, 257, 3)
    ga, gb = random_graph(300, 300)[0], random_graph(1025, 1025)[0]
    g = np.concatenate([ga, c["g"] + 300, gb + 557], axis=1)
    return c, plan_of(eng, g, 300 + 257 + 1025)


def test_sums_are_bit_identical(eng):
    c = case(eng, 2049, 3)
    for weighting in WEIGHTINGS:
        kw = dict(pos=c["dpos"][3], weighting=weighting)
        a, b = eng.edge_diff_sums(c["dpred"], c["dtar"], c["dmask"], c["plan"], **kw), eng.edge_diff_sums(c["dpred"], c["dtar"], c["dmask"], c["plan"], **kw)
        assert torch.equal(a, b)                                        # two runs
        alone = eng.edge_diff_sums(c["dpred"][3:4].clone(), c["dtar"][3:4].clone(), c["dmask"][3].clone(), c["plan"], **kw)
        assert torch.equal(alone[0], a[3])                              # a segment of an S = 5 launch, launched alone
        raw, intact = raw_call(eng, c["plan"], 0, 2049, c["dpred"], c["dtar"], c["dmask"], c["dpos"][3], 3, 3, weighting)
        assert intact and torch.equal(raw, a)                           # NaN-filled work, a sentinel behind the sums


def test_window_of_a_union_is_the_mesh_itself(eng):
    c, union = union_case(eng)
    for weighting in WEIGHTINGS:
        kw = dict(pos=c["dpos"][2], weighting=weighting)
        own = eng.edge_diff_sums(c["dpred"], c["dtar"], c["dmask"], c["plan"], **kw)
        assert torch.equal(eng.edge_diff_sums(c["dpred"], c["dtar"], c["dmask"], union, row0=300, seg_rows=257, **kw), own)
        coef = torch.tensor([[0.5, -1.0, 2.0]], dtype=torch.float64, device="cuda").repeat(5, 1)
        g_own = eng.edge_diff_bwd(c["dpred"], c["dtar"], c["dmask"], c["plan"], coef, **kw)
        assert torch.equal(eng.edge_diff_bwd(c["dpred"], c["dtar"], c["dmask"], union, coef, row0=300, seg_rows=257, **kw), g_own)
    # an edge that leaves the window is skipped, in the sums and in both halves of the backward: a window of 200 rows of the 257
    n = 200
    keep = (c["g"] < n).all(0)
    assert not keep.all()
    inner = plan_of(eng, c["g"][:, keep], n)
    args = (c["dpred"][:, :n].contiguous(), c["dtar"][:, :n].contiguous(), c["dmask"][:, :n].contiguous())
    pos = c["dpos"][2][:n].contiguous()
    for weighting in WEIGHTINGS:
        kw = dict(pos=pos, weighting=weighting)
        assert torch.equal(eng.edge_diff_sums(*args, c["plan"], row0=0, seg_rows=n, **kw), eng.edge_diff_sums(*args, inner, **kw))
        assert torch.equal(eng.edge_diff_bwd(*args, c["plan"], coef, row0=0, seg_rows=n, **kw), eng.edge_diff_bwd(*args, inner, coef, **kw))


def test_a_zero_one_mask_only_drops_terms(eng):
    """The sums under an explicit 0/1 mask are bit-equal to those of an all-ones mask on the graph without the masked-out edges."""
    c = case(eng, 1025, 3)
    ones = torch.ones_like(c["dmask"][0])
    for s in (0, 4):
        m = c["mask"][s]
        keep = (m[c["g"][0]] != 0) & (m[c["g"][1]] != 0)
        thin = plan_of(eng, c["g"][:, keep], 1025)
        for weighting in WEIGHTINGS:
            kw = dict(pos=c["dpos"][2], weighting=weighting)
            a = eng.edge_diff_sums(c["dpred"][s:s + 1], c["dtar"][s:s + 1], c["dmask"][s], c["plan"], **kw)
            b = eng.edge_diff_sums(c["dpred"][s:s + 1], c["dtar"][s:s + 1], ones, thin, **kw)
            assert torch.equal(a, b)


# ------------------------------------------------------------------------------------------------ backward
@pytest.mark.parametrize("weighting", WEIGHTINGS)
@pytest.mark.parametrize("k,n", list(enumerate(ROWS)))
def test_backward_against_the_closed_form(eng, k, n, weighting):
    C, p = (3, 8, 1)[k % 3], (2, 3, 1)[(k // 3 + k) % 3]
    c = case(eng, n, C)
    rng = np.random.default_rng(n)
    coef = rng.standard_normal((5, C))
    if C > 1:
        coef[:, 0] = 0.0                                                # a zero channel
    dcoef = dev(coef)
    got, intact = raw_call(eng, c["plan"], 0, n, c["dpred"], c["dtar"], c["dmask"], c["dpos"][p], C, p, weighting, coef=dcoef)
    assert intact                                                       # the sentinel behind grad
    if n == 0:
        return
    want, A = ref_grad(c["pred"], c["tar"], c["mask"], c["g"], c["pos"][:, :p], weighting, coef)
    ratio = grad_ratio(got, want, A)
    print(f"[edge_diff_bwd vs closed form] rows {n} C {C} p {p} {weighting}: {ratio:.4f} of the bound")
    assert ratio <= 1.0
    assert C == 1 or not bool(got[..., 0].any())                        # the zero coefficient: exact zeros in that column
    assert not bool(got[dev(c["mask"]) == 0].any())                     # masked-out rows get exactly 0
    again, _ = raw_call(eng, c["plan"], 0, n, c["dpred"], c["dtar"], c["dmask"], c["dpos"][p], C, p, weighting, coef=dcoef)
    assert torch.equal(again, got)                                      # two runs
    assert torch.equal(eng.edge_diff_bwd(c["dpred"], c["dtar"], c["dmask"], c["plan"], dcoef, pos=c["dpos"][p], weighting=weighting, row0=0, seg_rows=n), got)
    base = torch.randn(5, n, C, device="cuda")
    acc, intact = raw_call(eng, c["plan"], 0, n, c["dpred"], c["dtar"], c["dmask"], c["dpos"][p], C, p, weighting, coef=dcoef, accumulate=1, base=base)
    assert intact and torch.equal(acc, base + got)                      # fl32(base + fl32(g)), bit for bit
    out = base.clone()
    assert eng.edge_diff_bwd(c["dpred"], c["dtar"], c["dmask"], c["plan"], dcoef, pos=c["dpos"][p], weighting=weighting, row0=0, seg_rows=n, out=out) is out
    assert torch.equal(out, acc)


@pytest.mark.parametrize("weighting", WEIGHTINGS)
def test_backward_is_the_adjoint_of_the_sums(eng, weighting):
    """sum grad . v against the central difference of sum_c k_c DE[c] by the fp64 definition at pred +- h v (h = 1e-3): the function
    is quadratic in pred, so the central difference is exact up to rounding.  Relative 1e-6."""
    c = case(eng, 1025, 3, S=1)
    rng = np.random.default_rng(5)
    k, v = rng.standard_normal(3), rng.standard_normal((1, 1025, 3))
    grad = eng.edge_diff_bwd(c["dpred"], c["dtar"], c["dmask"], c["plan"], dev(k), pos=c["dpos"][2], weighting=weighting).double().cpu().numpy()
    d0 = (c["pred"] - c["tar"]).astype(np.float64)                      # the fp32-rounded d, then fp64 throughout
    i, j = c["g"]
    _, mw = edge_weights(c["mask"], c["g"], c["pos"][:, :2], weighting)

    def F(d):
        return float(((mw[..., None] * (d[:, i] - d[:, j]) ** 2).sum(1) * k).sum())

    h = 1e-3
    fd = (F(d0 + h * v) - F(d0 - h * v)) / (2 * h)
    lhs = float((grad * v).sum())
    print(f"[edge_diff_bwd adjoint] {weighting}: {lhs:.12e} vs {fd:.12e}, relative {abs(lhs - fd) / abs(fd):.2e}")
    assert abs(lhs - fd) <= 1e-6 * abs(fd)


# ------------------------------------------------------------------------------------------------ edge_difference_loss on the device
LOSS_CONFIGS = {
    "physical-mse": dict(shape="batch", pos="shared", kw=dict()),
    "normalized-rmse-weights": dict(shape="batch", pos="shared", kw=dict(space="normalized", kind="rmse", channel_weights=[0.5, 2.0, 1.0])),
    "per-sample-positions": dict(shape="batch", pos="per", kw=dict(kind="rmse")),
    "flat-union": dict(shape="flat", pos="shared", kw=dict(channel_weights=[1.0, 0.0, 3.0])),
}


@pytest.mark.parametrize("weighting", WEIGHTINGS)
@pytest.mark.parametrize("name", list(LOSS_CONFIGS))
def test_loss_on_the_device_against_the_fp64_definition(eng, name, weighting):
    """Value: H is a ratio of two sums, each within (n + 16) 2^-53 of the definition, and a handful of fp64 operations -- below
    2^-40 relative for every shape here -- then ONE rounding to fp32; two fp64 numbers that close round to the same or to adjacent
    floats: |got - want| <= 2^-23 |want|.  Gradient: the backward tolerance, with k_c from the fp64 definition."""
    cfgd = LOSS_CONFIGS[name]
    c = case(eng, 257, 3)
    S = 5 if cfgd["shape"] == "batch" else 1
    pred, tar, m = c["pred"][:S], c["tar"][:S], c["mask"][:S]
    pos = c["pos"][:, :2]
    if cfgd["pos"] == "per":
        pos = np.stack([pos + np.float32(0.01 * s) * np.arange(257, dtype=np.float32)[:, None] for s in range(S)])
    std = torch.tensor([0.5, 2.0, 1.25], dtype=torch.float64)
    kw = dict(cfgd["kw"], weighting=weighting)
    if kw.get("space") == "normalized":
        kw["std"] = std
    shape = (lambda a: a) if cfgd["shape"] == "batch" else (lambda a: a[0])
    # the definition, fp64 on the host
    sums = ref_sums(pred, tar, m, c["g"], pos, weighting)
    a = eng.Objective(kw.get("space", "physical"), kw.get("kind", "mse"), kw.get("channel_weights")).coefficients(std, 3, "cpu").numpy()
    ME, H = sums[:, 0].sum(), float((a * sums[:, 1:4].sum(0)).sum() / (sums[:, 0].sum() * 3))
    want = H ** 0.5 if kw.get("kind") == "rmse" else H
    k = a / (ME * 3) if kw.get("kind", "mse") == "mse" else a / (2 * want * ME * 3)
    want_grad, A = ref_grad(pred, tar, m, c["g"], pos, weighting, k)
    cpu = eng.edge_difference_loss(torch.tensor(shape(pred)), torch.tensor(shape(tar)), torch.tensor(shape(m)), torch.tensor(c["g"]),
                                   torch.tensor(shape(pos) if pos.ndim == 3 else pos), **kw)
    assert abs(float(cpu) - want) <= 2.0 ** -23 * want
    # the device
    dp = dev(shape(pred)).requires_grad_()
    dstd = std.cuda()
    if "std" in kw:
        kw["std"] = dstd
    args = (dev(shape(tar)), dev(shape(m)), dev(c["g"]), dev(shape(pos) if pos.ndim == 3 else pos))
    loss = eng.edge_difference_loss(dp, *args, **kw)
    assert loss.dtype == torch.float32 and loss.dim() == 0 and loss.is_cuda
    (3 * loss).backward()                                               # an upstream factor scales the coefficients
    err = abs(float(loss.detach()) - want) / want
    ratio = grad_ratio(dp.grad.reshape(S, 257, 3), 3 * want_grad, 3 * A)
    print(f"[edge_difference_loss on the device] {name} {weighting}: value {err:.2e} (bound {2.0 ** -23:.2e}), gradient {ratio:.4f} of the bound")
    assert err <= 2.0 ** -23 and ratio <= 1.0
    p1 = dev(shape(pred)).requires_grad_()
    eng.edge_difference_loss(p1, *args, **kw).backward()
    assert grad_ratio(p1.grad.reshape(S, 257, 3), want_grad, A) <= 1.0 and not torch.equal(p1.grad, dp.grad)


def test_loss_and_backward_replay_from_a_graph(eng):
    c = case(eng, 257, 3)
    tar, m, g, pos = c["dtar"], c["dmask"], dev(c["g"]), c["dpos"][2]

    def run(p):
        loss = eng.edge_difference_loss(p, tar, m, g, pos, weighting="quotient", kind="rmse")
        return loss, torch.autograd.grad(loss, p)[0]

    static = c["dpred"].clone().requires_grad_()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            run(static)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        loss, grad = run(static)
    new = c["dpred"] * 0.5 + 1.0
    with torch.no_grad():
        static.copy_(new)
    graph.replay()
    torch.cuda.synchronize()
    e_loss, e_grad = run(new.clone().requires_grad_())
    assert torch.equal(loss, e_loss) and torch.equal(grad, e_grad) and bool(grad.any())


# ------------------------------------------------------------------------------------------------ evaluation
def host_edge_error(eng, pred, tar, mask, g, pos, relative, weighting):
    """get_edge_error restated from the definition (torch fp64 on the host): (mean [C], std [C])."""
    sums = eng.edge_difference_sums(pred.cpu(), tar.cpu().reshape(pred.shape), mask.cpu().reshape(pred.shape[0], -1), g.cpu(), pos.cpu(), weighting).numpy()
    C = pred.shape[-1]
    E = np.sqrt(sums[:, 1:1 + C] / sums[:, :1])
    if relative:
        E = E / np.sqrt(sums[:, 1 + C:] / sums[:, :1])
    return E.mean(0), E.std(0)


def check_get_edge_error(eng, tr, data, g, node_in, S):
    with torch.no_grad():
        pred = tr.get_pred(data)
    tar, mask = tr.get_label_mask(data)
    C = pred.shape[-1]
    pred = pred.reshape(S, -1, C)
    pos = node_in.reshape(S, -1, node_in.shape[-1])[..., C:-1]
    for relative in (True, False):
        for weighting in WEIGHTINGS:
            mean, std = tr.get_edge_error(data, relative=relative, weighting=weighting)
            assert isinstance(mean, np.ndarray) and mean.dtype == std.dtype == np.float32 and mean.shape == std.shape == (C,)
            want_mean, want_std = host_edge_error(eng, pred, tar, mask, g, pos, relative, weighting)
            e_mean = rel(mean, want_mean)
            e_std = rel(std, want_std) if S > 1 else float(np.abs(std).max())
            print(f"[Trainer.get_edge_error vs definition] S {S} relative={relative} {weighting}: mean {e_mean:.2e} std {e_std:.2e} (bound {REL_TOL:.0e})")
            assert np.isfinite(mean).all() and (mean > 0).all() and e_mean <= REL_TOL and e_std <= REL_TOL


def test_get_edge_error_consistent_mesh(eng):
    """B = 3 samples on the del300 mesh of tests/golden/graphs.npz."""
    z = load_golden("graphs")
    es, ids = z.levels("del300")
    B, N, C = 3, 300, 3
    torch.manual_seed(0)
    pos = z.t("del300/pos").float()
    state = torch.randn(B, N, C)
    node_in = torch.cat([state, pos.expand(B, N, 2), torch.zeros(B, N, 1)], -1)
    tar = state + 0.1 * torch.randn(B, N, C)
    mask = (torch.rand(B, N, 1) < 0.8).float()
    data = [node_in, tar, mask, [e.unsqueeze(0).repeat(B, 1, 1) for e in es], [i.unsqueeze(0).repeat(B, 1) for i in ids]]
    mcfg = model_cfg(True, depth=len(es) - 1)
    tr = eng.Trainer(eng.BSMS_Simulator(mcfg), mcfg, OPT)
    tr.iter(data)                                                       # the warm-up step: normaliser statistics
    assert tr.iter(data) is not None
    check_get_edge_error(eng, tr, data, es[0], node_in, B)


def test_get_edge_error_variable_meshes(eng):
    """The block-diagonal batch is ONE sample of sum N rows, as in get_error."""
    torch.manual_seed(0)
    mcfg = model_cfg(False)
    tr = eng.Trainer(eng.BSMS_Simulator(mcfg), mcfg, OPT)
    bank = eng.TrajectoryBank(make_cfg(False), dataset="cylinder_flow", process=tr.model.process)
    for t in (synthetic_traj(100, 4, 1), synthetic_traj(140, 4, 2), synthetic_traj(90, 5, 3)):
        bank.add(t)
    tr.iter(bank.batch([(0, 0), (1, 0), (2, 0)], train=False))
    assert tr.iter(bank.batch([(0, 1), (1, 2), (2, 3)], train=False)) is not None
    data = bank.batch([(2, 0), (0, 2), (1, 1)], train=False)
    check_get_edge_error(eng, tr, data, data[0].edge_index, data[0].x, 1)


def counted(eng, monkeypatch):
    L = eng._abi.lib()
    calls = {name: 0 for name in ("bsms_edge_diff_work_bytes", "bsms_edge_diff_sums", "bsms_edge_diff_bwd", "bsms_error_sums")}

    def wrap(name):
        real = getattr(L, name)

        def f(*a):
            calls[name] += 1
            return real(*a)
        return f

    for name in calls:
        monkeypatch.setattr(L, name, wrap(name))
    return calls


def test_rollout_bank_edge_errors_consistent_mesh(eng, monkeypatch):
    """Four trajectories of T = 4 on one mesh: the edge-difference accumulators against RolloutErrors.add fed with host-side edge
    differences (the differences as `results`, a zero target, mu_e as the mask), bit-equal between batch = 1 and batch = 4; the
    pointwise accumulators are those of a call without edge_errors, and without the argument no new entry is called."""
    trajs = [scaled(t, f) for t, f in zip(same_mesh_trajs(120, 4, 4, seed=9), (1.0, 3.0, 0.3, 10.0))]
    bank = eng.TrajectoryBank(make_cfg(True), dataset="airfoil")
    for t in trajs:
        bank.add(t)
    torch.manual_seed(0)
    mcfg = model_cfg(True)
    tr = eng.Trainer(eng.BSMS_Simulator(mcfg), mcfg, OPT)
    tr.iter(bank.batch([(k, 0) for k in range(4)], train=False))
    tr.iter(bank.batch([(k, 1) for k in range(4)], train=False))
    calls = counted(eng, monkeypatch)
    plain = eng.rollout_bank(tr, bank, batch=4)
    tr.get_error(bank.batch([(0, 0), (1, 0)], train=False))
    assert calls["bsms_edge_diff_sums"] == calls["bsms_edge_diff_bwd"] == calls["bsms_edge_diff_work_bytes"] == 0 and calls["bsms_error_sums"] == 5
    ee4, ee1 = eng.RolloutErrors(bank.device), eng.RolloutErrors(bank.device)
    e4, r4 = eng.rollout_bank(tr, bank, batch=4, keep_results=True, edge_errors=ee4)
    e1 = eng.rollout_bank(tr, bank, batch=1, edge_errors=ee1)
    assert calls["bsms_edge_diff_sums"] == 8 and calls["bsms_error_sums"] == 13 and calls["bsms_edge_diff_bwd"] == 0
    assert summaries_rel(e4.summary(), plain.summary())[1] and summaries_rel(e1.summary(), plain.summary())[1]
    assert summaries_rel(ee4.summary(), ee1.summary())[1] and float(ee4.all._num_accumulations) == 4
    g = bank.batch([(0, 0)], train=False)[3][0][0].cpu()
    i, j = g[0], g[1]
    ref = eng.RolloutErrors("cpu")
    for k, res in enumerate(r4):
        _, tar, mask, *_ = bank.trajectory(k)
        d = res.cpu() - tar.cpu()
        m = mask.cpu()
        ref.add(d[:, i] - d[:, j], torch.zeros(d.shape[0], g.shape[1], d.shape[2]), m[:, i] * m[:, j])
    on_host = {k: tuple(x.cpu() for x in v) for k, v in ee4.summary().items()}
    err = summaries_rel(on_host, ref.summary())[0]
    print(f"[rollout_bank edge_errors vs host-side edge differences] consistent mesh, summary: {err:.2e} (bound {RMSE_TOL:.0e})")
    assert err <= RMSE_TOL
    assert not summaries_rel(ee4.summary(), e4.summary())[1]            # not the pointwise figures


class Recorder:
    def __init__(self):
        self.sums = []

    def add_sums(self, sums):
        self.sums.append(sums.clone())


def test_rollout_bank_edge_errors_variable_meshes(eng):
    """Meshes of 100 and 140 nodes advanced as one union: each trajectory's sums are taken through its window of the union's plan
    (row0 = its first row) with its own slice of the positions, and equal the definition on its own mesh."""
    torch.manual_seed(0)
    mcfg = model_cfg(False)
    tr = eng.Trainer(eng.BSMS_Simulator(mcfg), mcfg, OPT)
    bank = eng.TrajectoryBank(make_cfg(False), dataset="cylinder_flow", process=tr.model.process)
    for t in (scaled(synthetic_traj(100, 5, 1), 1.0), scaled(synthetic_traj(140, 5, 2), 4.0)):
        bank.add(t)
    tr.iter(bank.batch([(0, 0), (1, 0)], train=False))
    tr.iter(bank.batch([(0, 1), (1, 2)], train=False))
    for weighting in WEIGHTINGS:
        rec = Recorder()
        _, kept = eng.rollout_bank(tr, bank, batch=2, keep_results=True, edge_errors=rec, edge_weighting=weighting)
        assert [tuple(s.shape) for s in rec.sums] == [(4, 10), (4, 10)]
        for k, (res, sums) in enumerate(zip(kept, rec.sums)):
            own = bank.batch([(k, 0)], train=False)
            _, tar, mask, *_ = bank.trajectory(k)
            want = eng.edge_difference_sums(res.cpu(), tar.cpu(), mask[0, :, 0].cpu(), own[0].edge_index.cpu(), own[0].x[:, 3:5].cpu(), weighting).numpy()
            got = sums.cpu().numpy()
            assert not got[:, 4:7].any()                                # [ME | DE | 0 | TE]
            tol = 2 * sums_tol(own[0].edge_index.shape[1])             # the kernel's order and torch's, each within the sums bound
            assert rel(got[:, :4], want[:, :4]) <= tol and rel(got[:, 7:], want[:, 4:]) <= tol, (k, weighting)
