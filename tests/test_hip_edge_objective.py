"""GPU: the objective with an edge-difference term, J = L + lambda T.

1. bsms_edge_diff_fold against the ordered fp64 sum, bit for bit.
2. bsms_sim_edge_objective_bwd against the COMPOSITION of the two merged entries it fuses -- bsms_sim_objective_bwd (w = 1, no carry)
   for the pointwise part and bsms_edge_diff_bwd with coef = k for the edge part, k formed here in NumPy fp64 by the header's formula
   from the sums read back -- bit for bit in the physical space; with edge_lambda = 0 and a carried pair against bsms_sim_objective_bwd;
   in the normalized space against NumPy fp64 within the bound derived below; loss, parts, determinism, sentinels.
3. The fused step against the CPU oracle under autograd, with `masked_loss(.., g=, pos=)` on CPU tensors as the oracle's loss, and
   against the autograd route on the device; the step's other forms (graph, recompute, frozen, input_grad, bf16, loss_parts).
4. Two gloo ranks, the Trainer with the config keys, and which entries a step calls.

The normalized-space bound, per element: 2^-21 (|w| (|gp| + |ge|) + |carry|) + 2^-40 |w| 2 k_c A, A = sum mu omega |d_r - d_o|.  The
value is w (gp + ge) + carry with gp = (d m) fl32(G a_c) -- at most eight fp32 roundings of 2^-24 each on terms no larger than the
operands' magnitudes (2^-21 leaves a factor of two) -- and ge carries the fp64 accumulation term of DESIGN.md 4.21.
Measured on one MI355X: at most 0.346 of the bound (profiles/edge_objective_parity.txt).

Graphs come from `hub_graph` below: degree-0 rows, a hub with 75 incoming edges (n >= 255), self-loops, duplicates, a one-directional
edge and coincident nodes joined by an edge; every mask leaves a live edge (ME > 0 is asserted)."""
import math
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from conftest import ROOT, KinkMargin, load_golden, rel_err
from oracle import bsms_oracle as ro
from test_hip_edge_diff import ref_grad
from test_hip_objective import SHAPE3, _golden_model, oracle3
from test_hip_unroll import MIN_MARGIN, _cuda, _f64, check, later_targets, make_oracle

pytestmark = pytest.mark.gpu

WEIGHTINGS = ["difference", "quotient"]
KIND_ID, SPACE_ID = {"rmse": 0, "mse": 1}, {"physical": 0, "normalized": 1}
_MEASURED = {}                     # name -> worst measured fraction of a bound (printed; profiles/edge_objective_parity.txt records them)


@pytest.fixture(scope="module")
def eng():
    import bsms_gnn_amd as eng
    return eng


def ptr(t):
    return None if t is None else t.data_ptr()


def stream():
    return torch.cuda.current_stream().cuda_stream


# ------------------------------------------------------------------------------------------------ cases
def hub_graph(n, seed):
    """(g [2, E] int64, pos [n, 3] float32) in a shuffled edge order."""
    rng = np.random.default_rng(1000 + seed)
    pos = rng.random((n, 3)).astype(np.float32)
    if n == 1:
        return np.array([[0, 0], [0, 0]], np.int64), pos                # two copies of the self-loop
    live = n - max(1, n // 16)                                          # the last rows have no edge at all
    a, b = rng.integers(0, live, 3 * n), rng.integers(0, live, 3 * n)
    edges = [np.stack([a, b]), np.stack([b, a]), np.array([[0, a[1], 1], [0, b[1], min(2, live - 1)]])]     # self-loop, duplicate, one direction
    if live >= 100:
        hub = rng.choice(live, 75, replace=False)
        edges.append(np.stack([hub, np.full(75, 7)]))                   # 75 incoming edges of row 7, none returned
    if live >= 6:
        pos[5] = pos[4]
        edges.append(np.array([[4, 5], [5, 4]]))
    g = np.concatenate(edges, axis=1).astype(np.int64)
    return g[:, rng.permutation(g.shape[1])], pos


def fields(S, n, C, seed):
    rng = np.random.default_rng(seed + 5)
    pred = rng.standard_normal((S, n, C)).astype(np.float32)
    tar = (2 * rng.standard_normal((S, n, C))).astype(np.float32)
    mask = (rng.random((S, n)) < 0.8).astype(np.float32)
    mask[:, :min(n, 3)] = 1.0                                           # a live edge in every segment (0 -> 0, and 0 <-> 1 when n > 1)
    return pred, tar, mask


def stats(C, seed, small=None):
    gen = torch.Generator().manual_seed(seed)
    mean = torch.randn(C, generator=gen, dtype=torch.float64)
    var = 0.5 + torch.rand(C, generator=gen, dtype=torch.float64)
    if small is not None:
        var[small] = var[small] * 1e-4
    return [mean.cuda(), (mean * mean + var).cuda(), torch.tensor(1e-8, dtype=torch.float64).cuda()]


def std_of(st):
    mean, meansq, eps = (t.cpu() for t in st)
    return torch.maximum(torch.nan_to_num(torch.sqrt(meansq - mean * mean)), eps)          # fp64, the ops of std_eps


_PLANS = {}


def plan_of(n, seed):
    from bsms_gnn_amd.graph import LevelPlan
    if (n, seed) not in _PLANS:
        g, pos = hub_graph(n, seed)
        _PLANS[(n, seed)] = (LevelPlan(torch.tensor(g), n, device="cuda"), g, pos)
    return _PLANS[(n, seed)]


class Case:
    """Device tensors of S segments of n rows on the graph `hub_graph(n, n)`; positions scaled per segment (coincident stays so)."""

    def __init__(self, eng, n, S, C, p, seed=0):
        self.n, self.S, self.C, self.p, self.R = n, S, C, p, S * n
        self.plan, self.g, pos = plan_of(n, n)
        self.pred, self.tar, self.mask = fields(S, n, C, 100 * n + 10 * S + C + seed)
        self.pos = np.stack([pos[:, :p] * np.float32(1 + s) for s in range(S)])
        self.d = {k: torch.tensor(getattr(self, k)).cuda() for k in ("pred", "tar", "mask", "pos")}
        self.o_stats, self.i_stats = stats(C, 7 * n + C, small=C // 2), stats(C + 1, 11 * n + C)
        self.weights = (0.5 + 1.5 * torch.rand(C, generator=torch.Generator().manual_seed(C), dtype=torch.float64))
        self.dw = self.weights.cuda()
        d = self.d
        self.sums = eng.error_sums(d["pred"].reshape(1, self.R, C), d["tar"].reshape(1, self.R, C), d["mask"].reshape(1, self.R, 1), self.R)[0]

    def edge_sums(self, eng, weighting):
        """([S, 1+2C] through a NaN-filled scratch, the fold's row [1+C] in front of a sentinel) -- device fp64."""
        L, d, C, S, n = eng._abi.lib(), self.d, self.C, self.S, self.n
        es = torch.full((S * (1 + 2 * C) + 8,), -7.0, dtype=torch.float64, device="cuda")
        work = torch.full((L.bsms_edge_diff_work_bytes(S, n) // 8 + 1,), float("nan"), dtype=torch.float64, device="cuda")
        eng._abi.check(L.bsms_edge_diff_sums(self.plan.handle, 0, n, ptr(d["pred"]), ptr(d["tar"]), ptr(d["mask"]), ptr(d["pos"]), S, C, self.p,
                                             WEIGHTINGS.index(weighting), n, n, n, n, ptr(es), ptr(work), stream()), "bsms_edge_diff_sums")
        row = torch.full((1 + C + 8,), -7.0, dtype=torch.float64, device="cuda")
        eng._abi.check(eng._abi.ext().bsms_edge_diff_fold(ptr(es), S, C, ptr(row), stream()), "bsms_edge_diff_fold")
        assert bool((es[S * (1 + 2 * C):] == -7.0).all()) and bool((row[1 + C:] == -7.0).all())
        return es[:S * (1 + 2 * C)].reshape(S, 1 + 2 * C), row[:1 + C].clone()

    def objective_bwd(self, eng, space, kind, w, weights=True, carry=None):
        """bsms_sim_objective_bwd over the R rows: (loss, chan, g_pred, grad_norm_pred)."""
        L, d, C, R = eng._abi.lib(), self.d, self.C, self.R
        loss, chan = torch.full((1,), -1.0, device="cuda"), torch.full((C,), -1.0, device="cuda")
        gp, gnp = torch.full((R, C), 7.0, device="cuda"), torch.full((R, C), 7.0, device="cuda")
        eng._abi.check(L.bsms_sim_objective_bwd(ptr(d["pred"]), ptr(d["tar"]), ptr(d["mask"]), R, C, *map(ptr, self.o_stats), *map(ptr, self.i_stats),
                                                ptr(self.sums), ptr(self.dw) if weights else None, SPACE_ID[space], KIND_ID[kind], w,
                                                ptr(carry[0]) if carry else None, ptr(carry[1]) if carry else None, ptr(loss), ptr(chan), ptr(gp),
                                                ptr(gnp), stream()), "bsms_sim_objective_bwd")
        return loss, chan, gp, gnp

    def edge_objective_bwd(self, eng, row, weighting, space, kind, lam, w, weights=True, carry=None):
        """The new entry, every output in front of a sentinel: (loss, parts, chan, g_pred, grad_norm_pred)."""
        L, d, C, R = eng._abi.lib(), self.d, self.C, self.R
        pad = 16
        outs = [torch.full((k + pad,), -7.0, device="cuda") for k in (1, 2, C, R * C, R * C)]
        eng._abi.check(eng._abi.ext().bsms_sim_edge_objective_bwd(self.plan.handle, self.n, self.S, ptr(d["pred"]), ptr(d["tar"]), ptr(d["mask"]), ptr(d["pos"]), C,
                                                     self.p, WEIGHTINGS.index(weighting), *map(ptr, self.o_stats), *map(ptr, self.i_stats), ptr(self.sums),
                                                     ptr(row), ptr(self.dw) if weights else None, SPACE_ID[space], KIND_ID[kind], lam, w,
                                                     ptr(carry[0]) if carry else None, ptr(carry[1]) if carry else None, *map(ptr, outs), stream()),
                       "bsms_sim_edge_objective_bwd")
        for o, k in zip(outs, (1, 2, C, R * C, R * C)):
            assert bool((o[k:] == -7.0).all()), "an output ran past its end"
        loss, parts, chan, gp, gnp = (o[:k].clone() for o, k in zip(outs, (1, 2, C, R * C, R * C)))
        return loss, parts, chan, gp.reshape(R, C), gnp.reshape(R, C)

    def header_terms(self, row, a, kind, lam):
        """(L, T, k [C], G) in Python fp64 by the header's formulas, operation for operation, from the sums read back."""
        C = self.C
        sums, es = self.sums.cpu().numpy(), row.cpu().numpy()
        MC = float(sums[0]) * float(C)
        Q = 0.0
        for c in range(C):
            Q += float(a[c]) * float(sums[1 + c]) / MC
        Lv = math.sqrt(Q) if kind == "rmse" else Q
        G = 1.0 / (Lv * MC) if kind == "rmse" else 2.0 / MC
        MEC = float(es[0]) * float(C)
        H = 0.0
        for c in range(C):
            H += float(a[c]) * float(es[1 + c]) / MEC
        T = math.sqrt(H) if kind == "rmse" else H
        k = np.array([(lam * float(a[c])) / ((2.0 * T) * MEC) if kind == "rmse" else (lam * float(a[c])) / MEC for c in range(C)])
        return Lv, T, k, G

    def carry(self, seed):
        gen = torch.Generator().manual_seed(seed)
        g_next, g_nin = torch.randn(self.R, self.C, generator=gen), torch.randn(self.R, self.C + 1, generator=gen)
        # The two halves of a carried element share their sign: |carry| = |g_pred_next| + |g_norm_in_next / std_in|, so the bound's |carry|
        # covers the rounding of each half (halves that cancel would leave a |carry| smaller than the rounding of one of them).
        g_nin[:, :self.C] = g_nin[:, :self.C].abs() * torch.sign(g_next)
        dead = torch.tensor(self.mask.reshape(-1)) == 0
        g_next[dead], g_nin[dead] = float("inf"), float("nan")          # must never reach the result
        return g_next.cuda(), g_nin.cuda()


# ------------------------------------------------------------------------------------------------ 1: the fold
@pytest.mark.parametrize("C", [1, 4, 8])
@pytest.mark.parametrize("S", [0, 1, 3, 70])
def test_fold_is_the_ordered_fp64_sum(eng, S, C):
    L = eng._abi.lib()
    gen = torch.Generator().manual_seed(10 * S + C)
    sums = (torch.randn(max(S, 1), 1 + 2 * C, generator=gen, dtype=torch.float64) * 1e3).abs()[:S]
    dsums = sums.cuda()
    out = torch.full((1 + C + 8,), -7.0, dtype=torch.float64, device="cuda")
    eng._abi.check(eng._abi.ext().bsms_edge_diff_fold(ptr(dsums) if S else None, S, C, ptr(out), stream()), "bsms_edge_diff_fold")
    want = np.zeros(1 + C)
    for s in range(S):                                                  # ascending, one addition after the other
        want = want + sums[s, :1 + C].numpy()
    assert np.array_equal(out[:1 + C].cpu().numpy(), want) and bool((out[1 + C:] == -7.0).all())


# ------------------------------------------------------------------------------------------------ 2: the backward entry
@pytest.mark.parametrize("S", [1, 3])
@pytest.mark.parametrize("n", [1, 255, 256, 257, 1025])
def test_backward_is_the_composition_of_the_two_merged_entries(eng, n, S):
    """Physical space with channel weights: a_c = w_c exactly, so k is formed here without the normaliser.  C = 1 / 3 / 4 / 8; the
    difference weighting, and the quotient at p = 1 / 2 / 3; both kinds; w = 1 and 0.37."""
    lam = 0.3
    for C in (1, 3, 4, 8):
        for weighting, p in (("difference", 2), ("quotient", 1), ("quotient", 2), ("quotient", 3)):
            if n == 1 and weighting == "quotient":
                continue                                                # one node: its only edge is the self-loop, which has no length -- ME == 0
            case = Case(eng, n, S, C, p)
            d = case.d
            es, row = case.edge_sums(eng, weighting)
            assert float(row[0]) > 0 and (n == 1 or bool((row[1:] > 0).all()))          # ME > 0: a live edge
            sd = std_of(case.o_stats)
            for kind in ("rmse", "mse"):
                if n == 1 and kind == "rmse":
                    continue                                            # one node: DE == 0, so T == 0 and k is 0 / 0 (not guarded, by design)
                Lv, T, k, G = case.header_terms(row, case.weights.numpy(), kind, lam)
                _, _, gp, _ = case.objective_bwd(eng, "physical", kind, 1.0)
                ge = eng.edge_diff_bwd(d["pred"], d["tar"], d["mask"], case.plan, torch.tensor(k).cuda(), pos=d["pos"], weighting=weighting)
                for w in (1.0, 0.37):
                    loss, parts, chan, g_pred, gnp = case.edge_objective_bwd(eng, row, weighting, "physical", kind, lam, w)
                    want = torch.tensor(w, dtype=torch.float32, device="cuda") * (gp + ge.reshape(case.R, C))
                    tag = (n, S, C, p, weighting, kind, w)
                    assert torch.equal(g_pred, want), (tag, float((g_pred - want).abs().max()))
                    out = ((g_pred * d["mask"].reshape(-1, 1)).double() * sd.cuda()).float()
                    assert torch.equal(gnp, out), tag
                    J = Lv + lam * T
                    assert abs(float(loss) - J) <= 2.0 ** -23 * J and abs(float(parts[0]) - Lv) <= 2.0 ** -23 * Lv, tag
                    assert abs(float(parts[1]) - T) <= 2.0 ** -23 * T, tag
                    assert bool((g_pred[d["mask"].reshape(-1) == 0] == 0).all()), tag      # a masked row: no loss term, no edge term


@pytest.mark.parametrize("kind", ["rmse", "mse"])
@pytest.mark.parametrize("n,S,C", [(257, 3, 3), (1025, 1, 8), (256, 3, 4)])
def test_zero_lambda_with_a_carried_pair_is_the_pointwise_entry(eng, n, S, C, kind):
    case = Case(eng, n, S, C, 2)
    carry = case.carry(n + C)
    for weighting in WEIGHTINGS:
        _, row = case.edge_sums(eng, weighting)
        loss0, chan0, gp0, gnp0 = case.objective_bwd(eng, "normalized", kind, 0.37, carry=carry)
        loss1, parts, chan1, gp1, gnp1 = case.edge_objective_bwd(eng, row, weighting, "normalized", kind, 0.0, 0.37, carry=carry)
        assert torch.equal(gp1, gp0) and torch.equal(gnp1, gnp0) and torch.equal(loss1, loss0) and torch.equal(chan1, chan0)
        assert torch.equal(parts[:1], loss0) and float(parts[1]) > 0
        assert bool(torch.isfinite(gp1).all()) and bool((gp1[case.d["mask"].reshape(-1) == 0] == 0).all())


@pytest.mark.parametrize("weighting", WEIGHTINGS)
@pytest.mark.parametrize("n,S,C", [(257, 3, 3), (1025, 1, 8), (255, 3, 1)])
def test_normalized_space_against_numpy_fp64(eng, n, S, C, weighting):
    case = Case(eng, n, S, C, 3 if C == 3 else 2)
    lam, w = 0.3, 0.37
    _, row = case.edge_sums(eng, weighting)
    assert float(row[0]) > 0
    sd = std_of(case.o_stats).numpy()
    sdi = std_of(case.i_stats).numpy()
    g_next, g_nin = case.carry(3 * n + C)
    D = (case.pred - case.tar).astype(np.float64).reshape(case.R, C)
    Mk = case.mask.astype(np.float64).reshape(case.R, 1)
    with np.errstate(invalid="ignore"):
        carry = np.where(Mk != 0, g_next.cpu().double().numpy() + g_nin.cpu().double().numpy()[:, :C] / sdi[:C], 0.0)
    worst = 0.0
    for kind in ("rmse", "mse"):
        for weights in (False, True):
            a = (case.weights.numpy() if weights else np.ones(C)) / sd ** 2
            Lv, T, k, G = case.header_terms(row, a, kind, lam)
            ge, A = ref_grad(case.pred, case.tar, case.mask, case.g, case.pos, weighting, k)
            ge, A = ge.reshape(case.R, C), A.reshape(case.R, C)
            gp = G * a[None, :] * Mk * D
            want = w * (gp + ge) + carry
            bound = 2.0 ** -21 * (abs(w) * (np.abs(gp) + np.abs(ge)) + np.abs(carry)) + 2.0 ** -40 * abs(w) * A
            outs = case.edge_objective_bwd(eng, row, weighting, "normalized", kind, lam, w, weights=weights, carry=(g_next, g_nin))
            again = case.edge_objective_bwd(eng, row, weighting, "normalized", kind, lam, w, weights=weights, carry=(g_next, g_nin))
            assert all(torch.equal(x, y) for x, y in zip(outs, again))                          # deterministic run to run
            loss, parts, chan, g_pred, gnp = outs
            err = np.abs(g_pred.cpu().double().numpy() - want)
            assert np.array_equal(err[bound == 0] == 0, np.ones((bound == 0).sum(), bool))      # no term at all: exactly 0
            frac = float((err[bound > 0] / bound[bound > 0]).max())
            worst = max(worst, frac)
            assert frac <= 1.0, (kind, weights, frac)
            J = Lv + lam * T
            assert abs(float(loss) - J) <= 2.0 ** -23 * J and abs(float(parts[0]) - Lv) <= 2.0 ** -23 * Lv and abs(float(parts[1]) - T) <= 2.0 ** -23 * T
            terms = a * case.sums.cpu().numpy()[1:1 + C] / (float(case.sums[0]) * C)
            assert np.abs(chan.cpu().double().numpy() - terms).max() <= 2.0 ** -23 * terms.max()
            out = ((g_pred.cpu() * torch.tensor(Mk, dtype=torch.float32)).double() * torch.tensor(sd)).float()
            assert torch.equal(gnp.cpu(), out)
    _MEASURED[f"normalized n={n} S={S} C={C} {weighting}"] = worst
    print(f"\n[n={n} S={S} C={C} {weighting}] worst measured fraction of the normalized-space bound: {worst:.3f}")


def test_shape_and_argument_errors_on_the_device(eng):
    case = Case(eng, 257, 1, 3, 2)
    L, d = eng._abi.lib(), case.d
    _, row = case.edge_sums(eng, "difference")
    gnp = torch.zeros(257, 3, device="cuda")
    call = lambda seg_rows, S: eng._abi.ext().bsms_sim_edge_objective_bwd(case.plan.handle, seg_rows, S, ptr(d["pred"]), ptr(d["tar"]), ptr(d["mask"]), None, 3, 2, 0,
                                                             *map(ptr, case.o_stats), None, None, None, ptr(case.sums), ptr(row), None, 0, 1, 0.1, 1.0,
                                                             None, None, None, None, None, None, ptr(gnp), stream())
    assert call(256, 1) == -2 and b"plan has 257 rows" in L.bsms_last_error()       # BSMS_E_SHAPE: not the plan's rows
    assert call(257, 1) == 0
    torch.cuda.synchronize()
    assert bool(torch.isfinite(gnp).all()) and float(gnp.abs().max()) > 0


# ------------------------------------------------------------------------------------------------ 3: the fused step against the oracle
CONFIGS = {"normalized/mse+difference": dict(space="normalized", kind="mse", channel_weights=None, edge_weight=0.3, edge_weighting="difference"),
           "physical/rmse+quotient": dict(space="physical", kind="rmse", channel_weights=[1.0, 1.0, 3.0], edge_weight=0.01, edge_weighting="quotient")}


def objective_of(eng, name, C=3):
    kw = dict(CONFIGS[name])
    if kw["channel_weights"] is not None:
        kw["channel_weights"] = kw["channel_weights"][:C]
    return eng.Objective(kw.pop("space"), kw.pop("kind"), kw.pop("channel_weights"), **kw)


def edge_oracle(eng, sim, data, later, step_weights, detach, obj, consistent=True, leaf_input=False):
    """tests/test_hip_unroll.py::unrolled_oracle with `masked_loss(.., g=, pos=)` on CPU tensors as the loss.  Returns (predictions,
    total, parameter gradients, per-step losses, node_in.grad or None)."""
    node_in, tar, mask, m_gs, m_ids = data
    if leaf_input:
        node_in = node_in.detach().clone().requires_grad_(True)
    C = tar.shape[-1]
    g = m_gs[0][0] if consistent else m_gs[0]
    pos = node_in.detach()[..., C:-1]                                    # [B, N, p]: every sample's own
    tars = [tar, *(later if later is not None else [])]
    std = sim._targetNormalizer.std_with_epsilon().detach()
    sim.zero_grad(set_to_none=True)
    cur, preds, losses, total = node_in, [], [], 0.0
    for k, w in enumerate(step_weights):
        pred = sim((cur, tars[k], mask, m_gs, m_ids), consistent, False)
        preds.append(pred.detach())
        loss_k = eng.masked_loss(pred, tars[k], mask, obj, std, g=g, pos=pos)
        if pred.dtype == torch.float64:                                 # the fp64 yardstick: J before masked_loss's rounding to fp32
            from bsms_gnn_amd.objective import channel_sums, edge_difference_sums, edge_term
            M, SE = channel_sums(pred, tars[k], mask)
            Q = (obj.coefficients(std, C, "cpu") * SE / (M * C)).sum()
            loss_k = (torch.sqrt(Q) if obj.kind == "rmse" else Q) + obj.edge_weight * edge_term(
                edge_difference_sums(pred, tars[k], mask, g, pos, obj.edge_weighting), obj, std)
        losses.append(float(loss_k.detach()))
        total = total + w * loss_k
        cur = torch.where(mask == 0, node_in, torch.cat([pred.detach() if detach else pred, node_in[..., C:]], dim=-1))
    total.backward()
    grads = {k: p.grad.clone() for k, p in sim.named_parameters() if p.grad is not None}
    return torch.stack(preds), float(total.detach()), grads, losses, (node_in.grad.detach().clone() if leaf_input else None)


_RUNS = {}


def oracle_runs(eng, key, ref, data, K, detach, obj, consistent=True, leaf_input=False):
    """fp32 on all threads, fp32 on one thread, fp64: once per configuration, shared, never modified."""
    if key not in _RUNS:
        later = later_targets(data[0], data[1], K)
        sw = [1.0] if K == 1 else [1.0, 0.5]
        with KinkMargin(ref) as km:
            pred32, loss32, g32, losses32, in32 = edge_oracle(eng, ref, data, later, sw, detach, obj, consistent, leaf_input)
        assert km.min >= MIN_MARGIN, (key, "the weight seed no longer keeps the ReLU inputs away from 0", km.min)
        nthreads = torch.get_num_threads()
        torch.set_num_threads(1)
        try:
            one = edge_oracle(eng, ref, data, later, sw, detach, obj, consistent, leaf_input)
        finally:
            torch.set_num_threads(nthreads)
        ref64 = ro.BSMS_Simulator(ref.cfg, dtype=torch.float64)
        ref64.load_state_dict(ref.state_dict())
        ref64.double()
        r64 = edge_oracle(eng, ref64, _f64(data), None if later is None else later.double(), sw, detach, obj, consistent, leaf_input)
        _RUNS[key] = dict(pred32=pred32, loss32=loss32, loss64=r64[1], g32=g32, g32_one=one[2], g64=r64[2], t32=0.0, t64=0.0, levels=key,
                          losses32=losses32, later=later, step_weights=sw, in32=in32, in32_one=one[4], in64=r64[4])
    return _RUNS[key]


def engine_of(eng, ref, **kw):
    mine = eng.BSMS_Simulator(ref.cfg)
    mine.load_state_dict(ref.state_dict())
    mine = mine.cuda()
    grads = eng.GradBuckets(list(mine.parameters()))
    return mine, grads, eng.FusedStep(mine, grads, **kw)


def autograd_route(eng, ref, gdata, obj, consistent=True, leaf_input=False):
    """What Trainer.get_loss(..).backward() runs: the model under autograd on the device, masked_loss with the level-0 graph."""
    auto = eng.BSMS_Simulator(ref.cfg)
    auto.load_state_dict(ref.state_dict())
    auto = auto.cuda()
    C = ref.cfg.out_dim
    if consistent:
        node_in, tar, mask, g = gdata[0], gdata[1], gdata[2], gdata[3][0][0]
        ni = node_in.clone().requires_grad_(True) if leaf_input else node_in
        pred = auto((ni, *gdata[1:]), True, False)
    else:
        node_in, tar, mask, g = gdata[0].x.unsqueeze(0), gdata[0].y.unsqueeze(0), gdata[0].mask.unsqueeze(0), gdata[0].edge_index
        ni, pred = node_in, auto(gdata, False, False)
    loss = eng.masked_loss(pred, tar, mask, obj, auto._targetNormalizer.std_with_epsilon(), g=g, pos=node_in[..., C:-1])
    loss.backward()
    torch.cuda.synchronize()
    return loss.detach(), {k: q.grad.detach().cpu() for k, q in auto.named_parameters() if q.grad is not None}, (ni.grad.detach() if leaf_input else None)


@pytest.mark.parametrize("name", list(CONFIGS))
@pytest.mark.parametrize("K,detach", [(1, False), (2, False), (2, True)])
def test_fused_step_follows_the_oracle(eng, graphs, K, detach, name):
    ref, data = oracle3(graphs)
    obj = objective_of(eng, name)
    r = dict(oracle_runs(eng, (name, K, detach), ref, data, K, detach, obj))
    mine, grads, step = engine_of(eng, ref, unroll=K, step_weights=r["step_weights"], detach=detach, objective=obj)
    gdata = _cuda(data)
    loss = step(gdata, True) if K == 1 else step(gdata, True, r["later"].cuda())
    torch.cuda.synchronize()
    preds = torch.stack([q.reshape(r["pred32"][0].shape) for q in step.predictions()]).cpu()
    got = step.step_losses().cpu().double()
    for k in range(K):
        e_p, e_l = rel_err(preds[k], r["pred32"][k]), abs(float(got[k]) - r["losses32"][k]) / r["losses32"][k]
        print(f"[{name} K={K} detach={detach}] step {k}: prediction {e_p:.2e}, loss {e_l:.2e} from the fp32 oracle")
        assert e_p <= 1e-5 and e_l <= 1e-5, (k, e_p, e_l)
    parts = step.loss_parts().cpu().double()
    assert abs(float(parts[0]) + obj.edge_weight * float(parts[1]) - float(loss)) <= 1e-6 * float(loss) and float(parts[1]) > 0
    r.update(pred=preds, loss=float(loss), gg={k: q.grad.detach().cpu() for k, q in mine.named_parameters() if q.requires_grad})
    check(r, f"{name} K={K} detach={detach}")
    if K == 1:                                                          # and the autograd route's gradients, to the same criterion
        a_loss, a_grads, _ = autograd_route(eng, ref, gdata, obj)
        assert abs(float(a_loss) - float(loss)) <= 1e-6 * float(loss)
        r.update(loss=float(a_loss), gg=a_grads)
        check(r, f"{name} autograd route")
        assert max(rel_err(a_grads[k], q.grad.detach().cpu()) for k, q in mine.named_parameters() if q.requires_grad) <= 1e-4


def blockdiag(eng, graphs):
    """The golden block-diagonal batch of tests/test_hip_unroll.py (del64 + del300 in one graph, 364 rows, depth 2)."""
    z = load_golden("blockdiag")
    es, ids = [z.t(f"cat/e{l}") for l in range(3)], [z.t(f"cat/ids{l}") for l in range(2)]
    pos = torch.cat([torch.tensor(graphs.np(f"{nm}/pos")[:, :2], dtype=torch.float32) for nm in ("del64", "del300")])
    n = pos.shape[0]
    gen = torch.Generator().manual_seed(5)
    state = torch.randn(n, 2, generator=gen)
    typ = (torch.rand(n, 1, generator=gen) < 0.2).float() * 4.0
    x, y, mask = torch.cat([state, pos, typ], -1), state + 0.1 * torch.randn(n, 2, generator=gen), (typ == 0).float()
    data = (x.unsqueeze(0), y.unsqueeze(0), mask.unsqueeze(0), es, ids)
    torch.manual_seed(26)
    ref = ro.BSMS_Simulator(ro.make_cfg(2, 32, 2, 2, 2))
    ref(data, False, True)
    sizes = [n, ids[0].numel(), ids[1].numel()]
    levels = [eng.LevelData(es[l], sizes[l], face=ids[l] if l < 2 else None, x=x if l == 0 else None, y=y if l == 0 else None,
                            mask=mask if l == 0 else None).to("cuda") for l in range(3)]
    return ref, data, levels


@pytest.mark.parametrize("name", list(CONFIGS))
def test_variable_mesh_batch_follows_the_oracle(eng, graphs, name):
    ref, data, levels = blockdiag(eng, graphs)
    obj = objective_of(eng, name, C=2)
    r = dict(oracle_runs(eng, ("blockdiag", name), ref, data, 1, False, obj, consistent=False))
    mine, grads, step = engine_of(eng, ref, objective=obj)
    loss = step(levels, False)
    torch.cuda.synchronize()
    assert step._buf["esums"].shape == (1, 5)                           # ONE segment of 364 rows through the union's plan
    pred = step.prediction().reshape(r["pred32"][0].shape).cpu()
    assert rel_err(pred, r["pred32"][0]) <= 1e-5 and abs(float(loss) - r["loss32"]) <= 1e-5 * r["loss32"]
    r.update(pred=pred.unsqueeze(0), loss=float(loss), gg={k: q.grad.detach().cpu() for k, q in mine.named_parameters() if q.requires_grad})
    check(r, f"blockdiag {name}")
    a_loss, a_grads, _ = autograd_route(eng, ref, levels, obj, consistent=False)
    assert abs(float(a_loss) - float(loss)) <= 1e-6 * float(loss)
    r.update(loss=float(a_loss), gg=a_grads)
    check(r, f"blockdiag {name} autograd route")


# ------------------------------------------------------------------------------------------------ the step's forms
def test_graph_replay_with_changing_targets_equals_eager(eng, graphs):
    sim, data = _golden_model(eng, graphs)
    obj = eng.Objective("normalized", "rmse", [2.0, 0.5], edge_weight=0.2, edge_weighting="quotient")
    grads = eng.GradBuckets(list(sim.parameters()))
    eager, gstep = eng.FusedStep(sim, grads, objective=obj), eng.FusedStep(sim, grads, use_graph=True, objective=obj)
    seen = set()
    for shift in (0.0, 0.25, 0.0):
        batch = (data[0], data[1] + shift * data[2], *data[2:])
        l0 = eager(batch, True)
        flat0, pred0, parts0 = grads.flat.clone(), eager.prediction().clone(), eager.loss_parts()
        grads.flat.fill_(float("nan"))
        l1 = gstep(batch, True)
        assert torch.equal(l1, l0) and torch.equal(grads.flat, flat0) and torch.equal(gstep.prediction(), pred0)
        assert torch.equal(gstep.loss_parts(), parts0) and bool(torch.isfinite(flat0).all())
        seen.add(float(l0))
    assert gstep._graphs is not None and len(seen) == 2


def test_recompute_frozen_processor_and_bf16(eng, graphs):
    ref, data = oracle3(graphs)
    gdata = _cuda(data)
    obj = objective_of(eng, "physical/rmse+quotient")
    later = later_targets(gdata[0], gdata[1], 2)
    res = {}
    for rec in (False, True):
        mine, grads, step = engine_of(eng, ref, unroll=2, step_weights=[1.0, 0.5], objective=obj, recompute=rec, input_grad=True)
        loss = step(gdata, True, later)
        res[rec] = (loss.clone(), grads.flat.clone(), step.input_grad().clone(), step.loss_parts())
    assert all(torch.equal(a, b) for a, b in zip(res[False], res[True]))                        # recompute: bit-equal
    # a frozen processor: the data gradients keep their bits
    mine, grads, step = engine_of(eng, ref, objective=obj, input_grad=True)
    l0 = step(gdata, True)
    gin0 = step.input_grad().clone()
    frozen = eng.BSMS_Simulator(ref.cfg)
    frozen.load_state_dict(ref.state_dict())
    frozen = frozen.cuda()
    for q in frozen.process.parameters():
        q.requires_grad_(False)
    fg = eng.GradBuckets([q for q in frozen.parameters() if q.requires_grad])
    fstep = eng.FusedStep(frozen, fg, objective=obj, input_grad=True)
    l1 = fstep(gdata, True)
    assert torch.equal(l1, l0) and torch.equal(fstep.input_grad(), gin0)
    for (k, a), (_, b) in zip(mine.named_parameters(), frozen.named_parameters()):
        if b.requires_grad:
            assert torch.equal(a.grad, b.grad), k
    # one bf16 step runs and is deterministic (the bf16 kernels need D = 128: the two-channel "split" shape of tests/test_hip_unroll.py)
    ref2, data2 = make_oracle("split", graphs)
    gdata2, obj2 = _cuda(data2), objective_of(eng, "physical/rmse+quotient", C=2)
    outs = []
    for prec in ("bf16", "bf16", "f32"):
        mine, grads, step = engine_of(eng, ref2, objective=obj2)
        mine.process.precision = prec
        outs.append((step(gdata2, True).clone(), grads.flat.clone(), step.loss_parts()))
    assert all(torch.equal(a, b) for a, b in zip(outs[0], outs[1])) and bool(torch.isfinite(outs[0][1]).all())
    assert abs(float(outs[0][0]) - float(outs[2][0])) <= 2e-2 * float(outs[2][0]) and not torch.equal(outs[0][1], outs[2][1])


def test_input_grad_equals_the_autograd_route(eng, graphs):
    """The "difference" weighting: the term does not depend on the positions, so the oracle's node_in.grad is the whole gradient (the
    gradient of the quotient's 1 / l^2 with respect to the positions is not formed, on either route of the device)."""
    ref, data = oracle3(graphs)
    obj = objective_of(eng, "normalized/mse+difference")
    r = oracle_runs(eng, ("input_grad",), ref, data, 1, False, obj, leaf_input=True)
    gdata = _cuda(data)
    mine, grads, step = engine_of(eng, ref, objective=obj, input_grad=True)
    step(gdata, True)
    got = step.input_grad().clone()
    step.input_grad().fill_(float("nan"))
    step(gdata, True)
    assert torch.equal(step.input_grad(), got)                          # deterministic, and the static buffer is overwritten
    _, _, auto = autograd_route(eng, ref, gdata, obj, leaf_input=True)
    dist_ = lambda a, b: float((a.double() - b.double()).abs().max() / b.double().abs().max())
    yard = max(dist_(r["in32"], r["in64"]), dist_(r["in32_one"], r["in64"]))
    for what, g in (("fused step", got.cpu()), ("autograd route", auto.cpu())):
        e = dist_(g, r["in64"])
        print(f"[input_grad] {what}: {e:.2e} from fp64; the fp32 oracle {yard:.2e} (factor 1.5)")
        assert e <= max(1e-5, 1.5 * yard), (what, e, yard)
    assert dist_(got.cpu(), auto.cpu()) <= 1e-5


# ------------------------------------------------------------------------------------------------ 4: two ranks, the Trainer, the calls
DP_OBJ = dict(space="normalized", kind="mse", channel_weights=[1.0, 3.0], edge_weight=0.2, edge_weighting="quotient")


def _worker(rank, world, port, out_path):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    torch.cuda.set_device(0)
    from conftest import Golden
    import bsms_gnn_amd as eng
    z, graphs = Golden("sim"), Golden("graphs")
    es, ids = graphs.levels("del300")
    torch.manual_seed(50 + rank)
    sim = eng.BSMS_Simulator(ro.make_cfg(2, 32, 3, 3, 2))
    if rank == 0:
        sim.load_state_dict(z.state_dict())
    sim = sim.cuda()
    c, sl = (lambda t: t.cuda()), slice(rank, rank + 1)
    data = (c(z.t("node_in")[sl]), c(z.t("tar")[sl]), c(z.t("mask")[sl]), [c(e.unsqueeze(0)) for e in es], [c(i.unsqueeze(0)) for i in ids])
    kw = dict(DP_OBJ)
    engine = eng.DataParallel(sim, bucket_bytes=64 << 10, objective=eng.Objective(kw.pop("space"), kw.pop("kind"), kw.pop("channel_weights"), **kw))
    loss = engine.step_loss_backward(data, True)
    torch.cuda.synchronize()
    torch.save({"loss": loss.detach().cpu(), "flat": engine.grads.flat.cpu(), "parts": engine.fused.loss_parts().cpu()}, f"{out_path}.{rank}")
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.timeout(300)
def test_two_ranks_equal_the_single_process_step(eng, graphs, tmp_path):
    """Two gloo ranks x B = 1 against the B = 2 step: ONE all-reduce of the widened fp64 row, so ME and DE are the batch's."""
    port = 29900 + (os.getpid() + 7) % 2000
    out = str(tmp_path / "res")
    mp.start_processes(_worker, args=(2, port, out), nprocs=2, join=True, start_method="spawn")
    r0, r1 = torch.load(out + ".0"), torch.load(out + ".1")
    assert torch.equal(r0["flat"], r1["flat"]) and torch.equal(r0["loss"], r1["loss"]) and torch.equal(r0["parts"], r1["parts"])
    sim, data = _golden_model(eng, graphs)
    kw = dict(DP_OBJ)
    obj = eng.Objective(kw.pop("space"), kw.pop("kind"), kw.pop("channel_weights"), **kw)
    grads = eng.GradBuckets(list(sim.parameters()))
    step = eng.FusedStep(sim, grads, objective=obj)
    loss = step(data, True)
    assert abs(float(r0["loss"]) - float(loss)) < 1e-5 * abs(float(loss))
    assert rel_err(r0["parts"], step.loss_parts().cpu()) < 1e-5 and rel_err(r0["flat"], grads.flat.cpu()) < 2e-5
    # and the oracle's B = 2 step has that loss
    ref = ro.BSMS_Simulator(ro.make_cfg(2, 32, 3, 3, 2))
    ref.load_state_dict(load_golden("sim").state_dict())
    cpu = tuple(_cpu(t) for t in data)
    want = edge_oracle(eng, ref, cpu, None, [1.0], False, obj)[1]
    assert abs(float(r0["loss"]) - want) <= 1e-5 * want


def _cpu(obj):
    return type(obj)(_cpu(o) for o in obj) if isinstance(obj, (list, tuple)) else obj.cpu()


def _trainer(eng, graphs, extra):
    ref, data = oracle3(graphs)
    D, H, depth = SHAPE3
    model_cfg = SimpleNamespace(out_dim=3, latent_dim=D, hidden_layer=H, unet_depth=depth, pos_dim=2, consistent_mesh=True, accumulation_steps=1, **extra)
    opt_cfg = SimpleNamespace(peak_lr=1e-3, weight_decay=1e-4, warmup_steps=2, decay_steps=20, gnorm_clip=1.0)
    torch.manual_seed(0)
    mine = eng.BSMS_Simulator(model_cfg)
    return eng.Trainer(mine, model_cfg, opt_cfg), data


def test_trainer_reads_the_keys_trains_and_round_trips(eng, graphs, tmp_path):
    keys = dict(loss_space="normalized", loss_kind="mse", loss_edge_weight=0.2, loss_edge_weighting="quotient")
    runs = []
    for _ in range(2):
        tr, data = _trainer(eng, graphs, keys)
        losses = [tr.iter(data) for _ in range(4)]                      # the warm-up, then three optimisation iterations
        runs.append(([float(l) for l in losses[1:]], tr.optimizer.flat_p.clone()))
    assert tr.objective == eng.Objective("normalized", "mse", edge_weight=0.2, edge_weighting="quotient") and tr.dp.fused._edge
    assert runs[0][0] == runs[1][0] and torch.equal(runs[0][1], runs[1][1]) and all(math.isfinite(l) for l in runs[0][0])
    assert runs[0][0][2] != runs[0][0][0]                               # the parameters move (the first step has the warm-up's zero rate)
    # get_loss reports J: masked_loss with the level-0 graph and the mesh positions of its own prediction
    pred, gdata = tr.get_pred(data).detach(), _cuda(data)
    want = eng.masked_loss(pred, gdata[1], gdata[2], tr.objective, tr.model._targetNormalizer.std_with_epsilon(), g=gdata[3][0][0], pos=gdata[0][..., 3:-1])
    assert torch.equal(tr.get_loss(data).detach(), want)
    plain = eng.masked_loss(pred, gdata[1], gdata[2], eng.Objective("normalized", "mse"), tr.model._targetNormalizer.std_with_epsilon())
    assert float(want) > float(plain)
    nxt = float(tr.get_loss(data))
    tr.save(str(tmp_path))
    tr2, _ = _trainer(eng, graphs, keys)
    tr2.restore(str(tmp_path), tr.train_step)
    assert float(tr2.get_loss(data)) == nxt
    assert float(tr2.iter(data)) == float(tr.iter(data))


def test_which_entries_a_step_calls(eng, graphs, monkeypatch):
    from bsms_gnn_amd import _abi
    real = _abi.lib()
    calls = []

    class Count:
        def __getattr__(self, name):
            calls.append(name)
            return getattr(real, name)

    real_ext = _abi.ext()

    class CountExt:
        def __getattr__(self, name):
            calls.append(name)
            return getattr(real_ext, name)

    monkeypatch.setattr(_abi, "lib", lambda: Count())
    monkeypatch.setattr(_abi, "ext", lambda: CountExt())
    new = {"bsms_edge_diff_sums", "bsms_edge_diff_fold", "bsms_sim_edge_objective_bwd", "bsms_edge_diff_work_bytes"}
    sim, data = _golden_model(eng, graphs)
    grads = eng.GradBuckets(list(sim.parameters()))
    outs = []
    for _ in range(2):                                                  # a step without an edge term, and a second built the same way
        grads.flat.fill_(float("nan"))
        step = eng.FusedStep(sim, grads, objective=eng.Objective("normalized", "mse", [1.0, 3.0]))
        outs.append((step(data, True).clone(), grads.flat.clone(), step.prediction().clone()))
        assert tuple(step._buf["osums"].shape) == (7,) and "esums" not in step._buf and "parts" not in step._buf
    assert not new & set(calls) and "bsms_sim_objective_bwd" in calls
    assert all(torch.equal(a, b) for a, b in zip(*outs))
    default = eng.FusedStep(sim, grads)
    default(data, True)
    assert not new & set(calls)
    del calls[:]
    step = eng.FusedStep(sim, grads, objective=eng.Objective("normalized", "mse", [1.0, 3.0], edge_weight=0.2))
    loss = step(data, True)
    assert tuple(step._buf["osums"].shape) == (10,) and tuple(step._buf["esums"].shape) == (2, 5)
    assert "bsms_sim_objective_bwd" not in calls and new <= set(calls)
    assert [c for c in calls if c in new and c != "bsms_edge_diff_work_bytes"] == ["bsms_edge_diff_sums", "bsms_edge_diff_fold", "bsms_sim_edge_objective_bwd"]
    assert float(loss) > float(outs[0][0])                              # J = L + lambda T with T > 0
