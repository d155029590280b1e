"""GPU: node-weighted objectives -- bsms_error_sums_w and bsms_sim_objective_bwd_w on their own (bit-equal to the
unweighted entries under unit and binary weights, NumPy fp64 under real ones, exact under a power-of-two rescaling), the fused step
with `Objective(node_weighted=True)` against the CPU oracle under autograd with the weighted loss restated here in torch, what must
not change (unit weights, the flag off, determinism, graph replay), every accelerated form of the step against the plain weighted
step, and the bank and the Trainer.

The definition (restated in `weighted_loss`): d = fl32(pred - tar), mu = m * omega, M = sum mu, SE_c = sum mu d_c^2 (fp64), a_c and
the rest as tests/test_hip_objective.py::loss_def.

Meshes: the 300-node `del300` golden batch (B = 2, C = 2) with the models of tests/test_hip_unroll.py (`make_oracle`: seeds chosen
for their ReLU margins over the unrolled forward, which no loss changes), and the golden block-diagonal batch of 364 rows.

Tolerances: the sums 1e-12 (tests/test_hip_eval.py::SUM_TOL: fp64 sums of non-negative terms in another order), the backward
kernel 1e-6 (tests/test_hip_objective.py::KERNEL_TOL), the step against the oracle 1e-5 on predictions and losses and the three-way
criterion of tests/test_hip_fullsize.py::check on the gradients."""
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from conftest import ROOT, load_golden, rel_err
from oracle import bsms_oracle as ro
from test_eval_host import rel
from test_hip_accumulate import bit_equal, engine_model, part, three_way
from test_hip_eval import SUM_TOL
from test_hip_fullsize import check
from test_hip_objective import KERNEL_TOL, KIND_ID, PAIRS, SPACE_ID, _kernel_inputs, _std
from test_hip_unroll import _cuda, _f64, later_targets, make_oracle

pytestmark = pytest.mark.gpu

GUARD = 64                   # NaNs on both sides of every operand: a read outside it poisons the result


@pytest.fixture(scope="module")
def eng():
    import bsms_gnn_amd as eng
    return eng


def guarded(host):
    """`host` on the device, in the middle of a buffer of NaNs."""
    flat = host.reshape(-1)
    buf = torch.full((flat.numel() + 2 * GUARD,), float("nan"), dtype=host.dtype, device="cuda")
    buf[GUARD:GUARD + flat.numel()] = flat.cuda()
    return buf[GUARD:GUARD + flat.numel()].view(host.shape)


def ptr(t):
    return None if t is None else t.data_ptr()


def spread_weights(gen, *shape):
    """Positive weights over about five decades, like the cell sizes of a graded mesh."""
    return torch.exp(2.5 * torch.randn(*shape, generator=gen)).float()


# ------------------------------------------------------------------------------------------------ the sums, through the C ABI
SENTINEL = -7.0


def raw_sums(eng, pred, tar, mask, weights, S, n, C, mask_stride, weight_stride=None):
    """One call of bsms_error_sums (weights None) or bsms_error_sums_w on guarded device operands; the output sits between sentinels."""
    L = eng._abi.lib()
    ncol = 1 + 3 * C
    out = torch.full((S * ncol + 16,), SENTINEL, dtype=torch.float64, device="cuda")
    sums = out[8:8 + S * ncol]
    work = torch.empty(L.bsms_error_sums_work_bytes(S, n), dtype=torch.uint8, device="cuda")
    s = torch.cuda.current_stream().cuda_stream
    if weights is None:
        rc = L.bsms_error_sums(ptr(pred), ptr(tar), ptr(mask), S, n, C, n, n, mask_stride, ptr(sums), ptr(work), s)
    else:
        rc = L.bsms_error_sums_w(ptr(pred), ptr(tar), ptr(mask), ptr(weights), S, n, C, n, n, mask_stride, weight_stride, ptr(sums), ptr(work), s)
    eng._abi.check(rc, "error sums")
    torch.cuda.synchronize()
    assert bool((out[:8] == SENTINEL).all()) and bool((out[8 + S * ncol:] == SENTINEL).all()), "wrote outside the sums"
    return sums.view(S, ncol).clone()


def sum_operands(S, n, C, seed):
    gen = torch.Generator().manual_seed(seed)
    pred, tar = torch.randn(S, n, C, generator=gen), 3.0 * torch.randn(S, n, C, generator=gen)
    mask = (torch.rand(S, n, generator=gen) < 0.7).float()
    return gen, pred, tar, mask


def np_weighted_sums(pred, tar, mask, w):
    """[S, 1+3C] fp64: tests/test_eval_host.py::np_error_sums with mu = double(mask) * double(weight) in the mask's place."""
    p, t = pred.numpy(), tar.numpy()
    S, n, _ = p.shape
    d = (p - t).astype(np.float32).astype(np.float64)
    td = t.astype(np.float64)
    mu = (np.broadcast_to(mask.numpy().reshape(-1, n), (S, n)).astype(np.float64) * np.broadcast_to(w.numpy().reshape(-1, n), (S, n)).astype(np.float64))[:, :, None]
    return np.concatenate([mu.sum(1), (mu * (d * d)).sum(1), (mu * np.abs(d)).sum(1), (mu * (td * td)).sum(1)], axis=1)


@pytest.mark.parametrize("S", [1, 3])
@pytest.mark.parametrize("C", [1, 3, 8])
@pytest.mark.parametrize("n", [0, 1, 255, 256, 257, 1023, 1024, 1025, 2049])
def test_unit_and_binary_weights_are_the_unweighted_sums_bit_for_bit(eng, n, C, S):
    """Items 1 and 2.  omega == 1: the sums of bsms_error_sums; omega in {0, 1}: those of bsms_error_sums under the mask m * omega,
    with rows of either kind (m = 0, omega = 1 and the reverse) wherever there are at least two rows.  Shared and per-segment
    strides of mask and weights."""
    gen, pred, tar, mask = sum_operands(S, n, C, 1000 * n + 10 * C + S)
    binary = (torch.rand(S, n, generator=gen) < 0.6).float()
    if n >= 2:
        mask[:, 0], binary[:, 0], mask[:, 1], binary[:, 1] = 0.0, 1.0, 1.0, 0.0
    dp, dt, dm, ones, db = (guarded(t) for t in (pred, tar, mask, torch.ones(S, n), binary))
    for what, ms, ws in (("per segment", n, n), ("shared weights", n, 0), ("shared mask", 0, n), ("both shared", 0, 0)):
        plain = raw_sums(eng, dp, dt, dm, None, S, n, C, ms)
        unit = raw_sums(eng, dp, dt, dm, ones, S, n, C, ms, ws)
        assert bit_equal(unit, plain), ("unit", what)
        got = raw_sums(eng, dp, dt, dm, db, S, n, C, ms, ws)
        # the mask m * omega of segment s: its own mask or segment 0's, times its own weights or segment 0's
        prod = (mask if ms else mask[:1].expand(S, n)) * (binary if ws else binary[:1].expand(S, n))
        want = raw_sums(eng, dp, dt, guarded(prod.contiguous()), None, S, n, C, n)
        assert bit_equal(got, want), ("binary", what)
        assert bool(torch.isfinite(got).all())
    if n == 0:
        assert bool((plain == 0).all())


@pytest.mark.parametrize("n,C,S", [(1, 3, 1), (257, 1, 3), (1025, 3, 3), (2049, 8, 2)])
def test_real_weights_against_numpy_fp64(eng, n, C, S):
    """Item 3: weights over several decades against NumPy fp64 on the same fp32 d; bit-identical from run to run; a segment's sums do
    not depend on the other segments of the launch; and `ops.error_sums(weights=)` is the same call."""
    gen, pred, tar, mask = sum_operands(S, n, C, 77 * n + C + S)
    w = spread_weights(gen, S, n)
    assert float(w.max() / w.min()) > 1e3 or n == 1
    dp, dt, dm, dw = (guarded(t) for t in (pred, tar, mask, w))
    for what, ws, wn in (("per segment", n, w), ("shared", 0, w[:1])):
        got = raw_sums(eng, dp, dt, dm, dw, S, n, C, n, ws)
        err = rel(got.cpu().numpy(), np_weighted_sums(pred, tar, mask, wn))
        print(f"[n={n} C={C} S={S} {what}] worst relative distance to NumPy fp64: {err:.2e}")
        assert err <= SUM_TOL, (what, err)
        assert bit_equal(got, raw_sums(eng, dp, dt, dm, dw, S, n, C, n, ws)), what
    last = S - 1
    alone = raw_sums(eng, guarded(pred[last:]), guarded(tar[last:]), guarded(mask[last:]), guarded(w[last:]), 1, n, C, n, n)
    assert bit_equal(alone[0], raw_sums(eng, dp, dt, dm, dw, S, n, C, n, n)[last])
    per = eng.error_sums(dp, dt, dm, n, weights=dw)
    assert bit_equal(per, raw_sums(eng, dp, dt, dm, dw, S, n, C, n, n))
    assert bit_equal(eng.error_sums(dp, dt, dm, n, weights=dw[0]), raw_sums(eng, dp, dt, dm, dw, S, n, C, n, 0))
    assert bit_equal(eng.error_sums(dp, dt, dm, n), raw_sums(eng, dp, dt, dm, None, S, n, C, n))       # None: the existing call
    with pytest.raises(ValueError):
        eng.error_sums(dp, dt, dm, n, weights=torch.ones(n + 1, device="cuda"))


# ------------------------------------------------------------------------------------------------ the backward entry
def bwd_call(eng, ops, R, C, sums, cw, space, kind, w_step, carried, weights=None, period=None, outs=None):
    """bsms_sim_objective_bwd (weights None) or bsms_sim_objective_bwd_w into sentinel-filled outputs; returns (rc, outputs)."""
    L = eng._abi.lib()
    dp, dt, dm, do, di, dgn, dgi = ops
    if outs is None:
        outs = (torch.full((1,), -1.0, device="cuda"), torch.full((C,), -1.0, device="cuda"), torch.full((R, C), 7.0, device="cuda"),
                torch.full((R, C), 7.0, device="cuda"))
    loss, chan, gp, gnp = outs
    tail = (R, C, *map(ptr, do), *map(ptr, di), ptr(sums), ptr(cw), space, kind, w_step, ptr(dgn) if carried else None,
            ptr(dgi) if carried else None, ptr(loss), ptr(chan), ptr(gp), ptr(gnp), torch.cuda.current_stream().cuda_stream)
    if weights is None and period is None:
        rc = L.bsms_sim_objective_bwd(ptr(dp), ptr(dt), ptr(dm), *tail)
    else:
        rc = L.bsms_sim_objective_bwd_w(ptr(dp), ptr(dt), ptr(dm), ptr(weights), period, *tail)
    torch.cuda.synchronize()
    return rc, outs


def bwd_operands(R, C):
    pred, tar, mask, o_stats, i_stats, g_next, g_nin, cw = _kernel_inputs(R, C, False)
    ops = (guarded(pred), guarded(tar), guarded(mask), [t.cuda() for t in o_stats], [t.cuda() for t in i_stats], guarded(g_next), guarded(g_nin))
    return pred, tar, mask, o_stats, i_stats, g_next, g_nin, cw, ops


@pytest.mark.parametrize("R", [1, 255, 256, 257, 1025])
def test_backward_with_unit_weights_is_the_unweighted_entry_bit_for_bit(eng, R):
    """Item 5a: all four (space, kind), unit and random channel weights, with and without a carried pair (step weight 0.375 with it),
    C = 3; the sums are the unweighted ones, which unit weights leave as they are."""
    C = 3
    pred, tar, mask, _, _, _, _, cw, ops = bwd_operands(R, C)
    sums = eng.error_sums(ops[0].reshape(1, R, C), ops[1].reshape(1, R, C), ops[2].reshape(1, R, 1), R)
    ones, dcw = guarded(torch.ones(R)), cw.cuda()
    for space, kind in PAIRS:
        for w_dev in (None, dcw):
            for carried, w_step in ((False, 1.0), (True, 0.375)):
                rc0, want = bwd_call(eng, ops, R, C, sums, w_dev, SPACE_ID[space], KIND_ID[kind], w_step, carried)
                rc1, got = bwd_call(eng, ops, R, C, sums, w_dev, SPACE_ID[space], KIND_ID[kind], w_step, carried, ones, R)
                assert rc0 == 0 and rc1 == 0
                assert all(bit_equal(a, b) for a, b in zip(got, want)), (space, kind, w_dev is not None, carried)
                assert bool(torch.isfinite(got[3]).all())


@pytest.mark.parametrize("R,C", [(1, 3), (257, 1), (1025, 3), (1025, 8)])
def test_backward_with_real_weights_against_numpy(eng, R, C):
    """Item 5b: tests/test_hip_objective.py::test_objective_bwd_kernel_against_numpy with mu = m * omega in the loss term -- and m
    alone in the carry and on the way out."""
    pred, tar, mask, o_stats, i_stats, g_next, g_nin, cw, ops = bwd_operands(R, C)
    gen = torch.Generator().manual_seed(R + C)
    omega = spread_weights(gen, R)
    dw = guarded(omega)
    D = (pred - tar).double().numpy()
    Mk, Om = mask.double().numpy()[:, None], omega.double().numpy()[:, None]
    mu = Mk * Om
    M_, SE = float(mu.sum()), (mu * D * D).sum(0)
    sums = torch.tensor(np.concatenate([[M_], SE, np.full(2 * C, np.nan)]), dtype=torch.float64).cuda()
    std_o, std_i = _std(o_stats), _std(i_stats)
    with np.errstate(invalid="ignore"):
        carry_full = np.where(Mk != 0, g_next.double().numpy() + g_nin.double().numpy()[:, :C] / std_i[:C], 0.0)
    worst = 0.0
    for space, kind in PAIRS:
        for w_dev, w_np in ((None, np.ones(C)), (cw.cuda(), cw.numpy())):
            a = w_np / std_o ** 2 if space == "normalized" else w_np
            terms = a * SE / (M_ * C)
            loss = terms.sum() if kind == "mse" else np.sqrt(terms.sum())
            G = 2.0 / (M_ * C) if kind == "mse" else 1.0 / (loss * M_ * C)
            for carried, w_step in ((False, 1.0), (True, 0.375)):
                rc, (loss_g, chan_g, gp_g, gnp_g) = bwd_call(eng, ops, R, C, sums, w_dev, SPACE_ID[space], KIND_ID[kind], w_step, carried, dw, R)
                assert rc == 0
                want_gp = w_step * (G * a[None, :] * mu * D) + (carry_full if carried else 0.0)
                want_gnp = want_gp * Mk * std_o
                tag = (space, kind, w_dev is not None, carried)
                assert abs(float(loss_g) - loss) <= KERNEL_TOL * loss, tag
                assert np.abs(chan_g.cpu().double().numpy() - terms).max() <= KERNEL_TOL * terms.max(), tag
                for out, want in ((gp_g, want_gp), (gnp_g, want_gnp)):
                    err = np.abs(out.cpu().double().numpy() - want).max() / np.abs(want).max()
                    worst = max(worst, err)
                    assert err <= KERNEL_TOL, (tag, err)
                    assert bool((out.cpu()[mask == 0] == 0).all()), tag
    print(f"\n[R={R} C={C}] worst relative distance to the fp64 restatement: {worst:.2e}")


def test_shared_weights_equal_the_tiled_ones(eng):
    """Item 5c: weight_period = N against the same weights tiled to [R], bit for bit (R = 3 * 257, a ragged last block)."""
    N, B, C = 257, 3, 3
    R = B * N
    _, _, _, _, _, _, _, cw, ops = bwd_operands(R, C)
    omega = spread_weights(torch.Generator().manual_seed(3), N)
    tiled = guarded(omega.repeat(B))
    sums = eng.error_sums(ops[0].reshape(1, R, C), ops[1].reshape(1, R, C), ops[2].reshape(1, R, 1), R, weights=tiled)
    for space, kind in PAIRS:
        _, want = bwd_call(eng, ops, R, C, sums, None, SPACE_ID[space], KIND_ID[kind], 0.375, True, tiled, R)
        rc, got = bwd_call(eng, ops, R, C, sums, None, SPACE_ID[space], KIND_ID[kind], 0.375, True, guarded(omega), N)
        assert rc == 0 and all(bit_equal(a, b) for a, b in zip(got, want)), (space, kind)


@pytest.mark.parametrize("k", [-20, 7])
def test_a_power_of_two_rescaling_changes_nothing_but_the_sums(eng, k):
    """Item 4: omega -> 2^k omega scales every sum exactly and leaves loss_out, chan_out, g_pred and grad_norm_pred bit-equal."""
    R, C = 1025, 3
    _, _, _, _, _, _, _, cw, ops = bwd_operands(R, C)
    omega = spread_weights(torch.Generator().manual_seed(9), R)
    scaled = omega * 2.0 ** k
    assert bool(torch.isfinite(scaled).all()) and float(scaled.min()) > 2.0 ** -100         # neither overflow nor subnormals
    d0, d1 = guarded(omega), guarded(scaled)
    views = (ops[0].reshape(1, R, C), ops[1].reshape(1, R, C), ops[2].reshape(1, R, 1))
    s0, s1 = eng.error_sums(*views, R, weights=d0), eng.error_sums(*views, R, weights=d1)
    assert bit_equal(s1, s0 * 2.0 ** k) and float(s0[0, 0]) > 0
    for space, kind in PAIRS:
        _, want = bwd_call(eng, ops, R, C, s0, cw.cuda(), SPACE_ID[space], KIND_ID[kind], 0.375, True, d0, R)
        _, got = bwd_call(eng, ops, R, C, s1, cw.cuda(), SPACE_ID[space], KIND_ID[kind], 0.375, True, d1, R)
        assert all(bit_equal(a, b) for a, b in zip(got, want)), (space, kind)


def test_backward_refusals_touch_no_output(eng):
    """Item 5d: NULL weights, a period that does not divide R (or is < 1), and bad C / space / kind in the documented order -- C
    before space and kind, those before any pointer; nothing is launched, so the sentinels stay."""
    R, C = 257, 3
    _, _, _, _, _, _, _, _, ops = bwd_operands(R, C)
    sums = torch.ones(1 + 3 * C, dtype=torch.float64, device="cuda")
    dw = guarded(torch.ones(R))
    outs = None
    for want_rc, kw in ((-1, dict(weights=None, period=R)), (-1, dict(weights=dw, period=7)), (-1, dict(weights=dw, period=0)),
                        (-1, dict(weights=dw, period=2 * R)), (-3, dict(weights=None, period=0, C=9, space=5)),
                        (-3, dict(weights=None, period=0, space=2)), (-3, dict(weights=None, period=0, kind=-1))):
        rc, outs = bwd_call(eng, ops, R, kw.get("C", C), sums, None, kw.get("space", 0), kw.get("kind", 0), 1.0, False, kw["weights"], kw["period"], outs)
        assert rc == want_rc, kw
        if "C" in kw:
            assert b"C=9" in eng._abi.lib().bsms_last_error()
    loss, chan, gp, gnp = outs
    assert float(loss) == -1.0 and bool((chan == -1.0).all()) and bool((gp == 7.0).all()) and bool((gnp == 7.0).all())
    L = eng._abi.lib()
    assert L.bsms_error_sums_w(ptr(ops[0]), ptr(ops[1]), ptr(ops[2]), None, 1, R, C, R, R, R, R, ptr(sums), ptr(sums), None) == -1


# ------------------------------------------------------------------------------------------------ the definition, in torch
def weighted_loss(pred, tar, mask, nw, space, kind, cw, std):
    """tests/test_hip_objective.py::loss_def with mu = m * omega in the mask's place; `nw` is [N], [B, N] or flat [rows]."""
    C = pred.shape[-1]
    d = (pred - tar).double()
    w = nw.double()
    mu = mask.double().reshape(*pred.shape[:-1], 1) * w.reshape(*w.shape, 1)
    M, SE = mu.sum(), (mu * d * d).reshape(-1, C).sum(0)
    a = torch.ones(C, dtype=torch.float64) if cw is None else torch.tensor(cw, dtype=torch.float64)
    if space == "normalized":
        a = a / std.double() ** 2
    Q = (a * SE / (M * C)).sum()
    return Q if kind == "mse" else torch.sqrt(Q)


def weighted_oracle(sim, data, later, step_weights, detach, objective, nw, consistent=True):
    """tests/test_hip_unroll.py::unrolled_oracle with the weighted loss of the definition."""
    node_in, tar, mask, m_gs, m_ids = data
    C = tar.shape[-1]
    tars = [tar, *(later if later is not None else [])]
    std = sim._targetNormalizer.std_with_epsilon().detach()
    sim.zero_grad(set_to_none=True)
    cur, preds, total = node_in, [], 0.0
    for k, w in enumerate(step_weights):
        pred = sim((cur, tars[k], mask, m_gs, m_ids), consistent, False)
        preds.append(pred.detach())
        total = total + w * weighted_loss(pred, tars[k], mask, nw, *objective, std)
        cur = torch.where(mask == 0, node_in, torch.cat([pred.detach() if detach else pred, node_in[..., C:]], dim=-1))
    total.backward()
    return torch.stack(preds), float(total.detach()), {k: q.grad.clone() for k, q in sim.named_parameters() if q.grad is not None}


def node_weights_for(kind, B=2, N=300):
    gen = torch.Generator().manual_seed(41)
    return spread_weights(gen, N) if kind == "shared" else spread_weights(gen, B, N)


def objective_of(eng, obj):
    return eng.Objective(*obj, node_weighted=True)


# ------------------------------------------------------------------------------------------------ 6: the fused step against the oracle
ORACLE_CASES = [(("physical", "rmse", None), 1, False, "shared"), (("normalized", "mse", [1.0, 3.0]), 1, False, "per-sample"),
                (("physical", "rmse", None), 2, False, "per-sample"), (("normalized", "mse", [1.0, 3.0]), 2, False, "shared"),
                (("physical", "rmse", None), 2, True, "shared"), (("normalized", "mse", [1.0, 3.0]), 2, True, "per-sample")]


@pytest.mark.parametrize("obj,K,detach,wkind", ORACLE_CASES, ids=[f"{o[0]}-{o[1]}-K{K}{'-detached' if d else ''}-{w}" for o, K, d, w in ORACLE_CASES])
def test_weighted_step_follows_the_oracle(eng, graphs, obj, K, detach, wkind):
    ref, data = make_oracle("ring", graphs)
    nw = node_weights_for(wkind)
    later, sw = later_targets(data[0], data[1], K), ([1.0] if K == 1 else [1.0, 0.5])
    key = ("node-weighted", obj[0], obj[1], K, detach, wkind)
    r = three_way(ref, key, lambda sim, d, lat: weighted_oracle(sim, d, lat, sw, detach, obj, nw), data, later)
    mine, grads = engine_model(eng, ref)
    step = eng.FusedStep(mine, grads, unroll=K, step_weights=sw, detach=detach, objective=objective_of(eng, obj))
    args = (_cuda(data), True) if K == 1 else (_cuda(data), True, later.cuda())
    loss = step(*args, node_weights=nw.cuda())
    torch.cuda.synchronize()
    preds = torch.stack([q.reshape(r["pred32"][0].shape) for q in step.predictions()]).cpu()
    std = ref._targetNormalizer.std_with_epsilon().detach()
    tars = [data[1], *(later if later is not None else [])]
    for k in range(K):
        want = float(weighted_loss(r["pred32"][k], tars[k], data[2], nw, *obj, std))
        e_p, e_l = rel_err(preds[k], r["pred32"][k]), abs(float(step.step_losses()[k]) - want) / want
        print(f"[{key}] step {k}: prediction {e_p:.2e}, loss {e_l:.2e} from the fp32 oracle")
        assert e_p <= 1e-5 and e_l <= 1e-5, (k, e_p, e_l)
    r.update(pred=preds, loss=float(loss), gg={k: q.grad.detach().cpu() for k, q in mine.named_parameters() if q.requires_grad})
    check(r, str(key))
    # and it is another loss than the unweighted one
    plain = eng.FusedStep(mine, grads, unroll=K, step_weights=sw, detach=detach, objective=eng.Objective(*obj))
    assert abs(float(plain(*args)) - float(loss)) > 1e-3 * abs(float(loss))


def test_weighted_step_on_a_block_diagonal_batch(eng, graphs):
    """The variable-mesh route with flat [rows] weights: the golden block-diagonal batch of tests/test_hip_unroll.py (del64 + del300,
    364 rows, depth 2, its weight seed), K = 1, normalized / mse."""
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
    obj, nw = ("normalized", "mse", [1.0, 3.0]), spread_weights(torch.Generator().manual_seed(8), n)
    r = three_way(ref, ("node-weighted", "blockdiag"), lambda sim, d, lat: weighted_oracle(sim, d, None, [1.0], False, obj, nw, consistent=False), data)
    mine, grads = engine_model(eng, ref)
    step = eng.FusedStep(mine, grads, objective=objective_of(eng, obj))
    loss = step(levels, False, node_weights=nw.cuda())
    torch.cuda.synchronize()
    r.update(pred=step.prediction().reshape(r["pred32"].shape).cpu(), loss=float(loss),
             gg={k: q.grad.detach().cpu() for k, q in mine.named_parameters() if q.requires_grad})
    check(r, "node-weighted blockdiag")
    with pytest.raises(ValueError):
        step(levels, False, node_weights=nw[:-1].cuda())               # neither [N], [B, N] nor [rows]


# ------------------------------------------------------------------------------------------------ 7: what must not change
OBJ = ("normalized", "rmse", [1.0, 3.0])


def snapshot(step, grads, loss):
    return loss.clone(), torch.stack([q.clone() for q in step.predictions()]), grads.flat.clone()


def test_unit_weights_are_the_unweighted_objective_bit_for_bit(eng, graphs):
    """All-ones weights ([N], [B, N] and flat [R]) against the same objective without the flag, K = 1 and K = 2 carried; two
    consecutive calls are bit-equal."""
    ref, data = make_oracle("ring", graphs)
    mine, grads = engine_model(eng, ref)
    gdata = _cuda(data)
    for K in (1, 2):
        sw, later = ([1.0] if K == 1 else [1.0, 0.5]), later_targets(gdata[0], gdata[1], K)
        args = (gdata, True) if K == 1 else (gdata, True, later)
        plain = eng.FusedStep(mine, grads, unroll=K, step_weights=sw, objective=eng.Objective(*OBJ))
        want = snapshot(plain, grads, plain(*args))
        step = eng.FusedStep(mine, grads, unroll=K, step_weights=sw, objective=objective_of(eng, OBJ))
        for shape in ((300,), (2, 300), (600,)):
            grads.flat.fill_(float("nan"))
            got = snapshot(step, grads, step(*args, node_weights=torch.ones(*shape, device="cuda")))
            assert all(bit_equal(a, b) for a, b in zip(got, want)), (K, shape)
            assert bit_equal(step.channel_losses(), plain.channel_losses())
    nw = node_weights_for("per-sample").cuda()
    first = snapshot(step, grads, step(*args, node_weights=nw))
    grads.flat.fill_(float("nan"))
    again = snapshot(step, grads, step(*args, node_weights=nw))
    assert all(bit_equal(a, b) for a, b in zip(first, again)) and bool(torch.isfinite(first[2]).all())
    assert not bit_equal(first[2], want[2])
    with pytest.raises(ValueError):
        step(*args)                                                    # the flag without weights
    with pytest.raises(ValueError):
        plain(*args, node_weights=nw)                                  # weights without the flag
    with pytest.raises(ValueError):
        step(*args, node_weights=nw.double())
    with pytest.raises(ValueError):
        step(*args, node_weights=-torch.ones(300))                     # a host tensor is looked at


def test_without_the_flag_neither_new_entry_is_called(eng, graphs, monkeypatch):
    L = eng._abi.lib()
    calls = {"bsms_error_sums_w": 0, "bsms_sim_objective_bwd_w": 0}

    def counted(name):
        real = getattr(L, name)

        def f(*a):
            calls[name] += 1
            return real(*a)
        return f

    for name in calls:
        monkeypatch.setattr(L, name, counted(name))
    ref, data = make_oracle("ring", graphs)
    mine, grads = engine_model(eng, ref)
    gdata = _cuda(data)
    later = later_targets(gdata[0], gdata[1], 2)
    for kw in (dict(), dict(objective=eng.Objective(*OBJ)), dict(objective=eng.Objective(*OBJ), unroll=2)):
        step = eng.FusedStep(mine, grads, **kw)
        step(gdata, True, later) if kw.get("unroll") else step(gdata, True)
        assert "nw" not in step._buf
    torch.cuda.synchronize()
    assert calls == {"bsms_error_sums_w": 0, "bsms_sim_objective_bwd_w": 0}
    step = eng.FusedStep(mine, grads, objective=objective_of(eng, OBJ), unroll=2)
    step(gdata, True, later, node_weights=node_weights_for("shared").cuda())
    torch.cuda.synchronize()
    assert calls == {"bsms_error_sums_w": 2, "bsms_sim_objective_bwd_w": 2}


def test_graph_replay_with_changing_weights_equals_eager(eng, graphs):
    """The captured step reads the step's own weight buffer: new weights before a replay are the eager step with them -- [B, N]
    twice, then [N], then the first again, all replays of ONE capture: the buffer holds a weight per row whatever shape came in."""
    ref, data = make_oracle("ring", graphs)
    mine, grads = engine_model(eng, ref)
    gdata = _cuda(data)
    obj = objective_of(eng, OBJ)
    eager, gstep = eng.FusedStep(mine, grads, objective=obj), eng.FusedStep(mine, grads, use_graph=True, objective=obj)
    gen = torch.Generator().manual_seed(2)
    w_a, w_b, w_c = spread_weights(gen, 2, 300).cuda(), spread_weights(gen, 2, 300).cuda(), spread_weights(gen, 300).cuda()
    seen, captured = [], None
    for nw in (w_a, w_b, w_c, w_a):
        want = snapshot(eager, grads, eager(gdata, True, node_weights=nw))
        grads.flat.fill_(float("nan"))
        got = snapshot(gstep, grads, gstep(gdata, True, node_weights=nw))
        assert all(bit_equal(a, b) for a, b in zip(got, want))
        seen.append(want[0])
        captured = captured or gstep._graphs
        assert gstep._graphs is captured                               # another shape of weights is no reason to capture again
    assert captured is not None and not bit_equal(seen[0], seen[1]) and bit_equal(seen[0], seen[3])


@pytest.mark.parametrize("kw", [dict(unroll=1), dict(unroll=2), dict(unroll=2, accumulate=2, reduction="mean")], ids=["K1", "K2", "K2-accumulate"])
def test_a_step_that_has_seen_shared_weights_takes_per_sample_ones(eng, graphs, kw):
    """One step object called with shared [N] weights first and with real [B, N] (then flat [R]) weights after it: loss, predictions
    and every gradient are those of a FRESH step that only ever saw the [B, N] weights, bit for bit -- nothing of the first call's
    shape survives in the step, its per-step buffer sets of the unrolled form included.  (With accumulate = 2 every call compared is
    micro-batch 0 of a cycle: the plain step into grads.flat.)"""
    ref, data = make_oracle("ring", graphs)
    gdata = _cuda(data)
    K = kw["unroll"]
    later = later_targets(gdata[0], gdata[1], K)
    args = (gdata, True) if K == 1 else (gdata, True, later)
    obj = objective_of(eng, ("physical", "mse", None))
    shared, per = node_weights_for("shared").cuda(), node_weights_for("per-sample").cuda()
    assert not bit_equal(per[0], per[1])
    mine, grads = engine_model(eng, ref)
    fresh = eng.FusedStep(mine, grads, objective=obj, **kw)
    want = snapshot(fresh, grads, fresh(*args, node_weights=per))
    mine2, grads2 = engine_model(eng, ref)
    step = eng.FusedStep(mine2, grads2, objective=obj, **kw)
    first = snapshot(step, grads2, step(*args, node_weights=shared))
    assert not bit_equal(first[2], want[2])
    for nw in (per, per.reshape(-1)):
        step.reset_accumulation()                                     # accumulate = 2: the next call is micro-batch 0 again
        grads2.flat.fill_(float("nan"))
        got = snapshot(step, grads2, step(*args, node_weights=nw))
        assert all(bit_equal(a, b) for a, b in zip(got, want)), tuple(nw.shape)
    # and back: the shared weights are their tiled form
    step.reset_accumulation()
    again = snapshot(step, grads2, step(*args, node_weights=shared.repeat(2)))
    assert all(bit_equal(a, b) for a, b in zip(again, first))


# ------------------------------------------------------------------------------------------------ 8: composition
def plain_weighted(eng, ref, freeze=(), precision=None, **kw):
    mine, grads = engine_model(eng, ref, freeze)
    if precision:
        mine.process.precision = precision
    step = eng.FusedStep(mine, grads, objective=objective_of(eng, OBJ), **kw)
    return mine, grads, step


def test_recompute_frozen_and_bf16_keep_the_bits(eng, graphs):
    """`recompute=True` against the plain weighted step (fp32 at D = 32, bf16 at D = 128), and a frozen processor: its gradients of the
    trainable MLPs are the all-trainable step's, bit for bit."""
    nw = node_weights_for("per-sample").cuda()
    for shape, precision in (("ring", None), ("split", "bf16")):
        ref, data = make_oracle(shape, graphs)
        gdata = _cuda(data)
        mine, grads, step = plain_weighted(eng, ref, precision=precision)
        want = snapshot(step, grads, step(gdata, True, node_weights=nw))
        assert bool(torch.isfinite(want[2]).all()) and float(want[2].abs().max()) > 0
        grads.flat.fill_(float("nan"))
        lean = eng.FusedStep(mine, grads, objective=objective_of(eng, OBJ), recompute=True)
        got = snapshot(lean, grads, lean(gdata, True, node_weights=nw))
        assert all(bit_equal(a, b) for a, b in zip(got, want)), (shape, precision)
        if precision == "bf16":                                        # bf16 against its own unit-weight twin: the unweighted objective
            plain = eng.FusedStep(mine, grads, objective=eng.Objective(*OBJ))
            base = snapshot(plain, grads, plain(gdata, True))
            unit = snapshot(step, grads, step(gdata, True, node_weights=torch.ones(300, device="cuda")))
            assert all(bit_equal(a, b) for a, b in zip(unit, base))
    ref, data = make_oracle("ring", graphs)
    gdata = _cuda(data)
    full_model, _, full = plain_weighted(eng, ref)
    l_full = full(gdata, True, node_weights=nw)
    want = {k: q.grad.clone() for k, q in full_model.named_parameters() if q.requires_grad}
    mine, grads, step = plain_weighted(eng, ref, freeze=("process",))
    l_frozen = step(gdata, True, node_weights=nw)
    assert bit_equal(l_frozen, l_full) and bit_equal(step.prediction(), full.prediction())
    live = [k for k, q in mine.named_parameters() if q.requires_grad]
    assert live and all(not k.startswith("process.") for k in live)
    for k, q in mine.named_parameters():
        if q.requires_grad:
            assert bit_equal(q.grad, want[k]), k
        else:
            assert q.grad is None, k


def test_input_gradient_with_weights(eng, graphs):
    """`input_grad=True` leaves loss, predictions and weight gradients of the weighted step bit-equal and `input_gradient(node_weights=)`
    hands out the same gradient; against the oracle's autograd gradient w.r.t. node_in by the criterion of
    tests/test_hip_input_grad.py: relative L2 to the fp64 oracle within max(1e-5, 3 x the fp32 oracle's own distance)."""
    ref, data = make_oracle("ring", graphs)
    nw = node_weights_for("shared")
    gdata = _cuda(data)
    mine, grads, step = plain_weighted(eng, ref)
    want = snapshot(step, grads, step(gdata, True, node_weights=nw.cuda()))
    grads.flat.fill_(float("nan"))
    ig = eng.FusedStep(mine, grads, objective=objective_of(eng, OBJ), input_grad=True)
    got = snapshot(ig, grads, ig(gdata, True, node_weights=nw.cuda()))
    assert all(bit_equal(a, b) for a, b in zip(got, want))
    g_in = ig.input_grad().clone()
    from bsms_gnn_amd.step import input_gradient
    loss2, g2 = input_gradient(mine, gdata, objective=objective_of(eng, OBJ), node_weights=nw.cuda())
    assert bit_equal(loss2, want[0]) and bit_equal(g2, g_in)
    ref64 = ro.BSMS_Simulator(ref.cfg, dtype=torch.float64)
    ref64.load_state_dict(ref.state_dict())
    ref64.double()
    oracle = {}
    for name, sim, d in (("f32", ref, data), ("f64", ref64, _f64(data))):
        x = d[0].clone().requires_grad_(True)
        pred = sim((x, *d[1:]), True, False)
        weighted_loss(pred, d[1], d[2], nw, *OBJ, sim._targetNormalizer.std_with_epsilon().detach()).backward()
        oracle[name] = x.grad.double()
    l2 = lambda a, b: float((a - b).norm() / b.norm())
    e_gpu, e_cpu = l2(g_in.cpu().double(), oracle["f64"]), l2(oracle["f32"], oracle["f64"])
    print(f"input gradient, relative L2 to the fp64 oracle: engine {e_gpu:.2e}, fp32 oracle {e_cpu:.2e}")
    assert e_gpu <= max(1e-5, 3.0 * e_cpu)
    with pytest.raises(ValueError):
        input_gradient(mine, gdata, objective=objective_of(eng, OBJ))


def test_two_micro_batches_accumulate_to_the_weighted_batch_step(eng, graphs):
    """accumulate = 2, reduction = "batch", sample 0 then sample 1 with their own weights: grads.flat is the recurrence of
    tests/test_hip_accumulate.py over the plain weighted steps, bit for bit, and the cycle is the oracle's ONE weighted step on both
    samples by the three-way criterion."""
    obj = ("normalized", "mse", [1.0, 3.0])
    ref, data = make_oracle("ring", graphs)
    nw = node_weights_for("per-sample")
    r = three_way(ref, ("node-weighted", "accumulate"), lambda sim, d, lat: weighted_oracle(sim, d, None, [1.0], False, obj, nw), data)
    mine, grads = engine_model(eng, ref)
    gdata, gw = _cuda(data), nw.cuda()
    plain = eng.FusedStep(mine, grads, objective=objective_of(eng, obj))
    alone = []
    for b in (0, 1):
        loss = plain(part(gdata, [b])[0], True, node_weights=gw[b:b + 1])
        alone.append((loss.clone(), grads.flat.clone()))
    grads.flat.fill_(float("nan"))
    step = eng.FusedStep(mine, grads, accumulate=2, reduction="batch", objective=objective_of(eng, obj))
    preds = []
    for b in (0, 1):
        loss = step(part(gdata, [b])[0], True, node_weights=gw[b:b + 1])
        assert bit_equal(loss, alone[b][0])
        preds.append(step.prediction().clone())
    ab = step.accumulation_coefficients()
    assert step.ready and bit_equal(grads.flat, (ab[0] * alone[0][1]) + (ab[1] * alone[1][1]))
    r.update(pred=torch.cat(preds).unsqueeze(0).cpu(), loss=float(step.accumulated_loss()),
             gg={k: q.grad.detach().cpu() for k, q in mine.named_parameters() if q.requires_grad})
    check(r, "node-weighted accumulate")


def _worker(rank, world, port, out_path):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    torch.cuda.set_device(0)
    from conftest import Golden
    import bsms_gnn_amd as eng
    from test_hip_node_weights import OBJ, node_weights_for
    z, graphs = Golden("sim"), Golden("graphs")
    es, ids = graphs.levels("del300")
    torch.manual_seed(50 + rank)
    sim = eng.BSMS_Simulator(ro.make_cfg(2, 32, 3, 3, 2))
    if rank == 0:
        sim.load_state_dict(z.state_dict())
    sim = sim.cuda()
    c, sl = (lambda t: t.cuda()), slice(rank, rank + 1)
    data = (c(z.t("node_in")[sl]), c(z.t("tar")[sl]), c(z.t("mask")[sl]), [c(e.unsqueeze(0)) for e in es], [c(i.unsqueeze(0)) for i in ids])
    engine = eng.DataParallel(sim, bucket_bytes=64 << 10, objective=eng.Objective(*OBJ, node_weighted=True))
    loss = engine.step_loss_backward(data, True, node_weights=node_weights_for("per-sample")[sl].cuda())
    torch.cuda.synchronize()
    torch.save({"loss": loss.detach().cpu(), "flat": engine.grads.flat.cpu(), "chan": engine.fused.channel_losses().cpu()}, f"{out_path}.{rank}")
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.timeout(300)
def test_two_ranks_equal_the_single_process_weighted_step(eng, graphs, tmp_path):
    """Two ranks over gloo on one GPU, one golden sample and its weights each: the all-reduced row is the weighted one, the result the
    single-process step on the whole batch.  The ranks are bit-identical to each other; against the single process the bounds are
    deliberately those of tests/test_hip_objective.py's two-rank case (loss and channel terms 1e-5, gradients 2e-5), not bit
    equality: the row is the sum of two per-rank fp64 rows instead of one sum over 600 rows, and every weight gradient is the
    all-reduced sum of two B = 1 gradients instead of one B = 2 reduction -- other summation orders, which no code here can align."""
    port = 31900 + os.getpid() % 2000
    out = str(tmp_path / "res")
    mp.start_processes(_worker, args=(2, port, out), nprocs=2, join=True, start_method="spawn")
    r0, r1 = torch.load(out + ".0"), torch.load(out + ".1")
    assert torch.equal(r0["flat"], r1["flat"]) and torch.equal(r0["loss"], r1["loss"])
    z = load_golden("sim")
    sim = eng.BSMS_Simulator(ro.make_cfg(2, 32, 3, 3, 2))
    sim.load_state_dict(z.state_dict())
    sim = sim.cuda()
    from test_hip_unroll import sim_batch
    data = _cuda(sim_batch(graphs, 3))
    grads = eng.GradBuckets(list(sim.parameters()))
    step = eng.FusedStep(sim, grads, objective=objective_of(eng, OBJ))
    loss = step(data, True, node_weights=node_weights_for("per-sample").cuda())
    assert abs(float(r0["loss"]) - float(loss)) < 1e-5 * abs(float(loss))
    assert rel_err(r0["chan"], step.channel_losses().cpu()) < 1e-5
    assert rel_err(r0["flat"], grads.flat.cpu()) < 2e-5


# ------------------------------------------------------------------------------------------------ 9: the bank and the Trainer
def test_measure_bank_on_a_consistent_mesh(eng):
    from test_datapipe import cfg as data_cfg
    from test_hip_databank import same_mesh_trajs
    dcfg = data_cfg(True, gamma=0.8)
    trajs = same_mesh_trajs(300, 5, 2, seed=4)
    plain, bank = eng.TrajectoryBank(dcfg, seed=3), eng.TrajectoryBank(dcfg, seed=3, node_weights="measure")
    for t in trajs:
        plain.add(t), bank.add(t)
    assert bank.bytes_resident == plain.bytes_resident + 2 * 300 * 4
    want = torch.from_numpy(eng.lumped_node_measure(trajs[0]["mesh_pos"][0], trajs[0]["cells"][0], "tri"))
    assert want.dtype == torch.float32 and float(want.min()) > 0
    picks = [(0, 3), (1, 0), (1, 2)]
    w = bank.node_weights(picks)
    assert w.shape == (3, 300) and w.is_cuda and all(bit_equal(w[b].cpu(), want) for b in range(3))
    batch, noise, w2 = bank.batch(picks, train=True, draw=5, return_noise=True, return_weights=True)
    base, base_noise = plain.batch(picks, train=True, draw=5, return_noise=True)
    assert bit_equal(w2, w) and bit_equal(noise, base_noise)
    for a, b in zip(batch[:3], base[:3]):
        assert bit_equal(a, b)
    got = bank.batch(picks, train=False, return_weights=True)
    assert len(got) == 2 and len(got[0]) == 5 and bit_equal(got[1], w)
    assert len(bank.batch(picks, train=False)) == 5                    # without the keyword: the parent's tuple
    with pytest.raises(ValueError):
        plain.node_weights(picks)
    with pytest.raises(ValueError):
        plain.batch(picks, return_weights=True)
    with pytest.raises(ValueError):
        eng.TrajectoryBank(dcfg, node_weights="area")
    moving = same_mesh_trajs(300, 5, 1, seed=4, moving=(0,))[0]
    with pytest.raises(ValueError):
        eng.TrajectoryBank(dcfg, node_weights="measure").add(moving)
    nocells = SimpleNamespace(**{**vars(dcfg), "field_names": [k for k in dcfg.field_names if k != "cells"]})
    late = eng.TrajectoryBank(nocells, node_weights="measure")
    late._hier = bank._hier                                            # a later trajectory of a consistent mesh reads cfg.field_names only
    with pytest.raises(ValueError):
        late.add(trajs[1])


def test_measure_bank_on_variable_meshes(eng):
    from test_datapipe import cfg as data_cfg, synthetic_traj
    from test_hip_databank import model_cfg
    dcfg = data_cfg(False, gamma=0.8)
    trajs = [synthetic_traj(100, 5, 1), synthetic_traj(140, 6, 2)]
    torch.manual_seed(0)
    process = eng.BSMS_Simulator(model_cfg(False)).cuda().process
    bank = eng.TrajectoryBank(dcfg, dataset="cylinder_flow", process=process, seed=9, node_weights="measure")
    for t in trajs:
        bank.add(t)
    want = [torch.from_numpy(eng.lumped_node_measure(t["mesh_pos"][0], t["cells"][0], "tri")) for t in trajs]
    picks = [(1, 2), (0, 1), (1, 0)]
    levels, w = bank.batch(picks, train=True, draw=2, return_weights=True)
    assert w.shape == (380,) and bit_equal(w.cpu(), torch.cat([want[1], want[0], want[1]]))
    assert levels[0].x.shape[0] == 380 and bit_equal(bank.node_weights(picks), w)


def _train(eng, iters=4):
    from test_datapipe import cfg as data_cfg
    from test_hip_databank import same_mesh_trajs
    dcfg = data_cfg(True, gamma=0.8)
    dcfg.noise_level = [0.02, 0.02, 0.01]
    bank = eng.TrajectoryBank(dcfg, seed=1, node_weights="measure")
    for t in same_mesh_trajs(120, 8, 2, seed=6):
        bank.add(t)
    model_cfg = SimpleNamespace(out_dim=3, latent_dim=32, hidden_layer=2, unet_depth=2, pos_dim=2, consistent_mesh=True,
                                accumulation_steps=1, loss_node_weights=True, loss_kind="mse")
    opt_cfg = SimpleNamespace(peak_lr=1e-3, weight_decay=1e-4, warmup_steps=2, decay_steps=20, gnorm_clip=1.0)
    torch.manual_seed(0)
    tr = eng.Trainer(eng.BSMS_Simulator(model_cfg), model_cfg, opt_cfg)
    losses = []
    for _ in range(iters):
        picks = bank.next_picks(2)
        out = tr.iter(bank.batch(picks), node_weights=bank.node_weights(picks))
        if out is not None:
            losses.append(out.clone())
    return tr, bank, losses


def test_trainer_trains_on_the_weighted_objective(eng):
    """model_cfg.loss_node_weights: one warm-up and three optimisation iterations, twice: the same losses and parameters bit for bit;
    get_loss is masked_loss with the weights; the keyword is required with the key."""
    tr, bank, losses = _train(eng)
    tr2, _, losses2 = _train(eng)
    assert tr.objective == eng.Objective(kind="mse", node_weighted=True) and tr.dp.fused.objective == tr.objective
    assert len(losses) == 3 and tr.train_step == 4 and all(bool(torch.isfinite(l)) for l in losses)
    assert all(bit_equal(a, b) for a, b in zip(losses, losses2)) and bit_equal(tr.optimizer.flat_p, tr2.optimizer.flat_p)
    picks = [(0, 1), (1, 3)]
    batch, w = bank.batch(picks, train=False, return_weights=True)
    pred = tr.get_pred(batch).detach()
    want = eng.masked_loss(pred, batch[1], batch[2], tr.objective, None, node_weights=w)
    got = tr.get_loss(batch, node_weights=w).detach()
    assert bit_equal(got, want)
    unweighted = eng.masked_loss(pred, batch[1], batch[2], eng.Objective(kind="mse"))
    assert abs(float(got) - float(unweighted)) > 1e-4 * float(got)
    with pytest.raises(ValueError):
        tr.iter(batch)
    with pytest.raises(ValueError):
        tr.get_loss(batch)
