"""GPU: the robust training objectives -- bsms_robust_sums and bsms_sim_robust_bwd on their own (NumPy fp64, the
AE column of bsms_error_sums, bit equalities under unit and rescaled weights, the carry of bsms_sim_objective_bwd), the fused step
with kind "mae" / "huber" against the CPU oracle under autograd with `masked_loss` (pinned against torch.nn.functional by
tests/test_robust_host.py), every accelerated form of the step against the plain one, the Trainer, two data-parallel ranks, and
what must not move.

The definition: d = fl32(pred - tar), mu = m or m * omega, s_c = 1 (physical) or std_c (normalized), u = double(d) / s_c,
rho = |u| (mae) or u^2 / 2 below delta_c and delta_c (|u| - delta_c / 2) above (huber), S_c = sum mu rho(u_c), loss = sum_c w_c S_c / (M C).

Meshes: the 300-node `del300` golden batch (B = 2, C = 2) with the models of tests/test_hip_unroll.py.  The oracle cases take their
TARGETS from the oracle's own prediction plus offsets of random sign and size 0.05 .. 2 in the objective's units (`offset_case`): no
residual is within round-off of the kink of |u|, so sign(d) is the same in fp32, in fp64 and on the GPU, and the Huber loss sees
both branches.

Tolerances: the sums 1e-12 (the figure bsms_error_sums_w is held to: fp64 sums of non-negative terms in another order), the
backward kernel 1e-6 (tests/test_hip_objective.py::KERNEL_TOL), the step against the oracle 1e-5 on predictions and losses and the
three-way criterion of tests/test_hip_fullsize.py::check (one factor, 1.5) on the gradients; bf16: the 1e-2 on the loss of
tests/test_hip_bf16.py."""
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from conftest import ROOT, rel_err
from oracle import bsms_oracle as ro
from test_eval_host import rel
from test_hip_accumulate import bit_equal, engine_model, part, three_way
from test_hip_fullsize import check
from test_hip_node_weights import SENTINEL, bwd_call, bwd_operands, guarded, ptr, raw_sums, snapshot, spread_weights, sum_operands
from test_hip_objective import KERNEL_TOL, _stats, _std
from test_hip_unroll import _cuda, _f64, make_oracle

pytestmark = pytest.mark.gpu

SUM_TOL = 1e-12
SPACE_ID, RKIND_ID = {"physical": 0, "normalized": 1}, {"mae": 0, "huber": 1}
PAIRS = [("physical", "mae"), ("physical", "huber"), ("normalized", "mae"), ("normalized", "huber")]


@pytest.fixture(scope="module")
def eng():
    import bsms_gnn_amd as eng
    return eng


def np_rho(u, delta, kind):
    au = np.abs(u)
    return au if kind == "mae" else np.where(au <= delta, 0.5 * u * u, delta * (au - 0.5 * delta))


def np_psi(u, delta, kind):
    return np.sign(u) if kind == "mae" else np.clip(u, -delta, delta)


# ------------------------------------------------------------------------------------------------ 1: bsms_robust_sums alone
def raw_robust(eng, pred, tar, mask, weights, S, n, C, mask_stride, weight_stride, stats, delta, space, kind, wide):
    """One call on guarded device operands.  `wide`: rows of 1 + 3C doubles instead of 1 + C; everything between and around the
    [M | S] fields is a sentinel that must survive, and `work` starts as NaNs."""
    L = eng._abi.lib()
    ncol, stride = 1 + C, (1 + 3 * C if wide else 1 + C)
    out = torch.full((S * stride + 16,), SENTINEL, dtype=torch.float64, device="cuda")
    rows = out[8:8 + S * stride].view(S, stride)
    work = torch.full((L.bsms_error_sums_work_bytes(S, n) // 8 + 1,), float("nan"), dtype=torch.float64, device="cuda")
    st = [None, None, None] if stats is None else [ptr(t) for t in stats]
    rc = L.bsms_robust_sums(ptr(pred), ptr(tar), ptr(mask), ptr(weights), S, n, C, n, n, mask_stride, weight_stride, *st, ptr(delta),
                            SPACE_ID[space], RKIND_ID[kind], rows.data_ptr(), stride, work.data_ptr(), torch.cuda.current_stream().cuda_stream)
    eng._abi.check(rc, "bsms_robust_sums")
    torch.cuda.synchronize()
    assert bool((out[:8] == SENTINEL).all()) and bool((out[8 + S * stride:] == SENTINEL).all()), "wrote outside the sums"
    assert bool((rows[:, ncol:] == SENTINEL).all()), "wrote past the 1 + C fields of a row"
    return rows[:, :ncol].clone()


def np_robust_sums(pred, tar, mask, w, std, delta, kind):
    p, t = pred.numpy(), tar.numpy()
    S, n, _ = p.shape
    u = (p - t).astype(np.float32).astype(np.float64) / std
    mu = np.broadcast_to(mask.numpy(), (S, n)).astype(np.float64)                # [S, n], or [1, n] shared by the segments
    if w is not None:
        mu = mu * np.broadcast_to(w.numpy(), (S, n)).astype(np.float64)
    return np.concatenate([mu.sum(1, keepdims=True), (mu[:, :, None] * np_rho(u, delta, kind)).sum(1)], axis=1)


@pytest.mark.parametrize("S", [1, 3])
@pytest.mark.parametrize("C", [1, 3, 8])
@pytest.mark.parametrize("n", [0, 1, 255, 256, 257, 1023, 1024, 1025, 2049])
def test_robust_sums(eng, n, C, S):
    """Both sides of a wave and of the 1024-row piece edge; per-segment and shared (stride 0) mask and weights; rows of 1 + C and
    of 1 + 3C doubles.  Rows with d == 0 exactly (row 0 of every segment) and with |u| == delta exactly (row 1, channel 0, in the
    physical space: d = 0.5 = delta_0) are among the data."""
    gen, pred, tar, mask = sum_operands(S, n, C, 31 * n + 7 * C + S)
    stats = _stats(C, gen, small=C // 2)
    std = _std(stats)
    delta = 0.3 + 1.2 * torch.rand(C, generator=gen, dtype=torch.float64)
    delta[0] = 0.5
    if n >= 1:
        pred[:, 0], mask[:, 0] = tar[:, 0], 1.0
    if n >= 2:
        tar[:, 1, 0], mask[:, 1] = 1.0, 1.0
        pred[:, 1, 0] = 1.5
    w = spread_weights(gen, S, n)
    dp, dt, dm, dw, ones = (guarded(t) for t in (pred, tar, mask, w, torch.ones(S, n)))
    dstats, ddelta = [t.cuda() for t in stats], delta.cuda()
    # MAE in the physical space IS the AE column (and M) of bsms_error_sums / _w, bit for bit
    for weights, ms, ws in ((None, n, 0), (None, 0, 0), (dw, n, n), (dw, 0, 0)):
        twin = raw_sums(eng, dp, dt, dm, weights, S, n, C, ms, ws)
        got = raw_robust(eng, dp, dt, dm, weights, S, n, C, ms, ws, None, None, "physical", "mae", wide=True)
        assert bit_equal(got[:, 0], twin[:, 0]) and bit_equal(got[:, 1:], twin[:, 1 + C:1 + 2 * C]), (weights is not None, ms)
    worst = 0.0
    for space, kind in PAIRS:
        s_np = std if space == "normalized" else np.ones(C)
        for wide in (False, True):
            plain = raw_robust(eng, dp, dt, dm, None, S, n, C, n, 0, dstats, ddelta, space, kind, wide)
            unit = raw_robust(eng, dp, dt, dm, ones, S, n, C, n, n, dstats, ddelta, space, kind, wide)
            assert bit_equal(unit, plain), (space, kind, "all-ones weights")
        assert bit_equal(plain, raw_robust(eng, dp, dt, dm, None, S, n, C, n, 0, dstats, ddelta, space, kind, False)), "two runs"
        worst = max(worst, rel(plain.cpu().numpy(), np_robust_sums(pred, tar, mask, None, s_np, delta.numpy(), kind)))
        for ms, ws, m_np, w_np in ((n, n, mask, w), (0, n, mask[:1], w), (n, 0, mask, w[:1])):
            got = raw_robust(eng, dp, dt, dm, dw, S, n, C, ms, ws, dstats, ddelta, space, kind, True)
            worst = max(worst, rel(got.cpu().numpy(), np_robust_sums(pred, tar, m_np, w_np, s_np, delta.numpy(), kind)))
            assert bool(torch.isfinite(got).all())
        # a segment's sums depend on its own rows only: the last segment alone, bit for bit
        last = S - 1
        whole = raw_robust(eng, dp, dt, dm, dw, S, n, C, n, n, dstats, ddelta, space, kind, False)
        alone = raw_robust(eng, guarded(pred[last:]), guarded(tar[last:]), guarded(mask[last:]), guarded(w[last:]), 1, n, C, n, n, dstats,
                           ddelta, space, kind, True)
        assert bit_equal(alone[0], whole[last]), (space, kind)
        if n == 0:
            assert bool((whole == 0).all())
    print(f"\n[n={n} C={C} S={S}] worst relative distance to NumPy fp64: {worst:.2e}")
    assert worst <= SUM_TOL, worst


# ------------------------------------------------------------------------------------------------ 2: bsms_sim_robust_bwd alone
def robust_bwd(eng, ops, R, C, sums, cw, delta, space, kind, w_step, carried, weights=None, period=0):
    """bsms_sim_robust_bwd into sentinel-guarded outputs; returns (loss, chan, g_pred, grad_norm_pred)."""
    L = eng._abi.lib()
    dp, dt, dm, do, di, dgn, dgi = ops
    loss, chan = guarded(torch.full((1,), -1.0)), guarded(torch.full((C,), -1.0))
    gp, gnp = guarded(torch.full((R, C), 7.0)), guarded(torch.full((R, C), 7.0))
    rc = L.bsms_sim_robust_bwd(ptr(dp), ptr(dt), ptr(dm), ptr(weights), period, R, C, *map(ptr, do), *map(ptr, di), ptr(sums), ptr(cw),
                               ptr(delta), SPACE_ID[space], RKIND_ID[kind], w_step, ptr(dgn) if carried else None,
                               ptr(dgi) if carried else None, ptr(loss), ptr(chan), ptr(gp), ptr(gnp), torch.cuda.current_stream().cuda_stream)
    eng._abi.check(rc, "bsms_sim_robust_bwd")
    torch.cuda.synchronize()
    for t in (loss, chan, gp, gnp):                          # the NaN guards on both sides of every output are still NaN
        base = t.reshape(-1)
        lo = torch.as_strided(base, (64,), (1,), base.storage_offset() - 64)
        hi = torch.as_strided(base, (64,), (1,), base.storage_offset() + base.numel())
        assert bool(torch.isnan(lo).all()) and bool(torch.isnan(hi).all()), "wrote outside an output"
    return loss, chan, gp, gnp


@pytest.mark.parametrize("C", [1, 3, 8])
@pytest.mark.parametrize("R", [1, 255, 257, 1025])
def test_robust_bwd_kernel(eng, R, C):
    """One thread, one ragged block, two and five blocks.  Every (space, kind); unit and random channel weights; per-channel delta; a
    step weight != 1 with the carried pair; no weights, all-ones weights (bit-equal), real weights with period R and, where R has a
    divisor, a vector shared by B = R / N samples (bit-equal to its tiled form); omega -> 4 omega with the sums scaled by 4 leaves
    every output's bits.  Row R - 1 has pred == tar (R > 1): sign(0) = 0, its loss gradient is exactly 0."""
    pred, tar, mask, o_stats, i_stats, g_next, g_nin, cw, _ = bwd_operands(R, C)
    if R > 1:
        pred[R - 1] = tar[R - 1]                             # (the operands' mask keeps row R - 1; a lone row keeps its residual)
    ops = (guarded(pred), guarded(tar), guarded(mask), [t.cuda() for t in o_stats], [t.cuda() for t in i_stats], guarded(g_next), guarded(g_nin))
    gen = torch.Generator().manual_seed(7 * R + C)
    omega = spread_weights(gen, R)
    delta = 0.3 + 1.2 * torch.rand(C, generator=gen, dtype=torch.float64)
    ddelta, dcw = delta.cuda(), cw.cuda()
    std_o, std_i = _std(o_stats), _std(i_stats)
    D = (pred - tar).double().numpy()
    Mk = mask.double().numpy()[:, None]
    with np.errstate(invalid="ignore"):
        carry_full = np.where(Mk != 0, g_next.double().numpy() + g_nin.double().numpy()[:, :C] / std_i[:C], 0.0)
    N = {1: 1, 255: 85, 257: None, 1025: 205}[R]
    worst = 0.0
    for space, kind in PAIRS:
        s_np = std_o if space == "normalized" else np.ones(C)
        u = D / s_np
        for om, dw_ in ((None, None), (omega, guarded(omega))):
            mu = Mk if om is None else Mk * om.double().numpy()[:, None]
            M_, S_ = float(mu.sum()), (mu * np_rho(u, delta.numpy(), kind)).sum(0)
            sums = torch.tensor(np.concatenate([[M_], S_, np.full(2 * C, np.nan)]), dtype=torch.float64).cuda()      # [M | S | never read]
            for w_dev, w_np in ((None, np.ones(C)), (dcw, cw.numpy())):
                terms = w_np * S_ / (M_ * C)
                for carried, w_step in ((False, 1.0), (True, 0.375)):
                    got = robust_bwd(eng, ops, R, C, sums, w_dev, ddelta, space, kind, w_step, carried, dw_, R)
                    tag = (space, kind, om is not None, w_dev is not None, carried)
                    want_gp = w_step * (np_psi(u, delta.numpy(), kind) * mu * (w_np / (M_ * C * s_np))[None, :]) + (carry_full if carried else 0.0)
                    want_gnp = want_gp * Mk * std_o
                    assert abs(float(got[0]) - terms.sum()) <= KERNEL_TOL * terms.sum(), tag
                    assert np.abs(got[1].cpu().double().numpy() - terms).max() <= KERNEL_TOL * terms.max(), tag
                    for out, want in ((got[2], want_gp), (got[3], want_gnp)):
                        err = np.abs(out.cpu().double().numpy() - want).max() / np.abs(want).max()
                        worst = max(worst, err)
                        assert err <= KERNEL_TOL, (tag, err)
                        assert bool((out.cpu()[mask == 0] == 0).all()), tag
                    if not carried and R > 1:
                        assert bool((got[2][R - 1] == 0).all()) and bool((got[3][R - 1] == 0).all()), (tag, "sign(0)")
                    if om is None:                           # all-ones weights: the NULL kernel, bit for bit
                        unit = robust_bwd(eng, ops, R, C, sums, w_dev, ddelta, space, kind, w_step, carried, guarded(torch.ones(R)), R)
                        assert all(bit_equal(a, b) for a, b in zip(unit, got)), tag
                        again = robust_bwd(eng, ops, R, C, sums, w_dev, ddelta, space, kind, w_step, carried, None, -5)   # period ignored
                        assert all(bit_equal(a, b) for a, b in zip(again, got)), tag
                    else:                                    # omega -> 4 omega: sums x 4, every output's bits stay
                        four = robust_bwd(eng, ops, R, C, sums * 4.0, w_dev, ddelta, space, kind, w_step, carried, guarded(4.0 * om), R)
                        assert all(bit_equal(a, b) for a, b in zip(four, got)), tag
        if N is not None:                                    # one weight vector shared by the R / N samples == its tiled form
            short = spread_weights(gen, N)
            sums = torch.tensor(np.concatenate([[float(Mk.sum())], np.ones(C)]), dtype=torch.float64).cuda()
            tiled = robust_bwd(eng, ops, R, C, sums, dcw, ddelta, space, kind, 0.375, True, guarded(short.repeat(R // N)), R)
            shared = robust_bwd(eng, ops, R, C, sums, dcw, ddelta, space, kind, 0.375, True, guarded(short), N)
            assert all(bit_equal(a, b) for a, b in zip(shared, tiled)), (space, kind)
    print(f"\n[R={R} C={C}] worst relative distance to the fp64 restatement: {worst:.2e}")


@pytest.mark.parametrize("R,C", [(257, 3), (1025, 8)])
def test_a_zero_loss_gradient_leaves_the_carry_of_the_squared_entry(eng, R, C):
    """pred == tar: psi = 0 and d = 0, so both entries write w * 0 + carry -- the carry and the way out through the de-normalisation
    are shared op for op, and the outputs are bit-equal (the squared entry under "mse": its coefficient is finite at SE = 0)."""
    _, tar, mask, o_stats, i_stats, g_next, g_nin, cw, _ = bwd_operands(R, C)
    ops = (guarded(tar.clone()), guarded(tar), guarded(mask), [t.cuda() for t in o_stats], [t.cuda() for t in i_stats], guarded(g_next), guarded(g_nin))
    sums = torch.tensor([float(mask.sum())] + [1.0] * (3 * C), dtype=torch.float64).cuda()
    delta = torch.full((C,), 0.7, dtype=torch.float64).cuda()
    for space in ("physical", "normalized"):
        rc, want = bwd_call(eng, ops, R, C, sums, cw.cuda(), SPACE_ID[space], 1, 0.375, True)
        assert rc == 0 and bool(torch.isfinite(want[3]).all()) and float(want[2].abs().max()) > 0
        for kind in ("mae", "huber"):
            got = robust_bwd(eng, ops, R, C, sums, cw.cuda(), delta, space, kind, 0.375, True)
            assert bit_equal(got[2], want[2]) and bit_equal(got[3], want[3]), (space, kind)


# ------------------------------------------------------------------------------------------------ 3: the fused step against the oracle
def rollout_predictions(ref, data, K):
    """The oracle's own K predictions by the rollout rule (no gradient): what the targets are built around."""
    node_in, tar, mask, m_gs, m_ids = data
    C = tar.shape[-1]
    cur, preds = node_in, []
    with torch.no_grad():
        for _ in range(K):
            pred = ref((cur, tar, mask, m_gs, m_ids), True, False)
            preds.append(pred)
            cur = torch.where(mask == 0, node_in, torch.cat([pred, node_in[..., C:]], dim=-1))
    return preds


_CASES = {}


def offset_case(graphs, objective, K, seed=17):
    """(ref, data, later): the `ring` oracle and the golden batch with targets = the oracle's prediction + e, e of random sign and
    |e| uniform in 0.05 .. 2 in the objective's units (times std_c in the normalized space)."""
    key = (objective.space, K, seed)
    if key not in _CASES:
        ref, data = make_oracle("ring", graphs)
        preds = rollout_predictions(ref, data, K)
        gen = torch.Generator().manual_seed(seed)
        s = ref._targetNormalizer.std_with_epsilon().detach().float() if objective.space == "normalized" else torch.ones(2)
        tars = []
        for p in preds:
            e = (0.05 + 1.95 * torch.rand(p.shape, generator=gen)) * (2.0 * (torch.rand(p.shape, generator=gen) < 0.5).float() - 1.0)
            tars.append(p + e * s)
        _CASES[key] = (ref, (data[0], tars[0], *data[2:]), (torch.stack(tars[1:]) if K > 1 else None), preds, s)
    return _CASES[key]


def assert_offsets(objective, preds, tars, mask, s):
    """On the CPU, before anything is compared: no residual near the kink, and (Huber) both branches well populated."""
    C = preds[0].shape[-1]
    keep = mask.reshape(-1) > 0
    d = torch.cat([(p - t).reshape(-1, C)[keep] for p, t in zip(preds, tars)]).double()
    u = d / s.double()
    print(f"[{objective.space} {objective.kind}] min |d| {float(d.abs().min()):.3e}, min |u| {float(u.abs().min()):.3e}")
    assert float(d.abs().min()) > 1e-3
    if objective.kind == "huber":
        inner = (u.abs() <= objective.delta_tensor(C, "cpu")).double().mean()
        assert 0.25 <= float(inner) <= 0.75, float(inner)


def robust_oracle(eng, sim, data, later, sw, detach, objective, nw):
    """tests/test_hip_unroll.py::unrolled_oracle with `masked_loss` as the loss of every step."""
    node_in, tar, mask, m_gs, m_ids = data
    C = tar.shape[-1]
    tars = [tar, *(later if later is not None else [])]
    std = sim._targetNormalizer.std_with_epsilon().detach()
    sim.zero_grad(set_to_none=True)
    cur, preds, total = node_in, [], 0.0
    for k, w in enumerate(sw):
        pred = sim((cur, tars[k], mask, m_gs, m_ids), True, False)
        preds.append(pred.detach())
        total = total + w * eng.masked_loss(pred, tars[k], mask, objective, std, node_weights=nw)
        cur = torch.where(mask == 0, node_in, torch.cat([pred.detach() if detach else pred, node_in[..., C:]], dim=-1))
    total.backward()
    return torch.stack(preds), float(total.detach()), {k: q.grad.clone() for k, q in sim.named_parameters() if q.grad is not None}


def objective_case(eng, name):
    if name == "mae":
        return eng.Objective("physical", "mae"), None
    if name == "huber":
        return eng.Objective("normalized", "huber", delta=1.0), None
    nw = spread_weights(torch.Generator().manual_seed(41), 2, 300)
    return eng.Objective("normalized", "huber", [1.0, 3.0], True, delta=(0.6, 1.4)), nw


@pytest.mark.parametrize("K,detach", [(1, False), (2, False), (2, True)], ids=["K1", "K2", "K2-detached"])
@pytest.mark.parametrize("name", ["mae", "huber", "huber-weighted"])
def test_fused_step_follows_the_oracle(eng, graphs, name, K, detach):
    objective, nw = objective_case(eng, name)
    ref, data, later, preds0, s = offset_case(graphs, objective, K)
    tars = [data[1], *(later if later is not None else [])]
    assert_offsets(objective, preds0, tars, data[2], s)
    sw = [1.0] if K == 1 else [1.0, 0.5]
    key = ("robust", name, K, detach)
    r = three_way(ref, key, lambda sim, d, lat: robust_oracle(eng, sim, d, lat, sw, detach, objective, nw), data, later)
    mine, grads = engine_model(eng, ref)
    step = eng.FusedStep(mine, grads, unroll=K, step_weights=sw, detach=detach, objective=objective)
    args = (_cuda(data), True) if K == 1 else (_cuda(data), True, later.cuda())
    kw = {} if nw is None else dict(node_weights=nw.cuda())
    loss = step(*args, **kw)
    torch.cuda.synchronize()
    got = torch.stack([q.reshape(r["pred32"][0].shape) for q in step.predictions()]).cpu()
    std = ref._targetNormalizer.std_with_epsilon().detach()
    for k in range(K):
        want = float(eng.masked_loss(r["pred32"][k], tars[k], data[2], objective, std, node_weights=nw))
        e_p, e_l = rel_err(got[k], r["pred32"][k]), abs(float(step.step_losses()[k]) - want) / want
        print(f"[{key}] step {k}: prediction {e_p:.2e}, loss {e_l:.2e} from the fp32 oracle")
        assert e_p <= 1e-5 and e_l <= 1e-5, (k, e_p, e_l)
    assert abs(float(step.channel_losses().sum(1)[0]) - float(step.step_losses()[0])) <= 1e-6 * float(step.step_losses()[0])
    r.update(pred=got, loss=float(loss), gg={k: q.grad.detach().cpu() for k, q in mine.named_parameters() if q.requires_grad})
    check(r, str(key))


# ------------------------------------------------------------------------------------------------ 4: composition
def huber(eng):
    return eng.Objective("normalized", "huber", [1.0, 3.0], delta=(0.6, 1.4))


def test_graph_replay_with_changing_targets_equals_eager(eng, graphs):
    objective = huber(eng)
    ref, data, _, _, _ = offset_case(graphs, objective, 1)
    mine, grads = engine_model(eng, ref)
    gdata = _cuda(data)
    other = (gdata[0], gdata[1] + 0.25 * torch.randn(gdata[1].shape, generator=torch.Generator().manual_seed(5)).cuda(), *gdata[2:])
    eager, gstep = eng.FusedStep(mine, grads, objective=objective), eng.FusedStep(mine, grads, use_graph=True, objective=objective)
    seen, captured = [], None
    for d in (gdata, other, gdata, other):
        want = snapshot(eager, grads, eager(d, True))
        grads.flat.fill_(float("nan"))
        got = snapshot(gstep, grads, gstep(d, True))
        assert all(bit_equal(a, b) for a, b in zip(got, want)) and bit_equal(gstep.channel_losses(), eager.channel_losses())
        seen.append(want)
        captured = captured or gstep._graphs
        assert gstep._graphs is captured
    assert captured is not None and not bit_equal(seen[0][0], seen[1][0])
    assert all(bit_equal(a, b) for a, b in zip(seen[0], seen[2])) and all(bit_equal(a, b) for a, b in zip(seen[1], seen[3]))   # deterministic


def test_two_micro_batches_accumulate_to_the_batch_step(eng, graphs):
    """accumulate = 2, reduction = "batch", sample 0 then sample 1: grads.flat is the recurrence over the plain steps' gradients with
    the coefficients bsms_accum_coef formed from the [M | S] rows (the mse algebra of the physical space, which IS the robust loss),
    bit for bit; and the cycle is the oracle's ONE step on both samples by the three-way criterion.  Twice: the same bits."""
    objective, nw = objective_case(eng, "huber-weighted")
    ref, data, _, _, _ = offset_case(graphs, objective, 1)
    r = three_way(ref, ("robust", "huber-weighted", 1, False), lambda sim, d, lat: robust_oracle(eng, sim, d, None, [1.0], False, objective, nw), data)
    mine, grads = engine_model(eng, ref)
    gdata, gw = _cuda(data), nw.cuda()
    plain = eng.FusedStep(mine, grads, objective=objective)
    alone = []
    for b in (0, 1):
        loss = plain(part(gdata, [b])[0], True, node_weights=gw[b:b + 1])
        alone.append((loss.clone(), grads.flat.clone()))
    runs = []
    for _ in range(2):
        grads.flat.fill_(float("nan"))
        step = eng.FusedStep(mine, grads, accumulate=2, reduction="batch", objective=objective)
        preds = []
        for b in (0, 1):
            loss = step(part(gdata, [b])[0], True, node_weights=gw[b:b + 1])
            assert bit_equal(loss, alone[b][0])
            preds.append(step.prediction().clone())
        ab = step.accumulation_coefficients()
        assert step.ready and bit_equal(grads.flat, (ab[0] * alone[0][1]) + (ab[1] * alone[1][1]))
        runs.append((grads.flat.clone(), step.accumulated_loss().clone()))
    assert all(bit_equal(a, b) for a, b in zip(*runs))
    r.update(pred=torch.cat(preds).unsqueeze(0).cpu(), loss=float(step.accumulated_loss()),
             gg={k: q.grad.detach().cpu() for k, q in mine.named_parameters() if q.requires_grad})
    check(r, "robust accumulate")
    # an unrolled cycle under "batch" is legal for a robust kind and runs
    two = eng.FusedStep(mine, grads, accumulate=2, unroll=2, reduction="batch", objective=objective)
    later = gdata[1].unsqueeze(0) + 0.1
    for b in (0, 1):
        d, lat = part(gdata, [b], later)
        out = two(d, True, lat, node_weights=gw[b:b + 1])
    assert two.ready and bool(torch.isfinite(out)) and bool(torch.isfinite(grads.flat).all())


def test_recompute_frozen_input_grad_and_bf16(eng, graphs):
    objective = huber(eng)
    ref, data, _, _, _ = offset_case(graphs, objective, 1)
    gdata = _cuda(data)
    mine, grads = engine_model(eng, ref)
    step = eng.FusedStep(mine, grads, objective=objective)
    want = snapshot(step, grads, step(gdata, True))
    assert bool(torch.isfinite(want[2]).all()) and float(want[2].abs().max()) > 0
    again = snapshot(step, grads, step(gdata, True))
    assert all(bit_equal(a, b) for a, b in zip(again, want))                                  # deterministic
    full = {k: q.grad.clone() for k, q in mine.named_parameters() if q.requires_grad}
    for kw in (dict(recompute=True), dict(input_grad=True)):
        grads.flat.fill_(float("nan"))
        other = eng.FusedStep(mine, grads, objective=objective, **kw)
        got = snapshot(other, grads, other(gdata, True))
        assert all(bit_equal(a, b) for a, b in zip(got, want)), kw
    # input_gradient(...) against the autograd route through the drop-in modules and masked_loss
    from bsms_gnn_amd.step import input_gradient
    loss2, g2 = input_gradient(mine, gdata, objective=objective)
    assert bit_equal(loss2, want[0]) and bit_equal(g2, other.input_grad())
    auto = eng.BSMS_Simulator(ref.cfg)
    auto.load_state_dict(ref.state_dict())
    auto = auto.cuda()
    x = gdata[0].clone().requires_grad_(True)
    eng.masked_loss(auto((x, *gdata[1:]), True, False), gdata[1], gdata[2], objective, auto._targetNormalizer.std_with_epsilon()).backward()
    e_in = rel_err(g2.cpu(), x.grad.cpu())
    print(f"input gradient, fused step against the autograd route: {e_in:.2e}")
    assert e_in <= 1e-6
    # a frozen processor: the other MLPs' gradients are the all-trainable step's, bit for bit
    frozen, fgrads = engine_model(eng, ref, ("process",))
    fstep = eng.FusedStep(frozen, fgrads, objective=objective)
    assert bit_equal(fstep(gdata, True), want[0]) and bit_equal(fstep.prediction(), step.prediction())
    live = [k for k, q in frozen.named_parameters() if q.requires_grad]
    assert live and all(not k.startswith("process.") and bit_equal(dict(frozen.named_parameters())[k].grad, full[k]) for k in live)
    # bf16 (D = 128): one step, finite, the loss within the bf16 tests' 1e-2 of the fp32 step's
    ref2, data2 = make_oracle("split", graphs)
    g2data = _cuda(data2)
    losses = {}
    for precision in (None, "bf16"):
        m2, gr2 = engine_model(eng, ref2)
        if precision:
            m2.process.precision = precision
        losses[precision] = float(eng.FusedStep(m2, gr2, objective=objective)(g2data, True))
        assert bool(torch.isfinite(gr2.flat).all()) and float(gr2.flat.abs().max()) > 0
    assert abs(losses["bf16"] - losses[None]) <= 1e-2 * abs(losses[None]), losses


def _train(eng, iters=4):
    from test_datapipe import cfg as data_cfg
    from test_hip_databank import same_mesh_trajs
    dcfg = data_cfg(True, gamma=0.8)
    dcfg.noise_level = [0.02, 0.02, 0.01]
    bank = eng.TrajectoryBank(dcfg, seed=1)
    for t in same_mesh_trajs(120, 8, 2, seed=6):
        bank.add(t)
    model_cfg = SimpleNamespace(out_dim=3, latent_dim=32, hidden_layer=2, unet_depth=2, pos_dim=2, consistent_mesh=True,
                                accumulation_steps=1, loss_kind="huber", loss_space="normalized", loss_delta=1.0)
    opt_cfg = SimpleNamespace(peak_lr=1e-3, weight_decay=1e-4, warmup_steps=2, decay_steps=20, gnorm_clip=1.0)
    torch.manual_seed(0)
    tr = eng.Trainer(eng.BSMS_Simulator(model_cfg), model_cfg, opt_cfg)
    losses = []
    for _ in range(iters):
        out = tr.iter(bank.batch(bank.next_picks(2)))
        if out is not None:
            losses.append(out.clone())
    return tr, bank, losses, (model_cfg, opt_cfg)


def test_trainer_trains_on_the_huber_objective(eng, tmp_path):
    """model_cfg.loss_kind = "huber": one warm-up and three optimisation iterations, twice: the same losses and parameters bit for
    bit; get_loss is masked_loss of its own prediction; save / restore brings the parameters and the objective back."""
    tr, bank, losses, cfgs = _train(eng)
    tr2, _, losses2, _ = _train(eng)
    assert tr.objective == eng.Objective("normalized", "huber", delta=1.0) and tr.dp.fused.objective == tr.objective
    assert len(losses) == 3 and tr.train_step == 4 and all(bool(torch.isfinite(l)) for l in losses)
    assert all(bit_equal(a, b) for a, b in zip(losses, losses2)) and bit_equal(tr.optimizer.flat_p, tr2.optimizer.flat_p)
    batch = bank.batch([(0, 1), (1, 3)], train=False)
    pred = tr.get_pred(batch).detach()
    std = tr.model._targetNormalizer.std_with_epsilon()
    want = eng.masked_loss(pred, batch[1], batch[2], tr.objective, std)
    assert bit_equal(tr.get_loss(batch).detach(), want)
    assert abs(float(want) - float(eng.masked_rmse(pred, batch[1], batch[2]))) > 1e-4 * float(want)
    tr.save(str(tmp_path))
    torch.manual_seed(1)
    fresh = eng.Trainer(eng.BSMS_Simulator(cfgs[0]), *cfgs)
    fresh.restore(str(tmp_path), tr.train_step)
    assert fresh.objective == tr.objective and fresh.train_step == tr.train_step
    assert bit_equal(fresh.get_loss(batch).detach(), want)
    nxt = bank.batch(bank.next_picks(2))
    assert bit_equal(fresh.iter(nxt), tr.iter(nxt))


def _worker(rank, world, port, out_path):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    torch.cuda.set_device(0)
    from conftest import Golden
    import bsms_gnn_amd as eng
    from test_hip_robust import objective_case, offset_case
    objective, nw = objective_case(eng, "huber-weighted")
    ref, data, _, _, _ = offset_case(Golden("graphs"), objective, 1)
    torch.manual_seed(50 + rank)                             # different init per rank: the broadcast must fix it
    sim = eng.BSMS_Simulator(ref.cfg)
    sim.load_state_dict(ref.state_dict())                    # (the normalisers' statistics; rank 1's weights come from rank 0)
    if rank == 1:
        for q in sim.parameters():
            q.data.normal_()
    sim = sim.cuda()
    c, sl = (lambda t: t.cuda()), slice(rank, rank + 1)
    local = (c(data[0][sl]), c(data[1][sl]), c(data[2][sl]), [c(g[:1]) for g in data[3]], [c(i[:1]) for i in data[4]])
    engine = eng.DataParallel(sim, bucket_bytes=64 << 10, objective=objective)
    loss = engine.step_loss_backward(local, True, node_weights=nw[sl].cuda())
    torch.cuda.synchronize()
    torch.save({"loss": loss.detach().cpu(), "flat": engine.grads.flat.cpu(), "pred": engine.fused.prediction().cpu(),
                "gg": {k: q.grad.detach().cpu() for k, q in sim.named_parameters() if q.requires_grad}}, f"{out_path}.{rank}")
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.timeout(300)
def test_two_ranks_follow_the_oracles_two_sample_step(eng, graphs, tmp_path):
    """Two ranks over gloo on one GPU, one sample and its weights each: the all-reduced rows are [M | S], the ranks are bit-identical,
    and the result is the oracle's step on both samples by the three-way criterion."""
    objective, nw = objective_case(eng, "huber-weighted")
    ref, data, _, _, _ = offset_case(graphs, objective, 1)
    r = three_way(ref, ("robust", "huber-weighted", 1, False), lambda sim, d, lat: robust_oracle(eng, sim, d, None, [1.0], False, objective, nw), data)
    port = 33900 + os.getpid() % 2000
    out = str(tmp_path / "res")
    mp.start_processes(_worker, args=(2, port, out), nprocs=2, join=True, start_method="spawn")
    r0, r1 = torch.load(out + ".0"), torch.load(out + ".1")
    assert torch.equal(r0["flat"], r1["flat"]) and torch.equal(r0["loss"], r1["loss"])
    r.update(pred=torch.cat([r0["pred"].reshape(1, 300, 2), r1["pred"].reshape(1, 300, 2)]).unsqueeze(0), loss=float(r0["loss"]), gg=r0["gg"])
    check(r, "robust two ranks")


# ------------------------------------------------------------------------------------------------ 5: nothing else moved
def test_the_two_routes_never_call_each_others_entries(eng, graphs, monkeypatch):
    L = eng._abi.lib()
    new, old = ("bsms_robust_sums", "bsms_sim_robust_bwd"), ("bsms_error_sums", "bsms_error_sums_w", "bsms_sim_objective_bwd", "bsms_sim_objective_bwd_w")
    calls = {name: 0 for name in new + old}

    def counted(name):
        real = getattr(L, name)

        def f(*a):
            calls[name] += 1
            return real(*a)
        return f

    for name in calls:
        monkeypatch.setattr(L, name, counted(name))
    objective, nw = objective_case(eng, "huber-weighted")
    ref, data, _, _, _ = offset_case(graphs, objective, 1)
    mine, grads = engine_model(eng, ref)
    gdata = _cuda(data)
    later = gdata[1].unsqueeze(0) + 0.1
    for kw in (dict(), dict(objective=eng.Objective("normalized", "mse")), dict(objective=eng.Objective("normalized", "mse"), unroll=2)):
        step = eng.FusedStep(mine, grads, **kw)
        step(gdata, True, later) if kw.get("unroll") else step(gdata, True)
    step = eng.FusedStep(mine, grads, objective=eng.Objective("normalized", "rmse", node_weighted=True))
    step(gdata, True, node_weights=nw.cuda())
    torch.cuda.synchronize()
    assert all(calls[name] == 0 for name in new), calls
    assert calls["bsms_error_sums"] == 3 and calls["bsms_sim_objective_bwd"] == 3 and calls["bsms_error_sums_w"] == 1
    before = dict(calls)
    for objective_, kw, extra in ((eng.Objective(kind="mae"), dict(), {}), (huber(eng), dict(unroll=2), {}),
                                  (objective, dict(accumulate=2), dict(node_weights=nw.cuda()))):
        step = eng.FusedStep(mine, grads, objective=objective_, **kw)
        step(gdata, True, later, **extra) if kw.get("unroll") else step(gdata, True, **extra)
    torch.cuda.synchronize()
    assert all(calls[name] == before[name] for name in old), calls
    assert calls["bsms_robust_sums"] == 4 and calls["bsms_sim_robust_bwd"] == 4
