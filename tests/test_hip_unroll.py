"""GPU: the unrolled (K-step) training loss of step.FusedStep -- K forwards chained by the reference's
rollout rule (utils/rollout_utils.py:57-62), K backwards in reverse order with the gradient carried from step to step
(or cut, `detach=True`) -- against the CPU oracle unrolled here under autograd, plus the three entries it adds
(bsms_sim_unroll_bwd, bsms_grad_accumulate, bsms_batch_targets) on their own, the trajectory bank's horizon, the Trainer and
two data-parallel ranks.

Everything runs on the 300-node `del300` hierarchy with the golden `sim` batch (B = 2, C = 2, p = 2, 67 rows with mask == 0);
later targets are state + (k + 1) (tar - state).

Tolerances.  Predictions and the total loss: 1e-5 relative to the fp32 oracle (the fp32 oracle itself is 4e-8 .. 9e-8 from its
fp64 run over three steps).  Gradients: the three-way criterion of tests/test_hip_fullsize.py (`check`, factors 1.5 / 2.5,
floor 1e-5): the engine's distance to the fp64 oracle against the larger of the fp32 oracle's two distances (all threads, one
thread).  On these shapes the oracle's own distances are ~1e-6 (worst) and ~4e-7 (median), so the floor binds."""
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
from test_hip_fullsize import check

pytestmark = pytest.mark.gpu

SHAPES = {"ring": (32, 3, 3), "split": (128, 2, 2), "d64": (64, 2, 2)}       # name -> (D, H, depth)
# Weight seeds.  A ReLU input within fp32 round-off of 0 may land on either side of the kink in two correct fp32 implementations,
# and ONE such flip moves whole weight gradients by 1e-3 .. 1e-2 (conftest.KinkMargin).  K steps on 600 rows have ~7e6 ReLU inputs
# and an arbitrary seed leaves the nearest ~1e-8 from 0.  These are the seeds, out of 0..399, whose CPU-oracle forward over the K
# steps keeps every ReLU input farthest from 0 (conftest.pick_seed's rule, searched once): 5.9e-7 / 2.5e-7 / 3.7e-7.
# `oracle_runs` measures the margin again on every run and asserts MIN_MARGIN: 2.5 units of fp32 round-off at 1.0 (6e-8), which is
# what two fp32 summation orders of an O(1) pre-activation differ by.  If the oracle's initialisation or the golden batch ever
# changes, that assertion fails instead of the gradient check turning flaky; search the seeds again then.
SEEDS = {"ring": 65, "split": 387, "d64": 150}
MIN_MARGIN = 1.5e-7


@pytest.fixture(scope="module")
def eng():
    import bsms_gnn_amd as eng
    return eng


# ------------------------------------------------------------------------------------------------ inputs and the oracle
def later_targets(node_in, tar, K):
    state = node_in[..., :tar.shape[-1]]
    return torch.stack([state + (k + 1) * (tar - state) for k in range(1, K)]) if K > 1 else None


def sim_batch(graphs, depth):
    z = load_golden("sim")
    es, ids = graphs.levels("del300")
    B = 2
    m_gs = [e.unsqueeze(0).repeat(B, 1, 1) for e in es[:depth + 1]]
    m_ids = [i.unsqueeze(0).repeat(B, 1) for i in ids[:depth]]
    return (z.t("node_in"), z.t("tar"), z.t("mask"), m_gs, m_ids)


def make_oracle(shape, graphs, golden=False):
    """The fp32 oracle of one model shape with warmed normalisers (`golden`: the golden checkpoint, which has the ring shape)."""
    D, H, depth = SHAPES[shape]
    z = load_golden("sim")
    data = sim_batch(graphs, depth)
    torch.manual_seed(SEEDS[shape])
    ref = ro.BSMS_Simulator(ro.make_cfg(2, D, H, depth, 2))
    if golden:
        ref.load_state_dict(z.state_dict())
    else:
        for k in range(3):
            ref((z.t(f"warm_in{k}"), z.t(f"warm_tar{k}"), data[2], data[3], data[4]), True, True)
    return ref, data


def unrolled_oracle(sim, data, later, weights, detach, consistent=True):
    """The definition: pred_k = model(in_k); in_{k+1} = where(m == 0, in_0, cat[pred_k, rest of in_0]); loss = sum_k w_k rmse_k."""
    node_in, tar, mask, m_gs, m_ids = data
    C = tar.shape[-1]
    tars = [tar, *(later if later is not None else [])]
    sim.zero_grad(set_to_none=True)
    cur, preds, loss = node_in, [], 0.0
    for k, w in enumerate(weights):
        pred = sim((cur, tars[k], mask, m_gs, m_ids), consistent, False)
        preds.append(pred.detach())
        loss = loss + w * ro.masked_rmse(pred, tars[k], mask)
        cur = torch.where(mask == 0, node_in, torch.cat([pred.detach() if detach else pred, node_in[..., C:]], dim=-1))
    loss.backward()
    return torch.stack(preds), float(loss.detach()), {k: p.grad.clone() for k, p in sim.named_parameters() if p.grad is not None}


def _f64(obj):
    if isinstance(obj, (list, tuple)):
        return type(obj)(_f64(o) for o in obj)
    return obj.double() if obj.is_floating_point() else obj


_ORACLE = {}


def oracle_runs(ref, data, later, weights, detach, key, consistent=True):
    """fp32 on all threads, fp32 on one thread, fp64: computed once per configuration and shared."""
    if key not in _ORACLE:
        with KinkMargin(ref) as km:
            pred32, loss32, g32 = unrolled_oracle(ref, data, later, weights, detach, consistent)
        print(f"[{key}] smallest |ReLU input| of the oracle over the {len(weights)} steps: {km.min:.2e}")
        assert km.min >= MIN_MARGIN, (key, "the weight seed no longer keeps the ReLU inputs away from 0", km.min)
        n = torch.get_num_threads()
        torch.set_num_threads(1)
        try:
            _, _, g32_one = unrolled_oracle(ref, data, later, weights, detach, consistent)
        finally:
            torch.set_num_threads(n)
        ref64 = ro.BSMS_Simulator(ref.cfg, dtype=torch.float64)
        ref64.load_state_dict(ref.state_dict())
        ref64.double()
        _, loss64, g64 = unrolled_oracle(ref64, _f64(data), None if later is None else later.double(), weights, detach, consistent)
        _ORACLE[key] = dict(pred32=pred32, loss32=loss32, loss64=loss64, g32=g32, g32_one=g32_one, g64=g64, t32=0.0, t64=0.0, levels=key)
    return _ORACLE[key]


def _cuda(obj):
    if isinstance(obj, (list, tuple)):
        return type(obj)(_cuda(o) for o in obj)
    return obj.cuda()


def engine_step(eng, ref, data, later, weights, detach, precision=None, consistent=True, gpu_data=None):
    mine = eng.BSMS_Simulator(ref.cfg)
    mine.load_state_dict(ref.state_dict())
    mine = mine.cuda()
    if precision:
        mine.process.precision = precision
    grads = eng.GradBuckets(list(mine.parameters()))
    step = eng.FusedStep(mine, grads, unroll=len(weights), step_weights=weights, detach=detach)
    loss = step(_cuda(data) if gpu_data is None else gpu_data, consistent, None if later is None else later.cuda())
    torch.cuda.synchronize()
    return mine, grads, step, loss


def compare(eng, ref, data, later, weights, detach, key, consistent=True, gpu_data=None):
    r = dict(oracle_runs(ref, data, later, weights, detach, key, consistent))
    mine, grads, step, loss = engine_step(eng, ref, data, later, weights, detach, consistent=consistent, gpu_data=gpu_data)
    preds = torch.stack([p.reshape(r["pred32"][0].shape) for p in step.predictions()]).cpu()
    for k in range(len(weights)):
        e = rel_err(preds[k], r["pred32"][k])
        print(f"[{key}] step {k}: prediction {e:.2e} from the fp32 oracle")
        assert e <= 1e-5, (key, k, e)
    assert torch.equal(step.prediction(), step.predictions()[-1])
    want = [float(ro.masked_rmse(r["pred32"][k], t, data[2])) for k, t in enumerate([data[1], *(later if later is not None else [])])]
    assert torch.allclose(step.step_losses().cpu(), torch.tensor(want), rtol=1e-5, atol=0)
    r.update(pred=preds, loss=float(loss), gg={k: p.grad.detach().cpu() for k, p in mine.named_parameters() if p.requires_grad})
    check(r, str(key))
    return r


def median_distance(ga, gb):
    return float(np.median([rel_err(ga[k], gb[k]) for k in sorted(gb)]))


# ------------------------------------------------------------------------------------------------ 1: unroll = 1 is today's step
@pytest.mark.parametrize("shape,precision", [("ring", None), ("split", None), ("split", "bf16")])
def test_unroll_one_is_the_existing_step_bit_for_bit(eng, graphs, shape, precision):
    ref, data = make_oracle(shape, graphs)
    mine = eng.BSMS_Simulator(ref.cfg)
    mine.load_state_dict(ref.state_dict())
    mine = mine.cuda()
    if precision:
        mine.process.precision = precision
    gdata = _cuda(data)
    grads = eng.GradBuckets(list(mine.parameters()))
    base = eng.FusedStep(mine, grads)
    l0 = base(gdata, True)
    flat0, pred0 = grads.flat.clone(), base.prediction().clone()
    grads.flat.fill_(float("nan"))
    one = eng.FusedStep(mine, grads, unroll=1, step_weights=[1.0], detach=False)
    l1 = one(gdata, True, later_targets=None)
    assert torch.equal(l0, l1) and torch.equal(one.prediction(), pred0) and torch.equal(grads.flat, flat0)
    assert torch.equal(one.step_losses(), l0.reshape(1)) and len(one.predictions()) == 1
    with pytest.raises(ValueError):
        one(gdata, True, later_targets=later_targets(gdata[0], gdata[1], 2))


# ------------------------------------------------------------------------------------------------ 2, 3: K steps against the oracle
@pytest.mark.parametrize("shape", ["ring", "split"])
def test_three_steps_match_the_unrolled_oracle(eng, graphs, shape):
    """Full back-propagation through time and the detached ("pushforward") form, K = 3, both against the oracle; and the two must
    really differ -- a carry that is silently dropped would make them equal (the oracle's own two gradients are asserted to be that far apart too,
    so the guard means something for these seeds; measured on the CPU oracle: a median relative distance of 1.0 for both shapes)."""
    ref, data = make_oracle(shape, graphs)
    later, w = later_targets(data[0], data[1], 3), [1 / 3] * 3
    full = compare(eng, ref, data, later, w, False, (shape, 3, "bptt"))
    cut = compare(eng, ref, data, later, w, True, (shape, 3, "detached"))
    assert torch.equal(full["pred"], cut["pred"]) and full["loss"] == cut["loss"]         # the forward does not know about detach
    d_gpu, d_cpu = median_distance(full["gg"], cut["gg"]), median_distance(full["g32"], cut["g32"])
    print(f"[{shape}] BPTT vs detached gradients, median relative distance: engine {d_gpu:.3f}, oracle {d_cpu:.3f}")
    assert d_cpu >= 0.1 and d_gpu >= 0.1, (d_cpu, d_gpu)


@pytest.mark.parametrize("detach", [False, True])
def test_four_steps_with_uneven_weights_at_d64(eng, graphs, detach):
    ref, data = make_oracle("d64", graphs)
    compare(eng, ref, data, later_targets(data[0], data[1], 4), [0.4, 0.3, 0.2, 0.1], detach, ("d64", 4, "detached" if detach else "bptt"))


# ------------------------------------------------------------------------------------------------ 4: variable meshes
def test_two_steps_on_a_block_diagonal_batch(eng, graphs):
    """consistent=False at K = 2 on the golden block-diagonal batch (del64 + del300 in one graph, 364 rows, depth 2)."""
    z = load_golden("blockdiag")
    es, ids = [z.t(f"cat/e{l}") for l in range(3)], [z.t(f"cat/ids{l}") for l in range(2)]
    pos = torch.cat([torch.tensor(graphs.np(f"{nm}/pos")[:, :2], dtype=torch.float32) for nm in ("del64", "del300")])
    n = pos.shape[0]
    gen = torch.Generator().manual_seed(5)
    state = torch.randn(n, 2, generator=gen)
    typ = (torch.rand(n, 1, generator=gen) < 0.2).float() * 4.0
    x, y, mask = torch.cat([state, pos, typ], -1), state + 0.1 * torch.randn(n, 2, generator=gen), (typ == 0).float()
    assert n == 364 and 0 < int((mask == 0).sum()) < n
    data = (x.unsqueeze(0), y.unsqueeze(0), mask.unsqueeze(0), es, ids)
    torch.manual_seed(26)                                              # kink margin 2.0e-6 over the two steps (see SEEDS)
    ref = ro.BSMS_Simulator(ro.make_cfg(2, 32, 2, 2, 2))
    ref(data, False, True)
    sizes = [n, ids[0].numel(), ids[1].numel()]
    levels = [eng.LevelData(es[l], sizes[l], face=ids[l] if l < 2 else None, x=x if l == 0 else None, y=y if l == 0 else None,
                            mask=mask if l == 0 else None).to("cuda") for l in range(3)]
    later = later_targets(data[0], data[1], 2)                         # [1, 1, rows, C]
    compare(eng, ref, data, later, [0.5, 0.5], False, ("blockdiag", 2, "bptt"), consistent=False, gpu_data=levels)
    # the documented variable-mesh layout [K-1, rows, C] gives the same step
    mine, grads, step, loss = engine_step(eng, ref, data, later, [0.5, 0.5], False, consistent=False, gpu_data=levels)
    flat = grads.flat.clone()
    assert torch.equal(step(levels, False, later[:, 0].cuda()), loss) and torch.equal(grads.flat, flat)


# ------------------------------------------------------------------------------------------------ 5: determinism, aliasing
def test_two_runs_are_bit_equal_and_grads_alias_the_flat_buffer(eng, graphs):
    ref, data = make_oracle("ring", graphs)
    later = later_targets(data[0], data[1], 3)
    mine, grads, step, l0 = engine_step(eng, ref, data, later, [1 / 3] * 3, False)
    flat0 = grads.flat.clone()
    grads.flat.fill_(float("nan"))                                     # whatever the buffer held is overwritten
    l1 = step(_cuda(data), True, later.cuda())
    assert torch.equal(l0, l1) and torch.equal(grads.flat, flat0) and bool(torch.isfinite(flat0).all())
    for p in grads.params:
        off, n = grads._slot[p]
        assert p.grad is not None and p.grad.data_ptr() == grads.flat.data_ptr() + 4 * off and p.grad.shape == p.shape
    with pytest.raises(ValueError):
        step(_cuda(data), True)                                        # unroll = 3 needs its later targets
    with pytest.raises(RuntimeError):
        step(_cuda(data), True, later[:1].cuda())                      # ... all K - 1 of them


# ------------------------------------------------------------------------------------------------ 6: bsms_sim_unroll_bwd alone
def _stats(C, gen):
    mean = torch.randn(C, generator=gen, dtype=torch.float64)
    return mean, mean * mean + 0.5 + torch.rand(C, generator=gen, dtype=torch.float64), torch.tensor(1e-8, dtype=torch.float64)


@pytest.mark.parametrize("C", [1, 8])
def test_sim_unroll_bwd_kernel(eng, C):
    """R = 257: two blocks and a ragged tail.  Without a carried pair and with w = 1 the launch IS bsms_sim_loss_bwd; with one it
    follows the fp64 restatement to 1e-6 (at most eight fp32 roundings of 6e-8 each), and rows with mask == 0 carry nothing."""
    L, R = eng._abi.lib(), 257
    gen = torch.Generator().manual_seed(C)
    pred, tar = torch.randn(R, C, generator=gen), torch.randn(R, C, generator=gen)
    mask = (torch.rand(R, generator=gen) < 0.8).float()
    mask[0], mask[R - 1] = 0.0, 1.0
    o_stats, i_stats = _stats(C, gen), _stats(C + 1, gen)
    g_next, g_nin = torch.randn(R, C, generator=gen), torch.randn(R, C + 1, generator=gen)
    g_next[mask == 0], g_nin[mask == 0] = float("inf"), float("nan")      # must never reach the result
    sums = torch.stack([(((pred - tar) ** 2) * mask[:, None]).sum(), mask.sum()]).float()
    d = lambda t: t.cuda()
    dp, dt, dm, ds, dgn, dgi = d(pred), d(tar), d(mask), d(sums), d(g_next), d(g_nin)
    do, di = [d(t) for t in o_stats], [d(t) for t in i_stats]
    s = torch.cuda.current_stream().cuda_stream
    p = lambda t: None if t is None else t.data_ptr()

    def run(w, nxt, nin):
        loss, gp, gnp = torch.full((1,), -1.0, device="cuda"), torch.full((R, C), 7.0, device="cuda"), torch.full((R, C), 7.0, device="cuda")
        eng._abi.check(L.bsms_sim_unroll_bwd(p(dp), p(dt), p(dm), R, C, *map(p, do), *map(p, di), p(ds), w, p(nxt), p(nin), p(loss), p(gp), p(gnp), s),
                       "bsms_sim_unroll_bwd")
        return loss.cpu(), gp.cpu(), gnp.cpu()

    loss0, gnp0 = torch.full((1,), -1.0, device="cuda"), torch.full((R, C), 7.0, device="cuda")
    eng._abi.check(L.bsms_sim_loss_bwd(p(dp), p(dt), p(dm), R, C, *map(p, do), p(ds), p(loss0), p(gnp0), s), "bsms_sim_loss_bwd")
    loss1, gp1, gnp1 = run(1.0, None, None)
    assert torch.equal(loss1, loss0.cpu()) and torch.equal(gnp1, gnp0.cpu())

    w = 0.375
    loss2, gp2, gnp2 = run(w, dgn, dgi)
    std = lambda st: np.maximum(np.sqrt(st[1].numpy() - st[0].numpy() ** 2), float(st[2]))
    P, T, M = pred.double().numpy(), tar.double().numpy(), mask.double().numpy()[:, None]
    S_, M_ = float(sums[0]), float(sums[1])
    loss = np.sqrt(S_ / M_ / C)
    with np.errstate(invalid="ignore"):
        carry = np.where(M != 0, g_next.double().numpy() + g_nin.double().numpy()[:, :C] / std(i_stats)[:C], 0.0)
    want_gp = w * ((P - T) * M / (loss * M_ * C)) + carry
    want_gnp = want_gp * M * std(o_stats)
    assert abs(float(loss2) - loss) <= 1e-6 * loss
    for got, want in ((gp2, want_gp), (gnp2, want_gnp)):
        assert np.abs(got.double().numpy() - want).max() <= 1e-6 * np.abs(want).max()
        assert bool((got[mask == 0] == 0).all())                       # exactly 0: no carry, no loss term on Dirichlet rows


@pytest.mark.parametrize("C", [1, 8])
def test_every_carried_entry_runs_the_one_tail(eng, C):
    """The step weight, the carry and the way out are ONE tail (csrc/objective_row.h: objective_tail) behind every loss-gradient entry
    that takes a carried pair.  With pred == target every loss term is exactly 0, whatever the (finite, non-zero) sums say, so g_pred
    and grad_norm_pred are the tail's alone: equal bit for bit across the entries, and equal to the tail restated in NumPy with the
    same roundings -- exact IEEE arithmetic, no tolerance.  R = 257: two blocks and a ragged tail; the rows with mask == 0 carry
    inf / nan, which must come out as exactly 0."""
    from bsms_gnn_amd.graph import LevelPlan
    L, X, R, w = eng._abi.lib(), eng._abi.ext(), 257, 0.375
    gen = torch.Generator().manual_seed(40 + C)
    pred = torch.randn(R, C, generator=gen)
    mask = (torch.rand(R, generator=gen) < 0.8).float()
    mask[0], mask[R - 1] = 0.0, 1.0
    o_stats, i_stats = _stats(C, gen), _stats(C + 1, gen)
    g_next, g_nin = torch.randn(R, C, generator=gen), torch.randn(R, C + 1, generator=gen)
    g_next[mask == 0], g_nin[mask == 0] = float("inf"), float("nan")      # must never reach the result
    pair = torch.tensor([3.0, 200.0])                                     # fp32 [S, M]
    row = torch.cat([torch.tensor([200.0]), 0.5 + torch.rand(C, generator=gen)]).double()          # fp64 [M | SE] or [M | S]
    erow = torch.cat([torch.tensor([300.0]), 0.5 + torch.rand(C, generator=gen)]).double()         # fp64 [ME | DE]
    weights, delta = 0.5 + torch.rand(R, generator=gen), (0.5 + torch.rand(C, generator=gen)).double()
    ring = torch.arange(R)
    plan = LevelPlan(torch.stack([torch.cat([ring, (ring + 1) % R]), torch.cat([(ring + 1) % R, ring])]), R, device="cuda")
    d = lambda t: t.cuda()
    dp, dm, dgn, dgi, dpair, drow, derow, dwt, ddl = (d(t) for t in (pred, mask, g_next, g_nin, pair, row, erow, weights, delta))
    dt = dp.clone()                                                       # pred == target exactly
    do, di = [d(t) for t in o_stats], [d(t) for t in i_stats]
    s = torch.cuda.current_stream().cuda_stream
    p = lambda t: None if t is None else t.data_ptr()
    rows, stats = (p(dp), p(dt), p(dm)), (*map(p, do), *map(p, di))

    def run(name, call):
        gp, gnp = torch.full((R, C), 7.0, device="cuda"), torch.full((R, C), 7.0, device="cuda")
        eng._abi.check(call((w, p(dgn), p(dgi), None), (p(gp), p(gnp), s)), name)
        return name, gp.cpu(), gnp.cpu()

    MSE, PHYSICAL, NORMALIZED, MAE, HUBER = 0, 0, 1, 0, 1
    got = [
        run("bsms_sim_unroll_bwd", lambda c, o: L.bsms_sim_unroll_bwd(*rows, R, C, *stats, p(dpair), *c, *o)),
        run("bsms_sim_objective_bwd", lambda c, o: L.bsms_sim_objective_bwd(*rows, R, C, *stats, p(drow), None, NORMALIZED, MSE, *c, None, *o)),
        run("bsms_sim_objective_bwd_w", lambda c, o: L.bsms_sim_objective_bwd_w(*rows, p(dwt), R, R, C, *stats, p(drow), None, PHYSICAL, MSE, *c, None, *o)),
        run("bsms_sim_robust_bwd(mae)", lambda c, o: L.bsms_sim_robust_bwd(*rows, None, 1, R, C, *stats, p(drow), None, None, NORMALIZED, MAE, *c, None, *o)),
        run("bsms_sim_robust_bwd(huber, weights)", lambda c, o: L.bsms_sim_robust_bwd(*rows, p(dwt), R, R, C, *stats, p(drow), None, p(ddl), PHYSICAL, HUBER,
                                                                                       *c, None, *o)),
        run("bsms_sim_edge_objective_bwd", lambda c, o: X.bsms_sim_edge_objective_bwd(plan.handle, R, 1, *rows, None, C, 2, 0, *stats, p(drow), p(derow), None,
                                                                                      PHYSICAL, MSE, 0.25, *c, None, None, *o)),
    ]
    std = lambda st: np.maximum(np.nan_to_num(np.sqrt(st[1].numpy() - st[0].numpy() * st[0].numpy())), float(st[2]))      # fp64
    m = mask.numpy()[:, None]
    with np.errstate(invalid="ignore"):
        through_norm = (g_nin.numpy()[:, :C].astype(np.float64) / std(i_stats)[:C]).astype(np.float32)
        g_state = np.where(m != 0, g_next.numpy() + through_norm, np.float32(0))
    assert g_state.dtype == np.float32 and np.isfinite(g_state).all() and (g_state[mask.numpy() != 0] != 0).all()
    want_gnp = ((g_state * m).astype(np.float64) * std(o_stats)).astype(np.float32)
    for name, gp, gnp in got:
        assert torch.equal(gp, torch.from_numpy(g_state)), name
        assert torch.equal(gnp, torch.from_numpy(want_gnp)), name
        assert torch.equal(gp, got[0][1]) and torch.equal(gnp, got[0][2]), name
        assert bool((gp[mask == 0] == 0).all()) and bool((gnp[mask == 0] == 0).all()), name


# ------------------------------------------------------------------------------------------------ 7: bsms_grad_accumulate alone
@pytest.mark.parametrize("n", [1, 1023, (1 << 20) + 3, 4 * 2048 * 256 + 4 * 300 + 3])   # the last: past the 2048 x 256 grid stride of float4s
def test_grad_accumulate_kernel(eng, n):
    L, s = eng._abi.lib(), torch.cuda.current_stream().cuda_stream
    gen = torch.Generator().manual_seed(n)
    acc, g = torch.randn(n + 2, generator=gen).cuda(), torch.randn(n + 2, generator=gen).cuda()
    want, guard = acc[:n] + g[:n], acc[n:].clone()
    eng._abi.check(L.bsms_grad_accumulate(acc.data_ptr(), g.data_ptr(), n, 0, s), "bsms_grad_accumulate")
    assert torch.equal(acc[:n], want) and torch.equal(acc[n:], guard)            # bit-equal to torch's fp32 add; nothing past n
    acc[:n] = float("nan")
    eng._abi.check(L.bsms_grad_accumulate(acc.data_ptr(), g.data_ptr(), n, 1, s), "bsms_grad_accumulate")
    assert torch.equal(acc[:n], g[:n]) and torch.equal(acc[n:], guard)           # first: stale contents (NaNs) are overwritten
    if n > 8:                                                                    # a 4-byte-aligned pair takes the scalar path
        a2, g2 = acc[1:n].clone(), g[2:n + 1]
        w2 = a2 + g2
        a3 = torch.empty(n, device="cuda")
        a3[1:] = a2
        eng._abi.check(L.bsms_grad_accumulate(a3[1:].data_ptr(), g2.data_ptr(), n - 1, 0, s), "bsms_grad_accumulate")
        assert torch.equal(a3[1:], w2)


# ------------------------------------------------------------------------------------------------ 8: bank horizon, bsms_batch_targets
def _state(traj, t):
    return torch.cat([torch.tensor(traj["velocity"][t]), torch.tensor(traj["density"][t])], -1)


def test_bank_horizon_consistent_mesh(eng):
    from test_datapipe import cfg as data_cfg
    from test_hip_databank import same_mesh_trajs
    dcfg = data_cfg(True, gamma=0.8)
    trajs = same_mesh_trajs(300, 7, 2, seed=4)                        # 300 rows x 3 channels = 900 floats: four blocks per sample, ragged
    one, three = eng.TrajectoryBank(dcfg, seed=3), eng.TrajectoryBank(dcfg, seed=3, horizon=3)
    for t in trajs:
        one.add(t), three.add(t)
    assert one.lengths == [6, 6] and three.lengths == [4, 4]
    picks = [(0, 3), (1, 0), (1, 3), (0, 1)]
    (batch, later, noise) = three.batch(picks, train=True, draw=5, return_noise=True)
    want, want_noise = one.batch(picks, train=True, draw=5, return_noise=True)
    assert float(noise.abs().max()) > 0 and torch.equal(noise, want_noise)
    for name, a, b in zip(("node_in", "node_tar", "node_mask"), batch, want):
        assert torch.equal(a, b), name                                # the first step is today's batch, noise and gamma correction included
    assert later.shape == (2, 4, 300, 3) and later.is_contiguous()
    for j in range(2):
        for b, (si, ti) in enumerate(picks):
            assert torch.equal(later[j, b].cpu(), _state(trajs[si], ti + 2 + j)), (j, b)
    assert len(three.batch(picks, train=False)) == 2 and len(three.batch(picks, train=False, horizon=1)) == 5
    assert three.batch(picks[:2], train=False, horizon=2)[1].shape == (1, 2, 300, 3)
    with pytest.raises(IndexError):
        three.batch([(0, 4)])                                         # T - 3: frame t + 3 does not exist
    assert one.batch([(0, 4)], horizon=2)[1].shape == (1, 1, 300, 3)  # ... frame t + 2 does
    with pytest.raises(ValueError):
        eng.TrajectoryBank(dcfg, horizon=7).add(trajs[0])             # 7 frames cannot feed 7 steps
    assert three.trajectory(0)[0].shape[0] == 6                       # rollouts still see every frame
    picks = three.next_picks(100)
    assert len(picks) == 8 and all(ti < 4 for _, ti in picks)


def test_bank_horizon_variable_meshes(eng):
    from test_datapipe import cfg as data_cfg, synthetic_traj
    from test_hip_databank import model_cfg
    dcfg = data_cfg(False, gamma=0.8)
    trajs = [synthetic_traj(100, 5, 1), synthetic_traj(140, 6, 2)]
    torch.manual_seed(0)
    process = eng.BSMS_Simulator(model_cfg(False)).cuda().process
    one = eng.TrajectoryBank(dcfg, dataset="cylinder_flow", process=process, seed=9)
    three = eng.TrajectoryBank(dcfg, dataset="cylinder_flow", process=process, seed=9, horizon=3)
    for t in trajs:
        one.add(t), three.add(t)
    assert three.lengths == [2, 3]
    picks = [(1, 2), (0, 1), (1, 0)]
    levels, later = three.batch(picks, train=True, draw=2)
    want = one.batch(picks, train=True, draw=2)
    for name in ("x", "y", "mask"):
        assert torch.equal(getattr(levels[0], name), getattr(want[0], name)), name
    assert later.shape == (2, 380, 3)
    for j in range(2):
        assert torch.equal(later[j].cpu(), torch.cat([_state(trajs[si], ti + 2 + j) for si, ti in picks])), j
    with pytest.raises(IndexError):
        three.batch([(0, 2)])                                         # T - 3 of the five-frame trajectory


# ------------------------------------------------------------------------------------------------ 9: the Trainer
def test_trainer_with_three_unrolled_steps_follows_the_cpu_loop(eng):
    """Warm-up + three optimisation iterations of Trainer.iter fed from TrajectoryBank(horizon=3) == the same loop written with
    the unrolled CPU oracle, torch clip_grad_norm_ and torch.optim.AdamW; tolerances of
    test_hip_training.py::test_trainer_iterations_follow_cpu_reference_loop."""
    from test_datapipe import cfg as data_cfg
    from test_hip_databank import same_mesh_trajs
    dcfg = data_cfg(True, gamma=0.8)
    dcfg.noise_level = [0.02, 0.02, 0.01]
    bank = eng.TrajectoryBank(dcfg, seed=1, horizon=3)
    for t in same_mesh_trajs(120, 8, 2, seed=6):
        bank.add(t)
    model_cfg = SimpleNamespace(out_dim=3, latent_dim=32, hidden_layer=2, unet_depth=2, pos_dim=2, consistent_mesh=True,
                                accumulation_steps=1, unroll_steps=3)
    opt_cfg = SimpleNamespace(peak_lr=1e-3, weight_decay=1e-4, warmup_steps=2, decay_steps=20, gnorm_clip=1.0)
    torch.manual_seed(0)
    ref = ro.BSMS_Simulator(model_cfg)
    mine = eng.BSMS_Simulator(model_cfg)
    mine.load_state_dict(ref.state_dict())
    tr = eng.Trainer(mine, model_cfg, opt_cfg)
    assert tr.dp.fused.unroll == 3 and tr.dp.fused.detach is False
    opt = torch.optim.AdamW([p for p in ref.parameters() if p.requires_grad], lr=opt_cfg.peak_lr, weight_decay=opt_cfg.weight_decay)
    sch = eng.WarmupCosineDecay(opt_cfg.peak_lr, opt_cfg.warmup_steps, opt_cfg.decay_steps)
    losses, losses_ref = [], []
    cpu = lambda o: type(o)(cpu(x) for x in o) if isinstance(o, (list, tuple)) else o.cpu()
    for it in range(4):
        batch, later = bank.sample(2)
        data, lat = cpu(batch), later.cpu()
        if it < model_cfg.accumulation_steps:
            ref(data, True, True)
        else:
            opt.zero_grad()
            _, loss, _ = unrolled_oracle(ref, data, lat, [1 / 3] * 3, False)
            torch.nn.utils.clip_grad_norm_(ref.parameters(), opt_cfg.gnorm_clip)
            for group in opt.param_groups:
                group["lr"] = sch.lr()
            opt.step()
            sch.step()
            losses_ref.append(loss)
        out = tr.iter((batch, later))
        if out is not None:
            losses.append(float(out))
    assert len(losses) == 3 and tr.train_step == 4
    for a, b in zip(losses, losses_ref):
        assert abs(a - b) < 2e-4 * abs(b), (losses, losses_ref)
    for (k, p), (_, q) in zip(ref.named_parameters(), mine.named_parameters()):
        if p.requires_grad:
            assert rel_err(q.detach().cpu(), p.detach()) < 2e-3, k
    with pytest.raises(ValueError):
        tr.iter(batch)                                                # unroll_steps = 3 takes (batch, later_targets)
    assert torch.isfinite(tr.get_loss(batch))                         # get_loss is the single-step loss, unchanged


# ------------------------------------------------------------------------------------------------ 10: two ranks
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
    torch.manual_seed(50 + rank)                                      # different init per rank: the broadcast must fix it
    sim = eng.BSMS_Simulator(ro.make_cfg(2, 32, 3, 3, 2))
    if rank == 0:
        sim.load_state_dict(z.state_dict())
    sim = sim.cuda()
    c, sl = (lambda t: t.cuda()), slice(rank, rank + 1)
    data = (c(z.t("node_in")[sl]), c(z.t("tar")[sl]), c(z.t("mask")[sl]), [c(e.unsqueeze(0)) for e in es], [c(i.unsqueeze(0)) for i in ids])
    engine = eng.DataParallel(sim, bucket_bytes=64 << 10, unroll=2)
    loss = engine.step_loss_backward(data, True, later_targets(data[0], data[1], 2))
    torch.cuda.synchronize()
    torch.save({"loss": loss.detach().cpu(), "flat": engine.grads.flat.cpu(), "step_losses": engine.fused.step_losses().cpu()}, f"{out_path}.{rank}")
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.timeout(300)
def test_two_ranks_equal_the_single_process_step(eng, graphs, tmp_path):
    """Two ranks over gloo on one GPU, one golden sample each, K = 2: one all-reduce of the [K, 2] loss sums, one of the flat
    gradients; the result is the single-process step on the whole batch (tolerances of tests/test_hip_dp.py)."""
    port = 29900 + os.getpid() % 2000
    out = str(tmp_path / "res")
    mp.start_processes(_worker, args=(2, port, out), nprocs=2, join=True, start_method="spawn")
    r0, r1 = torch.load(out + ".0"), torch.load(out + ".1")
    assert torch.equal(r0["flat"], r1["flat"]) and torch.equal(r0["loss"], r1["loss"])         # bit-identical across ranks
    ref, data = make_oracle("ring", graphs, golden=True)
    mine, grads, step, loss = engine_step(eng, ref, data, later_targets(data[0], data[1], 2), [0.5, 0.5], False)
    assert abs(float(r0["loss"]) - float(loss)) < 1e-5 * abs(float(loss))
    assert rel_err(r0["step_losses"], step.step_losses().cpu()) < 1e-5
    assert rel_err(r0["flat"], grads.flat.cpu()) < 2e-5
