"""GPU: the training objectives -- bsms_sim_objective_bwd on its own against NumPy fp64 and against the kernel
of the default loss, the default route of step.FusedStep left bit for bit where it was, the fused step (single and unrolled)
against the CPU oracle under autograd with the loss restated here in torch, the autograd route, the Trainer, two data-parallel
ranks and the HIP-graph replay.

The definition (restated in `loss_def`): d = fl32(pred - tar), M = sum m, SE_c = sum m d_c^2 (fp64), a_c = w_c (physical) or
w_c / std_c^2 (normalized), Q = sum_c a_c SE_c / (M C), loss = Q (mse) or sqrt(Q) (rmse).

Meshes: the 300-node `del300` hierarchy.  Items 3, 5, 7, 8 use the golden `sim` batch (B = 2, C = 2).  Item 4 and the Trainer need
three channels (weights [1, 1, 3]): `three_channel_batch` adds a third channel to the golden batch that lives in units 1e-3 of
the others -- state AND target, so that the target normaliser's std of that channel is 1e-3 of the others (it normalises
tar - state), as the density of the airfoil data against its velocities.

Tolerances.  Kernel against NumPy: 1e-6 of the largest entry, the figure tests/test_hip_unroll.py::test_sim_unroll_bwd_kernel uses
for bsms_sim_unroll_bwd against its restatement (same arithmetic depth: at most eight fp32 roundings of 6e-8 each).  Fused step
against the oracle: predictions and losses 1e-5, gradients by the three-way criterion of tests/test_hip_fullsize.py (`check`)."""
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
from test_hip_unroll import MIN_MARGIN, _cuda, _f64, check, later_targets, sim_batch

pytestmark = pytest.mark.gpu

KERNEL_TOL = 1e-6            # tests/test_hip_unroll.py::test_sim_unroll_bwd_kernel, see the module docstring
PAIRS = [("physical", "rmse"), ("physical", "mse"), ("normalized", "rmse"), ("normalized", "mse")]
SPACE_ID, KIND_ID = {"physical": 0, "normalized": 1}, {"rmse": 0, "mse": 1}
SHAPE3 = (32, 3, 3)          # D, H, depth of the three-channel model of item 4
# Weight seed of the three-channel model: out of 0..399 the one whose CPU-oracle forward over the two unrolled steps keeps every
# ReLU input farthest from 0 (the rule of tests/test_hip_unroll.py::SEEDS, searched once on the CPU oracle: 5.5e-7).  `oracle_runs3`
# measures it on every run and asserts MIN_MARGIN.
SEED3 = 64


@pytest.fixture(scope="module")
def eng():
    import bsms_gnn_amd as eng
    return eng


# ------------------------------------------------------------------------------------------------ the definition, in torch
def loss_def(pred, tar, mask, space, kind, weights, std):
    """The definition; fp64 from the subtraction on (which happens in the dtype of `pred`).  Returns (loss, per-channel terms)."""
    C = pred.shape[-1]
    d = (pred - tar).double()
    m = mask.double().reshape(*pred.shape[:-1], 1)
    M, SE = m.sum(), (m * d * d).reshape(-1, C).sum(0)
    a = torch.ones(C, dtype=torch.float64) if weights is None else torch.tensor(weights, dtype=torch.float64)
    if space == "normalized":
        a = a / std.double() ** 2
    terms = a * SE / (M * C)
    Q = terms.sum()
    return (Q if kind == "mse" else torch.sqrt(Q)), terms


# ------------------------------------------------------------------------------------------------ 1: the kernel against NumPy fp64
def _stats(C, gen, small=None):
    """(mean, meansq, eps) of a normaliser; channel `small` has 1e-3 of the others' std."""
    mean = torch.randn(C, generator=gen, dtype=torch.float64)
    var = 0.5 + torch.rand(C, generator=gen, dtype=torch.float64)
    if small is not None:
        var[small] = var[small] * 1e-6
    return mean, mean * mean + var, torch.tensor(1e-8, dtype=torch.float64)


def _std(st):
    return np.maximum(np.sqrt(st[1].numpy() - st[0].numpy() ** 2), float(st[2]))


def _kernel_inputs(R, C, tail_zero):
    gen = torch.Generator().manual_seed(1000 * R + C)
    pred, tar = torch.randn(R, C, generator=gen), torch.randn(R, C, generator=gen)
    mask = (torch.rand(R, generator=gen) < 0.8).float()
    if R > 1:
        mask[0] = 0.0
    mask[R - 1] = 1.0
    if tail_zero:
        mask[R - 300:] = 0.0
        mask[R - 301] = 1.0
    o_stats, i_stats = _stats(C, gen, small=C // 2), _stats(C + 1, gen)
    g_next, g_nin = torch.randn(R, C, generator=gen), torch.randn(R, C + 1, generator=gen)
    g_next[mask == 0], g_nin[mask == 0] = float("inf"), float("nan")      # must never reach the result
    weights = 0.5 + 1.5 * torch.rand(C, generator=gen, dtype=torch.float64)
    return pred, tar, mask, o_stats, i_stats, g_next, g_nin, weights


@pytest.mark.parametrize("R,C,tail_zero", [(R, C, False) for R in (1, 257, 1025) for C in (1, 3, 8)] + [(1025, 3, True)])
def test_objective_bwd_kernel_against_numpy(eng, R, C, tail_zero):
    """One thread, a ragged second block, five blocks; C = 1, 3, 8; every (space, kind), unit and random weights, with and without a
    carried pair.  The middle channel's std is 1e-3 of the others, so a wrong channel index is an O(1) error under `normalized`.
    About 20 % of the mask is zero (row 0 always, unless it is the only row); `tail_zero`: the last 300 rows as well, so the
    last block and a half see no unmasked row."""
    L = eng._abi.lib()
    pred, tar, mask, o_stats, i_stats, g_next, g_nin, weights = _kernel_inputs(R, C, tail_zero)
    d = lambda t: t.cuda()
    p = lambda t: None if t is None else t.data_ptr()
    dp, dt, dm, dgn, dgi, dw = d(pred), d(tar), d(mask), d(g_next), d(g_nin), d(weights)
    do, di = [d(t) for t in o_stats], [d(t) for t in i_stats]
    s = torch.cuda.current_stream().cuda_stream
    D = (pred - tar).double().numpy()                                   # d = fl32(pred - tar)
    Mk = mask.double().numpy()[:, None]
    M_, SE = float(Mk.sum()), (Mk * D * D).sum(0)
    sums = torch.tensor(np.concatenate([[M_], SE, np.full(2 * C, np.nan)]), dtype=torch.float64)      # [M | SE | never read]
    ds = d(sums)
    std_o, std_i = _std(o_stats), _std(i_stats)
    with np.errstate(invalid="ignore"):
        carry_full = np.where(Mk != 0, g_next.double().numpy() + g_nin.double().numpy()[:, :C] / std_i[:C], 0.0)

    def run(space, kind, w, w_step, carried):
        loss, chan = torch.full((1,), -1.0, device="cuda"), torch.full((C,), -1.0, device="cuda")
        gp, gnp = torch.full((R, C), 7.0, device="cuda"), torch.full((R, C), 7.0, device="cuda")
        eng._abi.check(L.bsms_sim_objective_bwd(p(dp), p(dt), p(dm), R, C, *map(p, do), *map(p, di), p(ds), p(w), SPACE_ID[space], KIND_ID[kind],
                                                w_step, p(dgn) if carried else None, p(dgi) if carried else None, p(loss), p(chan), p(gp),
                                                p(gnp), s), "bsms_sim_objective_bwd")
        return loss, chan, gp, gnp

    worst = 0.0
    for space, kind in PAIRS:
        for w_dev, w_np in ((None, np.ones(C)), (dw, weights.numpy())):
            a = w_np / std_o ** 2 if space == "normalized" else w_np
            terms = a * SE / (M_ * C)
            Q = terms.sum()
            loss = Q if kind == "mse" else np.sqrt(Q)
            G = 2.0 / (M_ * C) if kind == "mse" else 1.0 / (loss * M_ * C)
            for carried, w_step in ((False, 1.0), (True, 0.375)):
                got = run(space, kind, w_dev, w_step, carried)
                again = run(space, kind, w_dev, w_step, carried)
                assert all(torch.equal(x, y) for x, y in zip(got, again)), (space, kind, carried)      # deterministic
                loss_g, chan_g, gp_g, gnp_g = (t.cpu() for t in got)
                want_gp = w_step * (G * a[None, :] * Mk * D) + (carry_full if carried else 0.0)
                want_gnp = want_gp * Mk * std_o
                tag = (space, kind, w_dev is not None, carried)
                assert abs(float(loss_g) - loss) <= KERNEL_TOL * loss, tag
                assert np.abs(chan_g.double().numpy() - terms).max() <= KERNEL_TOL * terms.max(), tag
                for out, want in ((gp_g, want_gp), (gnp_g, want_gnp)):
                    err = np.abs(out.double().numpy() - want).max() / np.abs(want).max()
                    worst = max(worst, err)
                    assert err <= KERNEL_TOL, (tag, err)
                    assert bool((out[mask == 0] == 0).all()), tag          # exactly 0: no carry, no loss term on masked rows
    print(f"\n[R={R} C={C} tail_zero={tail_zero}] worst relative distance to the fp64 restatement: {worst:.2e}")


# ------------------------------------------------------------------------------------------------ 2: the old kernel as a cross-check
@pytest.mark.parametrize("R,C", [(257, 2), (1025, 3)])
def test_default_objective_agrees_with_the_loss_kernel(eng, R, C):
    """physical / rmse / unit weights through the new entry, sums from bsms_error_sums, against bsms_sim_loss_bwd on the fp32 pair
    formed from the same sums: the same loss from fp64 instead of fp32 sums -- equal to round-off, not bit for bit."""
    L = eng._abi.lib()
    pred, tar, mask, o_stats, _, _, _, _ = _kernel_inputs(R, C, False)
    d = lambda t: t.cuda()
    p = lambda t: None if t is None else t.data_ptr()
    dp, dt, dm, do = d(pred), d(tar), d(mask), [d(t) for t in o_stats]
    s = torch.cuda.current_stream().cuda_stream
    sums = eng.error_sums(dp.reshape(1, R, C), dt.reshape(1, R, C), dm.reshape(1, R, 1), R)          # [1, 1 + 3C]
    pair = torch.stack([sums[0, 1:1 + C].sum(), sums[0, 0]]).float()                                  # (S, M) as k_sim_epilogue lays them out
    loss0, gnp0 = torch.full((1,), -1.0, device="cuda"), torch.full((R, C), 7.0, device="cuda")
    eng._abi.check(L.bsms_sim_loss_bwd(p(dp), p(dt), p(dm), R, C, *map(p, do), p(pair), p(loss0), p(gnp0), s), "bsms_sim_loss_bwd")
    loss1, gnp1 = torch.full((1,), -1.0, device="cuda"), torch.full((R, C), 7.0, device="cuda")
    eng._abi.check(L.bsms_sim_objective_bwd(p(dp), p(dt), p(dm), R, C, *map(p, do), None, None, None, p(sums), None, 0, 0, 1.0, None, None,
                                            p(loss1), None, None, p(gnp1), s), "bsms_sim_objective_bwd")
    e_g, e_l = rel_err(gnp1.cpu(), gnp0.cpu()), abs(float(loss1) - float(loss0)) / float(loss0)
    print(f"\n[R={R} C={C}] new entry against bsms_sim_loss_bwd: gradient {e_g:.2e}, loss {e_l:.2e} (relative)")
    assert e_g <= KERNEL_TOL and e_l <= KERNEL_TOL


# ------------------------------------------------------------------------------------------------ 3: the default route is untouched
def _golden_model(eng, graphs):
    z = load_golden("sim")
    sim = eng.BSMS_Simulator(ro.make_cfg(2, 32, 3, 3, 2))
    sim.load_state_dict(z.state_dict())
    return sim.cuda(), _cuda(sim_batch(graphs, 3))


def test_default_objective_is_the_existing_step_bit_for_bit(eng, graphs):
    sim, data = _golden_model(eng, graphs)
    assert data[0].shape[0] * data[0].shape[1] == 600
    grads = eng.GradBuckets(list(sim.parameters()))
    results = []
    for kw in ({}, {"objective": None}, {"objective": eng.Objective()}):
        grads.flat.fill_(float("nan"))
        step = eng.FusedStep(sim, grads, **kw)
        loss = step(data, True)
        assert step._obj is None and "osums" not in step._buf            # the old entries, no objective buffers
        results.append((loss.clone(), step.prediction().clone(), grads.flat.clone()))
        with pytest.raises(ValueError):
            step.channel_losses()
    for r in results[1:]:
        assert all(torch.equal(a, b) for a, b in zip(r, results[0]))
    assert bool(torch.isfinite(results[0][2]).all()) and bool(torch.isfinite(results[0][0]))


# ------------------------------------------------------------------------------------------------ 4: the fused step against the oracle
def three_channel_batch(graphs, depth=3):
    """The golden batch with a third channel in units 1e-3 of the others (see the module docstring)."""
    node_in, tar, mask, m_gs, m_ids = sim_batch(graphs, depth)
    gen = torch.Generator().manual_seed(11)
    s3 = torch.randn(*tar.shape[:-1], 1, generator=gen)
    t3 = s3 + (tar - node_in[..., :2])[..., :1].flip(1) + 0.05 * torch.randn(*tar.shape[:-1], 1, generator=gen)
    node_in3 = torch.cat([node_in[..., :2], 1e-3 * s3, node_in[..., 2:]], -1)
    tar3 = torch.cat([tar, 1e-3 * t3], -1)
    return (node_in3.contiguous(), tar3.contiguous(), mask, m_gs, m_ids)


_REF3 = {}


def oracle3(graphs):
    """The fp32 three-channel oracle, warmed up on the batch (once per session; never modified afterwards)."""
    if not _REF3:
        D, H, depth = SHAPE3
        data = three_channel_batch(graphs, depth)
        torch.manual_seed(SEED3)
        ref = ro.BSMS_Simulator(ro.make_cfg(3, D, H, depth, 2))
        ref(data, True, True)
        _REF3.update(ref=ref, data=data)
    return _REF3["ref"], _REF3["data"]


def unrolled_oracle3(sim, data, later, step_weights, detach, space, kind, weights):
    """tests/test_hip_unroll.py::unrolled_oracle with the loss of the definition in place of the masked RMSE."""
    node_in, tar, mask, m_gs, m_ids = data
    C = tar.shape[-1]
    tars = [tar, *(later if later is not None else [])]
    std = sim._targetNormalizer.std_with_epsilon().detach()
    sim.zero_grad(set_to_none=True)
    cur, preds, losses, terms, total = node_in, [], [], [], 0.0
    for k, w in enumerate(step_weights):
        pred = sim((cur, tars[k], mask, m_gs, m_ids), True, False)
        preds.append(pred.detach())
        loss_k, terms_k = loss_def(pred, tars[k], mask, space, kind, weights, std)
        losses.append(float(loss_k.detach()))
        terms.append(terms_k.detach())
        total = total + w * loss_k
        cur = torch.where(mask == 0, node_in, torch.cat([pred.detach() if detach else pred, node_in[..., C:]], dim=-1))
    total.backward()
    grads = {k: p.grad.clone() for k, p in sim.named_parameters() if p.grad is not None}
    return torch.stack(preds), float(total.detach()), grads, losses, torch.stack(terms)


_ORACLE3 = {}


def oracle_runs3(graphs, K, detach, space, kind, weights):
    """fp32 on all threads, fp32 on one thread, fp64: computed once per configuration and shared (tests/test_hip_unroll.py::oracle_runs)."""
    key = (K, detach, space, kind, tuple(weights))
    if key not in _ORACLE3:
        ref, data = oracle3(graphs)
        later = later_targets(data[0], data[1], K)
        sw = [1.0] if K == 1 else [1.0, 0.5]
        with KinkMargin(ref) as km:
            pred32, loss32, g32, losses32, terms32 = unrolled_oracle3(ref, data, later, sw, detach, space, kind, weights)
        assert km.min >= MIN_MARGIN, (key, "the weight seed no longer keeps the ReLU inputs away from 0", km.min)
        n = torch.get_num_threads()
        torch.set_num_threads(1)
        try:
            g32_one = unrolled_oracle3(ref, data, later, sw, detach, space, kind, weights)[2]
        finally:
            torch.set_num_threads(n)
        ref64 = ro.BSMS_Simulator(ref.cfg, dtype=torch.float64)
        ref64.load_state_dict(ref.state_dict())
        ref64.double()
        _, loss64, g64, _, _ = unrolled_oracle3(ref64, _f64(data), None if later is None else later.double(), sw, detach, space, kind, weights)
        _ORACLE3[key] = dict(pred32=pred32, loss32=loss32, loss64=loss64, g32=g32, g32_one=g32_one, g64=g64, t32=0.0, t64=0.0, levels=key,
                             losses32=losses32, terms32=terms32, later=later, step_weights=sw, margin=km.min)
    return _ORACLE3[key]


def engine_step3(eng, graphs, K, detach, space, kind, weights):
    ref, data = oracle3(graphs)
    mine = eng.BSMS_Simulator(ref.cfg)
    mine.load_state_dict(ref.state_dict())
    mine = mine.cuda()
    grads = eng.GradBuckets(list(mine.parameters()))
    sw = [1.0] if K == 1 else [1.0, 0.5]
    step = eng.FusedStep(mine, grads, unroll=K, step_weights=sw, detach=detach, objective=eng.Objective(space, kind, weights))
    later = later_targets(data[0], data[1], K)
    args = (_cuda(data), True) if K == 1 else (_cuda(data), True, later.cuda())
    loss = step(*args)
    torch.cuda.synchronize()
    return mine, grads, step, loss, args


_DECODER_COLUMN = {}          # (kind, space) -> norm of the gradient of the decoder's output row of the small channel, unroll = 1


@pytest.mark.parametrize("space,kind", PAIRS)
@pytest.mark.parametrize("K,detach", [(1, False), (2, False), (2, True)])
def test_fused_step_follows_the_oracle(eng, graphs, K, detach, space, kind):
    weights = [1.0, 1.0, 3.0]
    r = dict(oracle_runs3(graphs, K, detach, space, kind, weights))
    mine, grads, step, loss, _ = engine_step3(eng, graphs, K, detach, space, kind, weights)
    preds = torch.stack([q.reshape(r["pred32"][0].shape) for q in step.predictions()]).cpu()
    got_losses, chan = step.step_losses().cpu().double(), step.channel_losses().cpu().double()
    assert chan.shape == (K, 3)
    for k in range(K):
        e_p, e_l = rel_err(preds[k], r["pred32"][k]), abs(float(got_losses[k]) - r["losses32"][k]) / r["losses32"][k]
        Q = float(got_losses[k]) if kind == "mse" else float(got_losses[k]) ** 2
        e_q = abs(float(chan[k].sum()) - Q) / Q
        print(f"[{space}/{kind} K={K} detach={detach}] step {k}: prediction {e_p:.2e}, loss {e_l:.2e} from the fp32 oracle; "
              f"sum of channel_losses {e_q:.2e} from Q; kink margin {r['margin']:.2e}")
        assert e_p <= 1e-5 and e_l <= 1e-5, (k, e_p, e_l)
        assert e_q <= 1e-6, (k, e_q)
        assert rel_err(chan[k], r["terms32"][k]) <= 1e-5, k
    r.update(pred=preds, loss=float(loss), gg={k: q.grad.detach().cpu() for k, q in mine.named_parameters() if q.requires_grad})
    check(r, f"{space}/{kind} K={K} detach={detach}")
    if K == 1:
        name, w_out = [(k, q) for k, q in mine.decode.named_parameters() if q.dim() == 2 and q.shape[0] == 3][-1]
        _DECODER_COLUMN[(kind, space)] = float(w_out.grad[2].norm())


@pytest.mark.parametrize("kind", ["rmse", "mse"])
def test_normalized_space_gives_the_small_channel_its_gradient(eng, graphs, kind):
    """The sanity bracket: the gradient of the decoder's output row of the channel in small units is more than 100x larger under
    `normalized` than under `physical` (on the CPU oracle alone: 4.9e6 x for rmse, 7.7e7 x for mse -- the target normaliser's
    stds are 0.100, 0.098, 1.0e-4, so a_2 = 3 / std_2^2 = 3e8 against 3)."""
    col = {}
    for space in ("physical", "normalized"):
        if (kind, space) not in _DECODER_COLUMN:                       # run on its own: take the step here
            mine = engine_step3(eng, graphs, 1, False, space, kind, [1.0, 1.0, 3.0])[0]
            w_out = [q for k, q in mine.decode.named_parameters() if q.dim() == 2 and q.shape[0] == 3][-1]
            _DECODER_COLUMN[(kind, space)] = float(w_out.grad[2].norm())
        col[space] = _DECODER_COLUMN[(kind, space)]
    print(f"[{kind}] decoder row of the small channel: |grad| physical {col['physical']:.3e}, normalized {col['normalized']:.3e}, "
          f"ratio {col['normalized'] / col['physical']:.3e}")
    assert col["physical"] > 0 and col["normalized"] > 100 * col["physical"]


# ------------------------------------------------------------------------------------------------ 5: autograd route == fused route
def test_autograd_route_equals_fused_route(eng, graphs):
    """masked_loss(sim(data)).backward() against FusedStep with the same objective; tolerances of
    tests/test_hip_training.py::test_fused_step_equals_autograd_step (loss and prediction 1e-6, gradients 2e-6)."""
    sim, data = _golden_model(eng, graphs)
    obj = eng.Objective("normalized", "mse", [1.0, 3.0])
    sim.zero_grad(set_to_none=True)
    pred = sim(data, True, False)
    loss = eng.masked_loss(pred, data[1], data[2], obj, sim._targetNormalizer.std_with_epsilon())
    loss.backward()
    want = {k: q.grad.clone() for k, q in sim.named_parameters() if q.grad is not None}
    sim.zero_grad(set_to_none=True)
    grads = eng.GradBuckets(list(sim.parameters()))
    step = eng.FusedStep(sim, grads, objective=obj)
    got_loss = step(data, True)
    assert abs(float(got_loss) - float(loss)) < 1e-6 * abs(float(loss))
    assert rel_err(step.prediction().cpu(), pred.detach().cpu()) < 1e-6
    assert set(k for k, q in sim.named_parameters() if q.grad is not None) == set(want)
    for k, q in sim.named_parameters():
        if q.requires_grad:
            assert rel_err(q.grad.cpu(), want[k].cpu()) < 2e-6, k
    # and it is another loss than the default one
    assert abs(float(got_loss) - float(eng.masked_rmse(pred.detach(), data[1], data[2]))) > 1e-3 * abs(float(got_loss))


# ------------------------------------------------------------------------------------------------ 6: the Trainer
def _trainer_losses(eng, graphs, extra, iters=5):
    ref, data = oracle3(graphs)
    D, H, depth = SHAPE3
    model_cfg = SimpleNamespace(out_dim=3, latent_dim=D, hidden_layer=H, unet_depth=depth, pos_dim=2, consistent_mesh=True,
                                accumulation_steps=1, **extra)
    opt_cfg = SimpleNamespace(peak_lr=1e-3, weight_decay=1e-4, warmup_steps=2, decay_steps=20, gnorm_clip=1.0)
    torch.manual_seed(0)
    fresh = ro.BSMS_Simulator(model_cfg)
    mine = eng.BSMS_Simulator(model_cfg)
    mine.load_state_dict(fresh.state_dict())
    tr = eng.Trainer(mine, model_cfg, opt_cfg)
    losses = [tr.iter(data) for _ in range(iters)]
    return tr, fresh, model_cfg, opt_cfg, data, [float(l) for l in losses if l is not None]


def test_trainer_reads_the_objective_and_follows_the_cpu_loop(eng, graphs):
    """loss_space = "normalized": warm-up + four optimisation iterations of Trainer.iter == the same loop written with the CPU
    oracle, the loss of the definition, torch clip_grad_norm_ and torch.optim.AdamW; tolerances of
    tests/test_hip_training.py::test_trainer_iterations_follow_cpu_reference_loop."""
    tr, ref, model_cfg, opt_cfg, data, losses = _trainer_losses(eng, graphs, dict(loss_space="normalized"))
    assert tr.objective == eng.Objective("normalized") and tr.dp.fused.objective == tr.objective and tr.dp.fused._obj is not None
    opt = torch.optim.AdamW([q for q in ref.parameters() if q.requires_grad], lr=opt_cfg.peak_lr, weight_decay=opt_cfg.weight_decay)
    sch = eng.WarmupCosineDecay(opt_cfg.peak_lr, opt_cfg.warmup_steps, opt_cfg.decay_steps)
    losses_ref = []
    for it in range(5):
        if it < model_cfg.accumulation_steps:
            ref(data, True, True)
            continue
        opt.zero_grad()
        loss = loss_def(ref(data, True, False), data[1], data[2], "normalized", "rmse", None, ref._targetNormalizer.std_with_epsilon())[0]
        loss.backward()
        torch.nn.utils.clip_grad_norm_(ref.parameters(), opt_cfg.gnorm_clip)
        for group in opt.param_groups:
            group["lr"] = sch.lr()
        opt.step()
        sch.step()
        losses_ref.append(float(loss))
    assert len(losses) == 4 and tr.train_step == 5
    for a, b in zip(losses, losses_ref):
        assert abs(a - b) < 2e-4 * abs(b), (losses, losses_ref)
    for (k, q), (_, g) in zip(ref.named_parameters(), tr.model.named_parameters()):
        if q.requires_grad:
            assert rel_err(g.detach().cpu(), q.detach()) < 2e-3, k
    # get_loss reports the same objective: masked_loss of its own prediction, not the masked RMSE
    pred, gdata = tr.get_pred(data).detach(), _cuda(data)
    want = eng.masked_loss(pred, gdata[1], gdata[2], tr.objective, tr.model._targetNormalizer.std_with_epsilon())
    assert torch.equal(tr.get_loss(data).detach(), want)
    assert abs(float(want) - float(eng.masked_rmse(pred, gdata[1], gdata[2]))) > 0.5 * float(want)


def test_trainer_without_the_keys_is_the_default_route(eng, graphs):
    """Absent keys: the default objective on the old entries -- the same losses, bit for bit, as with the default spelled out, and as
    the bare FusedStep of item 3 runs them."""
    tr0, _, _, _, _, l0 = _trainer_losses(eng, graphs, {})
    tr1, _, _, _, _, l1 = _trainer_losses(eng, graphs, dict(loss_space="physical", loss_kind="rmse", loss_channel_weights=None))
    assert tr0.objective.is_default and tr0.dp.fused._obj is None and tr1.dp.fused._obj is None
    assert len(l0) == 4 and l0 == l1
    assert torch.equal(tr0.optimizer.flat_p, tr1.optimizer.flat_p)
    tr2, _, _, _, _, l2 = _trainer_losses(eng, graphs, dict(loss_space="normalized"), iters=2)
    assert l2[0] != l0[0]


# ------------------------------------------------------------------------------------------------ 7: two ranks
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
    engine = eng.DataParallel(sim, bucket_bytes=64 << 10, objective=eng.Objective("normalized", "mse", [1.0, 3.0]))
    loss = engine.step_loss_backward(data, True)
    torch.cuda.synchronize()
    torch.save({"loss": loss.detach().cpu(), "flat": engine.grads.flat.cpu(), "chan": engine.fused.channel_losses().cpu()}, f"{out_path}.{rank}")
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.timeout(300)
def test_two_ranks_equal_the_single_process_step(eng, graphs, tmp_path):
    """Two ranks over gloo on one GPU, one golden sample each, normalized / mse: one all-reduce of the fp64 sums, one of the flat
    gradients; the result is the single-process step on the whole batch (launcher and tolerances of tests/test_hip_dp.py)."""
    port = 29900 + os.getpid() % 2000
    out = str(tmp_path / "res")
    mp.start_processes(_worker, args=(2, port, out), nprocs=2, join=True, start_method="spawn")
    r0, r1 = torch.load(out + ".0"), torch.load(out + ".1")
    assert torch.equal(r0["flat"], r1["flat"]) and torch.equal(r0["loss"], r1["loss"])         # bit-identical across ranks
    sim, data = _golden_model(eng, graphs)
    grads = eng.GradBuckets(list(sim.parameters()))
    step = eng.FusedStep(sim, grads, objective=eng.Objective("normalized", "mse", [1.0, 3.0]))
    loss = step(data, True)
    assert abs(float(r0["loss"]) - float(loss)) < 1e-5 * abs(float(loss))
    assert rel_err(r0["chan"], step.channel_losses().cpu()) < 1e-5
    assert rel_err(r0["flat"], grads.flat.cpu()) < 2e-5


# ------------------------------------------------------------------------------------------------ 8: graph capture
def test_graph_replay_equals_the_eager_step(eng, graphs):
    sim, data = _golden_model(eng, graphs)
    obj = eng.Objective("normalized", "rmse", [2.0, 0.5])
    grads = eng.GradBuckets(list(sim.parameters()))
    eager = eng.FusedStep(sim, grads, objective=obj)
    l0 = eager(data, True)
    flat0, pred0, chan0 = grads.flat.clone(), eager.prediction().clone(), eager.channel_losses()
    gstep = eng.FusedStep(sim, grads, use_graph=True, objective=obj)
    for _ in range(2):                                                 # the capture's first replay, then a plain replay
        grads.flat.fill_(float("nan"))
        l1 = gstep(data, True)
        assert torch.equal(l1, l0) and torch.equal(grads.flat, flat0) and torch.equal(gstep.prediction(), pred0)
        assert torch.equal(gstep.channel_losses(), chan0)
    assert gstep._graphs is not None
