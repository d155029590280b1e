"""GPU: gradient accumulation -- micro-batches folded into the exact loss of all their samples.

1-2   bsms_grad_fold and bsms_accum_coef on their own, against the torch fp32 restatement (bit for bit) and NumPy fp64.
3-4   accumulate = 1 is the step as it was; the first micro-batch of a cycle is the plain step on it, bit for bit.
5     plumbing, bitwise: the accumulated buffer is the recurrence acc_t = fl32(fl32(a_t acc_{t-1}) + fl32(b_t g_t)) applied to the
      flat gradients of the plain step on every micro-batch alone, with the coefficients the step reports.
6-8   meaning: the two golden samples as two micro-batches of B = 1 against the CPU oracle's ONE step on the B = 2 batch under
      autograd -- default loss on three model shapes, two objectives, the unrolled mse loss, and reduction = "mean" against the
      oracle's (rmse_0 + rmse_1) / 2.
9     determinism and no state leaking from one cycle into the next.
10-11 the Trainer (gradient_accumulation_steps) against the CPU loop; a Trainer without the key.
12    two data-parallel ranks x two micro-batches against the oracle's four-sample step.

Everything runs on the 300-node `del300` hierarchy with the golden `sim` batch (B = 2, C = 2, p = 2; 267 / 266 unmasked rows), on the
model shapes and weight seeds of tests/test_hip_unroll.py (a forward of one sample is a part of the batch's forward: the ReLU
margins those seeds were picked for hold for every micro-batch).

Tolerances.  Kernels: bit-equality (grad_fold; `running`, the coefficients and the losses of accum_coef -- fp64 +, *, / and sqrt
are correctly rounded on both sides and each fp32 value is one rounding of an fp64 one).  Plumbing: bit-equality.  Meaning: the
accumulated loss 1e-5 from the fp32 oracle (on the CPU oracle alone the folded loss is 2e-8 from the big-batch one), gradients by
the three-way fp64 criterion of tests/test_hip_fullsize.py (`check`) with the factors it has."""
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
from test_hip_objective import loss_def
from test_hip_unroll import MIN_MARGIN, SHAPES, _cuda, _f64, later_targets, make_oracle, unrolled_oracle

pytestmark = pytest.mark.gpu

SPACE_ID, KIND_ID, REDUCTION_ID = {"physical": 0, "normalized": 1}, {"rmse": 0, "mse": 1}, {"batch": 0, "mean": 1}


@pytest.fixture(scope="module")
def eng():
    import bsms_gnn_amd as eng
    return eng


def bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int64)


def bit_equal(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(bits(a), bits(b))


# ------------------------------------------------------------------------------------------------ 1: bsms_grad_fold alone
COEFS = [(0.0, 1.0), (1.0, 1.0), (2.0 ** -0.5, np.pi / 7.0), (np.sqrt(267.0 / 533.0), np.sqrt(266.0 / 533.0)), (1.0 / 3.0, 2.0 / 3.0)]


@pytest.mark.parametrize("n", [1, 3, 255, 1023, 1024, 1025, 524289, 2097157])       # the last: past the 2048 x 256 x 4 grid stride
def test_grad_fold_kernel(eng, n):
    """Bit-equal to torch's (a32 * acc) + (b32 * g), three separate fp32 operations, on the 16-byte path (aligned pointers) and on
    the element path (both pointers, or one of them, offset by one float); nothing past n is touched; two runs are bit-equal."""
    L, s = eng._abi.lib(), torch.cuda.current_stream().cuda_stream
    gen = torch.Generator().manual_seed(n)
    acc0, g0 = torch.randn(n + 9, generator=gen).cuda(), torch.randn(n + 9, generator=gen).cuda()
    assert acc0.data_ptr() % 16 == 0 and g0.data_ptr() % 16 == 0
    for a, b in COEFS:
        coef = torch.tensor([a, b], dtype=torch.float32).cuda()
        for oa, og in ((0, 0), (1, 1), (0, 1), (1, 0)):
            runs = []
            for _ in range(2):
                acc, g = acc0.clone(), g0
                eng._abi.check(L.bsms_grad_fold(acc[oa:].data_ptr(), g[og:].data_ptr(), n, coef.data_ptr(), s), "bsms_grad_fold")
                runs.append(acc)
            want = (coef[0] * acc0[oa:oa + n]) + (coef[1] * g0[og:og + n])
            got = runs[0]
            assert bit_equal(got[oa:oa + n], want), (n, a, b, oa, og)
            assert bit_equal(got[:oa], acc0[:oa]) and bit_equal(got[oa + n:], acc0[oa + n:]), (n, oa, og, "sentinels")
            assert bit_equal(runs[0], runs[1])
    # (0, 1) hands g over and (1, 1) is the plain sum, whatever the path
    coef = torch.tensor([1.0, 1.0]).cuda()
    acc = acc0.clone()
    eng._abi.check(L.bsms_grad_fold(acc.data_ptr(), g0.data_ptr(), n, coef.data_ptr(), s), "bsms_grad_fold")
    assert bit_equal(acc[:n], acc0[:n] + g0[:n])


# ------------------------------------------------------------------------------------------------ 2: bsms_accum_coef alone
def _std(mean, meansq, eps):
    with np.errstate(invalid="ignore"):
        s = np.sqrt(meansq - mean * mean)
    return np.maximum(np.nan_to_num(s, nan=0.0), eps)


def coef_ref(t, m, n, run, C, rmse, mean_reduction):
    """The definition in NumPy fp64, one operation per line of include/bsms_hip.h.  Returns (Mc, Nc, Lc), a, b."""
    m, n, Cd = np.float64(m), np.float64(n), np.float64(C)
    q = n / (m * Cd)
    l = np.sqrt(q) if rmse else q
    if t == 0:
        return (m, n, l), np.float64(0.0), np.float64(1.0)
    Mp, Np, Lp = (np.float64(v) for v in run)
    Mc, Nc = Mp + m, Np + n
    if mean_reduction:
        td, t1 = np.float64(t), np.float64(t + 1)
        return (Mc, Nc, (Lp * td + l) / t1), td / t1, np.float64(1.0) / t1
    Qc = Nc / (Mc * Cd)
    Lc = np.sqrt(Qc) if rmse else Qc
    if rmse:
        den = Lc * Mc
        return (Mc, Nc, Lc), (Lp * Mp) / den, (l * m) / den
    return (Mc, Nc, Lc), Mp / Mc, m / Mc


def ulps32(a, b):
    a, b = np.float32(a), np.float32(b)
    return abs(int(a.view(np.int32)) - int(b.view(np.int32)))


@pytest.mark.parametrize("K", [1, 3])
@pytest.mark.parametrize("reduction", ["batch", "mean"])
@pytest.mark.parametrize("layout", ["pair", "row"])
def test_accum_coef_kernel_against_numpy(eng, layout, reduction, K):
    """t = 0, 1, 2 chained on a NaN-filled `running`, every (space, kind): `running` bit-equal to the fp64 formula, (a, b) -- step
    0's -- and loss_out bit-equal to its single rounding to fp32.  The row has the 1 + 3C fields of bsms_error_sums with NaNs in
    the fields the entry must not read; the pair ignores space, statistics and weights (NaN statistics are handed in)."""
    L, s, C = eng._abi.lib(), torch.cuda.current_stream().cuda_stream, 3
    gen = np.random.default_rng(17 * K + (layout == "row"))
    mean = gen.standard_normal(C)
    meansq = mean * mean + (0.5 + gen.random(C)) * np.array([1.0, 1e-6, 1.0])       # the middle channel in small units
    eps, weights = np.float64(1e-8), 0.5 + 1.5 * gen.random(C)
    p = lambda x: None if x is None else x.data_ptr()
    dev = lambda a, dt=torch.float64: torch.tensor(np.asarray(a), dtype=dt).cuda()
    d_mean, d_meansq, d_eps, d_w = dev(mean), dev(meansq), dev(eps), dev(weights)
    nan_stats = torch.full((C,), float("nan"), dtype=torch.float64).cuda()
    for space in ("physical", "normalized"):
        for kind in ("rmse", "mse"):
            for w in ((None,) if layout == "pair" else (None, weights)):
                running = torch.full((K, 3), float("nan"), dtype=torch.float64).cuda()
                coef, loss = torch.full((2,), float("nan")).cuda(), torch.full((K,), float("nan")).cuda()
                run_ref = [None] * K
                for t in range(3):
                    M = np.floor(200 + 100 * gen.random(K))                        # unmasked rows: whole numbers
                    if layout == "pair":
                        S = np.float32(M * C * (0.01 + gen.random(K)))
                        host = np.stack([S, np.float32(M)], 1).astype(np.float32)  # float (S, M)
                        sums, stride = dev(host, torch.float32), 2
                        m_n = [(np.float64(host[k, 1]), np.float64(host[k, 0])) for k in range(K)]
                        stats = (nan_stats, nan_stats, nan_stats)
                    else:
                        SE = M[:, None] * (0.01 + gen.random((K, C))) * np.array([1.0, 1e-6, 1.0])
                        host = np.full((K, 1 + 3 * C), np.nan)
                        host[:, 0], host[:, 1:1 + C] = M, SE
                        sums, stride = dev(host), 1 + 3 * C
                        a_c = np.ones(C) if w is None else w.copy()
                        if space == "normalized":
                            sd = _std(mean, meansq, eps)
                            a_c = a_c / (sd * sd)
                        m_n = []
                        for k in range(K):
                            n = np.float64(0.0)
                            for c in range(C):
                                n = n + a_c[c] * SE[k, c]
                            m_n.append((M[k], n))
                        stats = (d_mean, d_meansq, d_eps)
                    eng._abi.check(L.bsms_accum_coef(p(sums), int(layout == "row"), stride, C, *map(p, stats), p(None if w is None else d_w),
                                                     SPACE_ID[space], KIND_ID[kind], REDUCTION_ID[reduction], t, K, p(running), p(coef),
                                                     p(loss), s), "bsms_accum_coef")
                    got_run, got_coef, got_loss = running.cpu().numpy(), coef.cpu().numpy(), loss.cpu().numpy()
                    for k in range(K):
                        run_ref[k], a, b = coef_ref(t, *m_n[k], run_ref[k], C, kind == "rmse", reduction == "mean")
                        tag = (layout, space, kind, reduction, w is not None, t, k)
                        want_run = np.array(run_ref[k], dtype=np.float64)
                        assert np.array_equal(got_run[k].view(np.int64), want_run.view(np.int64)), (tag, got_run[k], want_run)
                        assert ulps32(got_loss[k], np.float32(run_ref[k][2])) == 0, (tag, got_loss[k], run_ref[k][2])
                        if k == 0:
                            assert ulps32(got_coef[0], np.float32(a)) == 0 and ulps32(got_coef[1], np.float32(b)) == 0, (tag, got_coef, a, b)
                            if t == 0:
                                assert got_coef[0] == 0.0 and got_coef[1] == 1.0
                    assert np.isfinite(got_run).all() and np.isfinite(got_coef).all() and np.isfinite(got_loss).all()


# ------------------------------------------------------------------------------------------------ models, micro-batches, the step
def engine_model(eng, ref, freeze=()):
    mine = eng.BSMS_Simulator(ref.cfg)
    mine.load_state_dict(ref.state_dict())
    mine = mine.cuda()
    for name in freeze:
        getattr(mine, name).requires_grad_(False)
    return mine, eng.GradBuckets(list(mine.parameters()))


def part(data, idx, later=None):
    """The samples `idx` of a consistent-mesh batch (and of its later targets [K-1, B, N, C]) as a batch of their own."""
    node_in, tar, mask, m_gs, m_ids = data
    n = len(idx)
    out = (node_in[idx].contiguous(), tar[idx].contiguous(), mask[idx].contiguous(), [g[:n] for g in m_gs], [i[:n] for i in m_ids])
    return out, (None if later is None else later[:, idx].contiguous())


def run(step, data, later):
    return step(data, True) if later is None else step(data, True, later)


# ------------------------------------------------------------------------------------------------ 3, 4: what does not change
@pytest.mark.parametrize("shape", ["ring", "split"])
def test_accumulate_one_is_the_existing_step_bit_for_bit(eng, graphs, shape):
    ref, data = make_oracle(shape, graphs)
    mine, grads = engine_model(eng, ref)
    gdata = _cuda(data)
    base = eng.FusedStep(mine, grads)
    l0 = base(gdata, True)
    flat0, pred0 = grads.flat.clone(), base.prediction().clone()
    for kw in (dict(accumulate=1), dict(accumulate=1, reduction="mean")):
        grads.flat.fill_(float("nan"))
        one = eng.FusedStep(mine, grads, **kw)
        l1 = one(gdata, True)
        assert bit_equal(l0, l1) and bit_equal(one.prediction(), pred0) and bit_equal(grads.flat, flat0)
        assert one.ready and one.micro_index == 0 and one._acc is None and one._gscratch is None        # no new buffer, no new launch


@pytest.mark.parametrize("kw", [dict(), dict(reduction="mean"), dict(unroll=2, reduction="mean"), dict(objective=("normalized", "mse", [1.0, 3.0]))],
                         ids=["default", "mean", "unroll2-mean", "objective"])
def test_first_micro_batch_is_the_plain_step_on_it(eng, graphs, kw):
    ref, data = make_oracle("ring", graphs)
    mine, grads = engine_model(eng, ref)
    kw = dict(kw)
    if "objective" in kw:
        kw["objective"] = eng.Objective(*kw["objective"])
    K = kw.get("unroll", 1)
    gdata = _cuda(data)
    d0, lat0 = part(gdata, [0], later_targets(gdata[0], gdata[1], K))
    plain_kw = {k: v for k, v in kw.items() if k != "reduction"}
    plain = eng.FusedStep(mine, grads, **plain_kw)
    l0 = run(plain, d0, lat0)
    flat0, pred0 = grads.flat.clone(), plain.prediction().clone()
    grads.flat.fill_(float("nan"))
    acc = eng.FusedStep(mine, grads, accumulate=2, **kw)
    l1 = run(acc, d0, lat0)
    assert bit_equal(l0, l1) and bit_equal(acc.prediction(), pred0) and bit_equal(grads.flat, flat0)
    assert acc.micro_index == 1 and not acc.ready
    assert acc.accumulation_coefficients().tolist() == [0.0, 1.0]
    assert abs(float(acc.accumulated_loss()) - float(l0)) <= 1e-6 * abs(float(l0))      # one micro-batch: the cumulative loss is its own


# ------------------------------------------------------------------------------------------------ 5: plumbing, bitwise
OBJ = ("normalized", "rmse", [1.0, 3.0])
PLUMBING = {
    "m2": dict(parts=[[0], [1]]),
    "m3": dict(parts=[[0], [1], [0, 1]]),
    "unequal": dict(parts=[[0, 1], [0]]),
    "m2-mean": dict(parts=[[0], [1]], reduction="mean"),
    "m3-mean": dict(parts=[[0], [1], [0, 1]], reduction="mean"),
    "unequal-mean": dict(parts=[[0, 1], [0]], reduction="mean"),
    "objective-m3": dict(parts=[[0], [1], [0, 1]], objective=OBJ),
    "objective-unequal": dict(parts=[[0, 1], [0]], objective=OBJ),
    "objective-mean": dict(parts=[[0], [1]], objective=OBJ, reduction="mean"),
    "unroll2-mse-carried": dict(parts=[[0], [1], [0, 1]], unroll=2, objective=("physical", "mse", None)),
    "unroll2-mse-detached": dict(parts=[[0, 1], [0]], unroll=2, objective=("physical", "mse", None), detach=True),
    "unroll2-mean-default": dict(parts=[[0], [1], [0, 1]], unroll=2, reduction="mean"),
    "frozen": dict(parts=[[0], [1], [0, 1]], freeze=("encode", "process")),
    "frozen-unequal-mean": dict(parts=[[0, 1], [0]], freeze=("encode", "process"), reduction="mean"),
}


@pytest.mark.parametrize("case", sorted(PLUMBING))
def test_accumulated_buffer_is_the_recurrence_bit_for_bit(eng, graphs, case):
    """The plain step on every micro-batch alone gives g_t; the accumulating step reports (a_t, b_t); grads.flat after the cycle must
    be acc_0 = g_0, acc_t = fl32(fl32(a_t acc_{t-1}) + fl32(b_t g_t)), restated with torch fp32 operations, bit for bit.  The
    micro-batch losses a call returns are the plain step's, and `ready` / `micro_index` count the cycle."""
    cfg = dict(PLUMBING[case])
    parts, freeze, reduction = cfg.pop("parts"), cfg.pop("freeze", ()), cfg.pop("reduction", "batch")
    if "objective" in cfg:
        cfg["objective"] = eng.Objective(*cfg["objective"])
    K = cfg.get("unroll", 1)
    ref, data = make_oracle("ring", graphs)
    mine, grads = engine_model(eng, ref, freeze)
    frozen_before = {k: q.detach().clone() for k, q in mine.named_parameters() if not q.requires_grad}
    gdata = _cuda(data)
    later = later_targets(gdata[0], gdata[1], K)
    micro = [part(gdata, idx, later) for idx in parts]
    plain = eng.FusedStep(mine, grads, **cfg)
    alone = []
    for d, lat in micro:
        loss = run(plain, d, lat)
        alone.append((loss.clone(), grads.flat.clone()))
    grads.flat.fill_(float("nan"))
    M = len(parts)
    step = eng.FusedStep(mine, grads, accumulate=M, reduction=reduction, **cfg)
    want = None
    for t, (d, lat) in enumerate(micro):
        assert step.micro_index == t and not step.ready
        loss = run(step, d, lat)
        assert bit_equal(loss, alone[t][0]), (case, t, "a call returns the micro-batch's own loss")
        ab = step.accumulation_coefficients()
        if t == 0:
            want = alone[0][1]
            assert ab.tolist() == [0.0, 1.0]
        else:
            want = (ab[0] * want) + (ab[1] * alone[t][1])
            a, b = float(ab[0]), float(ab[1])
            print(f"[{case}] fold {t}: a = {a:.9g}, b = {b:.9g}")
            assert np.isfinite(a) and np.isfinite(b) and 0.0 < a < 1.0 and 0.0 < b <= 1.0
            if reduction == "mean":
                assert a == float(np.float32(t / (t + 1))) and b == float(np.float32(1 / (t + 1)))
        assert bit_equal(grads.flat, want), (case, t)
    assert step.ready and step.micro_index == M
    assert bool(torch.isfinite(grads.flat).all()) and float(grads.flat.abs().max()) > 0
    if reduction == "mean":                                                  # the reported loss: the running mean of the micro-batch losses
        mean = sum(float(l) for l, _ in alone) / M
        assert abs(float(step.accumulated_loss()) - mean) <= 1e-6 * abs(mean)
    # frozen parameters: untouched, no slot, no .grad
    assert any(k.startswith("encode.") for k in frozen_before) == bool(freeze)
    for k, q in mine.named_parameters():
        if not q.requires_grad:
            assert q not in grads._slot and q.grad is None and bit_equal(q.detach(), frozen_before[k]), k
    # the (M+1)-th call starts a new cycle by itself: it is micro-batch 0 again
    run(step, *micro[0])
    assert step.micro_index == 1 and not step.ready and bit_equal(grads.flat, alone[0][1])
    step.reset_accumulation()
    assert step.micro_index == 0


# ------------------------------------------------------------------------------------------------ 6-8: meaning, against the oracle
def big_batch_oracle(sim, data, later, step_weights, detach, objective):
    """ONE step on the whole batch under autograd: tests/test_hip_unroll.py::unrolled_oracle, with the loss of the definition in
    place of the masked RMSE when an objective is given."""
    if objective is None:
        return unrolled_oracle(sim, data, later, step_weights, detach)
    node_in, tar, mask, m_gs, m_ids = data
    C = tar.shape[-1]
    tars = [tar, *(later if later is not None else [])]
    std = sim._targetNormalizer.std_with_epsilon().detach()
    sim.zero_grad(set_to_none=True)
    cur, preds, total = node_in, [], 0.0
    for k, w in enumerate(step_weights):
        pred = sim((cur, tars[k], mask, m_gs, m_ids), True, False)
        preds.append(pred.detach())
        total = total + w * loss_def(pred, tars[k], mask, *objective, std)[0]
        cur = torch.where(mask == 0, node_in, torch.cat([pred.detach() if detach else pred, node_in[..., C:]], dim=-1))
    total.backward()
    return torch.stack(preds), float(total.detach()), {k: q.grad.clone() for k, q in sim.named_parameters() if q.grad is not None}


def mean_oracle(sim, data, parts):
    """reduction = "mean": (rmse_0 + ... + rmse_{M-1}) / M over the micro-batches, one backward."""
    sim.zero_grad(set_to_none=True)
    preds, total = [], 0.0
    for idx in parts:
        d, _ = part(data, idx)
        pred = sim(d, True, False)
        preds.append(pred.detach())
        total = total + ro.masked_rmse(pred, d[1], d[2]) / len(parts)
    total.backward()
    return torch.cat(preds).unsqueeze(0), float(total.detach()), {k: q.grad.clone() for k, q in sim.named_parameters() if q.grad is not None}


_ORACLE = {}


def three_way(ref, key, fn, data, later=None):
    """fp32 on all threads, fp32 on one thread, fp64 (tests/test_hip_unroll.py::oracle_runs): once per configuration, shared."""
    if key not in _ORACLE:
        with KinkMargin(ref) as km:
            pred32, loss32, g32 = fn(ref, data, later)
        print(f"[{key}] smallest |ReLU input| of the oracle: {km.min:.2e}")
        assert km.min >= MIN_MARGIN, (key, "the weight seed no longer keeps the ReLU inputs away from 0", km.min)
        n = torch.get_num_threads()
        torch.set_num_threads(1)
        try:
            g32_one = fn(ref, data, later)[2]
        finally:
            torch.set_num_threads(n)
        ref64 = ro.BSMS_Simulator(ref.cfg, dtype=torch.float64)
        ref64.load_state_dict(ref.state_dict())
        ref64.double()
        _, loss64, g64 = fn(ref64, _f64(data), None if later is None else later.double())
        _ORACLE[key] = dict(pred32=pred32, loss32=loss32, loss64=loss64, g32=g32, g32_one=g32_one, g64=g64, t32=0.0, t64=0.0, levels=key)
    return dict(_ORACLE[key])


def accumulate_cycle(eng, ref, data, parts, later=None, **kw):
    """One cycle over `parts` on the engine; returns what `check` looks at: predictions in batch order, the accumulated loss and the
    gradients."""
    mine, grads = engine_model(eng, ref)
    gdata = _cuda(data)
    glater = None if later is None else later.cuda()
    step = eng.FusedStep(mine, grads, accumulate=len(parts), **kw)
    preds = []
    for idx in parts:
        d, lat = part(gdata, idx, glater)
        run(step, d, lat)
        preds.append(torch.stack([q.clone() for q in step.predictions()]))            # [K, b, N, C]
    torch.cuda.synchronize()
    assert step.ready
    return dict(pred=torch.cat(preds, 1).cpu(), loss=float(step.accumulated_loss()),
                gg={k: q.grad.detach().cpu() for k, q in mine.named_parameters() if q.requires_grad}), step, grads


@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_two_micro_batches_are_the_big_batch_step(eng, graphs, shape):
    """reduction = "batch", default loss: sample 0 then sample 1 == the oracle's one step on both."""
    ref, data = make_oracle(shape, graphs)
    r = three_way(ref, (shape, "default"), lambda sim, d, lat: big_batch_oracle(sim, d, None, [1.0], False, None), data)
    got, step, _ = accumulate_cycle(eng, ref, data, [[0], [1]])
    print(f"[{shape}] accumulated loss {got['loss']:.8f}, oracle fp32 {r['loss32']:.8f} fp64 {r['loss64']:.8f}: "
          f"{abs(got['loss'] - r['loss32']) / r['loss32']:.2e} from fp32")
    r.update(got)
    check(r, f"accumulate {shape}")
    ab = step.accumulation_coefficients().tolist()                        # near 1/2 each (the two losses are close), but not the "mean" pair
    assert 0.3 < ab[0] < 0.7 and 0.3 < ab[1] < 0.7 and ab != [0.5, 0.5]


@pytest.mark.parametrize("objective", [("normalized", "mse", [1.0, 3.0]), ("physical", "rmse", [1.0, 3.0])], ids=["normalized-mse", "physical-rmse-w"])
def test_objectives_accumulate_to_the_big_batch_step(eng, graphs, objective):
    ref, data = make_oracle("ring", graphs)
    r = three_way(ref, ("ring", objective[0], objective[1]), lambda sim, d, lat: big_batch_oracle(sim, d, None, [1.0], False, objective), data)
    got, _, _ = accumulate_cycle(eng, ref, data, [[0], [1]], objective=eng.Objective(*objective))
    r.update(got)
    check(r, f"accumulate {objective[0]}/{objective[1]}")


def test_unrolled_mse_accumulates_to_the_big_batch_step(eng, graphs):
    """unroll = 2, kind = "mse", the gradient carried from step to step: against the unrolled oracle on the big batch."""
    ref, data = make_oracle("ring", graphs)
    later, w, objective = later_targets(data[0], data[1], 2), [0.5, 0.5], ("physical", "mse", None)
    r = three_way(ref, ("ring", "unroll2", "mse"), lambda sim, d, lat: big_batch_oracle(sim, d, lat, w, False, objective), data, later)
    got, _, _ = accumulate_cycle(eng, ref, data, [[0], [1]], later, unroll=2, step_weights=w, objective=eng.Objective(*objective))
    r.update(got)
    check(r, "accumulate unroll=2 mse carried")


def test_mean_reduction_is_the_mean_of_the_micro_batch_losses(eng, graphs):
    """reduction = "mean" against the oracle's (rmse_0 + rmse_1) / 2 -- and that is another gradient than "batch" gives."""
    ref, data = make_oracle("ring", graphs)
    parts = [[0], [1]]
    r = three_way(ref, ("ring", "mean"), lambda sim, d, lat: mean_oracle(sim, d, parts), data)
    got, step, grads = accumulate_cycle(eng, ref, data, parts, reduction="mean")
    flat_mean = grads.flat.clone()
    r.update(got)
    check(r, "accumulate mean")
    assert step.accumulation_coefficients().tolist() == [0.5, 0.5]
    _, _, grads_b = accumulate_cycle(eng, ref, data, parts)
    assert not bit_equal(flat_mean, grads_b.flat)


# ------------------------------------------------------------------------------------------------ 9: determinism, no leak
@pytest.mark.parametrize("kw", [dict(), dict(unroll=2, objective=("physical", "mse", None))], ids=["default", "unroll2-mse"])
def test_cycles_are_bit_equal_and_leave_no_state(eng, graphs, kw):
    ref, data = make_oracle("ring", graphs)
    kw = dict(kw)
    if "objective" in kw:
        kw["objective"] = eng.Objective(*kw["objective"])
    gdata = _cuda(data)
    later = later_targets(gdata[0], gdata[1], kw.get("unroll", 1))
    first = [part(gdata, idx, later) for idx in ([0], [1], [0, 1])]
    second = [part(gdata, idx, later) for idx in ([1], [0, 1], [0])]

    def cycle(step, grads, micro):
        for d, lat in micro:
            run(step, d, lat)
        assert step.ready
        return grads.flat.clone(), step.accumulated_loss(), step.accumulation_coefficients()

    mine, grads = engine_model(eng, ref)
    step = eng.FusedStep(mine, grads, accumulate=3, **kw)
    a = cycle(step, grads, first)
    grads.flat.fill_(float("nan"))                                       # whatever the buffer held is overwritten by micro-batch 0
    b = cycle(step, grads, first)
    assert all(bit_equal(x, y) for x, y in zip(a, b))
    c = cycle(step, grads, second)                                         # a cycle behind two others ...
    mine2, grads2 = engine_model(eng, ref)
    fresh = eng.FusedStep(mine2, grads2, accumulate=3, **kw)
    d = cycle(fresh, grads2, second)                                       # ... is the cycle of a fresh object
    assert all(bit_equal(x, y) for x, y in zip(c, d))
    assert not bit_equal(a[0], c[0])


# ------------------------------------------------------------------------------------------------ 10, 11: the Trainer
def _trainer(eng, opt_extra):
    cfg = ro.make_cfg(2, 32, 3, 3, 2)
    model_cfg = SimpleNamespace(consistent_mesh=True, accumulation_steps=1)
    opt_cfg = SimpleNamespace(peak_lr=1e-3, weight_decay=1e-4, warmup_steps=2, decay_steps=20, gnorm_clip=1.0, **opt_extra)
    torch.manual_seed(0)
    ref = ro.BSMS_Simulator(cfg)
    mine = eng.BSMS_Simulator(cfg)
    mine.load_state_dict(ref.state_dict())
    return eng.Trainer(mine, model_cfg, opt_cfg), ref, model_cfg, opt_cfg


def test_trainer_accumulates_two_micro_batches_per_optimizer_step(eng, graphs):
    """gradient_accumulation_steps = 2 on B = 1 micro-batches == the CPU loop (oracle, torch clip_grad_norm_, torch AdamW, the
    schedule) on the B = 2 batch over three optimizer steps; bounds of
    tests/test_hip_training.py::test_trainer_iterations_follow_cpu_reference_loop (losses 2e-4, parameters 2e-3)."""
    from test_hip_unroll import sim_batch
    data = sim_batch(graphs, 3)
    tr, ref, model_cfg, opt_cfg = _trainer(eng, dict(gradient_accumulation_steps=2))
    assert tr.accumulate == 2 and tr.dp.fused.accumulate == 2 and tr.dp.fused.reduction == "batch"
    opt = torch.optim.AdamW([q for q in ref.parameters() if q.requires_grad], lr=opt_cfg.peak_lr, weight_decay=opt_cfg.weight_decay)
    sch = eng.WarmupCosineDecay(opt_cfg.peak_lr, opt_cfg.warmup_steps, opt_cfg.decay_steps)
    ref(data, True, True)                                                  # warm-up: statistics only, on the whole batch in both loops
    assert tr.iter(data) is None and tr.train_step == 1 and tr.last_accumulated_loss is None
    losses_ref, losses = [], []
    for it in range(3):
        opt.zero_grad()
        loss = ro.masked_rmse(ref(data, True, False), data[1], data[2])
        loss.backward()
        torch.nn.utils.clip_grad_norm_(ref.parameters(), opt_cfg.gnorm_clip)
        for group in opt.param_groups:
            group["lr"] = sch.lr()
        opt.step()
        sch.step()
        losses_ref.append(float(loss.detach()))
        for j in (0, 1):
            before = tr.optimizer.flat_p.clone()
            own = tr.iter(part(data, [j])[0])
            assert own is not None and bool(torch.isfinite(own))
            assert tr.train_step == 2 + 2 * it + j                         # train_step counts calls
            if j == 0:                                                     # a non-final call changes no parameter, steps nothing
                assert bit_equal(tr.optimizer.flat_p, before) and tr.optimizer.step_count == it and tr.lr_scheduler.last_epoch == it
                assert not tr.dp.fused.ready
            else:
                assert tr.optimizer.step_count == it + 1 and tr.lr_scheduler.last_epoch == it + 1 and tr.dp.fused.ready
                if it > 0:                                                 # (the first optimizer step sees lr = 0)
                    assert not bit_equal(tr.optimizer.flat_p, before)
        losses.append(float(tr.last_accumulated_loss))
    assert tr.optimizer.step_count == 3 and tr.train_step == 7
    for a, b in zip(losses, losses_ref):
        assert abs(a - b) < 2e-4 * abs(b), (losses, losses_ref)
    for (k, q), (_, g) in zip(ref.named_parameters(), tr.model.named_parameters()):
        if q.requires_grad:
            assert rel_err(g.detach().cpu(), q.detach()) < 2e-3, k


def test_trainer_restore_drops_the_partial_cycle(eng, graphs, tmp_path):
    from test_hip_unroll import sim_batch
    data = sim_batch(graphs, 3)
    tr, _, _, _ = _trainer(eng, dict(gradient_accumulation_steps=2, accumulation_reduction="mean"))
    assert tr.dp.fused.reduction == "mean"
    tr.iter(data)
    tr.iter(part(data, [0])[0])
    assert tr.dp.fused.micro_index == 1
    tr.save(str(tmp_path))                                                 # inside a cycle: the partial sum is not kept
    tr.restore(str(tmp_path), tr.train_step)
    assert tr.dp.fused.micro_index == 0 and tr.optimizer.step_count == 0


def test_trainer_without_the_key_is_the_route_it_was(eng, graphs):
    """Absent, None or 1: accumulate = 1 -- no accumulation buffer, an optimizer step per call, the same bits."""
    from test_hip_unroll import sim_batch
    data = sim_batch(graphs, 3)
    results = []
    for extra in ({}, dict(gradient_accumulation_steps=1), dict(gradient_accumulation_steps=None, accumulation_reduction=None)):
        tr, _, _, _ = _trainer(eng, extra)
        losses = [tr.iter(data) for _ in range(4)]
        assert tr.accumulate == 1 and tr.dp.fused.accumulate == 1 and tr.dp.fused._acc is None and tr.dp.fused._gscratch is None
        assert tr.optimizer.step_count == 3 and tr.last_accumulated_loss is None
        results.append((torch.stack(losses[1:]), tr.optimizer.flat_p.clone()))
    # the bare pieces a Trainer without the key always drove: FusedStep + FusedAdamW + the schedule
    cfg = ro.make_cfg(2, 32, 3, 3, 2)
    torch.manual_seed(0)
    ref = ro.BSMS_Simulator(cfg)
    mine = eng.BSMS_Simulator(cfg)
    mine.load_state_dict(ref.state_dict())
    mine = mine.cuda()
    gdata = _cuda(data)
    mine(gdata, True, True)
    grads = eng.GradBuckets(list(mine.parameters()))
    step, opt = eng.FusedStep(mine, grads), eng.FusedAdamW(grads, lr=1e-3, weight_decay=1e-4, max_grad_norm=1.0)
    sch = eng.WarmupCosineDecay(1e-3, 2, 20)
    losses = []
    for _ in range(3):
        losses.append(step(gdata, True))
        opt.step(sch.lr())
        sch.step()
    results.append((torch.stack(losses), opt.flat_p.clone()))
    for r in results[1:]:
        assert bit_equal(r[0], results[0][0]) and bit_equal(r[1], results[0][1])


# ------------------------------------------------------------------------------------------------ 12: two ranks x two micro-batches
def four_samples(graphs):
    """The golden batch plus its first warm-up batch (same mesh, same mask): four samples.  With the "ring" weights the oracle's
    forward keeps every ReLU input 1.5e-6 from 0 on these four (measured on the CPU oracle; `three_way` asserts MIN_MARGIN)."""
    from test_hip_unroll import sim_batch
    z = load_golden("sim")
    node_in, tar, mask, m_gs, m_ids = sim_batch(graphs, 3)
    rep = lambda t: torch.cat([t, t])
    return (torch.cat([node_in, z.t("warm_in0")]), torch.cat([tar, z.t("warm_tar0")]), rep(mask), [rep(g) for g in m_gs], [rep(i) for i in m_ids])


def _worker(rank, world, port, out_path):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    torch.cuda.set_device(0)
    from conftest import Golden
    import bsms_gnn_amd as eng
    graphs = Golden("graphs")
    ref, _ = make_oracle("ring", graphs)
    torch.manual_seed(50 + rank)                                      # different init per rank: the broadcast must fix it
    sim = eng.BSMS_Simulator(ref.cfg)
    if rank == 0:
        sim.load_state_dict(ref.state_dict())
    sim = sim.cuda()
    data = _cuda(four_samples(graphs))
    engine = eng.DataParallel(sim, bucket_bytes=64 << 10, accumulate=2)
    flats = []
    for t in range(2):                                                # rank r takes samples r and 2 + r
        engine.step_loss_backward(part(data, [2 * t + rank])[0], True)
        flats.append(engine.grads.flat.cpu())
    torch.cuda.synchronize()
    torch.save({"loss": engine.fused.accumulated_loss().cpu(), "flat": engine.grads.flat.cpu(), "after_first": flats[0],
                "coef": engine.fused.accumulation_coefficients().cpu(),
                "grads": {k: q.grad.detach().cpu() for k, q in sim.named_parameters() if q.requires_grad},
                "pred": engine.fused.prediction().cpu()}, f"{out_path}.{rank}")
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.timeout(300)
def test_two_ranks_times_two_micro_batches_equal_the_four_sample_step(eng, graphs, tmp_path):
    """World 2 x accumulate = 2 over gloo on one GPU: the loss sums are all-reduced per micro-batch, the flat gradients once after
    the last fold; every rank folds with the same coefficients and the reduced buffer is the gradient of the loss over the four
    samples (`check` against the oracle's four-sample step)."""
    port = 29900 + os.getpid() % 2000
    out = str(tmp_path / "res")
    mp.start_processes(_worker, args=(2, port, out), nprocs=2, join=True, start_method="spawn")
    r0, r1 = torch.load(out + ".0"), torch.load(out + ".1")
    assert bit_equal(r0["flat"], r1["flat"]) and bit_equal(r0["loss"], r1["loss"]) and bit_equal(r0["coef"], r1["coef"])
    assert not bit_equal(r0["after_first"], r1["after_first"])           # nothing was reduced inside the cycle: each rank's own samples
    ref, _ = make_oracle("ring", graphs)
    data = four_samples(graphs)
    r = three_way(ref, ("ring", "four samples"), lambda sim, d, lat: big_batch_oracle(sim, d, None, [1.0], False, None), data)
    # the predictions the ranks hold are those of their last micro-batch: samples 2 and 3
    got_pred = r["pred32"].clone()
    got_pred[0, 2], got_pred[0, 3] = r0["pred"][0], r1["pred"][0]
    r.update(pred=got_pred, loss=float(r0["loss"]), gg=r0["grads"])
    check(r, "two ranks x two micro-batches")
