"""GPU: the small stand-alone kernels at production-size launches -- the fused clip + AdamW step (csrc/optim.hip) and the row-sum
family (csrc/rowsum.hip) -- through the C ABI.

A. bsms_adamw_step against an fp64 NumPy restatement of torch.optim.AdamW + clip_grad_norm_, with torch's own fp32 CPU step as the
   third party, at sizes that cross the stride of the partial-sum kernel (256 blocks x 256 threads = 65 536 elements), the grid stride of
   the update kernel (2048 blocks x 256 = 524 288) and both with a ragged tail at the size of the real model (~1.9 M parameters).
   Criteria: (distance) max|a - b| / max|b| of params / exp_avg / exp_avg_sq to fp64 is at most 2 x the same distance of torch-fp32,
   plus 2^-23 (one rounding of the tensor scale, for the cases where torch happens to be exact; the factor 2 is the three-way form of
   tests/test_hip_parity.py: it allows another, equally good rounding sequence such as fmaf contraction); (norm) the relative error
   of grad_norm_out to the fp64 norm is no worse than torch-fp32's at the same n, floored at 1e-6 where torch is exact.  Measured
   figures: profiles/primitive_parity.txt.
B. The row sums bit for bit (torch.equal) against the sequential fp32 sum in the caller's edge order, in BOTH launch regimes: every
   launch of csrc/rowsum.hip takes the DEEP (latency) instantiation when workers x lanes < kDeepBelowThreads = 400 * 1024 and the
   plain (bandwidth) one otherwise, and the suite's other bit-exact checks all sit far below that line."""
import numpy as np
import pytest
import torch

from oracle import bsms_oracle as ro

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    import bsms_gnn_amd as eng
    return eng


def _s():
    return torch.cuda.current_stream().cuda_stream


# ==================================================================================================== A: fused clip + AdamW
GUARD = 5                                   # elements past n in params / exp_avg / exp_avg_sq that no launch may touch
F32 = lambda x: float(np.float32(x))        # the C entry takes `float`: every party gets the fp32-rounded hyper-parameter
HYPER = dict(lr=F32(1e-3), b1=F32(0.9), b2=F32(0.999), eps=F32(1e-8), wd=F32(1e-2))
N_PARTIAL_STRIDE, N_GRID_STRIDE, N_MODEL = 256 * 256 + 1, 2048 * 256 + 3, 1_900_037
SIZES = [1, 255, N_PARTIAL_STRIDE, N_GRID_STRIDE, N_MODEL]


def ref_step64(p, g, m, v, step, lr, b1, b2, eps, wd, max_norm):
    """torch.optim.AdamW (decoupled decay, lerp, second moment, two bias corrections, addcdiv) after clip_grad_norm_, in fp64."""
    total = float(np.sqrt(np.sum(g * g)))
    if max_norm > 0:
        g = g * min(max_norm / (total + 1e-6), 1.0)
    p = p * (1.0 - lr * wd)
    m = m + (g - m) * (1.0 - b1)
    v = v * b2 + (1.0 - b2) * g * g
    denom = np.sqrt(v) / np.sqrt(1.0 - b2 ** step) + eps
    return p - (lr / (1.0 - b1 ** step)) * (m / denom), m, v, total


def torch_step32(p, g, m, v, step, lr, b1, b2, eps, wd, max_norm):
    """The same step by torch itself in fp32 on the CPU (single-tensor path); state handed in and out as CPU tensors."""
    q = torch.nn.Parameter(p.clone())
    q.grad = g.clone()
    opt = torch.optim.AdamW([q], lr=lr, betas=(b1, b2), eps=eps, weight_decay=wd, foreach=False)
    opt.state[q] = {"step": torch.tensor(float(step - 1)), "exp_avg": m.clone(), "exp_avg_sq": v.clone()}
    total = float(torch.nn.utils.clip_grad_norm_([q], max_norm if max_norm > 0 else float("inf")))
    opt.step()
    return q.detach(), opt.state[q]["exp_avg"], opt.state[q]["exp_avg_sq"], total


def dist(a, b):
    """max|a - b| / max|b| in fp64 (0 for an all-zero pair)."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    scale = float(np.abs(b).max())
    return float(np.abs(a - b).max()) / scale if scale > 0 else float(np.abs(a).max())


class Fused:
    """Device state of one bsms_adamw_step problem: params / exp_avg / exp_avg_sq with GUARD elements past n."""

    def __init__(self, eng, p, m, v):
        self.eng, self.n = eng, p.numel()
        gen = torch.Generator().manual_seed(12345)
        self.guard = [torch.randn(GUARD, generator=gen) + 7.0 for _ in range(3)]
        self.p, self.m, self.v = (torch.cat([t, gd]).cuda() for t, gd in zip((p, m, v), self.guard))
        self.norm = torch.full((1,), -1.0, device="cuda")
        self.work = torch.empty(max(int(eng._abi.lib().bsms_adamw_work_bytes()), 4), dtype=torch.uint8, device="cuda")

    def step(self, g, step, lr, b1, b2, eps, wd, max_norm, norm_out=True, work=True):
        g = g.cuda()
        self.eng._abi.check(self.eng._abi.lib().bsms_adamw_step(
            self.p.data_ptr(), g.data_ptr(), self.m.data_ptr(), self.v.data_ptr(), self.n, lr, b1, b2, eps, wd, step, max_norm,
            self.norm.data_ptr() if norm_out else None, self.work.data_ptr() if work else None, _s()), "bsms_adamw_step")
        torch.cuda.synchronize()
        for t, gd in zip((self.p, self.m, self.v), self.guard):
            assert torch.equal(t[self.n:].cpu(), gd), "a launch wrote past n"
        return self.state()

    def state(self):
        return tuple(t[:self.n].cpu() for t in (self.p, self.m, self.v))


def check_three_way(tag, got, t32, r64):
    """The distance criterion on (params, exp_avg, exp_avg_sq); returns the figures for the record."""
    out = []
    for name, a, t, r in zip(("params", "exp_avg", "exp_avg_sq"), got, t32, r64):
        assert bool(torch.isfinite(a).all()), (tag, name)
        d_k, d_t = dist(a.numpy(), r), dist(t.numpy(), r)
        print(f"  {tag} {name}: kernel {d_k:.3e}  torch-fp32 {d_t:.3e}")
        assert d_k <= 2.0 * d_t + 2.0 ** -23, (tag, name, d_k, d_t)
        out.append((d_k, d_t))
    return out


def check_norm(tag, got, t32, r64):
    e_k, e_t = abs(got - r64) / r64, abs(t32 - r64) / r64
    print(f"  {tag} grad norm: fp64 {r64:.9e}  kernel rel err {e_k:.3e}  torch-fp32 rel err {e_t:.3e}")
    assert e_k <= max(e_t, 1e-6), (tag, e_k, e_t)
    return e_k, e_t


@pytest.mark.parametrize("n", SIZES)
def test_adamw_three_way_fp64(eng, n):
    """Four consecutive steps, gradients large and small in turn (clipped and unclipped steps alternate, as in
    test_fused_adamw_matches_torch); every party carries its own state in its own precision."""
    gen = torch.Generator().manual_seed(n)
    p0 = torch.randn(n, generator=gen)
    zeros = torch.zeros(n)
    fused = Fused(eng, p0, zeros, zeros)
    t32 = (p0, zeros, zeros)
    r64 = (p0.double().numpy(), np.zeros(n), np.zeros(n))
    print()
    for step in range(1, 5):
        g = torch.randn(n, generator=gen) * (3.0 if step % 2 == 0 else 0.01)
        hp = dict(step=step, max_norm=1.0, **HYPER)
        got = fused.step(g, **hp)
        *t32, t_norm = torch_step32(t32[0], g, t32[1], t32[2], **hp)
        *r64, r_norm = ref_step64(r64[0], g.double().numpy(), r64[1], r64[2], **hp)
        check_norm(f"n={n} step={step}", float(fused.norm), t_norm, r_norm)
        check_three_way(f"n={n} step={step}", got, t32, r64)


def _edge_problem(moments=False, zero_grad=False, gscale=3.0):
    n = N_GRID_STRIDE
    gen = torch.Generator().manual_seed(77)
    p = torch.randn(n, generator=gen)
    g = torch.zeros(n) if zero_grad else torch.randn(n, generator=gen) * gscale
    m = torch.randn(n, generator=gen) * 0.1 if moments else torch.zeros(n)
    v = torch.rand(n, generator=gen) * 0.01 + 1e-4 if moments else torch.zeros(n)
    return p, g, m, v


def _three_parties(eng, p, g, m, v, hp, norm_out=True, work=True):
    fused = Fused(eng, p, m, v)
    got = fused.step(g, norm_out=norm_out, work=work, **hp)
    *t32, t_norm = torch_step32(p, g, m, v, **hp)
    *r64, r_norm = ref_step64(p.double().numpy(), g.double().numpy(), m.double().numpy(), v.double().numpy(), **hp)
    return fused, got, t32, r64, t_norm, r_norm


def test_adamw_norm_without_clipping(eng):
    """max_grad_norm = 0 with grad_norm_out set: the norm is written, the update is unclipped."""
    p, g, m, v = _edge_problem()
    hp = dict(step=1, max_norm=0.0, **HYPER)
    fused, got, t32, r64, t_norm, r_norm = _three_parties(eng, p, g, m, v, hp)
    print()
    assert r_norm > 100.0                                                 # a clip at 1.0 would have changed the update a lot
    check_norm("no clip, norm out", float(fused.norm), t_norm, r_norm)
    check_three_way("no clip, norm out", got, t32, r64)


def test_adamw_clipping_without_norm_out(eng):
    """max_grad_norm > 0 with grad_norm_out null: the update is clipped, nothing is reported."""
    p, g, m, v = _edge_problem()
    hp = dict(step=1, max_norm=1.0, **HYPER)
    fused, got, t32, r64, _, _ = _three_parties(eng, p, g, m, v, hp, norm_out=False)
    print()
    check_three_way("clip, no norm out", got, t32, r64)
    assert float(fused.norm) == -1.0                                      # the scalar was not handed over: untouched


def test_adamw_no_norm_no_work(eng):
    """Clipping off, no norm asked for, `work` null: one launch, unclipped update."""
    p, g, m, v = _edge_problem()
    hp = dict(step=1, max_norm=0.0, **HYPER)
    _, got, t32, r64, _, _ = _three_parties(eng, p, g, m, v, hp, norm_out=False, work=False)
    print()
    check_three_way("no clip, no work", got, t32, r64)
    with pytest.raises(eng._abi.BsmsError):                               # ... but a norm without the work buffer is an error
        Fused(eng, p, m, v).step(g, work=False, **{**hp, "max_norm": 1.0})


def test_adamw_lr_zero(eng):
    """lr = 0 (the first step of the warm-up schedule): params bit-equal to the input, the moments still move."""
    p, g, m, v = _edge_problem(moments=True)
    hp = dict(step=1, max_norm=1.0, **{**HYPER, "lr": 0.0})
    _, got, t32, r64, _, _ = _three_parties(eng, p, g, m, v, hp)
    print()
    assert torch.equal(got[0], p)
    assert not torch.equal(got[1], m) and not torch.equal(got[2], v)
    check_three_way("lr=0", got, t32, r64)


def test_adamw_weight_decay_zero(eng):
    p, g, m, v = _edge_problem(moments=True)
    hp = dict(step=3, max_norm=1.0, **{**HYPER, "wd": 0.0})
    _, got, t32, r64, _, _ = _three_parties(eng, p, g, m, v, hp)
    print()
    check_three_way("wd=0", got, t32, r64)


def test_adamw_zero_gradient(eng):
    """An all-zero gradient: norm 0, clip coefficient 1, everything finite; from zero moments the parameters move by the decay only."""
    p, g, m, v = _edge_problem(zero_grad=True)
    hp = dict(step=1, max_norm=1.0, **HYPER)
    fused, got, t32, r64, t_norm, r_norm = _three_parties(eng, p, g, m, v, hp)
    print()
    assert float(fused.norm) == 0.0 and t_norm == 0.0 and r_norm == 0.0
    assert all(bool(torch.isfinite(t).all()) for t in got)
    assert float(got[1].abs().max()) == 0.0 and float(got[2].abs().max()) == 0.0
    assert np.array_equal(r64[0], p.double().numpy() * (1.0 - HYPER["lr"] * HYPER["wd"]))     # the reference: decay only
    check_three_way("zero grad", got, t32, r64)
    assert not torch.equal(got[0], p)


def test_adamw_large_step_with_moments(eng):
    """step = 100000 (both bias corrections ~1) with non-zero incoming moments."""
    p, g, m, v = _edge_problem(moments=True, gscale=0.05)
    hp = dict(step=100000, max_norm=1.0, **HYPER)
    fused, got, t32, r64, t_norm, r_norm = _three_parties(eng, p, g, m, v, hp)
    print()
    check_norm("step=100000", float(fused.norm), t_norm, r_norm)
    check_three_way("step=100000", got, t32, r64)


def test_adamw_bitwise_repeatable(eng):
    """Two identical calls from identical state give bit-identical results (every block re-reduces the partials in one fixed order)."""
    p, g, m, v = _edge_problem(moments=True)
    hp = dict(step=2, max_norm=1.0, **HYPER)
    a, sa, t32, r64, _, _ = _three_parties(eng, p, g, m, v, hp)
    b = Fused(eng, p, m, v)
    sb = b.step(g, **hp)
    assert all(torch.equal(x, y) for x, y in zip(sa, sb)) and torch.equal(a.norm, b.norm)
    print()
    check_three_way("repeatable", sa, t32, r64)                           # ... and they are the right bits to repeat


# ==================================================================================================== B: row sums, both launch regimes
# csrc/rowsum.hip: `constexpr int64_t kDeepBelowThreads = 400 * 1024`.  launch_rowsum gives a row L lanes (the power of two >= D/4,
# at most 64) and launches the DEEP instantiation (batches of 32 slots, then 8, then the tail) iff deep_regime(workers, L), that is
# workers * L < kDeepBelowThreads, with workers = B * n_out; rowsum_plan_order_bf16 takes the same decision from workers * D/4.
DEEP_BELOW = 400 * 1024
HUB_DEG = 6 * 32 + 16 + 8 + 5              # one row with 32-slot batches (16-slot ones in the bf16 kernel), then 8-slot batches, then a tail
LAT_N = 1531


def lanes(D):
    d4, L = (D + 3) // 4, 1
    while L < d4 and L < 64:
        L *= 2
    return L


def regime_nodes(D, regime, B, per_row=None):
    """Number of output rows that puts B * rows * L at most at HALF the threshold (latency) / at least at TWICE it (bandwidth)."""
    L = lanes(D) if per_row is None else per_row
    if regime == "latency":
        n = min(LAT_N, (DEEP_BELOW // 2) // (B * L))
        assert B * n * L <= DEEP_BELOW // 2
    else:
        n = -(-2 * DEEP_BELOW // (B * L)) + 3                             # + 3: not a multiple of the rows of a workgroup
        assert B * n * L >= 2 * DEEP_BELOW
    return n


def degree_graph(n, seed, src_hub=False):
    """As random_graph(..., hub=) of test_hip_parity.py with E ~ 6 N: random sources, the last N/8 rows receive nothing, one hub row of
    degree >= HUB_DEG.  A condition on the INPUT (not a tolerance): rows of every degree 0..8 exist, so every tail size 1..7 of the
    kernels' switch is taken, as is a row that is exactly one 8-slot batch."""
    rng = np.random.default_rng(seed)
    e = 6 * n
    src = rng.integers(0, n, e)
    dst = rng.integers(0, n - n // 8, e)
    dst[dst == 6] = 7
    dst[1 + rng.choice(e - 1, HUB_DEG, replace=False)] = 6                # exactly HUB_DEG edges
    if src_hub:                                                           # (the by-source sums of bsms_edge_conv: a deep row there too)
        src[src == 10] = 11
        src[1 + rng.choice(e - 1, HUB_DEG, replace=False)] = 10
        src[0] = n - 1                                                    # oracle cal_ew: degree(send) must cover all n nodes
    deg = np.bincount(dst, minlength=n)
    assert set(range(9)) <= set(deg.tolist()) and deg[6] == HUB_DEG and int(deg[n - n // 8:].sum()) == 0
    if src_hub:
        sdeg = np.bincount(src, minlength=n)
        assert set(range(1, 9)) <= set(sdeg.tolist()) and sdeg[10] == HUB_DEG
    return torch.tensor(np.stack([src, dst]), dtype=torch.int64)


def sequential_row_sums(x, dst, n):
    """The definition, in NumPy: every destination row adds its edges one after the other in the caller's order, in fp32."""
    x, dst = x.numpy(), dst.numpy()
    order = np.argsort(dst, kind="stable")
    deg = np.bincount(dst, minlength=n)
    start = np.concatenate([[0], np.cumsum(deg)[:-1]])
    out = np.zeros((x.shape[0], n, x.shape[2]), np.float32)
    for k in range(int(deg.max())):                                       # the k-th edge of every row that has one
        rows = np.nonzero(deg > k)[0]
        out[:, rows] = out[:, rows] + x[:, order[start[rows] + k]]
    return torch.from_numpy(out)


def test_reference_order_is_sequential():
    """oracle.scatter_sum IS the per-row sequential fp32 sum in the caller's edge order: pinned, not assumed (no kernel involved)."""
    n = regime_nodes(128, "latency", 2)
    g = degree_graph(n, 128)
    x = torch.randn(2, g.shape[1], 128, generator=torch.Generator().manual_seed(1))
    assert torch.equal(ro.scatter_sum(x, g[1], -2, n), sequential_row_sums(x, g[1], n))


WIDTHS = [4, 32, 64, 96, 128, 160, 192, 224, 256, 260]


@pytest.mark.parametrize("regime", ["latency", "bandwidth"])
@pytest.mark.parametrize("D", WIDTHS)
def test_segment_sum_fwd_both_regimes(eng, D, regime):
    """bsms_segment_sum_fwd in the caller's order (through the plan's perm) and in plan order (a pure stream)."""
    B = 2
    n = regime_nodes(D, regime, B)
    g = degree_graph(n, 1000 + D)
    e = g.shape[1]
    x = torch.randn(B, e, D, generator=torch.Generator().manual_seed(D))
    want = ro.scatter_sum(x, g[1], -2, n)
    plan = eng.LevelPlan(g.cuda(), n)
    perm = torch.from_numpy(plan.export()[2].astype(np.int64))            # plan slot -> the caller's edge
    L = eng._abi.lib()
    for plan_order, src in ((0, x.cuda()), (1, x[:, perm].contiguous().cuda())):
        out = torch.full((B * n * D + 4,), float("nan"), device="cuda")   # + guard
        eng._abi.check(L.bsms_segment_sum_fwd(plan.handle, src.data_ptr(), B, D, plan_order, out.data_ptr(), _s()), "segment_sum_fwd")
        assert torch.equal(out[:B * n * D].view(B, n, D).cpu(), want), (D, regime, plan_order)
        assert bool(torch.isnan(out[B * n * D:]).all())


def test_scatter_sum_autograd_bandwidth_regime(eng):
    """eng.scatter_sum with its backward (bsms_segment_sum_bwd: a gather by target) at D = 128 in the bandwidth regime."""
    B, D = 2, 128
    n = regime_nodes(D, "bandwidth", B)
    g = degree_graph(n, 2128)
    x = torch.randn(B, g.shape[1], D, generator=torch.Generator().manual_seed(5))
    xd = x.cuda().requires_grad_(True)
    got = eng.scatter_sum(xd, g[1].cuda(), dim=-2, dim_size=n)
    assert torch.equal(got.cpu(), ro.scatter_sum(x, g[1], -2, n))
    cot = torch.randn(B, n, D, generator=torch.Generator().manual_seed(6))
    got.backward(cot.cuda())
    assert torch.equal(xd.grad.cpu(), cot[:, g[1]])


@pytest.mark.parametrize("regime", ["latency", "bandwidth"])
@pytest.mark.parametrize("B", [1, 2])
@pytest.mark.parametrize("D", [128, 256])
def test_segment_sum_bf16_both_regimes(eng, D, B, regime):
    """bsms_segment_sum_bf16 (k_rowsum_bf16in, eight features per lane): bf16 messages in plan order, widened exactly, summed in slot
    order in fp32 -- exactly computable, so bit-equal to the oracle's sum of the widened tensor."""
    n = regime_nodes(D, regime, B, per_row=D // 4)
    g = degree_graph(n, 3000 + D + B)
    x = torch.randn(B, g.shape[1], D, generator=torch.Generator().manual_seed(D + B)).bfloat16()
    want = ro.scatter_sum(x.float(), g[1], -2, n)
    plan = eng.LevelPlan(g.cuda(), n)
    perm = torch.from_numpy(plan.export()[2].astype(np.int64))
    src = x[:, perm].contiguous().cuda()
    assert src.dtype == torch.bfloat16
    out = torch.full((B * n * D + 4,), float("nan"), device="cuda")
    eng._abi.check(eng._abi.lib().bsms_segment_sum_bf16(plan.handle, src.data_ptr(), B, D, out.data_ptr(), _s()), "segment_sum_bf16")
    assert torch.equal(out[:B * n * D].view(B, n, D).cpu(), want)
    assert bool(torch.isnan(out[B * n * D:]).all())


def test_segment_sum_bf16_rejects_other_widths(eng):
    n = LAT_N
    g = degree_graph(n, 3064)
    plan = eng.LevelPlan(g.cuda(), n)
    src = torch.zeros(1, g.shape[1], 64, dtype=torch.bfloat16, device="cuda")
    out = torch.zeros(1, n, 64, device="cuda")
    with pytest.raises(eng._abi.BsmsError, match="BSMS_E_UNSUPPORTED"):
        eng._abi.check(eng._abi.lib().bsms_segment_sum_bf16(plan.handle, src.data_ptr(), 1, 64, out.data_ptr(), _s()), "segment_sum_bf16")


@pytest.fixture(scope="module")
def conv_case():
    """A random graph with a pool of every other node, sized so that even the pooled (kept-row) outputs are in the bandwidth regime."""
    B, D = 2, 128
    n = 2 * regime_nodes(D, "bandwidth", B)
    g = degree_graph(n, 4128, src_hub=True)
    ids = torch.arange(0, n, 2)
    ew, _ = ro.cal_ew(torch.ones(n, 1), g)
    gen = torch.Generator().manual_seed(9)
    return dict(B=B, D=D, n=n, g=g, ids=ids, ew=ew, fine=torch.randn(B, n, D, generator=gen), coarse=torch.randn(B, ids.numel(), D, generator=gen))


@pytest.mark.parametrize("pooled", [0, 1])
@pytest.mark.parametrize("aggregating", [1, 0])
def test_edge_conv_bandwidth_regime(eng, conv_case, aggregating, pooled):
    """bsms_edge_conv (weighted; mapped when prolonging; kept rows when restricting) with the caller's weights and with weights bound
    by bsms_plan_bind_edge_weights (compact lists for the pooled transitions), against the oracle's edge_conv with unpool / row
    selection as tests/test_hip_parity.py builds them at small size."""
    c = conv_case
    B, D, n, g, ids, ew = c["B"], c["D"], c["n"], c["g"], c["ids"], c["ew"]
    nk = ids.numel()
    assert B * (nk if aggregating and pooled else n) * lanes(D) >= 2 * DEEP_BELOW
    x = c["coarse"] if (pooled and not aggregating) else c["fine"]
    if aggregating:
        want = ro.edge_conv(x, g, ew)
        want = want[:, ids] if pooled else want
    else:
        want = ro.edge_conv(ro.unpool(x, n, ids) if pooled else x, g, ew, False)
    L = eng._abi.lib()
    plan = eng.LevelPlan(g.cuda(), n, ids=ids.cuda())
    xd, ewd = x.cuda(), ew.cuda()
    for bound in (False, True):
        eng._abi.check(L.bsms_plan_bind_edge_weights(plan.handle, ewd.data_ptr() if bound else None, _s()), "bind_edge_weights")
        assert (L.bsms_plan_bound_edge_weights(plan.handle) or 0) == (ewd.data_ptr() if bound else 0)
        out = torch.full((want.numel() + 4,), float("nan"), device="cuda")
        eng._abi.check(L.bsms_edge_conv(plan.handle, xd.data_ptr(), B, D, ewd.data_ptr(), aggregating, pooled, out.data_ptr(), _s()), "edge_conv")
        assert torch.equal(out[:want.numel()].view(want.shape).cpu(), want), (aggregating, pooled, bound)
        assert bool(torch.isnan(out[want.numel():]).all())
