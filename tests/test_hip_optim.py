"""GPU: the general optimizer step (bsms_optim_step, csrc/optim.hip) -- parameter groups, the moving average of the
weights and the non-finite guard -- through the C ABI, then through FusedAdamW / Trainer.

The pin is bit-equality with the entry that exists, bsms_adamw_step: the degenerate call as a whole; inside a multi-group call
every group against the old entry run over the WHOLE array with that group's weight decay and lr = fl32(lr * lr_scale),
restricted to the group's elements.  Everything that is compared with fp64 uses the yardsticks of tests/test_hip_primitives.py
unchanged (ref_step64, torch_step32, dist, check_three_way: distance to fp64 <= 2 x torch-fp32's + 2^-23); the `ema` buffer is
held to the same criterion with torch.lerp in fp32 as the third party.  Elements past n (GUARD sentinels, also behind `ema`) are
checked after every call."""
import ctypes as C
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from conftest import load_golden, rel_err
from oracle import bsms_oracle as ro
from test_hip_primitives import F32, GUARD, HYPER, Fused, check_three_way, dist, ref_step64, torch_step32

pytestmark = pytest.mark.gpu

OK, E_INVALID_ARG, E_SHAPE = 0, -1, -2
N_STRIDE = 524_288 + 300                     # crosses the 2048 x 256 grid stride of k_adamw (and 512 chunks of 1024 here)


@pytest.fixture(scope="module")
def eng():
    import bsms_gnn_amd as eng
    return eng


def _s():
    return torch.cuda.current_stream().cuda_stream


class Groups:
    """A bsms_optim_groups_t handle for rows of (offset, count, lr_scale, weight_decay)."""

    def __init__(self, eng, rows, n):
        self.eng, G = eng, eng._abi.OptimGroup
        arr = (G * len(rows))(*[G(*r) for r in rows])
        self.h = C.c_void_p()
        eng._abi.check(eng._abi.lib().bsms_optim_groups_create(C.cast(arr, C.c_void_p), len(rows), n, C.cast(C.byref(self.h), eng._abi.PP)),
                       "bsms_optim_groups_create")

    def __del__(self):
        self.eng._abi.lib().bsms_optim_groups_destroy(self.h)


class New:
    """Device state of one bsms_optim_step problem: params / exp_avg / exp_avg_sq (/ ema) with GUARD sentinels past n, the same
    sentinel values as test_hip_primitives.Fused.  `shift` > 0 starts every array that many floats into its allocation: no
    16-byte alignment."""

    def __init__(self, eng, p, m, v, ema=None, counters=None, shift=0):
        self.eng, self.n, self.shift = eng, p.numel(), shift
        gen = torch.Generator().manual_seed(12345)
        self.guard = [torch.randn(GUARD, generator=gen) + 7.0 for _ in range(3)]
        self.guard.append(self.guard[0] + 1.0)
        hosts = [p, m, v] + ([ema] if ema is not None else [])
        self._alloc = [torch.cat([torch.zeros(shift), t, gd]).cuda() for t, gd in zip(hosts, self.guard)]
        self.arrays = [t[shift:] for t in self._alloc]
        self.p, self.m, self.v = self.arrays[:3]
        self.ema = self.arrays[3] if ema is not None else None
        self.norm = torch.full((1,), -1.0, device="cuda")
        self.work = torch.empty(int(eng._abi.lib().bsms_optim_work_bytes()), dtype=torch.uint8, device="cuda")
        self.counters = None if counters is None else torch.tensor(counters, dtype=torch.int64, device="cuda")

    def call(self, g, groups=None, step=1, lr=0.0, b1=0.0, b2=0.0, eps=0.0, wd=0.0, max_norm=0.0, norm_out=True, work=True,
             ema_decay=0.0, n=None):
        """The raw call: returns the error code; `g` is a device tensor."""
        return self.eng._abi.lib().bsms_optim_step(
            self.p.data_ptr(), g.data_ptr(), self.m.data_ptr(), self.v.data_ptr(), self.n if n is None else n,
            None if groups is None else groups.h, lr, b1, b2, eps, wd, step, max_norm,
            None if self.ema is None else self.ema.data_ptr(), ema_decay, None if self.counters is None else self.counters.data_ptr(),
            self.norm.data_ptr() if norm_out else None, self.work.data_ptr() if work else None, _s())

    def step(self, g, **kw):
        gd = torch.cat([torch.zeros(self.shift), g]).cuda()[self.shift:]
        self.eng._abi.check(self.call(gd, **kw), "bsms_optim_step")
        torch.cuda.synchronize()
        self.check_guards()
        return self.state()

    def check_guards(self):
        for t, gd in zip(self.arrays, self.guard):
            assert torch.equal(t[self.n:].cpu(), gd), "a launch wrote past n"

    def state(self):
        return tuple(t[:self.n].cpu() for t in self.arrays)


def bits_equal(a, b):
    return all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(a, b))


def problem(n, seed, moments=True):
    gen = torch.Generator().manual_seed(seed)
    p = torch.randn(n, generator=gen)
    m = torch.randn(n, generator=gen) * 0.1 if moments else torch.zeros(n)
    v = torch.rand(n, generator=gen) * 0.01 + 1e-4 if moments else torch.zeros(n)
    return p, m, v, gen


# ==================================================================================================== 1: degenerate call = old entry
@pytest.mark.parametrize("clip,norm_out", [(True, True), (True, False), (False, True), (False, False)])
@pytest.mark.parametrize("n,shift", [(1, 0), (255, 0), (257, 0), (1000, 0), (N_STRIDE, 0), (5000, 1)])
def test_degenerate_call_is_the_old_entry_bit_for_bit(eng, n, shift, clip, norm_out):
    """groups = ema = counters = NULL: three consecutive steps, large and small gradients in turn.  (5000, 1): every array starts
    4 bytes past a 16-byte boundary, so the full chunks take the element-wise path as well."""
    p, m, v, gen = problem(n, n, moments=False)
    old, new = Fused(eng, p, m, v), New(eng, p, m, v, shift=shift)
    for step in range(1, 4):
        g = torch.randn(n, generator=gen) * (3.0 if step % 2 == 0 else 0.01)
        hp = dict(step=step, max_norm=1.0 if clip else 0.0, **HYPER)
        want = old.step(g, norm_out=norm_out, **hp)
        got = new.step(g, norm_out=norm_out, **hp)
        assert bits_equal(got, want), (n, step)
        assert torch.equal(new.norm, old.norm) and (norm_out or float(new.norm) == -1.0)
    assert not torch.equal(want[0], p)


# ==================================================================================================== 2: groups
SIZES = [1, 3, 255, 256, 257, 1024, 1]
SCALES = [1.0, 0.1, 3.0, 1.0, 0.0, 1.0, 3.0, 0.1, 1.0]          # drawn from {0, 0.1, 1, 3}
DECAYS = [0.01, 0.3, 0.0, 0.3, 0.0, 0.0, 0.01, 0.01, 0.3]       # drawn from {0, 0.01, 0.3}; group 4 is (0, 0): frozen in effect


def table(n, boundary=None):
    """Groups of SIZES, then the rest -- cut once more at `boundary` when given."""
    sizes = SIZES + ([n - sum(SIZES)] if boundary is None else [boundary - sum(SIZES), n - boundary])
    offs = np.concatenate([[0], np.cumsum(sizes)])
    assert offs[-1] == n and min(sizes) >= 1
    return [(int(o), int(c), F32(s), F32(w)) for o, c, s, w in zip(offs, sizes, SCALES, DECAYS)]


def torch_groups32(rows, p, g, m, v, step, lr, b1, b2, eps, max_norm):
    """torch.optim.AdamW with one param group per row, fp32 on the CPU, after clip_grad_norm_ over all of them."""
    qs = []
    for off, cnt, _, _ in rows:
        q = torch.nn.Parameter(p[off:off + cnt].clone())
        q.grad = g[off:off + cnt].clone()
        qs.append(q)
    opt = torch.optim.AdamW([{"params": [q], "lr": F32(np.float32(lr) * np.float32(s)), "weight_decay": w} for q, (_, _, s, w) in zip(qs, rows)],
                            lr=lr, betas=(b1, b2), eps=eps, foreach=False)
    for q, (off, cnt, _, _) in zip(qs, rows):
        opt.state[q] = {"step": torch.tensor(float(step - 1)), "exp_avg": m[off:off + cnt].clone(), "exp_avg_sq": v[off:off + cnt].clone()}
    torch.nn.utils.clip_grad_norm_(qs, max_norm if max_norm > 0 else float("inf"))
    opt.step()
    cat = lambda key: torch.cat([opt.state[q][key] for q in qs])
    return torch.cat([q.detach() for q in qs]), cat("exp_avg"), cat("exp_avg_sq")


def ref_groups64(rows, p, g, m, v, step, lr, b1, b2, eps, max_norm):
    """The fp64 restatement: the clip coefficient from the whole gradient, then ref_step64 per group on the clipped gradient."""
    total = float(np.sqrt(np.sum(g * g)))
    if max_norm > 0:
        g = g * min(max_norm / (total + 1e-6), 1.0)
    out = [np.empty_like(p), np.empty_like(p), np.empty_like(p)]
    for off, cnt, s, w in rows:
        sl = slice(off, off + cnt)
        res = ref_step64(p[sl], g[sl], m[sl], v[sl], step, float(np.float32(lr) * np.float32(s)), b1, b2, eps, w, 0.0)
        for dst, r in zip(out, res[:3]):
            dst[sl] = r
    return out


def run_group_table(eng, n, rows, seed):
    """Two steps with the moments carried.  Per step: every group bit-equal to the old entry over the whole array with
    (fl32(lr * s), wd) of the group; the whole array within the three-way criterion of torch's param groups and of fp64."""
    p, m, v, gen = problem(n, seed)
    new = New(eng, p, m, v)
    handle = Groups(eng, rows, n)
    t32, r64 = (p, m, v), tuple(t.double().numpy() for t in (p, m, v))
    cur = (p, m, v)
    hp = {k: HYPER[k] for k in ("lr", "b1", "b2", "eps")}
    print()
    for step in (1, 2):
        g = torch.randn(n, generator=gen) * (3.0 if step == 2 else 0.01)            # step 2 is clipped
        got = new.step(g, groups=handle, step=step, max_norm=1.0, wd=123.0, **hp)    # with a handle the scalar decay is not read
        by_hyper = {}
        for off, cnt, s, w in rows:
            if (s, w) not in by_hyper:
                lr_k = F32(np.float32(hp["lr"]) * np.float32(s))
                old = Fused(eng, *cur)
                by_hyper[(s, w)] = (old.step(g, step=step, max_norm=1.0, wd=w, **{**hp, "lr": lr_k}), old.norm.clone())
            want, norm = by_hyper[(s, w)]
            sl = slice(off, off + cnt)
            assert bits_equal([t[sl] for t in got], [t[sl] for t in want]), (step, off, cnt, s, w)
            assert torch.equal(new.norm, norm)
            if s == 0.0 and w == 0.0:                                                # lr 0, decay 0: parameters stay, moments move
                assert torch.equal(got[0][sl], cur[0][sl]) and not torch.equal(got[1][sl], cur[1][sl]) and not torch.equal(got[2][sl], cur[2][sl])
        t32 = torch_groups32(rows, t32[0], g, t32[1], t32[2], step=step, max_norm=1.0, **hp)
        r64 = ref_groups64(rows, r64[0], g.double().numpy(), r64[1], r64[2], step=step, max_norm=1.0, **hp)
        check_three_way(f"groups n={n} step={step}", got, t32, r64)
        cur = got
    return got


def test_groups_small_table(eng):
    n = 6000
    rows = table(n)
    assert any(r[2] == 0.0 and r[3] == 0.0 for r in rows) and sum(r[2] == 1.0 for r in rows) >= 3
    run_group_table(eng, n, rows, 21)


def test_groups_across_the_grid_stride(eng):
    """The same table on the 524 588-element array, one boundary at element 524 287 (the last element of k_adamw's first stride)."""
    rows = table(N_STRIDE, boundary=524_287)
    assert rows[-1][0] == 524_287 and rows[-1][1] == N_STRIDE - 524_287
    run_group_table(eng, N_STRIDE, rows, 22)


def test_one_group_split_into_five_is_the_same_bits(eng):
    n = 6000
    p, m, v, gen = problem(n, 23)
    g = torch.randn(n, generator=gen)
    s, w = F32(0.1), F32(0.3)
    cuts = [0, 1, 1025, 2048, 2051, n]
    one = Groups(eng, [(0, n, s, w)], n)
    five = Groups(eng, [(a, b - a, s, w) for a, b in zip(cuts, cuts[1:])], n)
    hp = dict(step=2, max_norm=1.0, **{k: HYPER[k] for k in ("lr", "b1", "b2", "eps")})
    a = New(eng, p, m, v).step(g, groups=one, **hp)
    b = New(eng, p, m, v).step(g, groups=five, **hp)
    assert bits_equal(a, b) and not torch.equal(a[0], p)


# ==================================================================================================== 3: EMA
@pytest.mark.parametrize("decay", [0.9, 0.3])
def test_ema_three_way_fp64(eng, decay):
    """Three steps over the group table with an average kept; 0.9 and 0.3 take the two forms of the lerp.  The parameters and
    moments are bit-equal to a run without `ema`."""
    n = 6000
    rows, d = table(n), F32(decay)
    p, m, v, gen = problem(n, 31)
    e0 = p + 0.05 * torch.randn(n, generator=gen)
    handle = Groups(eng, rows, n)
    with_ema, without = New(eng, p, m, v, ema=e0), New(eng, p, m, v)
    hp = {k: HYPER[k] for k in ("lr", "b1", "b2", "eps")}
    t32, r64 = (p, m, v), tuple(t.double().numpy() for t in (p, m, v))
    e32, e64 = e0.clone(), e0.double().numpy()
    print()
    for step in (1, 2, 3):
        g = torch.randn(n, generator=gen) * (3.0 if step == 2 else 0.01)
        got = with_ema.step(g, groups=handle, step=step, max_norm=1.0, ema_decay=d, **hp)
        assert bits_equal(got[:3], without.step(g, groups=handle, step=step, max_norm=1.0, **hp))
        t32 = torch_groups32(rows, t32[0], g, t32[1], t32[2], step=step, max_norm=1.0, **hp)
        r64 = ref_groups64(rows, r64[0], g.double().numpy(), r64[1], r64[2], step=step, max_norm=1.0, **hp)
        e32 = torch.lerp(e32, t32[0], 1.0 - d)
        e64 = e64 + (r64[0] - e64) * (1.0 - d)
        check_three_way(f"ema {decay} step={step}", got[:3], t32, r64)
        d_k, d_t = dist(got[3].numpy(), e64), dist(e32.numpy(), e64)
        print(f"  ema {decay} step={step} ema: kernel {d_k:.3e}  torch.lerp-fp32 {d_t:.3e}")
        assert d_k <= 2.0 * d_t + 2.0 ** -23, (decay, step, d_k, d_t)


@pytest.mark.parametrize("n,shift", [(6000, 0), (6000, 3)])
def test_ema_decay_zero_and_one(eng, n, shift):
    p, m, v, gen = problem(n, 32)
    e0 = torch.randn(n, generator=gen)
    g = torch.randn(n, generator=gen)
    hp = dict(step=1, max_norm=1.0, **HYPER)
    follow = New(eng, p, m, v, ema=e0, shift=shift).step(g, ema_decay=0.0, **hp)
    assert bits_equal([follow[3]], [follow[0]]) and not torch.equal(follow[0], p)        # decay 0: the average IS the new parameters
    keep = New(eng, p, m, v, ema=e0, shift=shift).step(g, ema_decay=1.0, **hp)
    assert bits_equal([keep[3]], [e0]) and bits_equal(keep[:3], follow[:3])               # decay 1: the average does not move


# ==================================================================================================== 4: the guard
def _bad(n, where, value, gen):
    g = torch.randn(n, generator=gen)
    g[where] = value
    return g


@pytest.mark.parametrize("n,where,value", [(1000, -1, float("inf")), (1000, 0, float("nan")), (N_STRIDE, 524_288 + 100, float("nan"))],
                         ids=["inf-last", "nan-first", "nan-past-grid-stride"])
def test_guard_skips_a_non_finite_gradient(eng, n, where, value):
    a, s = 2, 1
    p, m, v, gen = problem(n, 41)
    e0 = p + 0.05 * torch.randn(n, generator=gen)
    rows = [(0, n // 3, F32(1.0), F32(0.01)), (n // 3, n - n // 3, F32(1.0), F32(0.01))]
    handle = Groups(eng, rows, n)
    new = New(eng, p, m, v, ema=e0, counters=[a, s])
    hp = {k: HYPER[k] for k in ("lr", "b1", "b2", "eps")}
    for max_norm in (1.0, 0.0):                                                       # the norm is formed with clipping off too
        got = new.step(_bad(n, where, value, gen), groups=handle, step=0, max_norm=max_norm, ema_decay=F32(0.9), **hp)
        s += 1
        assert bits_equal(got, (p, m, v, e0)), "a skipped step wrote"
        assert new.counters.tolist() == [a, s]
        assert not np.isfinite(float(new.norm))
    # the next finite gradient is step a + 1
    g = torch.randn(n, generator=gen) * 0.01
    got = new.step(g, groups=handle, step=0, max_norm=1.0, ema_decay=F32(0.9), **hp)
    assert new.counters.tolist() == [a + 1, s] and np.isfinite(float(new.norm))
    full = dict(step=a + 1, max_norm=1.0, **HYPER)
    *t32, _ = torch_step32(p, g, m, v, **full)
    *r64, _ = ref_step64(*(t.double().numpy() for t in (p, g, m, v)), **full)
    print()
    check_three_way(f"guard n={n}: step {a + 1} after a skip", got[:3], t32, r64)
    assert not bits_equal([got[3]], [e0])


def _finite_sequence(eng, n, seed):
    p, m, v, gen = problem(n, seed, moments=False)
    new, old = New(eng, p, m, v, counters=[0, 0]), Fused(eng, p, m, v)
    t32, r64 = (p, m, v), tuple(t.double().numpy() for t in (p, m, v))
    for step in (1, 2, 3):
        g = torch.randn(n, generator=gen) * (3.0 if step == 2 else 0.01)
        got = new.step(g, step=0, max_norm=1.0, **HYPER)
        hp = dict(step=step, max_norm=1.0, **HYPER)
        want = old.step(g, **hp)
        *t32, _ = torch_step32(t32[0], g, t32[1], t32[2], **hp)
        *r64, _ = ref_step64(r64[0], g.double().numpy(), r64[1], r64[2], **hp)
        check_three_way(f"guard, finite step {step}", got, t32, r64)
        for name, x, y, r in zip(("params", "exp_avg", "exp_avg_sq"), got, want, r64):   # ... and with the old entry as the third party
            assert dist(x.numpy(), r) <= 2.0 * dist(y.numpy(), r) + 2.0 ** -23, (step, name)
        assert torch.equal(new.norm, old.norm)
    assert new.counters.tolist() == [3, 0]
    return got


def test_guard_counts_three_finite_steps_on_the_device(eng):
    """The step number comes from the device counter; the old entry at step = 1, 2, 3 is the comparison.  Two runs: the same bits."""
    print()
    first = _finite_sequence(eng, 70_000, 42)
    assert bits_equal(first, _finite_sequence(eng, 70_000, 42))


def test_guard_counts_an_overflowing_sum_of_squares_as_non_finite(eng):
    """Finite gradients whose sum of squares exceeds fp32: the norm is inf, the step is skipped (documented in bsms_hip.h)."""
    n = 300
    p, m, v, _ = problem(n, 43)
    new = New(eng, p, m, v, counters=[0, 0])
    got = new.step(torch.full((n,), 1e20), step=0, max_norm=1.0, **HYPER)
    assert bits_equal(got, (p, m, v)) and new.counters.tolist() == [0, 1] and float(new.norm) == float("inf")


# ==================================================================================================== 5: capture
def test_step_with_everything_captures_into_a_graph(eng):
    n = 6000
    rows = table(n)
    p, m, v, gen = problem(n, 51)
    e0 = p.clone()
    g = torch.randn(n, generator=gen).cuda()
    handle = Groups(eng, rows, n)
    kw = dict(groups=handle, step=0, max_norm=1.0, ema_decay=F32(0.9), **{k: HYPER[k] for k in ("lr", "b1", "b2", "eps")})
    eager = New(eng, p, m, v, ema=e0, counters=[0, 0])
    for _ in range(3):
        assert eager.call(g, **kw) == OK
    torch.cuda.synchronize()
    cap = New(eng, p, m, v, ema=e0, counters=[0, 0])
    graph, rcs = torch.cuda.CUDAGraph(), []
    with torch.cuda.graph(graph, capture_error_mode="thread_local"):
        rcs.append(cap.call(g, **kw))
    assert rcs == [OK]
    torch.cuda.synchronize()
    assert bits_equal(cap.state(), (p, m, v, e0)) and cap.counters.tolist() == [0, 0]      # captured, not run
    for _ in range(3):
        graph.replay()
    torch.cuda.synchronize()
    cap.check_guards()
    assert bits_equal(cap.state(), eager.state()) and cap.counters.tolist() == eager.counters.tolist() == [3, 0]
    assert torch.equal(cap.norm, eager.norm)


# ==================================================================================================== 6: refusals on the device
def test_step_refusals_touch_nothing(eng):
    n = 3000
    L = eng._abi.lib()
    seven = torch.full((n,), 7.0)
    g = torch.randn(n).cuda()
    handle = Groups(eng, [(0, n - 1, 1.0, 0.0)], n - 1)
    hp = dict(max_norm=1.0, **HYPER)
    cases = [
        ("handle n != call n", dict(groups=handle, step=1), False, E_SHAPE, b"group table covers"),
        ("counters without work", dict(step=0, work=False), True, E_INVALID_ARG, b"work buffer"),
        ("counters with step != 0", dict(step=1), True, E_INVALID_ARG, b"with counters"),
        ("ema_decay 1.5", dict(step=1, ema_decay=1.5), False, E_INVALID_ARG, b"ema_decay"),
        ("step 0 without counters", dict(step=0), False, E_SHAPE, b"step counts from 1"),
    ]
    for what, kw, counters, code, word in cases:
        new = New(eng, seven, seven, seven, ema=seven, counters=[7, 7] if counters else None)
        rc = new.call(g, **{**hp, **kw})
        msg = L.bsms_last_error()
        torch.cuda.synchronize()
        assert rc == code and word in msg, (what, rc, msg)
        new.check_guards()
        assert all(bool((t == 7.0).all()) for t in new.state()) and float(new.norm) == -1.0, what
        assert new.counters is None or new.counters.tolist() == [7, 7], what


# ==================================================================================================== 7: FusedAdamW / Trainer
MODEL_CFG = SimpleNamespace(consistent_mesh=True, accumulation_steps=1)
B = 2


def opt_cfg(**extra):
    return SimpleNamespace(peak_lr=1e-3, weight_decay=1e-4, warmup_steps=2, decay_steps=20, gnorm_clip=1.0, **extra)


@pytest.fixture(scope="module")
def small(eng, graphs):
    """The small golden model of test_trainer_iterations_follow_cpu_reference_loop: sim.npz on del300, make_cfg(2, 32, 3, 3, 2)."""
    z = load_golden("sim")
    es, ids = graphs.levels("del300")
    cfg = ro.make_cfg(2, 32, 3, 3, 2)
    torch.manual_seed(0)
    ref = ro.BSMS_Simulator(cfg)
    data = (z.t("node_in"), z.t("tar"), z.t("mask"), [e.unsqueeze(0).repeat(B, 1, 1) for e in es], [i.unsqueeze(0).repeat(B, 1) for i in ids])
    return SimpleNamespace(cfg=cfg, data=data, state={k: v.clone() for k, v in ref.state_dict().items()})


def make_trainer(eng, small, **extra):
    model = eng.BSMS_Simulator(small.cfg)
    model.load_state_dict(small.state)
    return eng.Trainer(model, MODEL_CFG, opt_cfg(**extra))


def run(tr, data, iters=5):
    return [float(out) for out in (tr.iter(data) for _ in range(iters)) if out is not None]


def test_trainer_param_groups_follow_the_cpu_oracle_loop(eng, small):
    """Warm-up + 4 steps with no_decay_bias and lr_scales = {"process": 0.1} == the same loop on the CPU oracle with
    torch.optim.AdamW param groups, at the tolerances of test_trainer_iterations_follow_cpu_reference_loop."""
    cfgo = opt_cfg(no_decay_bias=True, lr_scales={"process": 0.1})
    ref = ro.BSMS_Simulator(small.cfg)
    ref.load_state_dict(small.state)
    pg, scale_of = [], []
    for name, p in ref.named_parameters():
        if p.requires_grad:
            scale = 0.1 if name.startswith("process.") else 1.0
            pg.append({"params": [p], "weight_decay": 0.0 if p.dim() == 1 else cfgo.weight_decay})
            scale_of.append(scale)
    opt = torch.optim.AdamW(pg, lr=cfgo.peak_lr)
    sch = eng.WarmupCosineDecay(cfgo.peak_lr, cfgo.warmup_steps, cfgo.decay_steps)
    tr = make_trainer(eng, small, no_decay_bias=True, lr_scales={"process": 0.1})
    assert tr.optimizer._groups is not None and len(tr.optimizer.segments) > 10
    data, losses_ref = small.data, []
    for step in range(5):
        if step < MODEL_CFG.accumulation_steps:
            ref(data, True, True)
            continue
        opt.zero_grad()
        loss = ro.masked_rmse(ref(data, True, False), data[1], data[2])
        loss.backward()
        torch.nn.utils.clip_grad_norm_(ref.parameters(), cfgo.gnorm_clip)
        for gparam, scale in zip(opt.param_groups, scale_of):
            gparam["lr"] = sch.lr() * scale
        opt.step()
        sch.step()
        losses_ref.append(float(loss))
    losses = run(tr, data)
    assert len(losses) == 4
    for a, b in zip(losses, losses_ref):
        assert abs(a - b) < 2e-4 * abs(b), (losses, losses_ref)
    for (k, p), (_, q) in zip(ref.named_parameters(), tr.model.named_parameters()):
        if p.requires_grad:
            assert rel_err(q.detach().cpu(), p.detach()) < 2e-3, k
    # the groups did something: the same run without them ends elsewhere
    plain = make_trainer(eng, small)
    run(plain, data)
    assert not torch.equal(plain.optimizer.flat_p, tr.optimizer.flat_p)


def test_trainer_ema_model_save_restore(eng, small, tmp_path):
    data = small.data
    tr = make_trainer(eng, small, ema_decay=0.9, skip_nonfinite=True)
    opt = tr.optimizer
    e32, e64, history = opt.ema.cpu().clone(), opt.ema.cpu().double().numpy(), 0
    for it in range(5):
        out = tr.iter(data)
        if out is None:
            e32, e64 = opt.ema.cpu().clone(), opt.ema.cpu().double().numpy()      # warm-up: no step; the average is the initial parameters
            continue
        d = F32(opt.ema_decay_at(history))
        p_now = opt.flat_p.cpu()
        e32 = torch.lerp(e32, p_now, 1.0 - d)
        e64 = e64 + (p_now.double().numpy() - e64) * (1.0 - d)
        history += 1
    assert history == 4 and opt.ema_decay_at(0) == 0.1 and opt.ema_decay_at(100) == 0.9
    got = torch.cat([q.detach().reshape(-1) for q in sorted((q for q in tr.model.parameters() if q.requires_grad), key=lambda q: opt.grads._slot[q][0])])
    assert torch.equal(got, opt.flat_p)                                             # the slot order covers the flat array
    twin = dict(tr.ema_model().named_parameters())
    avg = torch.cat([twin[k].detach().reshape(-1) for k, q in sorted(((k, q) for k, q in tr.model.named_parameters() if q.requires_grad),
                                                                      key=lambda kq: opt.grads._slot[kq[1]][0])]).cpu()
    d_k, d_t = dist(avg.numpy(), e64), dist(e32.numpy(), e64)
    print(f"\n  trainer ema: engine {d_k:.3e}  torch.lerp-fp32 {d_t:.3e}")
    assert d_k <= 2.0 * d_t + 2.0 ** -23 and not torch.equal(avg, opt.flat_p.cpu())
    assert tr.ema_model() is tr.ema_model()
    # the saved average, loaded into a fresh model, predicts the same bits
    tr.save(str(tmp_path))
    fresh = eng.BSMS_Simulator(small.cfg)
    fresh.load_state_dict(torch.load(f"{tmp_path}/{tr.train_step}_ema_params.pth"))
    fresh = fresh.cuda()
    with torch.no_grad():
        before = tr.get_pred(data, ema=True).clone()
        want = fresh(tr.move_to_device(data), True, False)
        live = tr.get_pred(data)
    assert torch.equal(before, want) and not torch.equal(before, live)
    loss_ema, loss_live = float(tr.get_loss(data, ema=True)), float(tr.get_loss(data))
    assert np.isfinite(loss_ema) and loss_ema != loss_live
    assert np.all(np.isfinite(tr.get_error(data, ema=True)[0]))
    # save -> restore -> one iter on both
    again = make_trainer(eng, small, ema_decay=0.9, skip_nonfinite=True)
    again.restore(str(tmp_path), tr.train_step)
    assert torch.equal(again.optimizer.ema, opt.ema) and again.optimizer.counters.tolist() == opt.counters.tolist() == [4, 0]
    l1, l2 = tr.iter(data), again.iter(data)
    assert abs(float(l1) - float(l2)) < 1e-6 * abs(float(l1))
    assert (again.optimizer.applied_steps(), again.optimizer.skipped_steps()) == (opt.applied_steps(), opt.skipped_steps()) == (5, 0)
    with torch.no_grad():
        assert not torch.equal(tr.get_pred(data, ema=True), before)                 # the view followed the step: no copy to refresh
    # a checkpoint without the average (restore_opt_state=False): it restarts from the restored parameters
    cold = make_trainer(eng, small, ema_decay=0.9)
    cold.restore(str(tmp_path), 5, restore_opt_state=False)
    assert torch.equal(cold.optimizer.ema, cold.optimizer.flat_p)


def test_trainer_skips_a_non_finite_batch(eng, small):
    data = small.data
    tr = make_trainer(eng, small, skip_nonfinite=True)
    losses = run(tr, data, 3)
    assert len(losses) == 2 and all(np.isfinite(losses))
    before = [t.clone() for t in (tr.optimizer.flat_p, tr.optimizer.exp_avg, tr.optimizer.exp_avg_sq)]
    epoch = tr.lr_scheduler.last_epoch
    tar = data[1].clone()
    tar[0, 5, 0] = float("inf")
    bad = tr.iter((data[0], tar, data[2], data[3], data[4]))
    assert not np.isfinite(float(bad))
    assert bits_equal(before, (tr.optimizer.flat_p, tr.optimizer.exp_avg, tr.optimizer.exp_avg_sq))
    assert tr.optimizer.skipped_steps() == 1 and tr.optimizer.applied_steps() == 2 and tr.optimizer.step_count == 3
    assert not np.isfinite(float(tr.optimizer.grad_norm))
    assert tr.lr_scheduler.last_epoch == epoch + 1                                  # the schedule advances over a skipped step
    assert np.isfinite(float(tr.iter(data))) and tr.optimizer.applied_steps() == 3
    assert bool(torch.isfinite(tr.optimizer.flat_p).all()) and not torch.equal(before[0], tr.optimizer.flat_p)


def test_trainer_without_new_keys_is_the_old_trainer(eng, small):
    """No new key: no handle, no average, no counters, and the losses / parameters are bit-equal to a Trainer whose optimizer step
    is the call the class made before the options existed, written out here."""
    data = small.data
    tr, old = make_trainer(eng, small), make_trainer(eng, small)
    for o in (tr.optimizer, old.optimizer):
        assert o._groups is None and o.ema is None and o.counters is None and o.segments is None and not o.extended
    seen = []

    def parent_step(lr=None, o=old.optimizer):
        from bsms_gnn_amd.ops import bump_param_epoch
        o.step_count += 1
        b1, b2 = o.betas
        eng._abi.check(eng._abi.lib().bsms_adamw_step(
            o.flat_p.data_ptr(), o.grads.flat.data_ptr(), o.exp_avg.data_ptr(), o.exp_avg_sq.data_ptr(), o.flat_p.numel(),
            float(o.lr if lr is None else lr), b1, b2, o.eps, o.wd, o.step_count, float(o.max_norm), o.grad_norm.data_ptr(),
            o._work.data_ptr(), _s()), "bsms_adamw_step")
        bump_param_epoch()
        seen.append(o.step_count)

    old.optimizer.step = parent_step
    a, b = run(tr, data), run(old, data)
    assert a == b and len(a) == 4 and seen == [1, 2, 3, 4]
    assert bits_equal((tr.optimizer.flat_p, tr.optimizer.exp_avg, tr.optimizer.exp_avg_sq),
                      (old.optimizer.flat_p, old.optimizer.exp_avg, old.optimizer.exp_avg_sq))
    with pytest.raises(ValueError, match="no EMA"):
        tr.ema_model()
