"""GPU: the gradient of the (K-step) loss w.r.t. the step's input through step.FusedStep(input_grad=True) --
bsms_sim_input_grad on its own against NumPy fp64, bsms_bsgmp_bwd_pos_ev against the entries it combines, the fused step with
the flag against the step without it (nothing else moves), against the autograd route (one step) and against the CPU oracle
unrolled under autograd with `node_in` a leaf (K steps), graph replay, two data-parallel ranks and `input_gradient()`.

Everything runs on the 600-row golden `sim` batch (del300, B = 2, C = 2, p = 2, 67 rows with mask == 0) or the 364-row
block-diagonal batch, with the model shapes, weight seeds and later targets tests/test_hip_unroll.py pins.

Tolerances.  The kernel: 1e-6 of the column group's maximum (a result goes through at most three fp32 roundings of 6e-8 each: the
division's, g_pred + t, grad_in + contribution).  One step against the autograd route: 1e-6 per column group (the same kernels on
the same inputs; at most one fp32 add in another order).  K steps: the criterion of test_hip_pos_grad._three_way for node_in.grad,
per column group and on the state columns of the rows with mask == 0 -- the engine's distance to the fp64 oracle, in max-norm and in
relative L2, stays within max(1e-5, 3 x the larger of the fp32 oracle's two distances).  The fp32 oracle runs are 5e-7 .. 1.5e-6
from fp64 in every group on "ring" and "d64", so the floor binds."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from conftest import ROOT, KinkMargin, load_golden, rel_err
from oracle import bsms_oracle as ro
from test_hip_unroll import MIN_MARGIN, _cuda, _f64, _stats, later_targets, make_oracle

pytestmark = pytest.mark.gpu
C_, P_ = 2, 2                                                          # the golden batches: two state channels, two coordinates
GROUPS = {"state": slice(0, C_), "position": slice(C_, C_ + P_), "type": slice(C_ + P_, C_ + P_ + 1)}


@pytest.fixture(scope="module")
def eng():
    import bsms_gnn_amd as eng
    return eng


def _ptr(t):
    return None if t is None else t.data_ptr()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def bits(t):
    return t.detach().contiguous().reshape(-1).view(torch.uint8)


def bit_equal(a, b):
    return a.shape == b.shape and bool(torch.equal(bits(a), bits(b)))


# ------------------------------------------------------------------------------------------------ 1: bsms_sim_input_grad alone
@pytest.mark.parametrize("C,p", [(1, 1), (2, 2), (8, 7)])
@pytest.mark.parametrize("R", [1, 257, 1000])
def test_sim_input_grad_kernel(eng, R, C, p):
    """One thread, two blocks with a ragged tail, four blocks.  The mask holds 0, 1 and one 0.5 entry (R > 2), mask[0] = 0 and then
    mask[R-1] = 1 (at R = 1 the single row has mask 1).  Four (first_step, overwrite) combinations against the fp64 restatement."""
    L, W = eng._abi.lib(), C + p + 1
    gen = torch.Generator().manual_seed(1000 * R + 10 * C + p)
    mask = (torch.rand(R, generator=gen) < 0.7).float()
    if R > 2:
        mask[R // 2] = 0.5
    mask[0], mask[R - 1] = 0.0, 1.0
    stats = _stats(C + 1, gen)
    g_pred, g_nin, g_pos = torch.randn(R, C, generator=gen), torch.randn(R, C + 1, generator=gen), torch.randn(R, p, generator=gen)
    prev = torch.randn(R, W, generator=gen)
    std = np.maximum(np.sqrt(stats[1].numpy() - stats[0].numpy() ** 2), float(stats[2]))
    t = g_nin.double().numpy() / std
    M = mask.numpy()[:, None]
    d = lambda x: x.cuda()
    dgp, dgn, dgq, dm, dst = d(g_pred), d(g_nin), d(g_pos), d(mask), [d(x) for x in stats]
    nan_pred = torch.full((R, C), float("nan"), device="cuda")         # first_step = 0: g_pred is never read

    def run(first, over):
        out = torch.full((R + 1, W), 7.0, device="cuda")               # one guard row behind grad_in
        out[:R] = float("nan") if over else d(prev)
        eng._abi.check(L.bsms_sim_input_grad(_ptr(dgp if first else nan_pred), _ptr(dgn), _ptr(dgq), _ptr(dm), R, C, p, *map(_ptr, dst),
                                             first, over, _ptr(out), _stream()), "bsms_sim_input_grad")
        torch.cuda.synchronize()
        assert bool((out[R] == 7.0).all())                             # nothing behind row R - 1
        return out[:R].cpu()

    for first in (1, 0):
        for over in (1, 0):
            got = run(first, over)
            state = g_pred.double().numpy() + t[:, :C] if first else np.where(M == 0, t[:, :C], 0.0)
            want = np.concatenate([state, g_pos.double().numpy(), t[:, C:]], axis=1) + (0.0 if over else prev.double().numpy())
            assert bool(torch.isfinite(got).all()), (first, over)      # stale NaNs never reach the result
            for name, sl in (("state", slice(0, C)), ("position", slice(C, C + p)), ("type", slice(W - 1, W))):
                err, scale = np.abs(got.double().numpy()[:, sl] - want[:, sl]).max(), np.abs(want[:, sl]).max()
                assert err <= 1e-6 * scale, (first, over, name, err, scale)
            if not first:                                              # rows that went into the carry: exactly 0 is added
                rows = mask != 0
                keep = torch.zeros(int(rows.sum()), C) if over else prev[rows][:, :C]
                assert bit_equal(got[rows][:, :C], keep), (over,)
            assert bit_equal(run(first, over), got), (first, over)     # two launches


# ------------------------------------------------------------------------------------------------ 2: bsms_bsgmp_bwd_pos_ev
def test_bsgmp_bwd_pos_ev_equals_its_parts(eng, graphs):
    """del300 at D = 32, depth 3, B = 2, through the raw entries on one set of buffers: the forward runs again in front of every
    backward, every output starts as NaN.  Bit-equality between entries of one library needs no oracle: random weights and data."""
    from bsms_gnn_amd.ops import _param_ptrs
    D, H, B, depth, p = 32, 3, 2, 3, 2
    es, ids = graphs.levels("del300")
    base = torch.tensor(graphs.np("del300/pos")[:, :p], dtype=torch.float32)
    torch.manual_seed(3)
    net = eng.BSGMP(depth, D, H, p).cuda()
    n = base.shape[0]
    h, pos, cot = torch.randn(B, n, D), base + 0.05 * torch.randn(B, n, p), torch.randn(B, n, D)
    L, s = eng._abi.lib(), _stream()
    plans, ews, bottom = net.prepare([i.cuda() for i in ids[:depth]], [e.cuda() for e in es[:depth + 1]], n, torch.device("cuda"))
    plans = [*plans, bottom]
    pl, keep_pl = eng._abi.ptr_array([q.handle.value if hasattr(q.handle, "value") else q.handle for q in plans])
    ewp, keep_ew = eng._abi.ptr_array([e.data_ptr() for e in ews])
    params = net.block_params()
    pp, keep_pp = _param_ptrs(params)
    hd, pd, gd = h.cuda(), pos.cuda().contiguous(), cot.cuda()
    u8 = lambda nbytes: torch.empty(max(int(nbytes), 1), dtype=torch.uint8, device="cuda")
    saved, work = u8(L.bsms_bsgmp_saved_bytes_p(pl, depth, B, D, p, H, 0)), u8(L.bsms_bsgmp_work_bytes(pl, depth, B, D, p, H))
    pwork, out = u8(L.bsms_bsgmp_pos_work_bytes(pl, depth, B, p)), torch.empty_like(hd)
    common = lambda: (pl, ewp, depth, hd.data_ptr(), pd.data_ptr(), gd.data_ptr(), B, D, p, n * p, H, pp, saved.data_ptr(), work.data_ptr())

    def run(entry, tail, pos_grad=True, join=False):
        eng._abi.check(L.bsms_bsgmp_fwd_p(pl, ewp, depth, hd.data_ptr(), pd.data_ptr(), B, D, p, n * p, H, pp, out.data_ptr(), saved.data_ptr(),
                                          work.data_ptr(), 0, 0, s), "bsms_bsgmp_fwd")
        nan = lambda ref_t: torch.full_like(ref_t, float("nan"))
        gh, gpos, grads = nan(hd), nan(pd), [nan(q) for q in params]
        gp, keep = eng._abi.ptr_array([g.data_ptr() for g in grads])
        eng._abi.check(getattr(L, entry)(*common(), gh.data_ptr(), gp, 0, *tail(gpos), s), entry)
        if join:
            eng._abi.check(L.bsms_side_lanes_join(s), "bsms_side_lanes_join")
        torch.cuda.synchronize()
        assert bool(torch.isfinite(gh).all()) and all(bool(torch.isfinite(g).all()) for g in grads)
        return gh, (gpos if pos_grad else None), grads

    same = lambda a, b: bit_equal(a[0], b[0]) and all(bit_equal(u, v) for u, v in zip(a[2], b[2])) and \
        ((a[1] is None and b[1] is None) or bit_equal(a[1], b[1]))
    want_pos = run("bsms_bsgmp_bwd_pos", lambda gpos: (gpos.data_ptr(), pwork.data_ptr()))
    got_pos = run("bsms_bsgmp_bwd_pos_ev", lambda gpos: (0, None, gpos.data_ptr(), pwork.data_ptr()))
    assert bool(torch.isfinite(want_pos[1]).all()) and float(want_pos[1].abs().max()) > 0
    assert same(got_pos, want_pos)                                     # flags = 0, no events: bsms_bsgmp_bwd_pos
    want_ev = run("bsms_bsgmp_bwd_ev", lambda gpos: (0, None), pos_grad=False)
    got_ev = run("bsms_bsgmp_bwd_pos_ev", lambda gpos: (0, None, None, None), pos_grad=False)
    assert same(got_ev, want_ev)                                       # grad_pos = NULL: bsms_bsgmp_bwd_ev
    deferred = run("bsms_bsgmp_bwd_pos_ev", lambda gpos: (1, None, gpos.data_ptr(), pwork.data_ptr()), join=True)
    assert same(deferred, got_pos)                                     # BSMS_BWD_DEFER_JOIN + bsms_side_lanes_join


# ------------------------------------------------------------------------------------------------ the fused step with the flag
def make_step(eng, ref, weights=(1.0,), detach=False, precision=None, input_grad=True, objective=None, use_graph=False, mine=None, grads=None):
    if mine is None:
        mine = eng.BSMS_Simulator(ref.cfg)
        mine.load_state_dict(ref.state_dict())
        mine = mine.cuda()
        if precision:
            mine.process.precision = precision
    grads = eng.GradBuckets(list(mine.parameters())) if grads is None else grads
    step = eng.FusedStep(mine, grads, unroll=len(weights), step_weights=list(weights), detach=detach, objective=objective,
                         input_grad=input_grad, use_graph=use_graph)
    return mine, grads, step


def run_step(step, data, later, consistent=True):
    loss = step(data, consistent, later)
    torch.cuda.synchronize()
    return loss


# ------------------------------------------------------------------------------------------------ 3: nothing else moves
@pytest.mark.parametrize("objective", ["default", "normalized_mse"])
@pytest.mark.parametrize("K", [1, 3])
@pytest.mark.parametrize("shape", ["ring", "split"])
def test_nothing_else_moves(eng, graphs, shape, K, objective):
    ref, data = make_oracle(shape, graphs)
    obj = None if objective == "default" else eng.Objective("normalized", "mse", [1.0, 4.0])
    gdata, w = _cuda(data), [1.0 / K] * K
    later = None if K == 1 else later_targets(gdata[0], gdata[1], K)
    mine, grads, off = make_step(eng, ref, w, input_grad=False, objective=obj)
    l0 = run_step(off, gdata, later)
    flat0, preds0 = grads.flat.clone(), [q.clone() for q in off.predictions()]
    grads.flat.fill_(float("nan"))
    _, _, on = make_step(eng, ref, w, input_grad=True, objective=obj, mine=mine, grads=grads)
    l1 = run_step(on, gdata, later)
    assert bit_equal(l0, l1) and bit_equal(grads.flat, flat0) and bool(torch.isfinite(flat0).all())
    assert all(bit_equal(a, b) for a, b in zip(on.predictions(), preds0)) and bit_equal(on.step_losses(), off.step_losses())
    g1 = on.input_grad().clone()
    assert g1.shape == gdata[0].shape and bool(torch.isfinite(g1).all())
    on.input_grad().fill_(float("nan"))                                # whatever the static buffer held is overwritten
    l2 = run_step(on, gdata, later)
    assert bit_equal(l2, l1) and bit_equal(on.input_grad(), g1) and bit_equal(grads.flat, flat0)
    for name, sl in GROUPS.items():
        assert float(g1[..., sl].abs().max()) > 0, name


# ------------------------------------------------------------------------------------------------ 4: one step == the autograd route
@pytest.mark.parametrize("shape,precision", [("ring", None), ("split", None), ("split", "bf16")])
def test_single_step_equals_the_autograd_route(eng, graphs, shape, precision):
    ref, data = make_oracle(shape, graphs)
    gdata = _cuda(data)
    mine, grads, step = make_step(eng, ref, precision=precision)
    loss = run_step(step, gdata, None)
    got = step.input_grad().clone()
    auto = eng.BSMS_Simulator(ref.cfg)
    auto.load_state_dict(ref.state_dict())
    auto = auto.cuda()
    if precision:
        auto.process.precision = precision
    ni = gdata[0].clone().requires_grad_(True)
    want_loss = eng.masked_rmse(auto((ni, *gdata[1:]), True, False), gdata[1], gdata[2])
    want_loss.backward()
    torch.cuda.synchronize()
    want = ni.grad.detach()
    assert abs(float(loss) - float(want_loss.detach())) <= 1e-6 * abs(float(want_loss.detach()))
    for name, sl in GROUPS.items():
        e = rel_err(got[..., sl].cpu(), want[..., sl].cpu())
        print(f"[{shape} {precision or 'f32'}] {name}: fused step vs autograd route {e:.2e}, bit-equal: {bit_equal(got[..., sl], want[..., sl])}")
        assert float(want[..., sl].abs().max()) > 0 and e <= 1e-6, (shape, precision, name, e)


# ------------------------------------------------------------------------------------------------ 5: K steps against the oracle
def unrolled_oracle_input_grad(sim, data, later, weights, detach, consistent=True):
    """test_hip_unroll.unrolled_oracle with `node_in` a leaf: the definition of the input gradient.  Returns (loss, node_in.grad)."""
    node_in, tar, mask, m_gs, m_ids = data
    node_in = node_in.detach().clone().requires_grad_(True)
    C = tar.shape[-1]
    tars = [tar, *(later if later is not None else [])]
    sim.zero_grad(set_to_none=True)
    cur, loss = node_in, 0.0
    for k, w in enumerate(weights):
        pred = sim((cur, tars[k], mask, m_gs, m_ids), consistent, False)
        loss = loss + w * ro.masked_rmse(pred, tars[k], mask)
        cur = torch.where(mask == 0, node_in, torch.cat([pred.detach() if detach else pred, node_in[..., C:]], dim=-1))
    loss.backward()
    return float(loss.detach()), node_in.grad.detach().clone()


_ORACLE = {}


def oracle_input_grads(ref, data, later, weights, detach, key, consistent=True, fp64=True):
    """fp32 on all threads, fp32 on one thread, fp64 (the yardstick): once per configuration."""
    if key not in _ORACLE:
        with KinkMargin(ref) as km:
            loss32, g32 = unrolled_oracle_input_grad(ref, data, later, weights, detach, consistent)
        print(f"[{key}] smallest |ReLU input| of the oracle over the {len(weights)} steps: {km.min:.2e}")
        assert km.min >= MIN_MARGIN, (key, "the weight seed no longer keeps the ReLU inputs away from 0", km.min)
        r = dict(loss32=loss32, g32=g32)
        if fp64:
            n = torch.get_num_threads()
            torch.set_num_threads(1)
            try:
                _, r["g32_one"] = unrolled_oracle_input_grad(ref, data, later, weights, detach, consistent)
            finally:
                torch.set_num_threads(n)
            ref64 = ro.BSMS_Simulator(ref.cfg, dtype=torch.float64)
            ref64.load_state_dict(ref.state_dict())
            ref64.double()
            _, r["g64"] = unrolled_oracle_input_grad(ref64, _f64(data), None if later is None else later.double(), weights, detach, consistent)
        _ORACLE[key] = r
    return _ORACLE[key]


def _dist(a, b):
    a, b = a.double(), b.double()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-300)), float((a - b).norm() / b.norm().clamp_min(1e-300))


def three_way(key, got, r, mask):
    """The criterion of test_hip_pos_grad._three_way per column group, and on the state columns of the rows with mask == 0, where
    the oracle's gradient is 1e-3 .. 1e-4 of the group's maximum: an accumulation over k that went missing would hide inside the
    whole-group max-norm."""
    free = (mask.reshape(-1) == 0)
    assert 0 < int(free.sum()) < free.numel()
    flat = lambda t: t.reshape(-1, t.shape[-1])
    views = {name: (lambda t, sl=sl: flat(t)[:, sl]) for name, sl in GROUPS.items()}
    views["state, rows with mask == 0"] = lambda t: flat(t)[free][:, GROUPS["state"]]
    for name, v in views.items():
        g64 = v(r["g64"])
        assert float(g64.abs().max()) > 0, (key, name)                 # the group really receives a gradient
        (e_gpu, l_gpu), (e_n, l_n), (e_1, l_1) = _dist(v(got), g64), _dist(v(r["g32"]), g64), _dist(v(r["g32_one"]), g64)
        limit, limit2 = max(1e-5, 3.0 * max(e_n, e_1)), max(1e-5, 3.0 * max(l_n, l_1))
        print(f"[{key}] node_in.grad {name}: max-norm engine {e_gpu:.2e} | cpu32 all threads {e_n:.2e} one thread {e_1:.2e} (limit {limit:.2e}); "
              f"relative L2 engine {l_gpu:.2e} | cpu32 {l_n:.2e} / {l_1:.2e} (limit {limit2:.2e})")
        assert e_gpu <= limit and l_gpu <= limit2, (key, name, e_gpu, e_n, e_1, l_gpu, l_n, l_1)


def engine_input_grad(eng, ref, data, later, weights, detach, consistent=True, gpu_data=None):
    mine, grads, step = make_step(eng, ref, weights, detach)
    loss = run_step(step, _cuda(data) if gpu_data is None else gpu_data, None if later is None else later.cuda(), consistent)
    return float(loss), step.input_grad().clone().cpu()


def carried_distance(full, cut, mask):
    """Relative L2 distance between the BPTT and the detached input gradients on the state columns of the rows with mask != 0."""
    rows = (mask.reshape(-1) != 0)
    f = lambda t: t.reshape(-1, t.shape[-1])[rows][:, GROUPS["state"]].double()
    return float((f(full) - f(cut)).norm() / f(full).norm())


def test_three_steps_input_grad_matches_the_oracle(eng, graphs):
    """("ring", K = 3, equal weights), back-propagation through time and detached; and a carry that is silently dropped cannot pass."""
    ref, data = make_oracle("ring", graphs)
    later, w = later_targets(data[0], data[1], 3), [1 / 3] * 3
    res = {}
    for detach in (False, True):
        key = ("ring", 3, "detached" if detach else "bptt")
        r = oracle_input_grads(ref, data, later, w, detach, key)
        loss, got = engine_input_grad(eng, ref, data, later, w, detach)
        assert abs(loss - r["loss32"]) <= 1e-5 * abs(r["loss32"])
        three_way(key, got, r, data[2])
        res[detach] = (got, r["g32"])
    d_gpu, d_cpu = carried_distance(res[False][0], res[True][0], data[2]), carried_distance(res[False][1], res[True][1], data[2])
    print(f"[ring] BPTT vs detached input gradient, state columns, rows with mask != 0: engine {d_gpu:.3f}, oracle {d_cpu:.3f}")
    assert d_gpu >= 0.1 and d_cpu >= 0.1, (d_gpu, d_cpu)


def test_four_steps_input_grad_with_uneven_weights_at_d64(eng, graphs):
    ref, data = make_oracle("d64", graphs)
    later, w = later_targets(data[0], data[1], 4), [0.4, 0.3, 0.2, 0.1]
    r = oracle_input_grads(ref, data, later, w, False, ("d64", 4, "bptt"))
    loss, got = engine_input_grad(eng, ref, data, later, w, False)
    assert abs(loss - r["loss32"]) <= 1e-5 * abs(r["loss32"])
    three_way(("d64", 4, "bptt"), got, r, data[2])
    cut32 = oracle_input_grads(ref, data, later, w, True, ("d64", 4, "detached"), fp64=False)["g32"]       # for the carry guard only
    _, cut = engine_input_grad(eng, ref, data, later, w, True)
    d_gpu, d_cpu = carried_distance(got, cut, data[2]), carried_distance(r["g32"], cut32, data[2])
    print(f"[d64] BPTT vs detached input gradient, state columns, rows with mask != 0: engine {d_gpu:.3f}, oracle {d_cpu:.3f}")
    assert d_gpu >= 0.1 and d_cpu >= 0.1, (d_gpu, d_cpu)


def test_two_steps_input_grad_on_a_block_diagonal_batch(eng, graphs):
    """consistent=False at K = 2 on the golden block-diagonal batch (del64 + del300 in one graph, 364 rows, depth 2), built as
    test_hip_unroll.test_two_steps_on_a_block_diagonal_batch builds it."""
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
    torch.manual_seed(26)
    ref = ro.BSMS_Simulator(ro.make_cfg(2, 32, 2, 2, 2))
    ref(data, False, True)
    sizes = [n, ids[0].numel(), ids[1].numel()]
    levels = [eng.LevelData(es[l], sizes[l], face=ids[l] if l < 2 else None, x=x if l == 0 else None, y=y if l == 0 else None,
                            mask=mask if l == 0 else None).to("cuda") for l in range(3)]
    later = later_targets(data[0], data[1], 2)
    key = ("blockdiag", 2, "bptt")
    r = oracle_input_grads(ref, data, later, [0.5, 0.5], False, key, consistent=False)
    loss, got = engine_input_grad(eng, ref, data, later, [0.5, 0.5], False, consistent=False, gpu_data=levels)
    assert got.shape == (1, n, 5) and abs(loss - r["loss32"]) <= 1e-5 * abs(r["loss32"])
    three_way(key, got, r, mask)


# ------------------------------------------------------------------------------------------------ 6: graph replay
def test_graph_replay_equals_eager(eng, graphs):
    ref, data = make_oracle("ring", graphs)
    gdata = _cuda(data)
    mine, grads, eager = make_step(eng, ref)
    _, _, graph = make_step(eng, ref, use_graph=True, mine=mine, grads=grads)
    gen = torch.Generator().manual_seed(11)
    for it in range(3):
        ni = gdata[0].clone()
        ni[..., :C_] += 0.05 * it * torch.randn(ni[..., :C_].shape, generator=gen).cuda()
        batch = (ni, *gdata[1:])
        l0 = run_step(eager, batch, None)
        flat0, g0 = grads.flat.clone(), eager.input_grad().clone()
        grads.flat.fill_(float("nan"))
        l1 = run_step(graph, batch, None)
        assert bit_equal(l0, l1) and bit_equal(grads.flat, flat0) and bit_equal(graph.input_grad(), g0), it
        if it:
            assert not bit_equal(g0, prev)                             # the input really changed
        prev = g0


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
    engine = eng.DataParallel(sim, bucket_bytes=64 << 10, unroll=2, input_grad=True)
    loss = engine.step_loss_backward(data, True, later_targets(data[0], data[1], 2))
    torch.cuda.synchronize()
    torch.save({"loss": loss.detach().cpu(), "flat": engine.grads.flat.cpu(), "input_grad": engine.fused.input_grad().cpu()}, f"{out_path}.{rank}")
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.timeout(300)
def test_two_ranks_hold_their_own_samples_input_gradient(eng, graphs, tmp_path):
    """Two ranks over gloo on one GPU, one golden sample each, K = 2: each rank's input gradient is that of its sample in the
    single-process step on the whole batch -- the loss coefficient inside g_pred is the global one, nothing else crosses samples."""
    port = 29700 + os.getpid() % 2000
    out = str(tmp_path / "res")
    mp.start_processes(_worker, args=(2, port, out), nprocs=2, join=True, start_method="spawn")
    r = [torch.load(out + ".0"), torch.load(out + ".1")]
    assert bit_equal(r[0]["flat"], r[1]["flat"]) and bit_equal(r[0]["loss"], r[1]["loss"])
    ref, data = make_oracle("ring", graphs, golden=True)
    mine, grads, step = make_step(eng, ref, [0.5, 0.5])
    loss = run_step(step, _cuda(data), later_targets(data[0], data[1], 2).cuda())
    want = step.input_grad().cpu()
    assert abs(float(r[0]["loss"]) - float(loss)) < 1e-5 * abs(float(loss))
    for rank in (0, 1):
        assert r[rank]["input_grad"].shape == (1, 300, 5)
        for name, sl in GROUPS.items():
            e = rel_err(r[rank]["input_grad"][0][:, sl], want[rank][:, sl])
            print(f"rank {rank} {name}: {e:.2e} from the single-process step")
            assert e < 2e-5, (rank, name, e)


# ------------------------------------------------------------------------------------------------ 8: input_gradient()
def test_input_gradient_function(eng, graphs):
    ref, data = make_oracle("ring", graphs)
    gdata = _cuda(data)
    later = later_targets(gdata[0], gdata[1], 3)
    mine, grads, step = make_step(eng, ref, [1 / 3] * 3)
    l0 = run_step(step, gdata, later)
    want = step.input_grad().clone()
    model = eng.BSMS_Simulator(ref.cfg)
    model.load_state_dict(ref.state_dict())
    model = model.cuda()
    before = [q.detach().clone() for q in model.parameters()]
    loss, got = eng.input_gradient(model, gdata, later_targets=later)
    torch.cuda.synchronize()
    assert bit_equal(loss, l0) and bit_equal(got, want)
    assert all(bit_equal(a, b) for a, b in zip(model.parameters(), before))            # the parameters are left alone
    steps = dict(model._bsms_input_grad_steps)
    loss2, got2 = eng.input_gradient(model, gdata, later_targets=2.0 * later)           # other targets, the same K: the cached step
    torch.cuda.synchronize()
    assert dict(model._bsms_input_grad_steps) == steps and len([k for k in steps if k != "grads"]) == 1
    assert bit_equal(got, want) and not bit_equal(got2, want)                           # a clone: the second call did not touch the first result
    l1, g1 = eng.input_gradient(model, gdata)                                           # K = 1 from the absence of later targets
    assert len([k for k in model._bsms_input_grad_steps if k != "grads"]) == 2 and g1.shape == gdata[0].shape
    assert all(bit_equal(a, b) for a, b in zip(model.parameters(), before))
