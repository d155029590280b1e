"""GPU: the pack group (bsms_pack_group_*) -- one launch writes the weight packs of every MLP / GMP block of a
training step, and the forwards run with their `reuse` flags.

Every comparison is BYTE EQUALITY against the per-call prepack of the same build: the training forward with its own packs into one
`saved` buffer, the group launch + `reuse` into another, and the ENTIRE buffers compared -- packs, scale and bias headers, cleared
bound slots and every activation.  A `saved` buffer has bytes that no kernel writes (alignment gaps, rows of padding), so each pair
is run twice, pre-filled with two different sentinels: a byte the group path fails to write, or writes where the per-call path
does not, shows with at least one of them.

Shapes: a two-level U-Net on a 60-node Delaunay mesh, B = 2, hidden 3.  The group kernel gives a pack to ONE workgroup up to
128 x 128 and to 2 or 4 beyond (chain.hip: launch_prepack_group), its scan keeps 16 rows per thread in flight and its pack loop 6
dwords: D = 32 (one chunk, scale slot and bias in the same header, scan tail only), 96 (not a power of two: 3 chunks, 170 threads
of columns), 128 (the flagship: one workgroup per pack, one full scan round), 160 / 192 (two / three workgroups), 256 (four, the widest);
p = 2 and 3 (PACK_TRANSPOSE with 3 and 4 columns, ld = 2 D + p + 1 odd and even)."""
import ctypes as C

import numpy as np
import pytest
import torch

from test_hip_input_grad import bit_equal, make_step, run_step
from test_hip_unroll import _cuda, later_targets, make_oracle

pytestmark = pytest.mark.gpu
OK, E_INVALID_ARG, E_UNSUPPORTED = 0, -1, -3
B, H, NODES, DEPTH = 2, 3, 60, 2
SENTINELS = (0x55, 0xA7)


@pytest.fixture(scope="module")
def eng():
    import bsms_gnn_amd as eng
    return eng


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _filled(nbytes, byte):
    return torch.full((max(int(nbytes), 1),), byte, dtype=torch.uint8, device="cuda")


class Group:
    def __init__(self, eng):
        self.L, self.check = eng._abi.lib(), eng._abi.check
        self.h = C.c_void_p()
        self.check(self.L.bsms_pack_group_create(C.cast(C.byref(self.h), C.POINTER(C.c_void_p))), "bsms_pack_group_create")

    def launch(self):
        self.check(self.L.bsms_pack_group_launch(self.h, _stream()), "bsms_pack_group_launch")

    def close(self):
        torch.cuda.synchronize()
        self.L.bsms_pack_group_destroy(self.h)


_MESH = {}


def mesh(eng):
    """The 60-node hierarchy, built once: (points, m_gs, m_ids) on the device."""
    if not _MESH:
        from scipy.spatial import Delaunay
        pts = np.random.default_rng(7).random((NODES, 2))
        flat = eng.to_flat_edge(Delaunay(pts).simplices.astype(np.int64), "tri")
        m_gs, _, m_ids = eng.BistrideMultiLayerGraph(flat, DEPTH, NODES, pts).get_multi_layer_graphs()
        _MESH["m"] = (torch.tensor(pts, dtype=torch.float32), [torch.as_tensor(np.asarray(g), dtype=torch.int64).cuda() for g in m_gs],
                      [torch.as_tensor(np.asarray(i), dtype=torch.int64).cuda() for i in m_ids])
    return _MESH["m"]


class UNetCase:
    """bsms_bsgmp_fwd_p in training, per-call packs against group + reuse."""

    def __init__(self, eng, D, p, prec="f32", seed=0):
        from bsms_gnn_amd.ops import PRECISIONS, _param_ptrs
        self.eng, self.L, self.D, self.p, self.prec = eng, eng._abi.lib(), D, p, PRECISIONS[prec]
        pts, m_gs, m_ids = mesh(eng)
        torch.manual_seed(seed)
        self.net = eng.BSGMP(DEPTH, D, H, p).cuda()
        plans, self.ews, bottom = self.net.prepare(m_ids, m_gs, NODES, torch.device("cuda"))
        self.plans = [*plans, bottom]
        self.pl, self._k1 = eng._abi.ptr_array([q.handle.value if hasattr(q.handle, "value") else q.handle for q in self.plans])
        self.ewp, self._k2 = eng._abi.ptr_array([e.data_ptr() for e in self.ews])
        self.params = self.net.block_params()
        self.pp, self._k3 = _param_ptrs(self.params)
        pos = torch.cat([pts, torch.rand(NODES, p - 2)], dim=1) if p > 2 else pts
        self.h = torch.randn(B, NODES, D).cuda()
        self.pos = (pos.unsqueeze(0) + 0.01 * torch.randn(B, NODES, p)).cuda().contiguous()
        self.saved_bytes = self.L.bsms_bsgmp_saved_bytes_p(self.pl, DEPTH, B, D, p, H, self.prec)
        self.work = _filled(self.L.bsms_bsgmp_work_bytes(self.pl, DEPTH, B, D, p, H), 0)

    def forward(self, byte, grouped):
        saved, out = _filled(self.saved_bytes, byte), torch.full_like(self.h, float("nan"))
        g = None
        if grouped:
            g = Group(self.eng)
            self.eng._abi.check(self.L.bsms_pack_group_add_bsgmp(g.h, self.pl, DEPTH, B, self.D, self.p, H, self.pp, saved.data_ptr(), None,
                                                                 self.prec), "bsms_pack_group_add_bsgmp")
            g.launch()
        self.eng._abi.check(self.L.bsms_bsgmp_fwd_p(self.pl, self.ewp, DEPTH, self.h.data_ptr(), self.pos.data_ptr(), B, self.D, self.p,
                                                    NODES * self.p, H, self.pp, out.data_ptr(), saved.data_ptr(), self.work.data_ptr(),
                                                    1 if grouped else 0, self.prec, _stream()), "bsms_bsgmp_fwd_p")
        if g:
            g.close()
        torch.cuda.synchronize()
        return saved, out


def check_pairs(case, tag):
    for byte in SENTINELS:
        want_saved, want_out = case.forward(byte, grouped=False)
        got_saved, got_out = case.forward(byte, grouped=True)
        assert bool(torch.equal(got_saved, want_saved)), (tag, hex(byte), "saved", int((got_saved != want_saved).sum()))
        assert bit_equal(got_out, want_out), (tag, hex(byte), "out")
    return want_out


@pytest.mark.parametrize("p", [2, 3])
@pytest.mark.parametrize("D", [32, 96, 128, 160, 192, 256])
def test_unet_saved_buffers_are_bytewise_equal(eng, D, p):
    out = check_pairs(UNetCase(eng, D, p, seed=D + p), (D, p))
    assert bool(torch.isfinite(out).all()) and float(out.abs().max()) > 0


@pytest.mark.parametrize("prec", ["bf16", "bf16_nodes"])
def test_unet_bf16_precisions(eng, prec):
    """D = 128: one-plane packs with the bias in the header of chunk 0, the PACK_ROWS_BF16 images of the fused edge backward,
    BSMS_BF16_NODES with the first node Linear's bias in its FIRST pack."""
    out = check_pairs(UNetCase(eng, 128, 3, prec=prec, seed=5), prec)
    assert bool(torch.isfinite(out).all())


@pytest.mark.parametrize("D", [32, 128])
def test_zero_matrix_and_huge_entry(eng, D):
    """The exponent clamp of the matrix scale: a zero matrix (Ew < 13), a zero half of a mated pair, and one entry at 2^100."""
    c = UNetCase(eng, D, 2, seed=11)
    nl = 2 * (H + 1)
    with torch.no_grad():
        c.params[nl + 2].zero_()                       # block 0, edge Linear 1: a whole matrix of zeros
        c.params[0][:, :D].zero_()                     # block 0, first node Linear: the x half of the mated pair
        c.params[4 * (H + 1) + 2].zero_()              # block 1, node Linear 1
        c.params[4 * (H + 1) + nl][3, D // 2] = 2.0 ** 100     # block 1, first edge Linear: projections and fiber weights share it
        c.params[2 * 4 * (H + 1) + 4][D - 1, 0] = -2.0 ** 100  # block 2, node Linear 2
    check_pairs(c, ("clamp", D))


class MlpCase:
    def __init__(self, eng, D, in_dim, out_dim, ln, rows=150, seed=0):
        from bsms_gnn_amd.ops import _param_ptrs
        self.eng, self.L, self.shape = eng, eng._abi.lib(), (rows, in_dim, D, out_dim, H, ln)
        torch.manual_seed(seed)
        self.net = eng.MLP(in_dim, D, out_dim, H, bool(ln)).cuda()
        self.pp, self._k = _param_ptrs(self.net.flat_params())
        self.x = torch.randn(rows, in_dim).cuda()
        self.saved_bytes = self.L.bsms_mlp_saved_bytes(rows, in_dim, D, out_dim, H)
        self.work = _filled(self.L.bsms_mlp_work_bytes(rows, in_dim, D, out_dim, H), 0)
        self.out_dim = out_dim

    def forward(self, byte, grouped):
        R, i, D, o, h, ln = self.shape
        saved, y = _filled(self.saved_bytes, byte), torch.full((R, o), float("nan"), device="cuda")
        g = None
        if grouped:
            g = Group(self.eng)
            self.eng._abi.check(self.L.bsms_pack_group_add_mlp(g.h, R, i, D, o, h, ln, self.pp, saved.data_ptr(), None), "bsms_pack_group_add_mlp")
            g.launch()
        self.eng._abi.check(self.L.bsms_mlp_fwd_ex(self.x.data_ptr(), R, i, D, o, h, ln, self.pp, y.data_ptr(), saved.data_ptr(),
                                                   self.work.data_ptr(), 1 if grouped else 0, _stream()), "bsms_mlp_fwd_ex")
        if g:
            g.close()
        torch.cuda.synchronize()
        return saved, y


@pytest.mark.parametrize("kind", ["encoder", "decoder"])
@pytest.mark.parametrize("D", [32, 96, 128, 256])
def test_mlp_saved_buffers_are_bytewise_equal(eng, D, kind):
    """The encoder shape (in = C + 1 = 3, LayerNorm: a PACK_TRANSPOSE of the narrow first Linear) and the decoder shape (out = 3)."""
    c = MlpCase(eng, D, 3, D, 1, seed=D) if kind == "encoder" else MlpCase(eng, D, D, 3, 0, seed=D + 1)
    y = check_pairs(c, (kind, D))
    assert bool(torch.isfinite(y).all()) and float(y.abs().max()) > 0


def test_one_group_of_many_members_and_the_inference_layout(eng):
    """Encoder + U-Net + decoder in ONE group, as the fused step builds it (mates and bound arrays re-based across members); and the
    inference layout: packs in `work`, read by a forward-only call with `reuse` bit 0."""
    L, ck = eng._abi.lib(), eng._abi.check
    enc, dec, net = MlpCase(eng, 128, 3, 128, 1, rows=B * NODES, seed=1), MlpCase(eng, 128, 128, 3, 0, rows=B * NODES, seed=2), UNetCase(eng, 128, 2, seed=3)
    want = [c.forward(0x55, grouped=False) for c in (enc, net, dec)]
    saved = [_filled(c.saved_bytes, 0x55) for c in (enc, net, dec)]
    g = Group(eng)
    R = B * NODES
    ck(L.bsms_pack_group_add_mlp(g.h, R, 3, 128, 128, H, 1, enc.pp, saved[0].data_ptr(), None), "add enc")
    ck(L.bsms_pack_group_add_bsgmp(g.h, net.pl, DEPTH, B, 128, 2, H, net.pp, saved[1].data_ptr(), None, 0), "add unet")
    ck(L.bsms_pack_group_add_mlp(g.h, R, 128, 128, 3, H, 0, dec.pp, saved[2].data_ptr(), None), "add dec")
    g.launch()
    # sealed: the refusal comes from the host, and the tables on the device are untouched by it
    assert L.bsms_pack_group_add_mlp(g.h, R, 3, 128, 128, H, 1, enc.pp, saved[0].data_ptr(), None) == E_INVALID_ARG
    assert b"sealed" in L.bsms_last_error()
    assert L.bsms_pack_group_add_bsgmp(g.h, net.pl, DEPTH, B, 128, 2, H, net.pp, saved[1].data_ptr(), None, 0) == E_INVALID_ARG
    g.launch()                                                         # a second launch of the sealed group: the same bytes again
    y, out, pred = torch.empty(R, 128, device="cuda"), torch.empty_like(net.h), torch.empty(R, 3, device="cuda")
    ck(L.bsms_mlp_fwd_ex(enc.x.data_ptr(), R, 3, 128, 128, H, 1, enc.pp, y.data_ptr(), saved[0].data_ptr(), enc.work.data_ptr(), 1, _stream()), "enc")
    ck(L.bsms_bsgmp_fwd_p(net.pl, net.ewp, DEPTH, net.h.data_ptr(), net.pos.data_ptr(), B, 128, 2, NODES * 2, H, net.pp, out.data_ptr(),
                          saved[1].data_ptr(), net.work.data_ptr(), 1, 0, _stream()), "unet")
    ck(L.bsms_mlp_fwd_ex(dec.x.data_ptr(), R, 128, 128, 3, H, 0, dec.pp, pred.data_ptr(), saved[2].data_ptr(), dec.work.data_ptr(), 1, _stream()), "dec")
    g.close()
    for k, (got_saved, got_y) in enumerate(zip(saved, (y, out, pred))):
        assert bool(torch.equal(got_saved, want[k][0])) and bit_equal(got_y, want[k][1]), k
    # inference: a forward-only call fills the packs in `work`; a group fills a second buffer; with `reuse` the outputs agree
    a, b = torch.empty_like(net.h), torch.empty_like(net.h)
    args = lambda o, w, reuse: (net.pl, net.ewp, DEPTH, net.h.data_ptr(), net.pos.data_ptr(), B, 128, 2, NODES * 2, H, net.pp, o.data_ptr(), None,
                                w.data_ptr(), reuse, 0, _stream())
    ck(L.bsms_bsgmp_fwd_p(*args(a, net.work, 0)), "inference")
    w2 = _filled(net.work.numel(), 0xA7)
    g = Group(eng)
    ck(L.bsms_pack_group_add_bsgmp(g.h, net.pl, DEPTH, B, 128, 2, H, net.pp, None, w2.data_ptr(), 0), "add unet (inference)")
    g.launch()
    ck(L.bsms_bsgmp_fwd_p(*args(b, w2, 1)), "inference, reuse")
    g.close()
    assert bit_equal(a, b) and bit_equal(a, want[1][1])


def test_add_bsgmp_refusals_with_a_plan(eng):
    """The checks behind the plan table (tests/test_pack_group_host.py has those in front of it).  Nothing is added by a refused call."""
    L = eng._abi.lib()
    c = UNetCase(eng, 128, 2)
    g = Group(eng)
    call = lambda depth=DEPTH, width=128, p=2, hidden=H, params=c.pp, saved=0x1000, work=None, prec=0: \
        L.bsms_pack_group_add_bsgmp(g.h, c.pl, depth, B, width, p, hidden, params, saved, work, prec)
    for width in (16, 48, 288):
        assert call(width=width) == E_UNSUPPORTED, width
    assert call(p=0) == E_UNSUPPORTED and call(p=8) == E_UNSUPPORTED
    assert call(hidden=0) == E_UNSUPPORTED and call(hidden=8) == E_UNSUPPORTED
    assert call(prec=3) == E_UNSUPPORTED and call(prec=-1) == E_UNSUPPORTED
    assert call(width=96, prec=1) == E_UNSUPPORTED                     # the bf16 precisions: D = 128 / 256
    assert call(params=None) == E_INVALID_ARG and call(saved=None) == E_INVALID_ARG
    holes = [q.data_ptr() for q in c.params]
    holes[-3] = None                                                   # in the LAST block: the first 2L blocks must not have been added
    assert call(params=eng._abi.ptr_array(holes)[0]) == E_INVALID_ARG
    assert L.bsms_pack_group_launch(g.h, _stream()) == OK              # still empty: nothing to upload, not sealed
    assert call() == OK
    g.close()


def test_first_launch_is_refused_under_capture(eng):
    """The first launch uploads the tables with a blocking copy: refused on a capturing stream, fine once uploaded."""
    L = eng._abi.lib()
    c = MlpCase(eng, 32, 3, 32, 1)
    saved = _filled(c.saved_bytes, 0)
    g = Group(eng)
    eng._abi.check(L.bsms_pack_group_add_mlp(g.h, *c.shape, c.pp, saved.data_ptr(), None), "add")
    graph, rcs = torch.cuda.CUDAGraph(), []
    with torch.cuda.graph(graph, capture_error_mode="thread_local"):
        rcs.append(L.bsms_pack_group_launch(g.h, _stream()))
        msg = L.bsms_last_error()
    assert rcs == [E_INVALID_ARG] and b"capture" in msg
    g.launch()
    torch.cuda.synchronize()
    want = saved.clone()
    saved.fill_(0x33)
    graph2 = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph2, capture_error_mode="thread_local"):
        rcs.append(L.bsms_pack_group_launch(g.h, _stream()))
    assert rcs[-1] == OK
    graph2.replay()
    torch.cuda.synchronize()
    packs = want != 0                                                  # every byte the eager launch wrote as non-zero ...
    assert bool(torch.equal(saved[packs], want[packs])) and int(packs.sum()) > 1000
    del graph2
    g.close()


# ------------------------------------------------------------------------------------------------ FusedStep
def _state(step, grads):
    return [step.prediction().clone(), grads.flat.clone(), *(q.clone() for q in step.predictions())] if step.unroll > 1 else \
        [step.prediction().clone(), grads.flat.clone()]


def _per_call(eng, fn):
    """Run `fn` with the per-call prepacks inside the forwards (the 13 launches of the parent commit)."""
    eng.FusedStep.pack_group = False
    try:
        return fn()
    finally:
        eng.FusedStep.pack_group = True


STEP_CASES = {
    "plain": dict(shape="split"), "ring": dict(shape="ring"), "graph": dict(shape="split", use_graph=True), "frozen": dict(shape="split", frozen=True),
    "unroll2": dict(shape="split", K=2), "input_grad": dict(shape="ring", input_grad=True), "bf16": dict(shape="split", precision="bf16"),
}


def _run_case(eng, graphs, shape, K=1, use_graph=False, frozen=False, input_grad=False, precision=None, steps=3):
    ref, data = make_oracle(shape, graphs)
    gdata, w = _cuda(data), [1.0 / K] * K
    later = later_targets(gdata[0], gdata[1], K)
    mine = eng.BSMS_Simulator(ref.cfg)
    mine.load_state_dict(ref.state_dict())
    mine = mine.cuda()
    if precision:
        mine.process.precision = precision
    if frozen:
        mine.process.down_gmps[0].mlp_edge.requires_grad_(False)
    mine, grads, step = make_step(eng, ref, w, input_grad=input_grad, use_graph=use_graph, mine=mine)
    out = []
    for _ in range(steps):                                            # eager: per-call packs at step 0 (the group is built once the tables and
                                                                      # buffers repeat), the group at 1, the sealed group relaunched at 2
        grads.flat.fill_(float("nan"))
        loss = run_step(step, gdata, later)
        out.append([loss.clone(), *_state(step, grads), *([step.input_grad().clone()] if input_grad else [])])
    return out, step


@pytest.mark.parametrize("name", list(STEP_CASES))
def test_fused_step_equals_the_per_call_route(eng, graphs, name):
    """FusedStep with the pack group against FusedStep with per-call packs (FusedStep.pack_group = False: the launches of every other
    route): loss, prediction(s), every gradient and the input gradient, bit for bit, over two steps -- eager, under graph replay,
    with a frozen MLP, unrolled over two steps, with input_grad, in a bf16 precision."""
    want, _ = _per_call(eng, lambda: _run_case(eng, graphs, **STEP_CASES[name]))
    got, step = _run_case(eng, graphs, **STEP_CASES[name])
    assert step._pg is not None
    for k, (a, b) in enumerate(zip(got, want)):
        assert len(a) == len(b) and all(bit_equal(u, v) for u, v in zip(a, b)), (name, k)
        assert all(bool(torch.isfinite(u).all()) for u in a), (name, k)


def _autograd_step(eng, sim, data):
    sim.zero_grad(set_to_none=True)
    pred = sim(data, True, False)
    loss = eng.masked_rmse(pred, data[1], data[2])
    loss.backward()
    return loss.detach(), pred.detach(), {k: q.grad.clone() for k, q in sim.named_parameters() if q.grad is not None}


def test_fused_step_against_the_autograd_route(eng, graphs):
    """The module-tree / autograd route keeps its per-call packs.  Its U-Net and MLP kernels are the fused step's; the glue around them
    (normaliser, loss, the loss gradient) is re-associated, so the two routes agree to fp32 round-off and not bit for bit --
    tests/test_hip_training.py::test_fused_step_equals_autograd_step pins that at 1e-6 / 2e-6 and has done so since before the pack
    group.  What the pack group may change is pinned bit for bit above; here: the distance between the routes is what it was with
    per-call packs, to the last bit of every figure."""
    ref, data = make_oracle("ring", graphs)
    gdata = _cuda(data)
    sim = eng.BSMS_Simulator(ref.cfg)
    sim.load_state_dict(ref.state_dict())
    sim = sim.cuda()
    loss, pred, want = _autograd_step(eng, sim, gdata)
    sim.zero_grad(set_to_none=True)
    figures = []
    for grouped in (True, False):
        eng.FusedStep.pack_group = grouped
        try:
            grads = eng.GradBuckets(list(sim.parameters()))
            step = eng.FusedStep(sim, grads)
            step(gdata, True)                                          # (the group serves from the second step on)
            got = step(gdata, True)
            torch.cuda.synchronize()
            assert (step._pg is not None) == grouped
            figures.append([got.clone(), step.prediction().clone(), *(q.grad.clone() for k, q in sim.named_parameters() if k in want)])
        finally:
            eng.FusedStep.pack_group = True
    assert all(bit_equal(u, v) for u, v in zip(*figures))
    got = figures[0]
    assert abs(float(got[0]) - float(loss)) < 1e-6 * abs(float(loss))
    assert float((got[1].reshape(pred.shape) - pred).abs().max()) <= 1e-6 * float(pred.abs().max())
    for k, g in zip([k for k, _ in sim.named_parameters() if k in want], got[2:]):
        assert float((g - want[k]).norm()) <= 2e-6 * float(want[k].norm()), k


def _fresh_step(eng, sim):
    twin = eng.BSMS_Simulator(sim.cfg)
    twin.load_state_dict(sim.state_dict())
    twin = twin.cuda()
    grads = eng.GradBuckets(list(twin.parameters()))
    return twin, grads, eng.FusedStep(twin, grads)


def _grads_equal(a, b):
    """Every trainable parameter's gradient, bit for bit (the normalisers' statistics are parameters without a gradient)."""
    pairs = [(u, v) for u, v in zip(a.parameters(), b.parameters()) if u.requires_grad]
    return len(pairs) > 0 and all(v.requires_grad and u.grad is not None and v.grad is not None and bit_equal(u.grad, v.grad) for u, v in pairs)


def test_stale_pack_guard_and_pointer_change_guard(eng, graphs):
    """Every parameter changed IN PLACE between two steps: the second step packs the new values (equal to a fresh step on them).
    Then one parameter tensor re-allocated: the step rebuilds its group (another handle) and again equals a fresh step."""
    ref, data = make_oracle("split", graphs)
    gdata = _cuda(data)
    mine, grads, step = make_step(eng, ref, (1.0,), input_grad=False)
    run_step(step, gdata, None)                                        # per-call packs: the first step with these tables and buffers
    assert step._pg is None and step._pg_builds == 0
    run_step(step, gdata, None)
    first = grads.flat.clone()
    builds = step._pg_builds
    with torch.no_grad():
        for q in mine.parameters():
            q.mul_(1.0 + 0.05 * torch.rand_like(q))
    loss = run_step(step, gdata, None)
    assert step._pg_builds == builds == 1 and not bit_equal(grads.flat, first)      # same group, relaunched on the new values
    twin, tgrads, tstep = _fresh_step(eng, mine)
    tloss = run_step(tstep, gdata, None)
    assert bit_equal(loss, tloss) and bit_equal(step.prediction(), tstep.prediction())
    assert _grads_equal(mine, twin)
    # a re-allocated parameter tensor (an optimizer's flat buffer, .to(), load): new pointers in the tables and in the group
    q = mine.encode.flat_params()[0]
    old = q.data
    q.data = (old * 1.25).clone()
    assert q.data_ptr() != old.data_ptr()
    old.fill_(float("nan"))                                            # whoever still reads the old storage shows
    loss = run_step(step, gdata, None)
    assert step._pg is None and step._pg_builds == builds             # the group went with the old pointers; this step packed per call
    assert bit_equal(loss, run_step(step, gdata, None))
    assert step._pg is not None and step._pg_builds == builds + 1      # ... and the next one built the new group
    twin, tgrads, tstep = _fresh_step(eng, mine)
    tloss = run_step(tstep, gdata, None)
    assert bool(torch.isfinite(loss)) and bit_equal(loss, tloss) and bit_equal(step.prediction(), tstep.prediction())
    assert _grads_equal(mine, twin)


def test_changing_batches_never_build_a_group(eng, graphs):
    """A step whose buffers differ from those of the step before (variable meshes: new plans every batch; here: two batch sizes in
    turn) packs per call, as every step did before the group: no group is built, so none is destroyed -- nothing waits for the
    device.  Once the batch repeats, the group serves, and the results are the per-call ones bit for bit."""
    ref, data = make_oracle("split", graphs)
    gdata = _cuda(data)
    half = (gdata[0][:1], gdata[1][:1], gdata[2][:1], [g[:1] for g in gdata[3]], [i[:1] for i in gdata[4]])
    mine, grads, step = make_step(eng, ref, (1.0,), input_grad=False)
    seen = {}
    for k in range(6):
        d = gdata if k % 2 == 0 else half
        loss = run_step(step, d, None)
        assert step._pg is None and step._pg_builds == 0, k
        seen[k % 2] = (loss.clone(), step.prediction().clone(), grads.flat.clone())
    for k, d in ((0, gdata), (0, gdata), (1, half), (1, half)):
        loss = run_step(step, d, None)
        assert all(bit_equal(u, v) for u, v in zip((loss, step.prediction(), grads.flat), seen[k])), k
    assert step._pg is not None and step._pg_builds == 2
