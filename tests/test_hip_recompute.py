"""GPU: activation recomputation in the U-Net backward -- BSMS_FWD_LEAN / BSMS_BWD_RECOMPUTE at the C ABI,
`FusedStep(recompute=True)`, `BSGMP.recompute`, `DataParallel(recompute=)`, `model_cfg.recompute_activations`.

The lean forward keeps the inputs of the blocks only; the backward runs every block's training forward again, from that input, into
one of two blobs in `work`.  The same kernels see the same operands, so nothing may move: EVERY comparison here is against the same
engine with the flag off and is bit equality (byte views, so a NaN cannot hide).  No tolerance is involved anywhere.

Everything runs on the 300-node `del300` hierarchy with the golden `sim` batch (B = 2, C = 2, p = 2), model shapes and seeds of
tests/test_hip_unroll.py."""
import os
import sys
from types import SimpleNamespace

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from conftest import ROOT, load_golden
from oracle import bsms_oracle as ro
from test_hip_unroll import SHAPES, _cuda, later_targets, make_oracle

pytestmark = pytest.mark.gpu

LEAN, RECOMPUTE = 4, 2                     # BSMS_FWD_LEAN, BSMS_BWD_RECOMPUTE (include/bsms_hip.h)
PREC = {"f32": 0, "bf16": 1, "bf16_nodes": 2}
NAN = float("nan")


@pytest.fixture(scope="module")
def eng():
    import bsms_gnn_amd as eng
    return eng


def bits(t):
    return t.detach().contiguous().reshape(-1).view(torch.uint8)       # any dtype (the normalisers' statistics are fp64)


def bit_equal(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(bits(a), bits(b))


def align(n):
    return (n + 255) // 256 * 256


# ------------------------------------------------------------------------------------------------ the U-Net at the C ABI
class Unet:
    """A seeded BSGMP on the del300 hierarchy with its plans, edge weights and pointer tables: what the C entries take."""

    def __init__(self, eng, graphs, depth, D, H, seed=3):
        self.eng, self.depth, self.D, self.H, self.p, self.N = eng, depth, D, H, 2, 300
        torch.manual_seed(seed)
        self.net = eng.BSGMP(depth, D, H, 2).cuda()
        es, ids = graphs.levels("del300")
        plans, self.ews, bottom = self.net.prepare([i.cuda() for i in ids[:depth]], [e.cuda() for e in es[:depth + 1]], self.N, torch.device("cuda"))
        self.plans = [*plans, bottom]
        A = eng._abi
        self.pl, self._k0 = A.ptr_array([q.handle.value if hasattr(q.handle, "value") else q.handle for q in self.plans])
        self.ewp, self._k1 = A.ptr_array([e.data_ptr() for e in self.ews])
        self.params = self.net.block_params()
        self.pp, self._k2 = A.ptr_array([q.data_ptr() for q in self.params])

    def sizes(self, B, prec, flags):
        L = self.eng._abi.lib()
        a = (self.pl, self.depth, B, self.D, self.p, self.H)
        return L.bsms_bsgmp_saved_bytes_ex(*a, prec, flags), L.bsms_bsgmp_work_bytes_ex(*a, prec, flags)

    def run(self, h, pos, gout, prec=0, recompute=False, frozen=(), grad_pos=False, backwards=1):
        """Forward + `backwards` backwards through the C ABI.  `frozen`: {(block in storage order, 0 node MLP / 1 edge MLP)}.
        Every output starts as NaN; with `recompute` the part of `work` behind the unflagged layout -- the blobs -- is NaN-filled
        again before every backward, and the lean `saved` is followed by a sentinel region that must come back untouched."""
        A, L = self.eng._abi, self.eng._abi.lib()
        s = torch.cuda.current_stream().cuda_stream
        B, N, D, p, H, depth = h.shape[0], self.N, self.D, self.p, self.H, self.depth
        pbs = N * p if pos.dim() == 3 else 0
        flags = RECOMPUTE if recompute else 0
        nsaved, nwork = self.sizes(B, prec, flags)
        nwork0 = self.sizes(B, prec, 0)[1]
        assert nsaved > 0 or depth == 0
        assert nwork >= nwork0 > 0
        guard = 4096
        saved = torch.full((nsaved + guard,), 0xA5, dtype=torch.uint8, device="cuda")
        work = torch.full((nwork // 4,), NAN, device="cuda")
        out = torch.full_like(h, NAN)
        A.check(L.bsms_bsgmp_fwd_p(self.pl, self.ewp, depth, h.data_ptr(), pos.data_ptr(), B, D, p, pbs, H, self.pp, out.data_ptr(),
                                   saved.data_ptr(), work.data_ptr(), LEAN if recompute else 0, prec, s), "bsms_bsgmp_fwd_p")
        n = 2 * (H + 1)
        results = []
        for _ in range(backwards):
            if recompute:
                work[nwork0 // 4:] = NAN
            gts = [torch.full_like(q, NAN) for q in self.params]
            live = [(i // (2 * n), (i // n) % 2) not in frozen for i in range(len(gts))]
            gp, _k3 = A.ptr_array([g.data_ptr() if ok else None for g, ok in zip(gts, live)])
            gh = torch.full_like(h, NAN)
            common = (self.pl, self.ewp, depth, h.data_ptr(), pos.data_ptr(), gout.data_ptr(), B, D, p, pbs, H, self.pp, saved.data_ptr(),
                      work.data_ptr(), gh.data_ptr(), gp, prec, flags, None)
            gpos = None
            if grad_pos:
                gpos = torch.full_like(pos, NAN)
                pwork = torch.empty(L.bsms_bsgmp_pos_work_bytes(self.pl, depth, B, p), dtype=torch.uint8, device="cuda")
                A.check(L.bsms_bsgmp_bwd_pos_ev(*common, gpos.data_ptr(), pwork.data_ptr(), s), "bsms_bsgmp_bwd_pos_ev")
            else:
                A.check(L.bsms_bsgmp_bwd_ev(*common, s), "bsms_bsgmp_bwd_ev")
            torch.cuda.synchronize()
            assert bool((saved[nsaved:] == 0xA5).all()), "the backward wrote behind the saved buffer"
            r = dict(out=out.clone(), gh=gh, gpos=gpos, grads=gts, live=live)
            for t in (r["out"], gh, *([gpos] if grad_pos else []), *(g for g, ok in zip(gts, live) if ok)):
                assert bool(torch.isfinite(t).all())
            for g, ok in zip(gts, live):
                assert ok or bool(torch.isnan(g).all())                # a frozen MLP's entries are never written
            results.append(r)
        return results


def same(a, b, what):
    assert bit_equal(a["out"], b["out"]), (what, "out")
    assert bit_equal(a["gh"], b["gh"]), (what, "grad_h")
    assert (a["gpos"] is None) == (b["gpos"] is None)
    if a["gpos"] is not None:
        assert bit_equal(a["gpos"], b["gpos"]), (what, "grad_pos")
    assert a["live"] == b["live"]
    for i, (x, y) in enumerate(zip(a["grads"], b["grads"])):
        assert bit_equal(x, y), (what, "grads", i)


def inputs(unet, B, shared_pos, seed=11):
    gen = torch.Generator().manual_seed(seed)
    h = torch.randn(B, unet.N, unet.D, generator=gen).cuda()
    pos = torch.rand(*((unet.N, 2) if shared_pos else (B, unet.N, 2)), generator=gen).cuda()
    gout = torch.randn(B, unet.N, unet.D, generator=gen).cuda()
    return h, pos, gout


# ------------------------------------------------------------------------------------------------ 1: sizes
@pytest.mark.parametrize("depth", [0, 1, 3])
def test_size_queries(eng, graphs, depth):
    L = eng._abi.lib()
    B, D, H, p = 2, 32, 3, 2
    u = Unet(eng, graphs, depth, D, H)
    a = (u.pl, depth, B, D, p, H)
    full, work0 = L.bsms_bsgmp_saved_bytes_p(*a, 0), L.bsms_bsgmp_work_bytes(*a)
    assert u.sizes(B, 0, 0) == (full, work0) and u.sizes(B, 0, 1) == (full, work0)          # BSMS_BWD_DEFER_JOIN changes no size
    lean, work1 = u.sizes(B, 0, RECOMPUTE)
    level = lambda k: k if k <= depth else 2 * depth - k                                     # storage order: down, bottom, up
    blob = lambda lv: align(L.bsms_gmp_saved_bytes(B, u.plans[lv].N, u.plans[lv].E, D, H))   # carve_saved: one aligned take per block
    assert lean == full - sum(blob(level(k)) for k in range(2 * depth + 1))
    n_of = lambda lv: u.plans[lv].N
    assert lean == sum(align(4 * B * n_of(i) * D) + align(4 * B * n_of(i) * p) for i in range(1, depth + 1)) + \
        sum(align(4 * B * n_of(d) * D) for d in range(depth))                                # the block inputs and the coarse positions
    big, out0 = max(blob(lv) for lv in range(depth + 1)), align(4 * B * n_of(0) * D)
    assert big + out0 <= work1 - work0 <= 2 * big + out0
    assert work1 - work0 == (2 if depth else 1) * big + out0
    assert u.sizes(B, 0, 8) == (0, 0) and u.sizes(B, 0, RECOMPUTE | 4) == (0, 0)             # unknown bits
    assert u.sizes(B, 7, RECOMPUTE) == (0, 0)                                                # no such precision


@pytest.mark.parametrize("prec", ["bf16", "bf16_nodes"])
def test_lean_saved_holds_fp32_inputs_in_every_precision(eng, graphs, prec):
    u = Unet(eng, graphs, 2, 128, 3)
    L = eng._abi.lib()
    full = L.bsms_bsgmp_saved_bytes_p(u.pl, 2, 2, 128, 2, 3, PREC[prec])
    assert u.sizes(2, PREC[prec], 0)[0] == full
    lean = u.sizes(2, PREC[prec], RECOMPUTE)[0]
    assert 0 < lean < full and lean == u.sizes(2, 0, RECOMPUTE)[0]
    assert u.sizes(2, PREC[prec], 0)[1] == L.bsms_bsgmp_work_bytes(u.pl, 2, 2, 128, 2, 3)   # the unflagged work size knows no precision


# ------------------------------------------------------------------------------------------------ 2: the library, through the C ABI
CASES = [  # depth, D, H, shared pos, precision
    (0, 32, 3, False, "f32"),      # one block, one blob
    (1, 32, 3, False, "f32"),      # the third block is the first to reuse a blob
    (3, 32, 3, True, "f32"),       # every slot reused three times; a [N, p] pos
    (3, 32, 3, False, "f32"),
    (2, 64, 2, False, "f32"),
    (2, 128, 2, True, "f32"),
    (1, 256, 1, False, "f32"),
    (1, 96, 2, False, "f32"),      # the remaining widths, each with its own chain kernels
    (1, 160, 2, True, "f32"),
    (1, 192, 2, False, "f32"),
    (1, 224, 2, False, "f32"),
    (1, 256, 3, False, "bf16"),    # bf16 at the other width it exists at
    (2, 128, 3, False, "bf16"),    # the fused edge backward: e_Ps / e_Pd / e_wr in the blob
    (2, 128, 3, True, "bf16_nodes"),
    (1, 128, 2, False, "bf16"),    # bf16 without the fused edge backward (hidden = 2)
    (2, 32, 7, False, "f32"),      # the deepest block: blobs, pack table and weight-gradient table at their largest
    (1, 128, 5, True, "f32"),
    (1, 128, 5, False, "bf16"),    # bf16 on the generic ring kernels, above the fused depth
]


@pytest.mark.parametrize("depth,D,H,shared,prec", CASES, ids=lambda v: str(v))
def test_library_bits(eng, graphs, depth, D, H, shared, prec):
    u = Unet(eng, graphs, depth, D, H)
    h, pos, gout = inputs(u, 2, shared)
    (base,) = u.run(h, pos, gout, PREC[prec])
    first, second = u.run(h, pos, gout, PREC[prec], recompute=True, backwards=2)
    same(first, base, "recompute against the full pair")
    same(second, first, "a second backward on the same lean saved")      # nothing the backward needs lived in a blob


@pytest.mark.parametrize("depth,shared,prec", [(0, False, "f32"), (3, False, "f32"), (2, True, "f32"), (2, False, "bf16")])
def test_library_bits_with_grad_pos(eng, graphs, depth, shared, prec):
    D, H = (128, 3) if prec != "f32" else (32, 3)
    u = Unet(eng, graphs, depth, D, H)
    h, pos, gout = inputs(u, 2, shared)
    (base,) = u.run(h, pos, gout, PREC[prec], grad_pos=True)
    first, second = u.run(h, pos, gout, PREC[prec], recompute=True, grad_pos=True, backwards=2)
    same(first, base, "grad_pos")
    same(second, first, "grad_pos, second backward")


FROZEN = {
    "middle block": (1, {(1, 0), (1, 1)}),                       # execution order up, BOTTOM, down: a block that marks nothing between two that do
    "edge MLPs": (2, {(k, 1) for k in range(5)}),
    "every second block": (3, {(k, m) for k in (0, 2, 4, 6) for m in (0, 1)}),
    "everything": (2, {(k, m) for k in range(5) for m in (0, 1)}),
}


@pytest.mark.parametrize("name", sorted(FROZEN))
def test_library_bits_with_frozen_groups(eng, graphs, name):
    depth, frozen = FROZEN[name]
    u = Unet(eng, graphs, depth, 32, 3)
    h, pos, gout = inputs(u, 2, False)
    (base,) = u.run(h, pos, gout, frozen=frozen, grad_pos=True)
    first, second = u.run(h, pos, gout, frozen=frozen, grad_pos=True, recompute=True, backwards=2)
    same(first, base, name)
    same(second, first, name)
    (everything,) = u.run(h, pos, gout, recompute=True, grad_pos=True)
    for i, ok in enumerate(first["live"]):                               # ... and what is left equals the call with every entry
        assert not ok or bit_equal(first["grads"][i], everything["grads"][i]), i
    assert bit_equal(first["gh"], everything["gh"]) and bit_equal(first["gpos"], everything["gpos"])


def test_library_refusals_on_the_device(eng, graphs):
    u = Unet(eng, graphs, 1, 32, 3)
    h, pos, gout = inputs(u, 2, False)
    L, s = eng._abi.lib(), torch.cuda.current_stream().cuda_stream
    work = torch.empty(u.sizes(2, 0, RECOMPUTE)[1], dtype=torch.uint8, device="cuda")
    saved = torch.empty(u.sizes(2, 0, RECOMPUTE)[0], dtype=torch.uint8, device="cuda")
    out = torch.full_like(h, 7.0)
    fwd = lambda sv, reuse: L.bsms_bsgmp_fwd_p(u.pl, u.ewp, 1, h.data_ptr(), pos.data_ptr(), 2, 32, 2, 600, 3, u.pp, out.data_ptr(), sv,
                                               work.data_ptr(), reuse, 0, s)
    assert fwd(None, LEAN) == -1 and fwd(saved.data_ptr(), 8) == -1 and fwd(saved.data_ptr(), LEAN | 16) == -1
    gts = [torch.full_like(q, 7.0) for q in u.params]
    gp, _k = eng._abi.ptr_array([g.data_ptr() for g in gts])
    bwd = lambda sv, flags: L.bsms_bsgmp_bwd_ex(u.pl, u.ewp, 1, h.data_ptr(), pos.data_ptr(), gout.data_ptr(), 2, 32, 2, 600, 3, u.pp, sv,
                                                work.data_ptr(), out.data_ptr(), gp, 0, flags, s)
    assert bwd(None, RECOMPUTE) == -1 and bwd(saved.data_ptr(), 4) == -1 and bwd(saved.data_ptr(), RECOMPUTE | 64) == -1
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()) and all(bool((g == 7.0).all()) for g in gts)             # refused before the first launch


# ------------------------------------------------------------------------------------------------ 3: FusedStep
_REF = {}


def oracle(shape, graphs):
    if shape not in _REF:
        _REF[shape] = make_oracle(shape, graphs)
    return _REF[shape]


def build(eng, ref, recompute, precision=None, freeze=(), **kw):
    mine = eng.BSMS_Simulator(ref.cfg)
    mine.load_state_dict(ref.state_dict())
    mine = mine.cuda()
    if precision:
        mine.process.precision = precision
    for name in freeze:
        getattr(mine, name).requires_grad_(False)
    grads = eng.GradBuckets(list(mine.parameters()))
    grads.flat.fill_(NAN)                                               # whatever the buffer held is overwritten
    return mine, grads, eng.FusedStep(mine, grads, recompute=recompute, **kw)


def both(eng, ref, gdata, later=None, consistent=True, calls=1, precision=None, freeze=(), **kw):
    """The same step with the flag off and on, `calls` times each: every loss, prediction, gradient (and input gradient) bit-equal."""
    res = []
    for recompute in (False, True):
        mine, grads, step = build(eng, ref, recompute, precision, freeze, **kw)
        runs = []
        for _ in range(calls):
            loss = step(gdata, consistent, later)
            torch.cuda.synchronize()
            runs.append(dict(loss=loss.clone(), preds=[q.clone() for q in step.predictions()], flat=grads.flat.clone(),
                             ig=step.input_grad().clone() if kw.get("input_grad") else None))
        res.append((runs, step))
    (off, _), (on, step) = res
    for a, b in zip(off, on):
        assert bit_equal(a["loss"], b["loss"]) and bit_equal(a["flat"], b["flat"])
        assert kw.get("param_grad") is False or bool(torch.isfinite(b["flat"]).all())
        assert len(a["preds"]) == len(b["preds"]) and all(bit_equal(x, y) for x, y in zip(a["preds"], b["preds"]))
        assert (a["ig"] is None and b["ig"] is None) or (bit_equal(a["ig"], b["ig"]) and bool(torch.isfinite(b["ig"]).all()))
    return off, on, step


@pytest.mark.parametrize("shape,precision", [("ring", None), ("split", None), ("d64", None), ("split", "bf16")])
def test_fused_step_three_calls(eng, graphs, shape, precision):
    """Three consecutive calls: equal to the flag-off step and to each other -- the blobs are reused from call to call."""
    ref, data = oracle(shape, graphs)
    off, on, step = both(eng, ref, _cuda(data), calls=3, precision=precision)
    assert step.recompute is True
    for r in on[1:]:
        assert bit_equal(r["flat"], on[0]["flat"]) and bit_equal(r["loss"], on[0]["loss"])


@pytest.mark.parametrize("shape,detach", [("ring", False), ("ring", True), ("split", False), ("d64", True)])
def test_fused_step_unrolled(eng, graphs, shape, detach):
    ref, data = oracle(shape, graphs)
    gdata = _cuda(data)
    both(eng, ref, gdata, later_targets(gdata[0], gdata[1], 3), calls=2, unroll=3, detach=detach)


def test_fused_step_other_objective_and_input_grad(eng, graphs):
    ref, data = oracle("ring", graphs)
    gdata = _cuda(data)
    obj = eng.Objective(space="normalized", kind="mse", channel_weights=[2.0, 0.5])
    both(eng, ref, gdata, objective=obj)
    both(eng, ref, gdata, later_targets(gdata[0], gdata[1], 2), unroll=2, objective=obj, input_grad=True)
    both(eng, ref, gdata, input_grad=True, calls=2)
    both(eng, ref, gdata, input_grad=True, param_grad=False)             # the data-only backward: every block marks nothing


def test_fused_step_accumulate(eng, graphs):
    ref, data = oracle("ring", graphs)
    both(eng, ref, _cuda(data), calls=4, accumulate=2)                   # two cycles of two micro-batches


def test_fused_step_frozen_processor(eng, graphs):
    ref, data = oracle("ring", graphs)
    both(eng, ref, _cuda(data), freeze=("process",), calls=2)
    both(eng, ref, _cuda(data), freeze=("encode", "decode"))


def test_fused_step_graph_replay_equals_eager(eng, graphs):
    ref, data = oracle("ring", graphs)
    gdata = _cuda(data)
    off, on, _ = both(eng, ref, gdata, calls=3, use_graph=True)          # capture, then two replays
    _, grads, eager = build(eng, ref, True)
    loss = eager(gdata, True)
    assert bit_equal(loss, on[2]["loss"]) and bit_equal(grads.flat, on[2]["flat"])


def test_fused_step_variable_meshes(eng, graphs):
    """consistent=False: the golden block-diagonal batch (del64 + del300 in one graph, 364 rows, depth 2; the B = 1 axis)."""
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
    both(eng, ref, levels, consistent=False, calls=2)
    both(eng, ref, levels, later_targets(data[0], data[1], 2)[:, 0].cuda(), consistent=False, unroll=2)


# ------------------------------------------------------------------------------------------------ 4: memory
def total_bytes(step):
    return sum(t.numel() * t.element_size() for t in step._arena._t.values() if t is not None)


def test_held_bytes(eng, graphs):
    ref, data = oracle("ring", graphs)
    gdata = _cuda(data)
    D, H, depth = SHAPES["ring"]
    u = Unet(eng, graphs, depth, D, H)
    full, lean = u.sizes(2, 0, 0)[0], u.sizes(2, 0, RECOMPUTE)[0]
    assert lean < full // 8                                              # the blocks' activations were nearly all of it
    held = {}
    for recompute in (False, True):
        for K in (1, 2, 4):
            _, _, step = build(eng, ref, recompute, unroll=K)
            with pytest.raises(RuntimeError):
                step.held_bytes()
            step(gdata, True, later_targets(gdata[0], gdata[1], K))
            held[recompute, K] = dict(step.held_bytes(), total=total_bytes(step))
            assert set(step.held_bytes()) == {"per_step", "shared"}
    for K in (1, 2, 4):
        assert held[True, K]["per_step"] == held[False, K]["per_step"] - (align(full) - align(lean))
    for recompute in (False, True):
        h1, h2, h4 = (held[recompute, K] for K in (1, 2, 4))
        assert h2["shared"] == h4["shared"]
        assert h4["total"] - h2["total"] == 2 * h4["per_step"] and h2["per_step"] == h4["per_step"]
        assert h1["total"] == h1["shared"] + h1["per_step"]
    # the blobs and the discard buffer are shared by the K steps: they live in `work`
    assert held[True, 4]["shared"] - held[False, 4]["shared"] == align(u.sizes(2, 0, RECOMPUTE)[1]) - align(u.sizes(2, 0, 0)[1])


# ------------------------------------------------------------------------------------------------ 5: the routes
@pytest.mark.parametrize("pos_grad", [False, True])
@pytest.mark.parametrize("shape,precision", [("ring", "f32"), ("split", "bf16")])
def test_autograd_route(eng, graphs, shape, precision, pos_grad):
    D, H, depth = SHAPES[shape]
    if precision != "f32":
        H = 3
    es, ids = graphs.levels("del300")
    m_gs, m_ids = [e.cuda() for e in es[:depth + 1]], [i.cuda() for i in ids[:depth]]
    gen = torch.Generator().manual_seed(2)
    h0, pos0, w = torch.randn(2, 300, D, generator=gen).cuda(), torch.rand(2, 300, 2, generator=gen).cuda(), torch.randn(2, 300, D, generator=gen).cuda()
    res = []
    for recompute in (False, True):
        torch.manual_seed(9)
        net = eng.BSGMP(depth, D, H, 2).cuda()
        net.precision = precision
        net.recompute = recompute
        h, pos = h0.clone().requires_grad_(True), pos0.clone().requires_grad_(pos_grad)
        y = net(h, m_ids, m_gs, pos)
        (y * w).sum().backward()
        torch.cuda.synchronize()
        res.append((y.detach(), h.grad, pos.grad, [q.grad for q in net.parameters()]))
    (y0, gh0, gp0, g0), (y1, gh1, gp1, g1) = res
    assert bit_equal(y0, y1) and bit_equal(gh0, gh1) and all(bit_equal(a, b) for a, b in zip(g0, g1))
    assert (gp1 is not None) == pos_grad and (not pos_grad or bit_equal(gp0, gp1))


def test_trainer_with_recompute_activations(eng, graphs):
    ref, data = oracle("ring", graphs)
    gdata = _cuda(data)
    opt_cfg = SimpleNamespace(peak_lr=1e-3, weight_decay=1e-2, warmup_steps=2, decay_steps=20, gnorm_clip=1.0)
    out = []
    for extra in ({}, {"recompute_activations": True}, {"recompute_activations": False}):
        model_cfg = SimpleNamespace(out_dim=2, latent_dim=32, hidden_layer=3, unet_depth=3, pos_dim=2, consistent_mesh=True,
                                    accumulation_steps=1, **extra)
        torch.manual_seed(0)
        m = eng.BSMS_Simulator(model_cfg)
        m.load_state_dict(ref.state_dict())
        tr = eng.Trainer(m, model_cfg, opt_cfg)
        assert tr.dp.fused is not None and tr.dp.fused.recompute is bool(extra.get("recompute_activations", False))
        tr.iter(gdata)                                                   # warm-up: normaliser statistics only
        start = [q.detach().clone() for q in tr.model.parameters()]
        losses = [tr.iter(gdata) for _ in range(3)]
        torch.cuda.synchronize()
        out.append((torch.stack(losses), [q.detach().clone() for q in tr.model.parameters()]))
        assert sum(not bit_equal(a, b) for a, b in zip(start, out[-1][1])) > 0                # the parameters did move
    for losses, params in out[1:]:
        assert bit_equal(losses, out[0][0]) and all(bit_equal(a, b) for a, b in zip(params, out[0][1]))


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
    c, sl = (lambda t: t.cuda()), slice(rank, rank + 1)
    data = (c(z.t("node_in")[sl]), c(z.t("tar")[sl]), c(z.t("mask")[sl]), [c(e.unsqueeze(0)) for e in es], [c(i.unsqueeze(0)) for i in ids])
    res = {}
    for recompute in (False, True):                                   # the same two ranks, without and with the flag
        torch.manual_seed(50 + rank)                                  # different init per rank: the broadcast must fix it
        sim = eng.BSMS_Simulator(ro.make_cfg(2, 32, 3, 3, 2))
        if rank == 0:
            sim.load_state_dict(z.state_dict())
        engine = eng.DataParallel(sim.cuda(), bucket_bytes=64 << 10, unroll=2, recompute=recompute)
        assert engine.fused.recompute is recompute
        loss = engine.step_loss_backward(data, True, later_targets(data[0], data[1], 2))
        torch.cuda.synchronize()
        res[recompute] = {"loss": loss.detach().cpu(), "flat": engine.grads.flat.cpu()}
    torch.save(res, f"{out_path}.{rank}")
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.timeout(300)
def test_two_ranks_with_recompute(eng, tmp_path):
    port = 29900 + os.getpid() % 2000
    out = str(tmp_path / "res")
    mp.start_processes(_worker, args=(2, port, out), nprocs=2, join=True, start_method="spawn")
    r0, r1 = torch.load(out + ".0"), torch.load(out + ".1")
    for r in (r0, r1):
        assert bit_equal(r[True]["flat"], r[False]["flat"]) and bit_equal(r[True]["loss"], r[False]["loss"])
        assert bool(torch.isfinite(r[True]["flat"]).all()) and float(r[True]["flat"].abs().max()) > 0
    assert bit_equal(r0[True]["flat"], r1[True]["flat"])               # bit-identical across ranks
