"""GPU: frozen parameters -- NULL entries in the `grads` tables of bsms_mlp_bwd*, bsms_gmp_bwd* and
bsms_bsgmp_bwd*, the launches that vanish with them, the no-store backward chains, and the Python layers on top (autograd
Functions, FusedStep, input_gradient(param_grad=False), DataParallel, Trainer).

Every comparison is BIT-EQUALITY against the same build called with nothing frozen: freezing removes launches and stores, the
arithmetic that remains is unchanged (the unfrozen path is pinned against the oracle elsewhere).  Weights and data are random:
bit-equality between two calls of one library needs no ReLU-kink margin."""
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
from test_hip_input_grad import bit_equal, make_step, run_step
from test_hip_unroll import _cuda, later_targets, make_oracle

pytestmark = pytest.mark.gpu
OK, E_INVALID_ARG, E_UNSUPPORTED = 0, -1, -3
FS_ROWS = 3072                    # chain_kernels.h: kFsMaxRowsBwd, the feature-split backward's row limit (D = 128)


@pytest.fixture(scope="module")
def eng():
    import bsms_gnn_amd as eng
    return eng


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _u8(nbytes):
    return torch.empty(max(int(nbytes), 1), dtype=torch.uint8, device="cuda")


def _nan(t):
    return torch.full_like(t, float("nan"))


def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def delaunay_edges(eng, n, seed):
    from scipy.spatial import Delaunay
    pts = np.random.default_rng(seed).random((n, 2))
    flat = eng.to_flat_edge(Delaunay(pts).simplices.astype(np.int64), "tri")
    return torch.tensor(pts, dtype=torch.float32), torch.tensor(flat, dtype=torch.int64)


def table(eng, tensors, live):
    """Pointer table with NULL entries where `live` is False."""
    return eng._abi.ptr_array([t.data_ptr() if keep else None for t, keep in zip(tensors, live)])


# ------------------------------------------------------------------------------------------------ 1: one GMP block at the C ABI
class GmpCase:
    def __init__(self, eng, D, B, g, pos, seed=0, p=2, H=3):
        from bsms_gnn_amd.graph import plan_for
        from bsms_gnn_amd.ops import _param_ptrs
        self.eng, self.L, self.D, self.B, self.p, self.H = eng, eng._abi.lib(), D, B, p, H
        n = pos.shape[0]
        torch.manual_seed(seed)
        self.net = eng.GMP(D, H, p).cuda()
        self.params = [*self.net.mlp_node.flat_params(), *self.net.mlp_edge.flat_params()]
        self.pp, self._keep = _param_ptrs(self.params)
        self.g = g.cuda()
        self.plan = plan_for(self.g, n)
        self.N, self.E = n, self.plan.E
        self.x, self.cot = torch.randn(B, n, D).cuda(), torch.randn(B, n, D).cuda()
        self.pos = (pos.unsqueeze(0) + 0.01 * torch.randn(B, n, p)).cuda().contiguous()
        L = self.L
        self.saved, self.work = _u8(L.bsms_gmp_saved_bytes(B, n, self.E, D, H)), _u8(L.bsms_gmp_work_bytes(B, n, self.E, D, H))
        self.pwork, self.out = _u8(L.bsms_gmp_pos_work_bytes(B, self.E, p)), torch.empty_like(self.x)

    def run(self, node, edge, whole_null=False):
        """Forward, then bsms_gmp_bwd_pos with the node / edge MLP's gradient entries there (True) or NULL (False)."""
        L, s, nl = self.L, _stream(), 2 * (self.H + 1)
        a = (self.plan.handle, self.x.data_ptr(), self.pos.data_ptr())
        shape = (self.B, self.D, self.p, self.N * self.p, self.H, self.pp)
        self.eng._abi.check(L.bsms_gmp_fwd(*a, *shape, self.out.data_ptr(), self.saved.data_ptr(), self.work.data_ptr(), s), "bsms_gmp_fwd")
        gx, gpos, grads = _nan(self.x), _nan(self.pos), [_nan(q) for q in self.params]
        gp, keep = table(self.eng, grads, [node] * nl + [edge] * nl)
        self.eng._abi.check(L.bsms_gmp_bwd_pos(*a, self.cot.data_ptr(), *shape, self.saved.data_ptr(), self.work.data_ptr(), gx.data_ptr(),
                                               None if whole_null else gp, gpos.data_ptr(), self.pwork.data_ptr(), s), "bsms_gmp_bwd_pos")
        torch.cuda.synchronize()
        return gx, gpos, grads[:nl], grads[nl:]


def check_freeze_patterns(c):
    want = c.run(True, True)
    assert all(bool(torch.isfinite(t).all()) for t in (want[0], want[1], *want[2], *want[3]))
    assert float(want[1].abs().max()) > 0
    for node, edge, whole in ((False, True, False), (True, False, False), (False, False, False), (False, False, True)):
        got = c.run(node, edge, whole)
        tag = (c.D, c.B * c.E, node, edge, whole)
        assert bit_equal(got[0], want[0]), ("grad_x", tag)
        assert bit_equal(got[1], want[1]), ("grad_pos", tag)
        for k, live in ((2, node), (3, edge)):
            if live:                                                       # the surviving MLP's 2 (H + 1) gradients
                assert all(bit_equal(u, v) for u, v in zip(got[k], want[k])), (k, tag)
            else:                                                          # a frozen MLP's tensors were not handed over: still NaN
                assert all(bool(torch.isnan(u).all()) for u in got[k]), (k, tag)


# name -> (D, nodes, B): the kernel family every backward chain of the block takes, and the row counts that select it
# (chain_launch.h: plan_bwd; a 7-wave edge tile has 112 rows, 224 with two row blocks per wave)
GMP_SHAPES = {
    # node MLP: k_fs_bwd (B N <= 3072); edge MLP: k_edge_bwd<8,1,LONE>, one round of 112-row tiles (B E <= 3072 here)
    "fs_d128": (128, 200, 2),
    # D = 64 / 96 have no single-round build: node and edge MLP on the ring kernel k_chain_bwd
    "ring_d64": (64, 700, 2),
    "ring_d96": (96, 700, 2),
    # D = 160: node and edge MLP on k_chain_bwd's single-round (LONE) build (tiles <= CUs)
    "lone_ring_d160": (160, 700, 2),
    # edge MLP: k_edge_bwd<8,1> (3072 < B E < CUs x 112: pick_edge_waves takes 4 waves, more tiles than CUs, so not the LONE build
    # that fs_d128 reaches -- the shape keeps its historical name); node MLP: k_chain_bwd LONE (B N > 3072)
    "edge_lone_d128": (128, 1100, 3),
    # edge MLP: k_edge_bwd<8,2>, more than one round of 224-row tiles (B E > CUs x 224)
    "edge_rb2_multi_d128": (128, 2600, 4),
    # edge MLP: k_edge_bwd<8,2,LONE>, one round of 224-row tiles (CUs x 112 <= B E <= CUs x 224): the airfoil step's lower levels
    "edge_rb2_lone_d128": (128, 1700, 4),
    # edge MLP: k_edge_bwd<16,1> (LONE build: one round)
    "edge_d256": (256, 700, 2),
    # edge MLP: k_edge_bwd<16,1>, more than one workgroup per CU's worth of 112-row tiles (B E > CUs x 112)
    "edge_multi_d256": (256, 1300, 4),
}


@pytest.mark.parametrize("name", list(GMP_SHAPES))
def test_gmp_block_freeze_patterns(eng, name):
    D, n, B = GMP_SHAPES[name]
    pos, g = delaunay_edges(eng, n, seed=n + D)
    c = GmpCase(eng, D, B, g, pos, seed=D)
    re, rn, cus = B * c.E, B * c.N, _cus()
    if name == "fs_d128":
        assert re <= FS_ROWS and rn <= FS_ROWS
    elif name in ("ring_d64", "ring_d96", "lone_ring_d160", "edge_d256"):
        assert 7000 <= re <= 9500 and rn <= cus * 64
    elif name == "edge_lone_d128":
        assert FS_ROWS < re < cus * 112 and rn > FS_ROWS
    elif name == "edge_rb2_lone_d128":
        assert cus * 112 <= re <= cus * 224
    elif name == "edge_multi_d256":
        assert re > cus * 112
    else:
        assert re > cus * 224
    # the kernels GMP_SHAPES names are the ones chosen on this device: (edge MLP, its no-store launch when frozen, node MLP)
    from test_chain_launch_host import launch_info
    named = {"fs_d128": ("edge_bwd rb1 store lone", "edge_bwd rb1 lone", "fs_bwd"),
             "ring_d64": ("chain_bwd",) * 3, "ring_d96": ("chain_bwd",) * 3, "lone_ring_d160": ("chain_bwd lone",) * 3,
             "edge_lone_d128": ("edge_bwd rb1 store", "edge_bwd rb1", "chain_bwd lone"),
             "edge_rb2_multi_d128": ("edge_bwd rb2 store", "edge_bwd rb2", None),
             "edge_rb2_lone_d128": ("edge_bwd rb2 store lone", "edge_bwd rb2 lone", None),
             "edge_d256": ("edge_bwd rb1 store lone", "edge_bwd rb1 lone", None),
             "edge_multi_d256": ("edge_bwd rb1 store", "edge_bwd rb1", None)}[name]
    got = tuple(launch_info(D, 1, tag, rows).text for tag, rows in (("edge", re), ("edge frozen", re), ("node", rn)))
    assert all(w is None or w == g for w, g in zip(named, got)), (name, got)
    check_freeze_patterns(c)


def test_gmp_block_degree_zero_row_and_ragged_tile(eng):
    """Node 0 receives nothing and node 1 sends nothing (empty CSR rows in both scatters), and B E is no multiple of 16: the last
    tile of the edge chain is ragged.  D = 128: k_edge_bwd and its no-store build."""
    D, n, B = 128, 300, 3
    pos, g = delaunay_edges(eng, n, seed=5)
    g = g[:, (g[1] != 0) & (g[0] != 1)]
    while (B * g.shape[1]) % 16 in (0, 8):
        g = g[:, :-1]
    c = GmpCase(eng, D, B, g, pos, seed=1)
    assert (B * c.E) % 16 != 0 and c.E == g.shape[1] and not bool((g[1] == 0).any()) and not bool((g[0] == 1).any())
    check_freeze_patterns(c)


# ------------------------------------------------------------------------------------------------ 2: bsms_mlp_bwd_ex, grads = NULL
MLP_SHAPES = {"encoder": (4, 128, 1), "decoder": (128, 3, 0), "ln": (128, 128, 1)}       # name -> (in, out, layer_norm); D = 128


@pytest.mark.parametrize("R", [50, 3073, 9000])                       # k_fs_bwd; one row past its limit; several tiles per workgroup
@pytest.mark.parametrize("shape", list(MLP_SHAPES))
def test_mlp_bwd_with_null_grads(eng, shape, R):
    from bsms_gnn_amd.ops import _param_ptrs
    in_dim, out_dim, ln = MLP_SHAPES[shape]
    D, H, L, s = 128, 3, eng._abi.lib(), _stream()
    torch.manual_seed(R + in_dim)
    net = eng.MLP(in_dim, D, out_dim, H, bool(ln)).cuda()
    params = net.flat_params()
    pp, keep = _param_ptrs(params)
    x, gy, y = torch.randn(R, in_dim).cuda(), torch.randn(R, out_dim).cuda(), torch.empty(R, out_dim).cuda()
    saved, work = _u8(L.bsms_mlp_saved_bytes(R, in_dim, D, out_dim, H)), _u8(L.bsms_mlp_work_bytes(R, in_dim, D, out_dim, H))
    shape_args = (R, in_dim, D, out_dim, H, ln, pp)

    def run(grads_mode, flags=0, want_gx=True):
        eng._abi.check(L.bsms_mlp_fwd(x.data_ptr(), *shape_args, y.data_ptr(), saved.data_ptr(), work.data_ptr(), s), "bsms_mlp_fwd")
        gx, grads = _nan(x), [_nan(q) for q in params]
        gp, keep2 = table(eng, grads, [grads_mode == "live"] * len(grads))
        eng._abi.check(L.bsms_mlp_bwd_ex(x.data_ptr(), gy.data_ptr(), *shape_args, saved.data_ptr(), work.data_ptr(),
                                         gx.data_ptr() if want_gx else None, None if grads_mode == "null" else gp, flags, s), "bsms_mlp_bwd_ex")
        eng._abi.check(L.bsms_side_lanes_join(s), "bsms_side_lanes_join")
        torch.cuda.synchronize()
        return gx, grads

    want, wgrads = run("live")
    assert bool(torch.isfinite(want).all()) and all(bool(torch.isfinite(t).all()) for t in wgrads)
    for mode in ("null", "null_entries"):
        for flags in (0, 1):                                           # 1 = BSMS_BWD_DEFER_JOIN: nothing to defer, nothing marked
            got, grads = run(mode, flags)
            assert bit_equal(got, want), (shape, R, mode, flags)
            assert all(bool(torch.isnan(t).all()) for t in grads)
    if shape == "encoder":                                             # neither grads nor grad_x: nothing to do, BSMS_OK
        got, _ = run("null", want_gx=False)
        assert bool(torch.isnan(got).all())


# ------------------------------------------------------------------------------------------------ 3: error paths (host checks)
def test_partly_null_and_bf16_null_are_refused_before_any_launch(eng, graphs):
    from bsms_gnn_amd.ops import _param_ptrs
    D, B, H, p = 128, 2, 3, 2
    pos, g = delaunay_edges(eng, 150, seed=2)
    c = GmpCase(eng, D, B, g, pos)
    L, s, nl = c.L, _stream(), 2 * (H + 1)
    a = (c.plan.handle, c.x.data_ptr(), c.pos.data_ptr())
    shape = (B, D, p, c.N * p, H, c.pp)
    eng._abi.check(L.bsms_gmp_fwd(*a, *shape, c.out.data_ptr(), c.saved.data_ptr(), c.work.data_ptr(), s), "bsms_gmp_fwd")
    for hole in (0, nl - 1, nl, 2 * nl - 1):                          # one entry missing in the node MLP / in the edge MLP
        gx, gpos, grads = torch.full_like(c.x, 7.0), torch.full_like(c.pos, 7.0), [torch.full_like(q, 7.0) for q in c.params]
        gp, keep = table(eng, grads, [i != hole for i in range(2 * nl)])
        rc = L.bsms_gmp_bwd_pos(*a, c.cot.data_ptr(), *shape, c.saved.data_ptr(), c.work.data_ptr(), gx.data_ptr(), gp, gpos.data_ptr(),
                                c.pwork.data_ptr(), s)
        assert rc == E_INVALID_ARG and b"partly null" in L.bsms_last_error(), hole
        torch.cuda.synchronize()
        assert all(bool((t == 7.0).all()) for t in (gx, gpos, *grads)), hole
    # bsms_mlp_bwd_ex
    net = eng.MLP(D, D, D, H, True).cuda()
    params = net.flat_params()
    pp, keep = _param_ptrs(params)
    R = 100
    x, gy, y = torch.randn(R, D).cuda(), torch.randn(R, D).cuda(), torch.empty(R, D).cuda()
    saved, work = _u8(L.bsms_mlp_saved_bytes(R, D, D, D, H)), _u8(L.bsms_mlp_work_bytes(R, D, D, D, H))
    eng._abi.check(L.bsms_mlp_fwd(x.data_ptr(), R, D, D, D, H, 1, pp, y.data_ptr(), saved.data_ptr(), work.data_ptr(), s), "bsms_mlp_fwd")
    gx, grads = torch.full_like(x, 7.0), [torch.full_like(q, 7.0) for q in params]
    gp, keep2 = table(eng, grads, [i != 3 for i in range(len(grads))])
    rc = L.bsms_mlp_bwd_ex(x.data_ptr(), gy.data_ptr(), R, D, D, D, H, 1, pp, saved.data_ptr(), work.data_ptr(), gx.data_ptr(), gp, 0, s)
    assert rc == E_INVALID_ARG and b"partly null" in L.bsms_last_error()
    torch.cuda.synchronize()
    assert all(bool((t == 7.0).all()) for t in (gx, *grads))
    # the U-Net: a hole in the LAST block that runs (storage block 0) is found before the first block is launched; null entries
    # under BSMS_BF16 are unsupported
    u = UnetCase(eng, graphs, D=128)
    for prec, live, want, text in ((0, lambda k, i: not (k == 0 and i == 5), E_INVALID_ARG, b"partly null"),
                                   (1, lambda k, i: k != 2, E_UNSUPPORTED, b"fp32"),
                                   (1, lambda k, i: not (k == 1 and i >= nl), E_UNSUPPORTED, b"fp32")):
        gh, gpos, grads = torch.full_like(u.h, 7.0), torch.full_like(u.pos, 7.0), [torch.full_like(q, 7.0) for q in u.params]
        gp, keep = table(eng, grads, [live(i // (2 * nl), i % (2 * nl)) for i in range(len(grads))])
        rc = L.bsms_bsgmp_bwd_pos_ev(*u.common(), gh.data_ptr(), gp, prec, 0, None, gpos.data_ptr(), u.pwork.data_ptr(), s)
        assert rc == want and text in L.bsms_last_error(), (prec, rc, L.bsms_last_error())
        torch.cuda.synchronize()
        assert all(bool((t == 7.0).all()) for t in (gh, gpos, *grads)), prec


# ------------------------------------------------------------------------------------------------ 4: the U-Net
class UnetCase:
    """del300, depth 2 (three levels, five blocks), B = 2, through the raw entries on one set of buffers."""

    def __init__(self, eng, graphs, D=128, H=3, B=2, depth=2, p=2):
        from bsms_gnn_amd.ops import _param_ptrs
        self.eng, self.L, self.D, self.H, self.B, self.depth, self.p = eng, eng._abi.lib(), D, H, B, depth, p
        es, ids = graphs.levels("del300")
        base = torch.tensor(graphs.np("del300/pos")[:, :p], dtype=torch.float32)
        torch.manual_seed(3)
        self.net = eng.BSGMP(depth, D, H, p).cuda()
        self.n = n = base.shape[0]
        self.h, self.cot = torch.randn(B, n, D).cuda(), torch.randn(B, n, D).cuda()
        self.pos = (base + 0.05 * torch.randn(B, n, p)).cuda().contiguous()
        L = self.L
        plans, self.ews, bottom = self.net.prepare([i.cuda() for i in ids[:depth]], [e.cuda() for e in es[:depth + 1]], n, torch.device("cuda"))
        self.plans = [*plans, bottom]
        self.pl, self._k1 = eng._abi.ptr_array([q.handle.value if hasattr(q.handle, "value") else q.handle for q in self.plans])
        self.ewp, self._k2 = eng._abi.ptr_array([e.data_ptr() for e in self.ews])
        self.params = self.net.block_params()
        self.pp, self._k3 = _param_ptrs(self.params)
        self.saved, self.work = _u8(L.bsms_bsgmp_saved_bytes_p(self.pl, depth, B, D, p, H, 0)), _u8(L.bsms_bsgmp_work_bytes(self.pl, depth, B, D, p, H))
        self.pwork, self.out = _u8(L.bsms_bsgmp_pos_work_bytes(self.pl, depth, B, p)), torch.empty_like(self.h)

    def common(self):
        return (self.pl, self.ewp, self.depth, self.h.data_ptr(), self.pos.data_ptr(), self.cot.data_ptr(), self.B, self.D, self.p, self.n * self.p,
                self.H, self.pp, self.saved.data_ptr(), self.work.data_ptr())

    def run(self, live, defer, whole_null=False):
        """`live(block, entry)` -> the entry is handed over.  `defer`: BSMS_BWD_DEFER_JOIN + one event per block + bsms_side_lanes_join."""
        L, s, eng = self.L, _stream(), self.eng
        eng._abi.check(L.bsms_bsgmp_fwd_p(self.pl, self.ewp, self.depth, self.h.data_ptr(), self.pos.data_ptr(), self.B, self.D, self.p,
                                          self.n * self.p, self.H, self.pp, self.out.data_ptr(), self.saved.data_ptr(), self.work.data_ptr(), 0, 0, s),
                       "bsms_bsgmp_fwd")
        per = 4 * (self.H + 1)
        gh, gpos, grads = _nan(self.h), _nan(self.pos), [_nan(q) for q in self.params]
        mask = [live(i // per, i % per) for i in range(len(grads))]
        gp, keep = table(eng, grads, mask)
        evs, evp = None, None
        if defer:
            evs = [torch.cuda.Event() for _ in range(2 * self.depth + 1)]
            for e in evs:
                e.record()
            evp, keep_ev = eng._abi.ptr_array([e.cuda_event for e in evs])
        eng._abi.check(L.bsms_bsgmp_bwd_pos_ev(*self.common(), gh.data_ptr(), None if whole_null else gp, 0, 1 if defer else 0, evp,
                                               gpos.data_ptr(), self.pwork.data_ptr(), s), "bsms_bsgmp_bwd_pos_ev")
        if defer:
            eng._abi.check(L.bsms_side_lanes_join(s), "bsms_side_lanes_join")
        torch.cuda.synchronize()
        if defer:
            assert all(e.query() for e in evs)                         # every block recorded its entry, frozen or not
        return gh, gpos, grads, mask


UNET_PATTERNS = {
    "all_frozen": lambda H: (lambda k, i: False),
    "all_frozen_null_table": lambda H: (lambda k, i: False),
    "every_other_edge_mlp": lambda H: (lambda k, i: not (k % 2 == 0 and i >= 2 * (H + 1))),
    "block_1_and_3_whole": lambda H: (lambda k, i: k not in (1, 3)),
}


@pytest.mark.parametrize("D", [128, 64])                              # k_edge_bwd and its no-store build; the ring kernel
def test_unet_freeze_patterns(eng, graphs, D):
    u = UnetCase(eng, graphs, D=D)
    want = u.run(lambda k, i: True, defer=False)
    assert all(bool(torch.isfinite(t).all()) for t in (want[0], want[1], *want[2]))
    for defer in (False, True):
        base = u.run(lambda k, i: True, defer)                         # "none": nothing frozen, with and without the deferred join
        assert bit_equal(base[0], want[0]) and bit_equal(base[1], want[1]) and all(bit_equal(a, b) for a, b in zip(base[2], want[2]))
        for name, make in UNET_PATTERNS.items():
            runs = [u.run(make(u.H), defer, whole_null=name.endswith("null_table")) for _ in range(2)]
            for got in runs:
                assert bit_equal(got[0], want[0]), ("grad_h", name, defer)
                assert bit_equal(got[1], want[1]), ("grad_pos", name, defer)
                for t, w, live in zip(got[2], want[2], got[3]):
                    assert bit_equal(t, w) if live else bool(torch.isnan(t).all()), (name, defer)
            assert all(bit_equal(a, b) for a, b in zip(runs[0][2], runs[1][2]))          # two runs


# ------------------------------------------------------------------------------------------------ 5: the fused step
def fresh_model(eng, ref, freeze=()):
    m = eng.BSMS_Simulator(ref.cfg)
    m.load_state_dict(ref.state_dict())
    m = m.cuda()
    for name in freeze:
        getattr(m, name).requires_grad_(False)
    return m


def slots(model, grads, parts=("encode", "decode")):
    out = {}
    for part in parts:
        for k, q in getattr(model, part).named_parameters():
            off, n = grads._slot[q]
            out[f"{part}.{k}"] = grads.flat[off:off + n].clone()
    return out


_STEP_CFGS = [("ring", 1, False, None), ("ring", 2, False, None), ("ring", 2, True, None), ("d64", 1, False, None), ("d64", 2, False, None),
              ("d64", 2, True, "normalized_mse")]


@pytest.mark.parametrize("shape,K,detach,objective", _STEP_CFGS)
def test_fused_step_processor_frozen_and_nothing_trainable(eng, graphs, shape, K, detach, objective):
    ref, data = make_oracle(shape, graphs)
    gdata, w = _cuda(data), [1.0 / K] * K
    later = None if K == 1 else later_targets(gdata[0], gdata[1], K)
    obj = None if objective is None else eng.Objective("normalized", "mse", [1.0, 4.0])
    full = fresh_model(eng, ref)
    assert eng.FusedStep.supports(full)
    _, g_full, s_full = make_step(eng, ref, w, detach, objective=obj, mine=full)
    l_full = run_step(s_full, gdata, later)
    want = dict(loss=l_full.clone(), preds=[q.clone() for q in s_full.predictions()], ig=s_full.input_grad().clone(), slots=slots(full, g_full))
    assert bool(torch.isfinite(want["ig"]).all()) and float(want["ig"].abs().max()) > 0

    part = fresh_model(eng, ref, freeze=("process",))
    assert eng.FusedStep.supports(part)                                # fails on the parent: any frozen parameter meant False
    _, g_part, s_part = make_step(eng, ref, w, detach, objective=obj, mine=part)
    assert g_part.flat.numel() == sum(q.numel() for q in [*part.encode.parameters(), *part.decode.parameters()])
    for _ in range(2):
        g_part.flat.fill_(float("nan"))
        l_part = run_step(s_part, gdata, later)
        assert bit_equal(l_part, want["loss"]) and all(bit_equal(a, b) for a, b in zip(s_part.predictions(), want["preds"]))
        assert bit_equal(s_part.input_grad(), want["ig"])
        got = slots(part, g_part)
        assert got.keys() == want["slots"].keys() and all(bit_equal(got[k], want["slots"][k]) for k in got)
    assert all(q.grad is None for q in part.process.parameters())

    none = fresh_model(eng, ref, freeze=("encode", "process", "decode"))
    g_none = eng.GradBuckets(list(none.parameters()))
    assert g_none.flat.numel() == 0 and g_none.params == []
    with pytest.raises(ValueError, match="nothing is trainable"):
        eng.FusedStep(none, g_none, unroll=K, step_weights=w, detach=detach, objective=obj)(gdata, True, later)
    _, _, s_none = make_step(eng, ref, w, detach, objective=obj, mine=none, grads=g_none)
    for _ in range(2):
        l_none = run_step(s_none, gdata, later)
        assert bit_equal(l_none, want["loss"]) and bit_equal(s_none.input_grad(), want["ig"])
    assert s_none._gscratch is None and all(q.grad is None for q in none.parameters())


def test_nothing_trainable_three_steps(eng, graphs):
    ref, data = make_oracle("ring", graphs)
    gdata, w = _cuda(data), [0.5, 0.3, 0.2]
    later = later_targets(gdata[0], gdata[1], 3)
    _, _, s_full = make_step(eng, ref, w)
    l_full = run_step(s_full, gdata, later)
    none = fresh_model(eng, ref, freeze=("encode", "process", "decode"))
    _, _, s_none = make_step(eng, ref, w, mine=none)
    l_none = run_step(s_none, gdata, later)
    assert bit_equal(l_none, l_full) and bit_equal(s_none.input_grad(), s_full.input_grad())


@pytest.mark.parametrize("freeze", [("process",), ("encode", "process", "decode")], ids=["processor", "everything"])
def test_frozen_graph_replay_equals_eager(eng, graphs, freeze):
    ref, data = make_oracle("ring", graphs)
    gdata = _cuda(data)
    mine = fresh_model(eng, ref, freeze)
    _, grads, eager = make_step(eng, ref, mine=mine)
    _, _, graph = make_step(eng, ref, use_graph=True, mine=mine, grads=grads)
    gen = torch.Generator().manual_seed(11)
    for it in range(3):
        ni = gdata[0].clone()
        ni[..., :2] += 0.05 * it * torch.randn(ni[..., :2].shape, generator=gen).cuda()
        batch = (ni, *gdata[1:])
        l0 = run_step(eager, batch, None)
        flat0, g0 = grads.flat.clone(), eager.input_grad().clone()
        grads.flat.fill_(float("nan"))
        l1 = run_step(graph, batch, None)
        assert bit_equal(l0, l1) and bit_equal(grads.flat, flat0) and bit_equal(graph.input_grad(), g0), it
        assert bool(torch.isfinite(flat0).all())
        if it:
            assert not bit_equal(g0, prev)
        prev = g0


def test_freezing_between_calls_rebuilds_the_tables(eng, graphs):
    """requires_grad_() between two calls of one step: the pointer guard notices it, and a frozen processor's slots stop moving."""
    ref, data = make_oracle("ring", graphs)
    gdata = _cuda(data)
    mine = fresh_model(eng, ref)
    _, grads, step = make_step(eng, ref, mine=mine)
    run_step(step, gdata, None)
    flat0 = grads.flat.clone()
    mine.process.requires_grad_(False)
    grads.flat.fill_(5.0)
    run_step(step, gdata, None)
    for part in ("encode", "decode"):
        for q in getattr(mine, part).parameters():
            off, n = grads._slot[q]
            assert bit_equal(grads.flat[off:off + n], flat0[off:off + n])
    for q in mine.process.parameters():
        off, n = grads._slot[q]
        assert bool((grads.flat[off:off + n] == 5.0).all())           # nothing writes a frozen MLP's slot
    mine.process.bottom_gmp.mlp_edge.seq[0].weight.requires_grad_(True)
    with pytest.raises(ValueError, match="frozen as a whole"):
        step(gdata, True, None)


def test_input_gradient_without_parameter_gradients(eng, graphs):
    ref, data = make_oracle("ring", graphs)
    gdata = _cuda(data)
    later = later_targets(gdata[0], gdata[1], 2)
    model = fresh_model(eng, ref)
    before = [q.detach().clone() for q in model.parameters()]
    loss, got = eng.input_gradient(model, gdata, later_targets=later, param_grad=False)
    torch.cuda.synchronize()
    assert all(q.grad is None for q in model.parameters()) and "grads" not in model._bsms_input_grad_steps
    want_loss, want = eng.input_gradient(fresh_model(eng, ref), gdata, later_targets=later, param_grad=True)
    torch.cuda.synchronize()
    assert bit_equal(loss, want_loss) and bit_equal(got, want)
    l1, g1 = eng.input_gradient(model, gdata, param_grad=False)         # K = 1
    w1, x1 = eng.input_gradient(model, gdata)                           # then with weight gradients, on the same model: its own step
    torch.cuda.synchronize()
    assert bit_equal(l1, w1) and bit_equal(g1, x1)
    assert len([k for k in model._bsms_input_grad_steps if k != "grads"]) == 3
    assert all(q.grad is not None for q in model.parameters() if q.requires_grad)
    assert all(bit_equal(a, b) for a, b in zip(model.parameters(), before))


# ------------------------------------------------------------------------------------------------ 6: the autograd route
@pytest.mark.parametrize("shape", ["ring", "d64"])
def test_autograd_route_with_a_frozen_processor(eng, graphs, shape):
    ref, data = make_oracle(shape, graphs)
    gdata = _cuda(data)

    def run(freeze):
        m = fresh_model(eng, ref, freeze)
        ni = gdata[0].clone().requires_grad_(True)
        eng.masked_rmse(m((ni, *gdata[1:]), True, False), gdata[1], gdata[2]).backward()
        torch.cuda.synchronize()
        return m, ni.grad.detach()

    full, want = run(())
    part, got = run(("process",))
    assert all(q.grad is None for q in part.process.parameters())     # on the parent they were all formed and then dropped by autograd
    assert bit_equal(got, want)
    for name in ("encode", "decode"):
        for (k, a), (_, b) in zip(getattr(part, name).named_parameters(), getattr(full, name).named_parameters()):
            assert a.grad is not None and bit_equal(a.grad, b.grad), (name, k)
    # one MLP of one block, and a mixed MLP (which keeps every gradient of that MLP)
    m = fresh_model(eng, ref)
    m.process.down_gmps[0].mlp_edge.requires_grad_(False)
    m.process.up_gmps[0].mlp_node.seq[0].bias.requires_grad_(False)
    ni = gdata[0].clone().requires_grad_(True)
    eng.masked_rmse(m((ni, *gdata[1:]), True, False), gdata[1], gdata[2]).backward()
    torch.cuda.synchronize()
    assert bit_equal(ni.grad, want)
    for (k, a), (_, b) in zip(m.named_parameters(), full.named_parameters()):
        if a.requires_grad:
            assert bit_equal(a.grad, b.grad), k
        else:
            assert a.grad is None, k


# ------------------------------------------------------------------------------------------------ 7: the Trainer
def test_trainer_with_a_frozen_processor(eng, graphs, tmp_path):
    ref, data = make_oracle("ring", graphs)
    gdata = _cuda(data)
    model_cfg = SimpleNamespace(out_dim=2, latent_dim=32, hidden_layer=3, unet_depth=3, pos_dim=2, consistent_mesh=True, accumulation_steps=1)
    opt_cfg = SimpleNamespace(peak_lr=1e-3, weight_decay=1e-2, warmup_steps=2, decay_steps=20, gnorm_clip=0.0)

    def trainer(freeze):
        torch.manual_seed(0)
        m = eng.BSMS_Simulator(model_cfg)
        m.load_state_dict(ref.state_dict())
        for name in freeze:
            getattr(m, name).requires_grad_(False)
        tr = eng.Trainer(m, model_cfg, opt_cfg)
        tr.iter(gdata)                                                 # warm-up: normaliser statistics only
        tr.lr_scheduler.last_epoch = 1                                 # (the schedule's first factor is 0: nothing would move)
        return tr

    full, part = trainer(()), trainer(("process",))
    assert part.dp.fused is not None                                   # the fused step, not the autograd route
    frozen0 = {k: (q.detach().clone(), q.data_ptr()) for k, q in part.model.process.named_parameters()}
    start = {k: q.detach().clone() for k, q in part.model.named_parameters()}
    l_full, l_part = full.iter(gdata), part.iter(gdata)
    torch.cuda.synchronize()
    assert bit_equal(l_full, l_part)
    for k, q in part.model.process.named_parameters():
        assert bit_equal(q, frozen0[k][0]) and q.data_ptr() == frozen0[k][1] and q.grad is None, k
    moved = 0
    for name in ("encode", "decode"):
        for (k, a), (_, b) in zip(getattr(part.model, name).named_parameters(), getattr(full.model, name).named_parameters()):
            assert bit_equal(a, b), (name, k)                          # AdamW is element-wise without clipping
            moved += int(not bit_equal(a, start[f"{name}.{k}"]))
    assert moved > 0
    part.save(str(tmp_path))
    after = {k: q.detach().clone() for k, q in part.model.named_parameters()}
    part.iter(gdata)
    part.restore(str(tmp_path), 2)
    torch.cuda.synchronize()
    for k, q in part.model.named_parameters():
        assert bit_equal(q, after[k]), k
    for k, q in part.model.process.named_parameters():
        assert q.data_ptr() == frozen0[k][1] and not q.requires_grad, k
    assert part.train_step == 2 and torch.isfinite(part.iter(gdata))


# ------------------------------------------------------------------------------------------------ 8: two ranks
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
    torch.manual_seed(50 + rank)
    sim = eng.BSMS_Simulator(ro.make_cfg(2, 32, 3, 3, 2))
    if rank == 0:
        sim.load_state_dict(z.state_dict())
    sim = sim.cuda()
    sim.process.requires_grad_(False)
    c, sl = (lambda t: t.cuda()), slice(rank, rank + 1)
    data = (c(z.t("node_in")[sl]), c(z.t("tar")[sl]), c(z.t("mask")[sl]), [c(e.unsqueeze(0)) for e in es], [c(i.unsqueeze(0)) for i in ids])
    engine = eng.DataParallel(sim, bucket_bytes=64 << 10, unroll=2, input_grad=True)
    assert engine.fused is not None
    loss = engine.step_loss_backward(data, True, later_targets(data[0], data[1], 2))
    torch.cuda.synchronize()
    torch.save({"loss": loss.detach().cpu(), "flat": engine.grads.flat.cpu()}, f"{out_path}.{rank}")
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.timeout(300)
def test_two_ranks_with_a_frozen_processor(eng, graphs, tmp_path):
    """Two ranks over gloo on one GPU, one golden sample each, K = 2, processor frozen: the all-reduced gradients of the encoder and
    the decoder are those of the single-process step on the whole batch (tolerance of tests/test_hip_unroll.py's two-rank test)."""
    port = 31300 + os.getpid() % 2000
    out = str(tmp_path / "res")
    mp.start_processes(_worker, args=(2, port, out), nprocs=2, join=True, start_method="spawn")
    r0, r1 = torch.load(out + ".0"), torch.load(out + ".1")
    assert torch.equal(r0["flat"], r1["flat"]) and torch.equal(r0["loss"], r1["loss"])
    ref, data = make_oracle("ring", graphs, golden=True)
    mine = fresh_model(eng, ref, freeze=("process",))
    _, grads, step = make_step(eng, ref, [0.5, 0.5], mine=mine)
    loss = run_step(step, _cuda(data), later_targets(data[0], data[1], 2).cuda())
    assert r0["flat"].numel() == grads.flat.numel() > 0
    assert abs(float(r0["loss"]) - float(loss)) < 1e-5 * abs(float(loss))
    assert rel_err(r0["flat"], grads.flat.cpu()) < 2e-5
