"""GPU: frozen MLPs in the bf16 precisions -- BSMS_BWD_FROZEN_BF16 at the U-Net's backward entries, the data-only
fused edge backward (csrc/efuse.hip: k_edge_data_bwd), the bf16-input plain scatter pair (csrc/rowsum.hip: k_rowsum_pair_bf16), and
the Python layers on top (FusedStep, input_gradient(param_grad=False), Trainer, DataParallel).

Every comparison is BIT-EQUALITY against the same build called with nothing frozen: freezing removes launches, stores and the
gradient waves; what is left computes every row as before.  The one distance that cannot be zero, two ranks against one process on
the whole batch (another order of the sums), is the same with and without frozen MLPs; the two-rank test says how it is bounded.
Weights and data are random: bit-equality between two calls of one library needs no ReLU-kink margin."""
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from conftest import ROOT, load_golden, rel_err
from oracle import bsms_oracle as ro
from test_hip_frozen import UNET_PATTERNS, _cus, _stream, _u8, delaunay_edges, fresh_model, slots, table
from test_hip_input_grad import bit_equal, make_step, run_step
from test_hip_unroll import _cuda, later_targets, sim_batch

pytestmark = pytest.mark.gpu
OK, E_UNSUPPORTED = 0, -3
DEFER, RECOMPUTE, LEAN, FROZEN_BF16 = 1, 2, 4, 32
PREC = {"bf16": 1, "bf16_nodes": 2}
TILE = 128                        # csrc/efuse.hip: DT_ROWS, the rows of a tile of k_edge_data_bwd (8 waves x 16)


@pytest.fixture(scope="module")
def eng():
    import bsms_gnn_amd as eng
    return eng


# ------------------------------------------------------------------------------------------------ 1: the raw U-Net entries
class Unet:
    """A U-Net through the raw entries on one set of buffers, in one bf16 precision.  `es` / `ids`: the hierarchy (depth 0: one block)."""

    def __init__(self, eng, es, ids, base, D, H, B, prec, p=2, seed=3):
        from bsms_gnn_amd.ops import _param_ptrs
        depth = len(ids)
        self.eng, self.L, self.D, self.H, self.B, self.depth, self.p, self.prec = eng, eng._abi.lib(), D, H, B, depth, p, prec
        torch.manual_seed(seed)
        self.net = eng.BSGMP(depth, D, H, p).cuda()
        self.n = n = base.shape[0]
        self.h, self.cot = torch.randn(B, n, D).cuda(), torch.randn(B, n, D).cuda()
        self.pos = (base + 0.05 * torch.randn(B, n, p)).cuda().contiguous()
        plans, self.ews, bottom = self.net.prepare([i.cuda() for i in ids], [e.cuda() for e in es], n, torch.device("cuda"))
        self.plans = [*plans, bottom]
        self.pl, self._k1 = eng._abi.ptr_array([q.handle.value if hasattr(q.handle, "value") else q.handle for q in self.plans])
        self.ewp, self._k2 = eng._abi.ptr_array([e.data_ptr() for e in self.ews])
        self.params = self.net.block_params()
        self.pp, self._k3 = _param_ptrs(self.params)
        self.out = torch.empty_like(self.h)
        self.pwork = _u8(self.L.bsms_bsgmp_pos_work_bytes(self.pl, depth, B, p))
        self._bufs = {}

    def sizes(self, flags):
        a = (self.pl, self.depth, self.B, self.D, self.p, self.H, self.prec)
        return self.L.bsms_bsgmp_saved_bytes_ex(*a, flags), self.L.bsms_bsgmp_work_bytes_ex(*a, flags)

    def run(self, live, flags=FROZEN_BF16, whole_null=False, sentinel=float("nan"), expect=OK):
        """Forward, then bsms_bsgmp_bwd_pos_ev with `live(block, entry)` -> the entry is handed over.  `work` is NaN-filled in
        between: the backward reads nothing of it that it has not written."""
        L, s, eng = self.L, _stream(), self.eng
        rec = flags & RECOMPUTE
        if rec not in self._bufs:
            nb = self.sizes(rec)
            assert nb[0] > 0 and nb[1] > 0
            self._bufs[rec] = (_u8(nb[0]), _u8(nb[1]))
        saved, work = self._bufs[rec]
        eng._abi.check(L.bsms_bsgmp_fwd_p(self.pl, self.ewp, self.depth, self.h.data_ptr(), self.pos.data_ptr(), self.B, self.D, self.p,
                                          self.n * self.p, self.H, self.pp, self.out.data_ptr(), saved.data_ptr(), work.data_ptr(),
                                          LEAN if rec else 0, self.prec, s), "bsms_bsgmp_fwd_p")
        work.fill_(0xFF)                                               # every fp32 / bf16 word a NaN
        per = 4 * (self.H + 1)
        fill = lambda t: torch.full_like(t, sentinel)
        gh, gpos, grads = fill(self.h), fill(self.pos), [fill(q) for q in self.params]
        mask = [live(i // per, i % per) for i in range(len(grads))]
        gp, keep = table(eng, grads, mask)
        evs, evp = None, None
        if flags & DEFER:
            evs = [torch.cuda.Event() for _ in range(2 * self.depth + 1)]
            for e in evs:
                e.record()
            evp, keep_ev = eng._abi.ptr_array([e.cuda_event for e in evs])
        rc = L.bsms_bsgmp_bwd_pos_ev(self.pl, self.ewp, self.depth, self.h.data_ptr(), self.pos.data_ptr(), self.cot.data_ptr(), self.B,
                                     self.D, self.p, self.n * self.p, self.H, self.pp, saved.data_ptr(), work.data_ptr(), gh.data_ptr(),
                                     None if whole_null else gp, self.prec, flags, evp, gpos.data_ptr(), self.pwork.data_ptr(), s)
        assert rc == expect, (rc, L.bsms_last_error())
        if flags & DEFER and rc == OK:
            eng._abi.check(L.bsms_side_lanes_join(s), "bsms_side_lanes_join")
        torch.cuda.synchronize()
        if flags & DEFER and rc == OK:
            assert all(e.query() for e in evs)
        return gh, gpos, grads, mask


def check_against(want, got, tag):
    assert bit_equal(got[0], want[0]), ("grad_h", tag)
    assert bit_equal(got[1], want[1]), ("grad_pos", tag)
    for t, w, live in zip(got[2], want[2], got[3]):
        assert bit_equal(t, w) if live else bool(torch.isnan(t).all()), tag       # a frozen slot keeps its sentinel


def all_live(k, i):
    return True


UNET_SHAPES = {"d128_h3": (128, 3), "d128_h2": (128, 2), "d256_h3": (256, 3),     # the fused kernels; the bf16 ring kernels (twice)
               "d128_h5": (128, 5)}                                               # ... and above the fused depth


@pytest.mark.parametrize("prec", list(PREC))
@pytest.mark.parametrize("shape", list(UNET_SHAPES))
def test_unet_freeze_patterns_in_bf16(eng, graphs, shape, prec):
    D, H = UNET_SHAPES[shape]
    es, ids = graphs.levels("del300")
    base = torch.tensor(graphs.np("del300/pos")[:, :2], dtype=torch.float32)
    u = Unet(eng, es[:3], ids[:2], base, D, H, 2, PREC[prec])
    for flags in (0, RECOMPUTE):                                       # the bit changes no size; 64 is unknown
        assert u.sizes(flags | FROZEN_BF16) == u.sizes(flags) and u.sizes(flags | DEFER | FROZEN_BF16) == u.sizes(flags)
    assert u.sizes(64) == (0, 0) and u.sizes(FROZEN_BF16 | 64) == (0, 0)
    want = u.run(all_live, flags=0)                                    # the parent's call
    assert all(bool(torch.isfinite(t).all()) for t in (want[0], want[1], *want[2])) and float(want[1].abs().max()) > 0
    check_against(want, u.run(all_live, flags=FROZEN_BF16), "nothing frozen, with the bit")
    for name, make in UNET_PATTERNS.items():
        whole = name.endswith("null_table")
        for flags in (FROZEN_BF16, FROZEN_BF16 | DEFER, FROZEN_BF16 | RECOMPUTE):
            runs = [u.run(make(H), flags, whole_null=whole) for _ in range(2 if flags == FROZEN_BF16 else 1)]
            for got in runs:
                check_against(want, got, (shape, prec, name, flags))
            if len(runs) == 2:
                assert all(bit_equal(a, b) for a, b in zip(runs[0][2], runs[1][2]))
        # without the bit the same call is refused before any launch: every output keeps its sentinel
        for flags in (0, DEFER, RECOMPUTE):
            got = u.run(make(H), flags, whole_null=whole, sentinel=7.0, expect=E_UNSUPPORTED)
            assert b"fp32" in u.L.bsms_last_error()
            assert all(bool((t == 7.0).all()) for t in (got[0], got[1], *got[2])), (name, flags)


# ------------------------------------------------------------------------------------------------ 2: kernel edges (one block: depth 0)
def ring_edges(n, E, seed):
    """`E` directed edges on `n` nodes: the two directions of a ring, then random chords -- any E, every node with both degrees > 0."""
    rng = np.random.default_rng(seed)
    i = np.arange(n)
    pairs = [np.stack([i, (i + 1) % n]), np.stack([(i + 1) % n, i])]
    while sum(q.shape[1] for q in pairs) < E:
        a, b = rng.integers(0, n, 4 * n), rng.integers(0, n, 4 * n)
        pairs.append(np.stack([a[a != b], b[a != b]]))
    g = np.unique(np.concatenate(pairs, axis=1), axis=1)
    g = g[:, rng.permutation(g.shape[1])]
    assert g.shape[1] >= E
    return torch.tensor(g[:, :E], dtype=torch.int64)


def block_case(eng, g, pos, B, prec, p=2, seed=1):
    return Unet(eng, [g], [], pos, 128, 3, B, PREC[prec], p=p, seed=seed)


EDGE_MLP = lambda k, i: i < 8                                         # the edge MLP of the block frozen (H = 3: entries 8..15)
BLOCK_PATTERNS = {"edge": EDGE_MLP, "node": lambda k, i: i >= 8, "both": lambda k, i: False}


def check_block(u, patterns=BLOCK_PATTERNS):
    want = u.run(all_live, flags=0)
    assert all(bool(torch.isfinite(t).all()) for t in (want[0], want[1], *want[2])) and float(want[1].abs().max()) > 0
    for name, live in patterns.items():
        runs = [u.run(live) for _ in range(2)]
        for got in runs:
            check_against(want, got, (u.B * u.plans[0].E, name))
        assert bit_equal(runs[0][0], runs[1][0]) and bit_equal(runs[0][1], runs[1][1])       # two runs


@pytest.mark.parametrize("prec", list(PREC))
def test_block_with_a_degree_zero_row(eng, prec):
    """Node 0 receives nothing and node 1 sends nothing: empty CSR rows in both halves of the scatter pair."""
    pos, g = delaunay_edges(eng, 300, seed=5)
    g = g[:, (g[1] != 0) & (g[0] != 1)]
    while (3 * g.shape[1]) % 16 in (0, 8):
        g = g[:, :-1]
    u = block_case(eng, g, pos, 3, prec)
    assert u.plans[0].E == g.shape[1] and not bool((g[1] == 0).any()) and not bool((g[0] == 1).any())
    check_block(u)


@pytest.mark.parametrize("B,E", [(2, 50), (1, TILE + 1), (3, TILE), (3, 43), (1, 5)],
                         ids=["below_one_tile", "one_row_past_a_tile", "three_whole_tiles", "one_row_past_a_tile_b3", "five_rows"])
def test_block_tile_edges(eng, B, E):
    n = 40
    assert (B * E < TILE) or (B * E == TILE + 1) or (B * E % TILE == 0)
    g = ring_edges(n, E, seed=E) if E >= 2 * n else ring_edges(n, 2 * n, seed=E)[:, :E]
    pos = torch.rand(n, 2)
    check_block(block_case(eng, g, pos, B, "bf16"), {"edge": EDGE_MLP})


@pytest.mark.parametrize("p", [1, 2, 3])
def test_block_position_widths(eng, p):
    n = 150
    g = ring_edges(n, 700, seed=p)
    check_block(block_case(eng, g, torch.rand(n, p), 2, "bf16", p=p), {"edge": EDGE_MLP, "both": BLOCK_PATTERNS["both"]})


def test_block_with_three_tiles_per_workgroup_and_a_ragged_last_one(eng):
    """B E > 3 x CUs x 128: every workgroup of k_edge_data_bwd runs three tiles or more (the deferred stores of g_0 cross tiles twice),
    and the last tile is ragged."""
    pos, g = delaunay_edges(eng, 2000, seed=9)
    B = 9
    while (B * g.shape[1]) % TILE == 0:
        g = g[:, :-1]
    u = block_case(eng, g, pos, B, "bf16_nodes")
    rows = B * u.plans[0].E
    assert rows > 3 * min(_cus(), 256) * TILE and rows % TILE != 0
    check_block(u, {"edge": EDGE_MLP})


# ------------------------------------------------------------------------------------------------ 3: the fused step
_REF = {}


def make_ref(graphs):
    """The fp32 oracle at D = 128, hidden 3, depth 2 with warmed normalisers, and the golden two-sample batch (built once, never changed)."""
    if not _REF:
        z = load_golden("sim")
        data = sim_batch(graphs, 2)
        torch.manual_seed(11)
        ref = ro.BSMS_Simulator(ro.make_cfg(2, 128, 3, 2, 2))
        for k in range(3):
            ref((z.t(f"warm_in{k}"), z.t(f"warm_tar{k}"), data[2], data[3], data[4]), True, True)
        _REF.update(ref=ref, data=data, gdata=_cuda(data))
    return _REF["ref"], _REF["data"], _REF["gdata"]


def bf_model(eng, ref, prec, freeze=()):
    m = fresh_model(eng, ref, freeze)
    m.process.precision = prec
    return m


FREEZES = {"processor": ("process",), "encoder": ("encode",), "all_but_decoder": ("encode", "process"),
           "nothing_trainable": ("encode", "process", "decode")}
PARTS = ("encode", "process", "decode")


def live_slots(model, grads, freeze):
    return slots(model, grads, tuple(q for q in PARTS if q not in freeze))


@pytest.mark.parametrize("K,detach,objective", [(1, False, None), (2, False, None), (2, True, "normalized_mse")],
                         ids=["k1", "k2_carried", "k2_detached_objective"])
@pytest.mark.parametrize("prec", list(PREC))
def test_fused_step_freeze_patterns(eng, graphs, prec, K, detach, objective):
    ref, _, gdata = make_ref(graphs)
    w = [1.0 / K] * K
    later = None if K == 1 else later_targets(gdata[0], gdata[1], K)
    obj = None if objective is None else eng.Objective("normalized", "mse", [1.0, 4.0])
    full = bf_model(eng, ref, prec)
    _, g_full, s_full = make_step(eng, ref, w, detach, objective=obj, mine=full)
    l_full = run_step(s_full, gdata, later)
    assert s_full._frozen_bit == 0
    want = dict(loss=l_full.clone(), preds=[q.clone() for q in s_full.predictions()], ig=s_full.input_grad().clone(),
                slots=slots(full, g_full, PARTS))
    assert bool(torch.isfinite(want["ig"]).all()) and float(want["ig"].abs().max()) > 0
    for name, freeze in FREEZES.items():
        part = bf_model(eng, ref, prec, freeze)
        assert eng.FusedStep.supports(part)                            # fails on the parent: a bf16 precision with anything frozen meant False
        _, g_part, s_part = make_step(eng, ref, w, detach, objective=obj, mine=part)
        for _ in range(2):
            g_part.flat.fill_(float("nan"))
            l_part = run_step(s_part, gdata, later)
            assert s_part._frozen_bit == FROZEN_BF16
            assert bit_equal(l_part, want["loss"]) and all(bit_equal(a, b) for a, b in zip(s_part.predictions(), want["preds"])), name
            assert bit_equal(s_part.input_grad(), want["ig"]), name
            got = live_slots(part, g_part, freeze)
            assert all(bit_equal(got[k], want["slots"][k]) for k in got), name
            assert len(got) == sum(1 for k in want["slots"] if k.split(".")[0] not in freeze)
        assert all(q.grad is None for f in freeze for q in getattr(part, f).parameters())


@pytest.mark.parametrize("prec", list(PREC))
def test_frozen_bf16_graph_replay_equals_eager(eng, graphs, prec):
    ref, _, gdata = make_ref(graphs)
    mine = bf_model(eng, ref, prec, ("process",))
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


def test_freezing_between_calls_rebuilds_the_tables_in_bf16(eng, graphs):
    ref, _, gdata = make_ref(graphs)
    mine = bf_model(eng, ref, "bf16")
    _, grads, step = make_step(eng, ref, mine=mine)
    run_step(step, gdata, None)
    flat0, ig0 = grads.flat.clone(), step.input_grad().clone()
    assert step._frozen_bit == 0
    mine.process.requires_grad_(False)
    grads.flat.fill_(5.0)
    run_step(step, gdata, None)
    assert step._frozen_bit == FROZEN_BF16 and bit_equal(step.input_grad(), ig0)
    for part in ("encode", "decode"):
        for q in getattr(mine, part).parameters():
            off, n = grads._slot[q]
            assert bit_equal(grads.flat[off:off + n], flat0[off:off + n])
    for q in mine.process.parameters():
        off, n = grads._slot[q]
        assert bool((grads.flat[off:off + n] == 5.0).all())           # nothing writes a frozen MLP's slot
    mine.process.requires_grad_(True)                                  # and back: the parent's calls again
    run_step(step, gdata, None)
    assert step._frozen_bit == 0 and bit_equal(grads.flat, flat0)


@pytest.mark.parametrize("prec", list(PREC))
def test_frozen_bf16_with_recompute(eng, graphs, prec):
    ref, _, gdata = make_ref(graphs)
    later = later_targets(gdata[0], gdata[1], 2)
    full = bf_model(eng, ref, prec)
    _, g_full, s_full = make_step(eng, ref, [0.5, 0.5], mine=full)
    l_full = run_step(s_full, gdata, later)
    want = slots(full, g_full)
    part = bf_model(eng, ref, prec, ("process",))
    g_part = eng.GradBuckets(list(part.parameters()))
    s_part = eng.FusedStep(part, g_part, unroll=2, step_weights=[0.5, 0.5], input_grad=True, recompute=True)
    g_part.flat.fill_(float("nan"))
    l_part = run_step(s_part, gdata, later)
    assert bit_equal(l_part, l_full) and bit_equal(s_part.input_grad(), s_full.input_grad())
    got = slots(part, g_part)
    assert got.keys() == want.keys() and all(bit_equal(got[k], want[k]) for k in got)


@pytest.mark.parametrize("prec", list(PREC))
def test_input_gradient_without_parameter_gradients_in_bf16(eng, graphs, prec):
    ref, _, gdata = make_ref(graphs)
    later = later_targets(gdata[0], gdata[1], 2)
    model = bf_model(eng, ref, prec)
    before = [q.detach().clone() for q in model.parameters()]
    loss, got = eng.input_gradient(model, gdata, later_targets=later, param_grad=False)
    torch.cuda.synchronize()
    assert all(q.grad is None for q in model.parameters()) and "grads" not in model._bsms_input_grad_steps
    full = bf_model(eng, ref, prec)
    _, _, s_full = make_step(eng, ref, [0.5, 0.5], mine=full)
    l_full = run_step(s_full, gdata, later)
    assert bit_equal(loss, l_full) and bit_equal(got, s_full.input_grad())
    assert all(bit_equal(a, b) for a, b in zip(model.parameters(), before))


# ------------------------------------------------------------------------------------------------ 4: the Trainer
def test_trainer_with_a_frozen_processor_in_bf16(eng, graphs, tmp_path):
    ref, _, gdata = make_ref(graphs)
    model_cfg = SimpleNamespace(out_dim=2, latent_dim=128, hidden_layer=3, unet_depth=2, pos_dim=2, consistent_mesh=True, accumulation_steps=1)
    opt_cfg = SimpleNamespace(peak_lr=1e-3, weight_decay=1e-2, warmup_steps=2, decay_steps=20, gnorm_clip=0.0)

    def trainer(freeze):
        torch.manual_seed(0)
        m = eng.BSMS_Simulator(model_cfg)
        m.load_state_dict(ref.state_dict())
        m.process.precision = "bf16"
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
    l_full, l_part = full.iter(gdata), part.iter(gdata)                # the first moving iteration: the same weights on both sides
    torch.cuda.synchronize()
    assert bit_equal(l_full, l_part) and part.dp.fused._frozen_bit == FROZEN_BF16
    for name in ("encode", "decode"):
        for (k, a), (_, b) in zip(getattr(part.model, name).named_parameters(), getattr(full.model, name).named_parameters()):
            assert bit_equal(a, b), (name, k)                          # AdamW is element-wise without clipping
    for _ in range(2):
        assert torch.isfinite(part.iter(gdata))
    torch.cuda.synchronize()
    for k, q in part.model.process.named_parameters():                 # three iterations: the frozen parameters have not moved
        assert bit_equal(q, frozen0[k][0]) and q.data_ptr() == frozen0[k][1] and q.grad is None, k
    assert sum(int(not bit_equal(q, start[k])) for k, q in part.model.named_parameters()) > 0
    part.save(str(tmp_path))
    after = {k: q.detach().clone() for k, q in part.model.named_parameters()}
    step = part.train_step
    part.iter(gdata)
    part.restore(str(tmp_path), step)
    torch.cuda.synchronize()
    for k, q in part.model.named_parameters():
        assert bit_equal(q, after[k]), k
    for k, q in part.model.process.named_parameters():
        assert q.data_ptr() == frozen0[k][1] and not q.requires_grad, k
    assert part.train_step == step and torch.isfinite(part.iter(gdata))


# ------------------------------------------------------------------------------------------------ 5: two ranks
def _worker(rank, world, port, state_path, out_path):
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
    data = (c(z.t("node_in")[sl]), c(z.t("tar")[sl]), c(z.t("mask")[sl]), [c(e.unsqueeze(0)) for e in es[:3]], [c(i.unsqueeze(0)) for i in ids[:2]])
    res = {}
    for name, freeze in (("full", False), ("part", True)):
        sim = eng.BSMS_Simulator(ro.make_cfg(2, 128, 3, 2, 2))
        sim.load_state_dict(torch.load(state_path))
        sim = sim.cuda()
        sim.process.precision = "bf16"
        if freeze:
            sim.process.requires_grad_(False)
        engine = eng.DataParallel(sim, bucket_bytes=64 << 10, unroll=2, input_grad=True)
        assert engine.fused is not None
        loss = engine.step_loss_backward(data, True, later_targets(data[0], data[1], 2))
        torch.cuda.synchronize()
        assert engine.fused._frozen_bit == (32 if freeze else 0)
        live = {f"{part}.{k}": engine.grads.flat[engine.grads._slot[q][0]:][:q.numel()].cpu()
                for part in ("encode", "decode") for k, q in getattr(sim, part).named_parameters()}
        res[name] = {"loss": loss.detach().cpu(), "live": live, "flat": engine.grads.flat.cpu(), "ig": engine.fused.input_grad().cpu()}
    torch.save(res, f"{out_path}.{rank}")
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.timeout(300)
def test_two_ranks_with_a_frozen_processor_in_bf16(eng, graphs, tmp_path):
    """Two ranks over gloo on one GPU, one golden sample each, K = 2, bf16.  The frozen-processor engine's loss, input gradient and
    all-reduced encoder / decoder gradients are the nothing-frozen engine's bit for bit, on both ranks, and so are the single-process
    step's on the whole batch.  Two ranks against one process is then the distance it is with nothing frozen; it cannot be zero (the
    loss sums and the weight-gradient sums are formed in another order, and a cotangent that differs in its last fp32 bit moves some
    bf16 roundings of the U-Net's backward by one bf16 step), so it is held to the size of ONE such step, 2^-8 relative -- what the
    gradients would differ by if every rounding had moved.  A missing all-reduce or a wrong sample is O(1)."""
    ref, data, gdata = make_ref(graphs)
    state = str(tmp_path / "state.pt")
    torch.save(ref.state_dict(), state)
    port = 31300 + os.getpid() % 2000
    out = str(tmp_path / "res")
    mp.start_processes(_worker, args=(2, port, state, out), nprocs=2, join=True, start_method="spawn")
    r0, r1 = torch.load(out + ".0"), torch.load(out + ".1")
    for r in (r0, r1):
        assert torch.equal(r["part"]["loss"], r["full"]["loss"]) and bit_equal(r["part"]["ig"], r["full"]["ig"])
        assert r["part"]["live"].keys() == r["full"]["live"].keys()
        assert all(bit_equal(r["part"]["live"][k], r["full"]["live"][k]) for k in r["part"]["live"])
    assert torch.equal(r0["part"]["flat"], r1["part"]["flat"]) and torch.equal(r0["part"]["loss"], r1["part"]["loss"])
    later = later_targets(gdata[0], gdata[1], 2)
    mine = bf_model(eng, ref, "bf16", ("process",))
    _, grads, step = make_step(eng, ref, [0.5, 0.5], mine=mine)
    loss = run_step(step, gdata, later)
    whole = bf_model(eng, ref, "bf16")
    _, g_whole, s_whole = make_step(eng, ref, [0.5, 0.5], mine=whole)
    l_whole = run_step(s_whole, gdata, later)
    one, one_whole = slots(mine, grads), slots(whole, g_whole)
    assert bit_equal(loss, l_whole) and one.keys() == r0["part"]["live"].keys() and all(bit_equal(one[k], one_whole[k]) for k in one)
    assert r0["part"]["flat"].numel() == grads.flat.numel() > 0
    step_bf16 = 2.0 ** -8
    print(f"two ranks against one process: loss {abs(float(r0['part']['loss']) - float(loss)) / abs(float(loss)):.2e}, "
          f"gradients {rel_err(r0['part']['flat'], grads.flat.cpu()):.2e} (bound {step_bf16:.2e})")
    assert abs(float(r0["part"]["loss"]) - float(loss)) < step_bf16 * abs(float(loss))
    assert rel_err(r0["part"]["flat"], grads.flat.cpu()) < step_bf16


# ------------------------------------------------------------------------------------------------ 6: what is called and launched
def test_the_bit_is_passed_exactly_when_something_is_frozen(eng, graphs, monkeypatch):
    L = eng._abi.lib()
    seen = []

    def watched(name, at):
        real = getattr(L, name)

        def f(*a):
            seen.append(a[at])
            return real(*a)
        return f

    monkeypatch.setattr(L, "bsms_bsgmp_bwd_ev", watched("bsms_bsgmp_bwd_ev", 17))
    monkeypatch.setattr(L, "bsms_bsgmp_bwd_pos_ev", watched("bsms_bsgmp_bwd_pos_ev", 17))
    ref, _, gdata = make_ref(graphs)
    for prec, freeze, input_grad, want in (("bf16", (), False, DEFER), ("bf16", (), True, DEFER), ("bf16_nodes", (), True, DEFER),
                                           ("f32", ("process",), True, DEFER), ("bf16", ("process",), False, DEFER | FROZEN_BF16),
                                           ("bf16_nodes", ("encode",), True, DEFER | FROZEN_BF16)):
        seen.clear()
        mine = bf_model(eng, ref, prec, freeze)
        _, _, step = make_step(eng, ref, mine=mine, input_grad=input_grad)
        run_step(step, gdata, None)
        assert seen == [want], (prec, freeze, seen)
    seen.clear()
    mine = bf_model(eng, ref, "bf16", ("process",))
    step = eng.FusedStep(mine, eng.GradBuckets(list(mine.parameters())), unroll=2, step_weights=[0.5, 0.5], input_grad=True, recompute=True)
    run_step(step, gdata, later_targets(gdata[0], gdata[1], 2))
    assert seen == [DEFER | RECOMPUTE | FROZEN_BF16] * 2


def kernel_counts(fn):
    """Kernel name -> launches during fn(), from the profiler's device activity."""
    from torch.profiler import ProfilerActivity, profile
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    counts = {}
    for ev in prof.events():
        if ev.device_type == torch.autograd.DeviceType.CUDA:
            counts[ev.name] = counts.get(ev.name, 0) + 1
    return counts


def test_a_frozen_edge_block_launches_no_reduce_and_no_projection_jobs(eng):
    n = 150
    u = block_case(eng, ring_edges(n, 700, seed=4), torch.rand(n, 2), 2, "bf16")
    u.run(all_live, flags=0)                                           # first launches (module load, LDS attributes) outside the trace
    u.run(EDGE_MLP)
    count = lambda c, key: sum(v for k, v in c.items() if key in k)
    full = kernel_counts(lambda: u.run(all_live, flags=0))
    assert count(full, "k_edge_fused_bwd") == 1 and count(full, "k_ef_reduce") == 1 and count(full, "k_edge_data_bwd") == 0
    assert count(full, "k_rowsum_pair_fiber") == 1 and count(full, "k_rowsum_pair_bf16") == 0
    part = kernel_counts(lambda: u.run(EDGE_MLP))
    assert count(part, "k_edge_data_bwd") == 1 and count(part, "k_edge_fused_bwd") == 0 and count(part, "k_ef_reduce") == 0
    assert count(part, "k_rowsum_pair_bf16") == 1 and count(part, "k_rowsum_pair_fiber") == 0
    # the narrow reduction of the first edge Linear is gone; the projections' two jobs share lane 1's launch with a job of the node MLP
    # (skipped there by the launch's mask), so the launch count can only fall once the node MLP is frozen as well: no k_wgrad* at all
    assert count(part, "k_small_reduce") == 0 < count(full, "k_small_reduce") and 0 < count(part, "k_wgrad") <= count(full, "k_wgrad")
    none = kernel_counts(lambda: u.run(BLOCK_PATTERNS["both"]))
    assert count(none, "k_wgrad") == 0 and count(none, "k_small_reduce") == 0 and count(none, "k_ef_reduce") == 0
    assert count(none, "k_edge_data_bwd") == 1 and count(none, "k_rowsum_pair_bf16") == 1
