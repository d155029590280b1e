"""GPU: hidden-layer depths 4 .. 7 (the envelope is hidden = 1 .. 7: csrc/chain.h kMaxStages) through the MLP, the GMP block, the
U-Net, the fused step, the pack group and the bf16 precisions.  The rest of the suite runs hidden 1, 2 and 3; at hidden = 7 the bound slots
[24 + H], the loader sequences (H + 2 packs of a node chain), the pack table (9 + 4 H = 37 of 40) and the weight-gradient table (2 H + 2 = 16
of 20) are full or nearly so, and the ring phase (packs x chunks modulo the ring depth) and every carve offset differ from those of hidden 3.

  1. blocks against the fp32 CPU oracle at every width, 1e-5 forward and backward as tests/test_hip_widths.py does at depth 3.  Gradient parity
     needs every ReLU input clear of zero (conftest.KinkMargin): a depth-7 net has many, so the shapes are tiny (37 nodes, 150 edges, one
     sample; 90 MLP rows), and EVERY case asserts the margin of the seed it found -- pick_seed returns its best try otherwise;
  2. the U-Net: against the oracle where a kink-free seed exists (D = 32), and one library call == the module tree bit for bit at every width;
  3. the launch regimes of D = 128 at hidden = 7, bit for bit (tests/test_hip_parity.py::test_feature_split_kernels_equal_the_ring_kernels);
  4. the fused step against the autograd step, the pack group against the per-call prepack;
  5. the bf16 precisions off their fused kernels (efuse.hip / efwd.hip are hidden = 3 only);
  6. hidden = 0 and 8 are refused before any launch, and a block's kernels stay inside the buffers its size queries ask for."""
import pytest
import torch

from conftest import KinkMargin, pick_seed, rel_err
from oracle import bsms_oracle as ro
from oracle.bf16_oracle import emulate, restore
from test_hip_widths import random_graph

pytestmark = pytest.mark.gpu
FWD_TOL, BWD_TOL = 1e-5, 1e-5
MARGIN = 1.5e-6
WIDTHS = [32, 64, 96, 128, 160, 192, 224, 256]
N_NODES, N_EDGES = 37, 150        # three 16-row node tiles and ten edge tiles, both ragged; a hub of degree >= 37, 4 targets of degree 0


@pytest.fixture(scope="module")
def eng():
    import bsms_gnn_amd as eng
    return eng


def dev(t):
    return t.cuda()


def load_sd(module, sd):
    module.load_state_dict(dict(sd), strict=True)
    return module.cuda()


def kink_free(build, first):
    """build(seed) -> (oracle, run, ...) of the first seed from `first` whose ReLU inputs all keep MARGIN; the margin is recomputed and
    ASSERTED, since pick_seed hands back its best try when none of them does."""
    seed = pick_seed(lambda s: build(s)[:2], first=first, tries=200, margin=MARGIN)
    made = build(seed)
    with KinkMargin(made[0]) as km, torch.no_grad():
        made[1]()
    assert km.min > MARGIN, ("no kink-free seed", first, seed, km.min)
    return made


def assert_grads(ref, mine, tag):
    for (k, pr), (_, pm) in zip(ref.named_parameters(), mine.named_parameters()):
        assert pm.grad is not None and rel_err(pm.grad.cpu(), pr.grad) < BWD_TOL, (tag, k, rel_err(pm.grad.cpu(), pr.grad))


# ------------------------------------------------------------------------------------------------ 1: blocks against the oracle
def gmp_problem(D, H, p):
    g = random_graph(N_NODES, N_EDGES, seed=D + H, hub=5)

    def build(seed):
        torch.manual_seed(seed)
        ref = ro.GMP(D, H, p)
        x, pos = torch.randn(1, N_NODES, D), torch.rand(1, N_NODES, p)
        return ref, (lambda: ref(x, g, pos)), x, pos

    return g, build


def check_gmp_against_oracle(eng, D, H, p):
    g, build = gmp_problem(D, H, p)
    ref, _, x0, pos0 = kink_free(build, D + H)
    x, pos = x0.clone().requires_grad_(True), pos0.clone().requires_grad_(True)
    y = ref(x, g, pos)
    cot = torch.randn_like(y)
    (y * cot).sum().backward()
    mine = load_sd(eng.GMP(D, H, p), ref.state_dict())
    xd, pd = dev(x0).requires_grad_(True), dev(pos0).requires_grad_(True)
    yd = mine(xd, dev(g), pd)
    (yd * dev(cot)).sum().backward()
    tag = (D, H, p)
    assert rel_err(yd.cpu(), y) < FWD_TOL, (tag, rel_err(yd.cpu(), y))
    assert rel_err(xd.grad.cpu(), x.grad) < BWD_TOL, (tag, rel_err(xd.grad.cpu(), x.grad))
    assert rel_err(pd.grad.cpu(), pos.grad) < BWD_TOL, (tag, rel_err(pd.grad.cpu(), pos.grad))
    assert_grads(ref, mine, tag)
    with torch.no_grad():                         # the inference carve (packs and messages in the gradient scratch) == the training forward
        assert torch.equal(mine(xd.detach(), dev(g), pd.detach()), yd.detach()), tag


@pytest.mark.parametrize("H", [4, 5, 6, 7])
@pytest.mark.parametrize("D", WIDTHS)
def test_gmp_against_oracle(eng, D, H):
    check_gmp_against_oracle(eng, D, H, 2)


def test_gmp_against_oracle_three_dim_positions(eng):
    check_gmp_against_oracle(eng, 64, 7, 3)


MLP_KINDS = {"encoder": lambda D: (3, D, True), "generic": lambda D: (D, D, True), "decoder": lambda D: (D, 3, False)}


def mlp_problem(D, H, kind):
    in_dim, out_dim, ln = MLP_KINDS[kind](D)

    def build(seed):
        torch.manual_seed(seed)
        ref = ro.MLP(in_dim, D, out_dim, H, ln)
        x = torch.randn(2, 45, in_dim)
        return ref, (lambda: ref(x)), x

    return (in_dim, out_dim, ln), build


@pytest.mark.parametrize("H", [4, 7])
@pytest.mark.parametrize("D", [32, 96, 128, 256])
@pytest.mark.parametrize("kind", list(MLP_KINDS))
def test_mlp_against_oracle(eng, kind, D, H):
    (in_dim, out_dim, ln), build = mlp_problem(D, H, kind)
    ref, _, x0 = kink_free(build, D + H)
    x = x0.clone().requires_grad_(True)
    y = ref(x)
    cot = torch.randn_like(y)
    (y * cot).sum().backward()
    mine = load_sd(eng.MLP(in_dim, D, out_dim, H, ln), ref.state_dict())
    xd = dev(x0).requires_grad_(True)
    yd = mine(xd)
    (yd * dev(cot)).sum().backward()
    tag = (kind, D, H)
    assert rel_err(yd.cpu(), y) < FWD_TOL, (tag, rel_err(yd.cpu(), y))
    assert rel_err(xd.grad.cpu(), x.grad) < BWD_TOL, (tag, rel_err(xd.grad.cpu(), x.grad))
    assert_grads(ref, mine, tag)
    with torch.no_grad():
        assert torch.equal(mine(xd.detach()), yd.detach()), tag


# ------------------------------------------------------------------------------------------------ 2: the U-Net
def unet_problem(graphs, D, H, B=1, depth=2):
    es, ids = graphs.levels("del64")
    pos = torch.tensor(graphs.np("del64/pos")[:, :2], dtype=torch.float32)
    n = pos.shape[0]
    pos = pos.expand(B, n, 2).contiguous()
    es, ids = es[: depth + 1], ids[:depth]

    def build(seed):
        torch.manual_seed(seed)
        ref = ro.BSGMP(depth, D, H, 2)
        h = torch.randn(B, n, D)
        return ref, (lambda: ref(h, ids, es, pos)), h

    return es, ids, pos, build


def run_unet(net, h0, ids, es, pos, cot, per_block):
    net.per_block = per_block
    try:
        net.zero_grad(set_to_none=True)
        h = dev(h0).requires_grad_(True)
        args = ([dev(i) for i in ids], [dev(e) for e in es], dev(pos))
        y = net(h, *args)
        (y * dev(cot)).sum().backward()
        with torch.no_grad():
            yi = net(h.detach(), *args)
        return y.detach().clone(), yi.clone(), h.grad.clone(), [q.grad.clone() for q in net.parameters()]
    finally:
        net.per_block = False


def test_unet_against_oracle_at_hidden_7(eng, graphs):
    """ro.BSGMP(2, 32, 7, 2) on the 64-node golden hierarchy, one sample: five blocks of depth 7.  (At D >= 64 this net has no kink-free seed
    among 200, so the wider U-Nets are pinned by section 1 plus the bit equality below.)"""
    D, H = 32, 7
    es, ids, pos, build = unet_problem(graphs, D, H)
    ref, _, h0 = kink_free(build, D + H)
    h = h0.clone().requires_grad_(True)
    y = ref(h, ids, es, pos)
    cot = torch.randn_like(y)
    (y * cot).sum().backward()
    net = load_sd(eng.BSGMP(2, D, H, 2), ref.state_dict())
    yd, yi, gh, grads = run_unet(net, h0, ids, es, pos, cot, per_block=False)
    assert torch.equal(yi, yd)
    assert rel_err(yd.cpu(), y) < FWD_TOL, rel_err(yd.cpu(), y)
    assert rel_err(gh.cpu(), h.grad) < BWD_TOL, rel_err(gh.cpu(), h.grad)
    for (k, pr), gm in zip(ref.named_parameters(), grads):
        assert rel_err(gm.cpu(), pr.grad) < BWD_TOL, (k, rel_err(gm.cpu(), pr.grad))


@pytest.mark.parametrize("H", [5, 7])
@pytest.mark.parametrize("D", WIDTHS)
def test_unet_single_call_equals_module_tree(eng, graphs, D, H):
    """bsms_bsgmp_fwd / _bwd against the per-module tree (test_hip_parity.py::test_bsgmp_single_call_equals_module_tree) at depth: five
    blocks in a row, each with a full pack table and weight-gradient table, in per-block scratch sets carved for this depth."""
    es, ids, pos, build = unet_problem(graphs, D, H, B=2)
    torch.manual_seed(D + H)
    net = eng.BSGMP(2, D, H, 2).cuda()
    h0, cot = torch.randn(2, pos.shape[1], D), torch.randn(2, pos.shape[1], D)
    one, tree = (run_unet(net, h0, ids, es, pos, cot, per_block=mode) for mode in (False, True))
    assert bool(torch.isfinite(one[0]).all()) and float(one[0].abs().max()) > 0
    for k, (a, b) in enumerate(zip(one[:3], tree[:3])):
        assert torch.equal(a, b), ("output", "inference output", "input gradient")[k]
    assert torch.equal(one[0], one[1])                                   # training forward == inference forward
    names = [k for k, _ in net.named_parameters()]
    assert len(one[3]) == len(names) == 5 * 4 * (H + 1)
    for k, a, b in zip(names, one[3], tree[3]):
        assert torch.equal(a, b) and float(a.abs().max()) > 0, k


# ------------------------------------------------------------------------------------------------ 3: launch regimes at D = 128
def test_feature_split_kernels_equal_the_ring_kernels_mlp_at_hidden_7(eng):
    """test_hip_parity.py::test_feature_split_kernels_equal_the_ring_kernels, its MLP half, at hidden = 7: 3000 rows (feature-split forward
    and backward) against the first 3000 of 30000 (ring kernels).  Forward and input gradient bit for bit; the forwards being equal, so are
    the ReLU masks, and the weight gradients differ by their split-K summation order alone: 2e-6 as there."""
    from test_chain_launch_host import launch_info
    torch.manual_seed(21)
    D, H, small, big = 128, 7, 3000, 30000
    for kind in ("encoder", "mlp", "decoder"):       # the launches named above are the ones chosen on this device
        assert [launch_info(D, 0, kind + " training", r, H).text for r in (small, big)] == ["fs_fwd", "chain_fwd"], kind
        assert [launch_info(D, 1, kind, r, H).text for r in (small, big)] == ["fs_bwd", "chain_bwd"], kind
    for in_dim, out_dim, ln in ((3, D, True), (D, D, True), (D, 3, False)):
        mlp = eng.MLP(in_dim, D, out_dim, H, ln).cuda()
        x = torch.randn(big, in_dim, device="cuda")
        with torch.no_grad():
            y_big, y_small = mlp(x), mlp(x[:small].contiguous())
        assert torch.equal(y_big[:small], y_small), (in_dim, out_dim)
        xs = x[:small].clone().requires_grad_(in_dim == D)
        xb = x.clone().requires_grad_(in_dim == D)
        ys, yb = mlp(xs), mlp(xb)
        assert torch.equal(ys.detach(), y_small) and torch.equal(yb.detach()[:small], y_small)
        r = torch.randn(big, out_dim, device="cuda")
        (ys * r[:small]).sum().backward()
        gs = {k: q.grad.clone() for k, q in mlp.named_parameters()}
        mlp.zero_grad(set_to_none=True)
        (yb * torch.cat([r[:small], torch.zeros(big - small, out_dim, device="cuda")])).sum().backward()
        if in_dim == D:
            assert torch.equal(xs.grad, xb.grad[:small]), (in_dim, out_dim)
        for k, q in mlp.named_parameters():
            print(f"[regimes, MLP {in_dim}->{out_dim} hidden 7] {k}: {rel_err(q.grad, gs[k]):.2e}")
            assert rel_err(q.grad, gs[k]) < 2e-6, (in_dim, out_dim, k, rel_err(q.grad, gs[k]))


def test_gmp_launch_regimes_are_bit_equal_at_hidden_7(eng):
    """A GMP block of n = 3000, e = 18000 at hidden = 7: one sample (18000 edge rows: the edge kernels with one row block per wave, 282
    tiles of 4 waves -- one round of resident workgroups, but more than one per CU, so not the single-round build; 3000 node rows:
    feature-split both ways) against the same sample repeated 2, 3 and 6 times -- 36000 and 54000 edge rows (two row blocks per wave, the
    bottom and the top of that window; 6000 node rows: feature-split forward, single-round ring backward; 9000: single-round ring both
    ways), 108000 (several rounds; 18000 node rows: the ring kernel).  Forward and input gradient of every copy of the sample bit for bit
    across all four; weight gradients / B within 2e-6 (equal forwards, equal ReLU masks: split-K order only; measured worst 1.2e-6, so
    the three-way fallback against fp64 was not needed)."""
    from test_chain_launch_host import launch_info
    from test_hip_parity import random_graph as parity_graph
    torch.manual_seed(21)
    D, H, n, e = 128, 7, 3000, 18000
    # the launches named above are the ones chosen on this device: B -> (edge forward, edge backward, node forward, node backward)
    named = {1: ("edge_fwd rb1 save", "edge_bwd rb1 store", "fs_fwd", "fs_bwd"),
             2: ("edge_fwd rb2 save lone", "edge_bwd rb2 store lone", "fs_fwd", "chain_bwd lone"),
             3: ("edge_fwd rb2 save lone", "edge_bwd rb2 store lone", "chain_fwd lone", "chain_bwd lone"),
             6: ("edge_fwd rb1 save", "edge_bwd rb2 store", "chain_fwd", "chain_bwd")}
    for B, want in named.items():
        got = (launch_info(D, 0, "edge training", B * e, H), launch_info(D, 1, "edge", B * e, H),
               launch_info(D, 0, "node training", B * n, H), launch_info(D, 1, "node", B * n, H))
        assert tuple(i.text for i in got) == want, (B, [i.text for i in got])
    g = dev(parity_graph(n, e, 5))
    gmp = eng.GMP(D, H, 2).cuda()
    x6, pos6 = torch.randn(6, n, D, device="cuda"), torch.rand(6, n, 2, device="cuda")
    x1, pos1 = x6[2:3].contiguous(), pos6[2:3].contiguous()
    with torch.no_grad():
        y1 = gmp(x1, g, pos1)
        assert torch.equal(gmp(x6, g, pos6)[2:3], y1)                    # sample 2 of a batch of six different ones

    def step(xx, pp):
        gmp.zero_grad(set_to_none=True)
        xx = xx.clone().requires_grad_(True)
        y = gmp(xx, g, pp)
        (y * y).sum().backward()
        return y.detach(), xx.grad, {k: q.grad.clone() for k, q in gmp.named_parameters()}

    ya, ga, wa = step(x1, pos1)
    assert torch.equal(ya, y1) and bool(torch.isfinite(ga).all())
    for B in (2, 3, 6):
        yb, gb, wb = step(x1.repeat(B, 1, 1).contiguous(), pos1.repeat(B, 1, 1).contiguous())
        for s in range(B):
            assert torch.equal(yb[s:s + 1], ya) and torch.equal(gb[s:s + 1], ga), (B, s)
        for k in wa:
            print(f"[regimes, GMP hidden 7, B = {B}] {k}: {rel_err(wb[k] / B, wa[k]):.2e}")
            assert rel_err(wb[k] / B, wa[k]) < 2e-6, (B, k, rel_err(wb[k] / B, wa[k]))


# ------------------------------------------------------------------------------------------------ 4: step, pack group
@pytest.mark.parametrize("D,H", [(32, 7), (128, 5)])
def test_fused_step_equals_autograd_step(eng, graphs, D, H):
    """test_hip_training.py::test_fused_step_equals_autograd_step at depth: loss and prediction 1e-6, gradients 2e-6, graph replay == eager."""
    from test_hip_training import _sim_batch
    cfg = ro.make_cfg(2, D, H, 3, 2)
    data = _sim_batch(eng, graphs)
    torch.manual_seed(3)
    sim = eng.BSMS_Simulator(cfg).cuda()
    sim(data, True, True)
    sim.zero_grad(set_to_none=True)
    pred = sim(data, True, False)
    loss = eng.masked_rmse(pred, data[1], data[2])
    loss.backward()
    want = {k: p.grad.clone() for k, p in sim.named_parameters() if p.grad is not None}
    sim.zero_grad(set_to_none=True)
    grads = eng.GradBuckets(list(sim.parameters()))
    step = eng.FusedStep(sim, grads)
    got_loss = step(data, True)
    assert abs(float(got_loss) - float(loss)) < 1e-6 * abs(float(loss))
    assert rel_err(step.prediction().cpu(), pred.detach().cpu()) < 1e-6
    assert set(k for k, p in sim.named_parameters() if p.grad is not None) == set(want)
    for k, p in sim.named_parameters():
        if p.requires_grad:
            assert rel_err(p.grad.cpu(), want[k].cpu()) < 2e-6, (k, rel_err(p.grad.cpu(), want[k].cpu()))
    eager = grads.flat.clone()
    gstep = eng.FusedStep(sim, grads, use_graph=True)
    l1 = float(gstep(data, True))
    assert torch.equal(grads.flat, eager) and l1 == float(got_loss)
    data2 = (data[0] * 1.01, data[1], data[2], data[3], data[4])
    l2 = float(gstep(data2, True))                                       # replay with new inputs
    assert l2 == float(step(data2, True)) and l2 != l1


BOUND_BYTES = 32 * 8192 * 4       # chain.h: kBoundSlots x kBoundWidth floats


def zero_runs(buf, at_least):
    """Number of maximal runs of zero bytes of `buf` (uint8) that are at least `at_least` long."""
    z = (buf == 0).to(torch.int8)
    edge = torch.diff(z, prepend=z.new_zeros(1), append=z.new_zeros(1))
    start, stop = (edge == 1).nonzero().flatten(), (edge == -1).nonzero().flatten()
    return int(((stop - start) >= at_least).sum())


def test_pack_group_at_hidden_7(eng, monkeypatch):
    """tests/test_hip_pack_group.py at hidden = 7, D = 128: the group launch writes the 37 packs of each of the five blocks (and the 16 / 17
    of an encoder / decoder) byte for byte as the per-call prepack does -- whole `saved` buffers compared, under two sentinels -- and clears
    all 32 bound slots of every member: after the group launch ALONE each member's `saved` holds a run of kBoundSlots x kBoundWidth x 4 zero
    bytes (a pack has no megabyte of zeros, and nothing else has been written yet)."""
    import test_hip_pack_group as pg
    monkeypatch.setattr(pg, "H", 7)
    L, ck = eng._abi.lib(), eng._abi.check
    unet = pg.UNetCase(eng, 128, 2, seed=7)
    out = pg.check_pairs(unet, "unet hidden 7")
    assert bool(torch.isfinite(out).all()) and float(out.abs().max()) > 0
    enc, dec = pg.MlpCase(eng, 128, 3, 128, 1, seed=8), pg.MlpCase(eng, 128, 128, 3, 0, seed=9)
    for c, tag in ((enc, "encoder hidden 7"), (dec, "decoder hidden 7")):
        y = pg.check_pairs(c, tag)
        assert bool(torch.isfinite(y).all()) and float(y.abs().max()) > 0
    # the bound slots, straight after the group launch
    for byte in pg.SENTINELS:
        saved = [pg._filled(c.saved_bytes, byte) for c in (unet, enc, dec)]
        g = pg.Group(eng)
        ck(L.bsms_pack_group_add_bsgmp(g.h, unet.pl, pg.DEPTH, pg.B, 128, 2, 7, unet.pp, saved[0].data_ptr(), None, unet.prec), "add unet")
        ck(L.bsms_pack_group_add_mlp(g.h, *enc.shape, enc.pp, saved[1].data_ptr(), None), "add encoder")
        ck(L.bsms_pack_group_add_mlp(g.h, *dec.shape, dec.pp, saved[2].data_ptr(), None), "add decoder")
        g.launch()
        g.close()
        assert [zero_runs(s, BOUND_BYTES) for s in saved] == [2 * pg.DEPTH + 1, 1, 1], hex(byte)


# ------------------------------------------------------------------------------------------------ 5: bf16 off the fused path
def rel_l2(a, b):
    a, b = a.double().flatten(), b.double().flatten()
    return float((a - b).norm() / b.norm().clamp_min(1e-300))


@pytest.mark.parametrize("prec", ["bf16", "bf16_nodes"])
@pytest.mark.parametrize("H", [4, 7])
def test_bf16_generic_ring_kernels_off_the_fused_depth(eng, graphs, H, prec):
    """D = 128 in the bf16 precisions at hidden 4 and 7: the generic bf16 ring kernels (efuse.hip / efwd.hip serve hidden = 3 only), one block
    on surf200 (pos_dim 3, ragged rows), one sample -- the shape of test_hip_bf16.py::test_bf16_resident_kernels_three_dim_mesh_ragged_rows.
      * training forward == inference forward, bit for bit;
      * forward against the documented arithmetic (oracle/bf16_oracle.py).  The project's bound is 3e-3 at depth 3.  Deeper, the emulation's
        own rounding-boundary noise is measured here on the CPU -- the distance between emulate(ref)(h) and emulate(ref)(h (1 + 1e-7 randn)) --
        and the bound is max(3e-3, 3 x that noise): the engine re-associates every layer's sums, not only the input.
        Measured (engine against the emulation / the emulation's noise): hidden 4: bf16 1.1e-4 / 9.2e-5, bf16_nodes 1.5e-3 / 1.6e-3 (bound
        4.7e-3); hidden 7: bf16 1.6e-5 / 1.2e-5, bf16_nodes 6.8e-4 / 5.9e-4.  The noise shrinks with depth: 3e-3 stays the bound but for
        bf16_nodes at hidden 4.
      * every gradient finite and non-zero; relative L2 to the fp32 oracle's gradient at most 2 x that of the emulation's autograd, per
        tensor (the kernels round a gradient before the product with W^T, the emulation after it; an indexing error is O(1)).
        Measured: every tensor of every case within 1.1 x.  This test found the bias gradient of the LAST node Linear in bf16_nodes at
        1.8e-3 of the fp32 one at any depth (emulation: 1.0e-3 at hidden 4, 1.7e-4 at hidden 7, ten times closer): it was the column sum of
        the gradient rows as stored in bf16, one 2^-9 rounding per row against a sum that cancels (bf16(g).sum(0) on the CPU: 1.77e-3).
        It is now summed from the unrounded LayerNorm backward (csrc/posgrad.hip: ln_bias_grad) and sits at the emulation's 1.7e-4."""
    es, ids = graphs.levels("surf200")
    pos0 = graphs.t("surf200/pos").float()
    n, D, node_level = pos0.shape[0], 128, prec == "bf16_nodes"
    torch.manual_seed(40 + H)
    ref = ro.BSGMP(0, D, H, 3)
    h, pos, r = torch.randn(1, n, D), pos0.unsqueeze(0), torch.randn(1, n, D)

    def oracle_grads(net):
        net.zero_grad(set_to_none=True)
        hh = h.clone().requires_grad_(True)
        y = net(hh, [], es[:1], pos)
        (y * r).sum().backward()
        return y.detach(), {"input": hh.grad.clone(), **{k: q.grad.clone() for k, q in net.named_parameters()}}

    _, g32 = oracle_grads(ref)
    emu = emulate(ref, node_level=node_level)
    try:
        want, gemu = oracle_grads(emu)
        with torch.no_grad():
            noise = rel_err(emu(h * (1 + 1e-7 * torch.randn_like(h)), [], es[:1], pos), want)
    finally:
        restore(ref)
    mine = eng.BSGMP(0, D, H, 3)
    mine.load_state_dict(ref.state_dict())
    mine = mine.cuda()
    mine.precision = prec
    hg = h.cuda().requires_grad_(True)
    got = mine(hg, [], [es[0].cuda()], pos.cuda())
    (got * r.cuda()).sum().backward()
    with torch.no_grad():
        assert torch.equal(mine(hg.detach(), [], [es[0].cuda()], pos.cuda()), got.detach())
    err, bound = rel_err(got.detach().cpu(), want), max(3e-3, 3.0 * noise)
    print(f"[bf16 depth, hidden {H}, {prec}] forward vs emulation {err:.2e}; emulation's own noise {noise:.2e}; bound {bound:.2e}")
    assert err < bound, (H, prec, err, noise)
    geng = {"input": hg.grad.cpu(), **{k: q.grad.cpu() for k, q in mine.named_parameters()}}
    assert set(geng) == set(g32)
    for k in g32:
        assert bool(torch.isfinite(geng[k]).all()) and float(geng[k].abs().max()) > 0, k
        mine_d, emu_d = rel_l2(geng[k], g32[k]), rel_l2(gemu[k], g32[k])
        print(f"[bf16 depth, hidden {H}, {prec}] {k}: engine {mine_d:.2e}, emulation {emu_d:.2e} of the fp32 gradient")
        assert mine_d <= 2.0 * emu_d, (H, prec, k, mine_d, emu_d)


@pytest.mark.parametrize("D,n", [(128, 4500), (256, 2100)])
def test_bf16_nodes_last_bias_gradient_over_many_rows(eng, D, n):
    """The fp32 bias-gradient sum of bf16_nodes (csrc/posgrad.hip: ln_bias_grad) where its launch is full: 128 workgroups take 8 rows a
    pass at D = 128 and 4 at D = 256, so 4500 / 2100 rows need five passes, the last one ragged (4500 = 8 x 562 + 4).  Same rule as above: the
    distance to the fp32 oracle's gradient at most 2 x the emulation's; a row counted twice or never is O(1 / rows) x rows."""
    H, p = 2, 2
    g = random_graph(n, 3 * n, seed=D, hub=5)
    torch.manual_seed(D)
    ref = ro.BSGMP(0, D, H, p)
    h, pos, r = torch.randn(1, n, D), torch.rand(1, n, p), torch.randn(1, n, D)
    key = f"bottom_gmp.mlp_node.seq.{2 * H}.bias"

    def oracle_bias(net):
        net.zero_grad(set_to_none=True)
        (net(h, [], [g], pos) * r).sum().backward()
        return dict(net.named_parameters())[key].grad.clone()

    b32 = oracle_bias(ref)
    try:
        bemu = oracle_bias(emulate(ref, node_level=True))
    finally:
        restore(ref)
    mine = eng.BSGMP(0, D, H, p)
    mine.load_state_dict(ref.state_dict())
    mine = mine.cuda()
    mine.precision = "bf16_nodes"
    (mine(h.cuda(), [], [g.cuda()], pos.cuda()) * r.cuda()).sum().backward()
    got = dict(mine.named_parameters())[key].grad.cpu()
    mine_d, emu_d = rel_l2(got, b32), rel_l2(bemu, b32)
    print(f"[bf16_nodes last bias, D = {D}, {n} rows] engine {mine_d:.2e}, emulation {emu_d:.2e} of the fp32 gradient")
    assert bool(torch.isfinite(got).all()) and mine_d <= 2.0 * emu_d, (D, n, mine_d, emu_d)


# ------------------------------------------------------------------------------------------------ 6: the edges of the envelope
@pytest.mark.parametrize("hidden", [0, 8])
def test_depths_outside_the_envelope_raise(eng, graphs, hidden):
    """hidden = 0 and 8 through the modules, training and no_grad: BsmsError from the host checks, nothing launched."""
    D = 128
    g = torch.tensor([[0, 1, 2], [1, 2, 0]]).cuda()
    x, pos = torch.randn(1, 3, D).cuda(), torch.rand(1, 3, 2).cuda()
    es, ids = graphs.levels("del64")
    n = graphs.np("del64/pos").shape[0]
    h, hpos = torch.randn(1, n, D).cuda(), torch.tensor(graphs.np("del64/pos")[:, :2], dtype=torch.float32).expand(1, n, 2).contiguous().cuda()
    calls = {
        "MLP": (eng.MLP(D, D, D, hidden, True).cuda(), lambda m, t: m(t.reshape(-1, D)), x),
        "GMP": (eng.GMP(D, hidden, 2).cuda(), lambda m, t: m(t, g, pos), x),
        "BSGMP": (eng.BSGMP(2, D, hidden, 2).cuda(), lambda m, t: m(t, [i.cuda() for i in ids[:2]], [e.cuda() for e in es[:3]], hpos), h),
        "BSGMP depth 0": (eng.BSGMP(0, D, hidden, 2).cuda(), lambda m, t: m(t, [], [es[0].cuda()], hpos), h),
    }
    for name, (module, call, t) in calls.items():
        with pytest.raises(eng._abi.BsmsError, match="hidden"):
            call(module, t.clone().requires_grad_(True))
        with torch.no_grad(), pytest.raises(eng._abi.BsmsError, match="hidden"):
            call(module, t)
    torch.cuda.synchronize()


def test_unet_size_queries_over_the_depth_range(eng, graphs):
    """The U-Net's size queries (they need plans, hence a device): 0 at hidden = 0 and 8, like those of a block, although the level inputs
    they also hold do not depend on the depth; non-zero and strictly increasing over 1 .. 7 -- with hidden = 3 taken out of the `work`
    sizes at D = 128, which also hold the partials of the fused edge backward there (tests/test_layout_host.py has the blocks')."""
    import test_hip_pack_group as pg
    from test_layout_host import increasing_over_the_depths
    L = eng._abi.lib()
    for D, p in ((32, 2), (128, 3), (256, 2)):
        u = pg.UNetCase(eng, D, p)
        for depth in (0, pg.DEPTH):
            a = (u.pl, depth, pg.B, D, p)
            queries = {"saved_bytes": lambda H: L.bsms_bsgmp_saved_bytes(*a, H), "saved_bytes_p": lambda H: L.bsms_bsgmp_saved_bytes_p(*a, H, 0),
                       "work_bytes": lambda H: L.bsms_bsgmp_work_bytes(*a, H), "infer_work_bytes": lambda H: L.bsms_bsgmp_infer_work_bytes(*a, H),
                       "saved_bytes_ex, recompute": lambda H: L.bsms_bsgmp_saved_bytes_ex(*a, H, 0, 2),
                       "work_bytes_ex, recompute": lambda H: L.bsms_bsgmp_work_bytes_ex(*a, H, 0, 2)}
            for name, q in queries.items():
                assert q(0) == 0 and q(8) == 0 and q(-1) == 0, (name, D, depth)
                sizes = [q(H) for H in range(1, 8)]
                lean = name.startswith("saved_bytes_ex")                 # the lean `saved` holds level inputs only: the same at every depth
                assert sizes[0] > 0 or (lean and depth == 0), (name, D, depth)
                assert increasing_over_the_depths(sizes, D, "work" in name) or (lean and len(set(sizes)) == 1), (name, D, depth, sizes)


GUARD = 1 << 16


def test_block_stays_inside_its_queried_buffers_at_hidden_7(eng):
    """bsms_gmp_fwd + bsms_gmp_bwd at hidden = 7, D = 128 on the shape of section 1, with `saved` and `work` of EXACTLY the queried sizes
    inside larger sentinel-filled allocations: the guard bytes in front of and behind both stay untouched (a carve that outgrows its size
    query at depth would run into them), and output and input gradient are those of the module path, bit for bit."""
    D, H, p, B = 128, 7, 2, 1
    L, ck = eng._abi.lib(), eng._abi.check
    s = torch.cuda.current_stream().cuda_stream
    g = random_graph(N_NODES, N_EDGES, seed=D + H, hub=5)
    torch.manual_seed(0)
    mod = eng.GMP(D, H, p).cuda()
    x, pos, cot = torch.randn(B, N_NODES, D).cuda(), torch.rand(B, N_NODES, p).cuda(), torch.randn(B, N_NODES, D).cuda()
    xm = x.clone().requires_grad_(True)
    ym = mod(xm, g.cuda(), pos)
    (ym * cot).sum().backward()
    plan = eng.LevelPlan(g.cuda(), N_NODES)
    params = [*mod.mlp_node.flat_params(), *mod.mlp_edge.flat_params()]
    pp, _k1 = eng._abi.ptr_array([q.data_ptr() for q in params])
    grads = [torch.empty_like(q) for q in params]
    gp, _k2 = eng._abi.ptr_array([t.data_ptr() for t in grads])
    sizes = (L.bsms_gmp_saved_bytes(B, N_NODES, N_EDGES, D, H), L.bsms_gmp_work_bytes(B, N_NODES, N_EDGES, D, H))
    assert min(sizes) > 0 and all(n % 256 == 0 for n in sizes)
    for byte in (0x55, 0xA7):
        outer = [torch.full((GUARD + n + GUARD,), byte, dtype=torch.uint8, device="cuda") for n in sizes]
        saved, work = (o[GUARD:GUARD + n] for o, n in zip(outer, sizes))
        assert saved.data_ptr() % 256 == 0 and work.data_ptr() % 256 == 0
        out, gx = torch.empty_like(x), torch.empty_like(x)
        ck(L.bsms_gmp_fwd(plan.handle, x.data_ptr(), pos.data_ptr(), B, D, p, N_NODES * p, H, pp, out.data_ptr(), saved.data_ptr(),
                          work.data_ptr(), s), "bsms_gmp_fwd")
        ck(L.bsms_gmp_bwd(plan.handle, x.data_ptr(), pos.data_ptr(), cot.data_ptr(), B, D, p, N_NODES * p, H, pp, saved.data_ptr(),
                          work.data_ptr(), gx.data_ptr(), gp, s), "bsms_gmp_bwd")
        torch.cuda.synchronize()
        for o, n, name in zip(outer, sizes, ("saved", "work")):
            assert bool((o[:GUARD] == byte).all()), (name, "front guard", hex(byte))
            assert bool((o[GUARD + n:] == byte).all()), (name, "rear guard", hex(byte))
        assert torch.equal(out, ym.detach()) and torch.equal(gx, xm.grad), hex(byte)
        for q, t in zip(params, grads):
            assert torch.equal(t, q.grad), hex(byte)
