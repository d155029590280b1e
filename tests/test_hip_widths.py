"""Latent widths between the four power-of-two ones: D = 96 / 160 / 192 / 224 (NB = 6 / 10 / 12 / 14 feature blocks) through
every layer that has a width -- MLP, GMP (with the position gradient), BSGMP, BSMS_Simulator, the fused step, inference and
rollout -- against the CPU oracle with the tolerances of test_hip_parity.py.  Widths outside the envelope still raise."""
import numpy as np
import pytest
import torch

from conftest import pick_seed, rel_err
from oracle import bsms_oracle as ro

pytestmark = pytest.mark.gpu
FWD_TOL, BWD_TOL = 1e-5, 1e-5
WIDTHS = [96, 160, 192, 224]


@pytest.fixture(scope="module")
def eng():
    import bsms_gnn_amd as eng
    return eng


def dev(t):
    return t.cuda()


def load_sd(module, sd):
    module.load_state_dict(dict(sd), strict=True)
    return module.cuda()


def random_graph(n, e, seed, hub):
    """Directed multigraph with degree-0 targets (the last n/8 nodes) and one target of degree >= 64."""
    rng = np.random.default_rng(seed)
    src = rng.integers(0, n, e)
    dst = rng.integers(0, n - n // 8, e)
    dst[: e // 4] = hub
    return torch.tensor(np.stack([src, dst]), dtype=torch.int64)


def assert_grads(ref, mine, tag=""):
    for (k, pr), (_, pm) in zip(ref.named_parameters(), mine.named_parameters()):
        assert rel_err(pm.grad.cpu(), pr.grad) < BWD_TOL, (tag, k)


# ------------------------------------------------------------------------------------ MLP
@pytest.mark.parametrize("D", WIDTHS)
@pytest.mark.parametrize("kind", ["encoder", "generic", "decoder"])
def test_mlp_against_oracle(eng, D, kind):
    in_dim, out_dim, ln, rows = {"encoder": (3, D, True, 700), "generic": (D, D, True, 513),
                                 "decoder": (D, 3, False, 600)}[kind]

    def build(seed):
        torch.manual_seed(seed)
        ref = ro.MLP(in_dim, D, out_dim, 3, ln)
        x = torch.randn(2, rows, in_dim, requires_grad=True)
        return ref, (lambda: ref(x)), x

    seed = pick_seed(lambda s: build(s)[:2], first=D + rows)
    ref, _, x = build(seed)
    mine = load_sd(eng.MLP(in_dim, D, out_dim, 3, ln), ref.state_dict())
    cot = torch.randn(2, rows, out_dim)
    y = ref(x)
    (y * cot).sum().backward()
    xd = dev(x.detach()).requires_grad_(True)
    yd = mine(xd)
    (yd * dev(cot)).sum().backward()
    assert rel_err(yd.cpu(), y) < FWD_TOL
    assert rel_err(xd.grad.cpu(), x.grad) < BWD_TOL
    assert_grads(ref, mine, kind)
    with torch.no_grad():                       # inference path (no saved activations) == training forward, bit for bit
        assert torch.equal(mine(xd.detach()), yd.detach())


# ------------------------------------------------------------------------------------ GMP
@pytest.mark.parametrize("D", WIDTHS)
@pytest.mark.parametrize("p", [2, 3])
def test_gmp_against_oracle(eng, D, p):
    n, e, B = 180, 1300, 2
    g = random_graph(n, e, D + p, hub=5)

    def build(seed):
        torch.manual_seed(seed)
        ref = ro.GMP(D, 3, p)
        x, pos = torch.randn(B, n, D), torch.rand(B, n, p)
        return ref, (lambda: ref(x, g, pos)), x, pos

    seed = pick_seed(lambda s: build(s)[:2], first=D)
    ref, _, x0, pos0 = build(seed)
    mine = load_sd(eng.GMP(D, 3, p), ref.state_dict())
    # [B,N,D] with per-sample positions [B,N,p], then [N,D] with [N,p]
    for x_b, pos_b in ((x0, pos0), (x0[0], pos0[0])):
        ref.zero_grad()
        mine.zero_grad()
        x = x_b.clone().requires_grad_(True)
        pos = pos_b.clone().requires_grad_(True)
        y = ref(x, g, pos)
        cot = torch.randn_like(y)
        (y * cot).sum().backward()
        xd = dev(x.detach()).requires_grad_(True)
        pd = dev(pos.detach()).requires_grad_(True)
        yd = mine(xd, dev(g), pd)
        (yd * dev(cot)).sum().backward()
        tag = tuple(x.shape)
        assert rel_err(yd.cpu(), y) < FWD_TOL, tag
        assert rel_err(xd.grad.cpu(), x.grad) < BWD_TOL, tag
        assert rel_err(pd.grad.cpu(), pos.grad) < BWD_TOL, tag
        assert_grads(ref, mine, tag)
        with torch.no_grad():
            assert torch.equal(mine(xd.detach(), dev(g), pd.detach()), yd.detach()), tag


# ------------------------------------------------------------------------------------ BSGMP
def _hierarchy(eng, n, depth, seed):
    from scipy.spatial import Delaunay
    pts = np.random.default_rng(seed).random((n, 2))
    flat = eng.to_flat_edge(Delaunay(pts).simplices.astype(np.int64), "tri")
    _, m_es, m_ids = eng.BistrideMultiLayerGraph(flat, depth, n, pts).get_multi_layer_graphs()
    return pts, [torch.tensor(e) for e in m_es], [torch.tensor(i) for i in m_ids]


@pytest.mark.parametrize("D", WIDTHS)
def test_bsgmp_against_oracle_and_single_call_equals_module_tree(eng, D):
    depth, B, n = 3, 1, 200     # few ReLU inputs: a seed whose pre-activations all keep the margin of pick_seed exists
    pts, es, ids = _hierarchy(eng, n, depth, D)
    pos = torch.tensor(pts, dtype=torch.float32).expand(B, n, 2).contiguous()

    def build(seed):
        torch.manual_seed(seed)
        ref = ro.BSGMP(depth, D, 3, 2)
        h = torch.randn(B, n, D)
        return ref, (lambda: ref(h, ids[:depth], es[: depth + 1], pos)), h

    seed = pick_seed(lambda s: build(s)[:2], first=D)
    ref, _, h0 = build(seed)
    h = h0.clone().requires_grad_(True)
    y = ref(h, ids[:depth], es[: depth + 1], pos)
    cot = torch.randn_like(y)
    (y * cot).sum().backward()
    net = load_sd(eng.BSGMP(depth, D, 3, 2), ref.state_dict())
    res = {}
    for mode in (False, True):
        net.per_block = mode
        try:
            net.zero_grad()
            hd = dev(h0).requires_grad_(True)
            yd = net(hd, [dev(i) for i in ids[:depth]], [dev(e) for e in es[: depth + 1]], dev(pos))
            (yd * dev(cot)).sum().backward()
            res[mode] = (yd.detach().clone(), hd.grad.clone(), [q.grad.clone() for q in net.parameters()])
        finally:
            net.per_block = False
    a, b = res[False], res[True]
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    assert all(torch.equal(u, v) for u, v in zip(a[2], b[2]))
    assert rel_err(a[0].cpu(), y) < FWD_TOL
    assert rel_err(a[1].cpu(), h.grad) < BWD_TOL
    for (k, pr), gm in zip(ref.named_parameters(), a[2]):
        assert rel_err(gm.cpu(), pr.grad) < BWD_TOL, k


# ------------------------------------------------------------------------------------ BSMS_Simulator
def _sim_problem(eng, D, B=2, n=160, depth=3, C=2):
    pts, es, ids = _hierarchy(eng, n, depth, 7)
    cfg = ro.make_cfg(C, D, 3, depth, 2)
    gs = [e.unsqueeze(0).repeat(B, 1, 1) for e in es]
    iis = [i.unsqueeze(0).repeat(B, 1) for i in ids]

    def build(seed):
        torch.manual_seed(seed)
        ref = ro.BSMS_Simulator(cfg)
        state = torch.randn(B, n, C)
        node_in = torch.cat([state, torch.tensor(pts, dtype=torch.float32).expand(B, n, 2), torch.zeros(B, n, 1)], -1)
        tar, mask = state + 0.1 * torch.randn(B, n, C), torch.ones(B, n, 1)
        mask[:, :10] = 0
        data = (node_in, tar, mask, gs, iis)
        ref(data, True, True)                   # one normaliser accumulation
        return ref, (lambda: ref(data, True, False)), data

    seed = pick_seed(lambda s: build(s)[:2], first=D)
    return cfg, build(seed)


@pytest.mark.parametrize("D", WIDTHS)
def test_simulator_step_fused_step_graph_and_rollout(eng, D):
    cfg, (ref, _, data) = _sim_problem(eng, D)
    loss_ref = ro.masked_rmse(ref(data, True, False), data[1], data[2])
    pred_ref = ref(data, True, False).detach()
    loss_ref.backward()
    sim = eng.BSMS_Simulator(cfg)
    sim.load_state_dict(ref.state_dict())
    sim = sim.cuda()
    gd = (dev(data[0]), dev(data[1]), dev(data[2]), [dev(g) for g in data[3]], [dev(i) for i in data[4]])
    # autograd step against the oracle
    pred = sim(gd, True, False)
    loss = eng.masked_rmse(pred, gd[1], gd[2])
    loss.backward()
    assert rel_err(pred.detach().cpu(), pred_ref) < FWD_TOL
    assert abs(float(loss) - float(loss_ref)) < 1e-5 * abs(float(loss_ref))
    want = {}
    for (k, pr), (_, pm) in zip(ref.named_parameters(), sim.named_parameters()):
        if pr.grad is not None:
            assert rel_err(pm.grad.cpu(), pr.grad) < BWD_TOL, k
            want[k] = pm.grad.clone()
    # inference forward == training forward, bit for bit
    with torch.no_grad():
        assert torch.equal(sim(gd, True, False), pred.detach())
    # the fused step (eager, then HIP graph) == the autograd step
    sim.zero_grad(set_to_none=True)
    grads = eng.GradBuckets(list(sim.parameters()))
    step = eng.FusedStep(sim, grads)
    got = step(gd, True)
    assert abs(float(got) - float(loss)) < 1e-6 * abs(float(loss))
    assert rel_err(step.prediction().cpu(), pred.detach().cpu()) < 1e-6
    for k, p in sim.named_parameters():
        if p.requires_grad:
            assert rel_err(p.grad.cpu(), want[k].cpu()) < 2e-6, k
    eager = grads.flat.clone()
    gstep = eng.FusedStep(sim, grads, use_graph=True)
    assert float(gstep(gd, True)) == float(got) and torch.equal(grads.flat, eager)
    # rollout: HIP graph == eager, 5 steps
    with torch.no_grad():
        ic, rmask = gd[0][:1], gd[2][:1]
        g1, i1 = [g[:1] for g in gd[3]], [i[:1] for i in gd[4]]
        outs = []
        for use_graph in (False, True):
            res = torch.zeros(5, ic.shape[1], 2, device="cuda")
            eng.rollout_one_traj(sim, ic, res, rmask, g1, i1, use_graph=use_graph)
            outs.append(res)
    assert torch.isfinite(outs[0]).all() and torch.equal(outs[0], outs[1])


# ------------------------------------------------------------------------------------ full size
def test_airfoil_b8_step_at_d192_matches_oracle(eng):
    from test_hip_fullsize import check, run_config
    from bench import WORKLOADS
    w = dict(WORKLOADS["airfoil"], latent=192)
    r = run_config(eng, "airfoil", 8, "dense", cfg=w)
    assert r["levels"][0] == (5233, 31354) and len(r["levels"]) == 6
    check(r, "airfoil B=8 L=5 D=192")


# ------------------------------------------------------------------------------------ refusals
@pytest.mark.parametrize("D", [48, 80, 288, 512])
def test_widths_outside_the_envelope_raise(eng, D):
    g = torch.tensor([[0, 1], [1, 0]]).cuda()
    with pytest.raises(eng._abi.BsmsError):
        eng.GMP(D, 1, 2).cuda()(torch.zeros(2, D).cuda(), g, torch.zeros(2, 2).cuda())
    with pytest.raises(eng._abi.BsmsError):
        eng.MLP(D, D, D, 2, True).cuda()(torch.zeros(5, D).cuda())


@pytest.mark.parametrize("D", [96, 192])
def test_bf16_precision_at_new_widths_raises(eng, D, monkeypatch):
    monkeypatch.setenv("BSMS_PRECISION", "bf16")
    cfg, (ref, _, data) = _sim_problem(eng, D)
    sim = eng.BSMS_Simulator(cfg)
    sim.load_state_dict(ref.state_dict())
    sim = sim.cuda()
    gd = (dev(data[0]), dev(data[1]), dev(data[2]), [dev(g) for g in data[3]], [dev(i) for i in data[4]])
    with pytest.raises(eng._abi.BsmsError):
        sim(gd, True, False)
    torch.cuda.synchronize()
