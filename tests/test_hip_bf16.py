"""GPU: the BSMS_BF16 precision of the U-Net (include/bsms_hip.h: bsms_precision; BASELINE.json configs[2] and [4]).

The reference has no mixed precision, so this mode has NO reference parity target; what is pinned instead:
  * SEMANTICS: against the CPU emulation of the documented arithmetic (oracle/bf16_oracle.py) -- the oracle's GMP with (a) the weights of the
    D x D Linears of the edge MLP rounded to bf16, (b) the activation entering each of those Linears rounded to bf16,
    (c) the messages rounded to bf16 before the aggregation, everything else fp32.  Forward tolerance 3e-3 of the tensor
    scale (an activation that sits within fp32 round-off of a bf16 rounding boundary may round the other way: one
    such element moves an output by ~2^-9 of one product).
  * ACCURACY vs fp32 (what a user trades): prediction <= 3e-2 of the tensor scale, loss <= 1e-2; every parameter
    gradient of the full-size airfoil step within 5e-2 relative L2 of the fp32 gradient with cosine >= 0.998 (measured
    worst 2.2e-2 / 0.99975, median 7.7e-3; bf16 has 8 significand bits: 2^-9 = 2e-3 per rounding, ~10 roundings deep
    per block, 11 blocks); on a 300-node toy mesh (40 nodes at the bottom level, B=2) 0.25 / 0.97 (measured 0.16 / 0.986).
  * the fused (no autograd) step and the autograd step agree in bf16 mode as they do in fp32."""
import numpy as np
import pytest
import torch

from conftest import load_golden, rel_err
from oracle import bsms_oracle as ro

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    import bsms_gnn_amd as eng
    return eng


from oracle.bf16_oracle import bf16, emulate, restore   # noqa: E402  (the documented arithmetic, stated in oracle/: VERDICT round 4 item 7)


def test_bf16_forward_matches_the_documented_arithmetic(eng, graphs):
    es, ids = graphs.levels("del300")
    torch.manual_seed(0)
    for depth, D in ((0, 128), (2, 128), (2, 256)):     # D = 256 on a small mesh: single-round launches with the deep one-plane ring
        ref = ro.BSGMP(depth, D, 3, 2)
        mine = eng.BSGMP(depth, D, 3, 2)
        mine.load_state_dict(ref.state_dict())
        mine = mine.cuda()
        mine.precision = "bf16"
        h, pos = torch.randn(2, 300, D), graphs.t("del300/pos").float().unsqueeze(0).repeat(2, 1, 1)
        if D == 256:                                    # ... as chosen on this device: one round, six slots where the two-plane ring has four
            from test_chain_launch_host import launch_info
            cus = torch.cuda.get_device_properties(0).multi_processor_count
            for l in range(depth + 1):
                i, f = launch_info(D, 0, "edge bf16", 2 * es[l].shape[1]), launch_info(D, 0, "edge plain stores", 2 * es[l].shape[1])
                assert (i.text, i.nring, f.text, f.nring) == ("chain_fwd bf16", 6, "chain_fwd lone", 4) and i.ntiles <= cus and i.nload == 2, l
        with torch.no_grad():
            want32 = ref(h, ids[:depth], es[: depth + 1], pos)
            want = emulate(ref)(h, ids[:depth], es[: depth + 1], pos)
            got = mine(h.cuda(), [i.cuda() for i in ids[:depth]], [e.cuda() for e in es[: depth + 1]], pos.cuda()).cpu()
        assert rel_err(got, want) < 3e-3, (depth, D)
        assert 1e-4 < rel_err(got, want32) < 3e-2, (depth, D)          # it really is a different precision, and a usable one
        # BSMS_BF16_NODES: the node MLP in bf16 as well, against ITS documented arithmetic
        mine.precision = "bf16_nodes"
        with torch.no_grad():
            want_n = emulate(ref, node_level=True)(h, ids[:depth], es[: depth + 1], pos)
            got_n = mine(h.cuda(), [i.cuda() for i in ids[:depth]], [e.cuda() for e in es[: depth + 1]], pos.cuda()).cpu()
        assert rel_err(got_n, want_n) < 3e-3, (depth, D, "bf16_nodes")
        assert 1e-4 < rel_err(got_n, want32) < 4e-2, (depth, D, "bf16_nodes")
        assert rel_err(got_n, want) > 1e-4                             # and it is not the edge-only precision
        emulate(ref, node_level=False)
        mine.precision = "bf16"
        # training forward (activations saved as bf16) == inference forward, bit for bit
        hh = h.cuda().requires_grad_(True)
        y = mine(hh, [i.cuda() for i in ids[:depth]], [e.cuda() for e in es[: depth + 1]], pos.cuda())
        assert torch.equal(y.detach().cpu(), got)
        y.square().mean().backward()
        assert torch.isfinite(hh.grad).all() and float(hh.grad.abs().max()) > 0


@pytest.mark.parametrize("B", [1, 3])
def test_bf16_resident_kernels_three_dim_mesh_ragged_rows(eng, graphs, B):
    """efwd.hip / efuse.hip on the shapes the airfoil tests never see: pos_dim = 3 (four fiber columns), B * E not a multiple of
    the 16-row forward tile / the 64-row backward tile, a single sample.  Forward against the documented arithmetic
    (oracle/bf16_oracle.py, 3e-3); every gradient against the autograd of that emulation (its casts round the gradients to
    bf16 where the kernels do, up to the order of two roundings): 1e-2 relative L2 for one block, 1e-1 three blocks deep -- an
    indexing or tail bug is an O(1) error in at least one tensor."""
    es, ids = graphs.levels("surf200")
    pos0 = graphs.t("surf200/pos").float()
    n, D = pos0.shape[0], 128
    assert pos0.shape[1] == 3 and (B * es[0].shape[1]) % 64 != 0
    for depth in (0, 1):
        torch.manual_seed(20 + depth)
        ref = ro.BSGMP(depth, D, 3, 3)
        mine = eng.BSGMP(depth, D, 3, 3)
        mine.load_state_dict(ref.state_dict())
        mine = mine.cuda()
        mine.precision = "bf16"
        h, pos, r = torch.randn(B, n, D), pos0.unsqueeze(0).repeat(B, 1, 1), torch.randn(B, n, D)
        emu = emulate(ref)
        hw = h.clone().requires_grad_(True)
        want = emu(hw, ids[:depth], es[: depth + 1], pos)
        (want * r).sum().backward()
        hg = h.cuda().requires_grad_(True)
        got = mine(hg, [i.cuda() for i in ids[:depth]], [e.cuda() for e in es[: depth + 1]], pos.cuda())
        (got * r.cuda()).sum().backward()
        assert rel_err(got.detach().cpu(), want.detach()) < 3e-3, (B, depth)
        gw = {k: p.grad for k, p in emu.named_parameters() if p.grad is not None}
        gg = {k: p.grad.cpu() for k, p in mine.named_parameters() if p.grad is not None}
        assert set(gg) == set(gw)
        gw["input"], gg["input"] = hw.grad, hg.grad.cpu()
        # measured: one block 3.6e-3 / cosine 0.99999; three blocks deep 4.9e-2 / 0.9988 (the emulation rounds a gradient AFTER
        # the product with W^T, the kernels BEFORE it, and the difference compounds through the blocks)
        _grads_close(gg, gw, f"surf200 p=3 B={B} depth={depth} bf16 vs emulation", l2_tol=1e-2 if depth == 0 else 1e-1, cos_tol=0.9999 if depth == 0 else 0.995)
        restore(ref)


def _grads_close(got, want, tag, l2_tol=5e-2, cos_tol=0.998):
    worst_l2, worst_cos, rows = 0.0, 1.0, []
    for k in want:
        a, b = got[k].double().flatten(), want[k].double().flatten()
        l2 = float((a - b).norm() / b.norm().clamp_min(1e-300))
        cos = float(torch.dot(a, b) / (a.norm() * b.norm()).clamp_min(1e-300))
        worst_l2, worst_cos = max(worst_l2, l2), min(worst_cos, cos)
        rows.append((l2, cos, k))
    rows.sort(reverse=True)
    print(f"[{tag}] gradients vs fp32: worst relative L2 {worst_l2:.3e}, worst cosine {worst_cos:.5f}, median L2 "
          f"{float(np.median([r[0] for r in rows])):.3e}; worst tensors: " + ", ".join(f"{k} {l2:.2e}" for l2, _, k in rows[:5]))
    assert worst_l2 < l2_tol and worst_cos > cos_tol, (tag, worst_l2, worst_cos)


def test_bf16_training_step_accuracy_vs_fp32_oracle(eng, graphs):
    """One simulator step (forward + masked RMSE + backward) in bf16 precision against the fp32 CPU oracle."""
    z = load_golden("sim")
    es, ids = graphs.levels("del300")
    B = z.np("node_in").shape[0]
    cfg = ro.make_cfg(2, 128, 3, 3, 2)
    torch.manual_seed(1)
    ref = ro.BSMS_Simulator(cfg)
    m_gs, m_ids = [e.unsqueeze(0).repeat(B, 1, 1) for e in es], [i.unsqueeze(0).repeat(B, 1) for i in ids]
    data = (z.t("node_in"), z.t("tar"), z.t("mask"), m_gs, m_ids)
    ref(data, True, True)
    pred_ref = ref(data, True, False)
    loss_ref = ro.masked_rmse(pred_ref, data[1], data[2])
    loss_ref.backward()
    want = {k: p.grad for k, p in ref.named_parameters() if p.grad is not None}
    mine = eng.BSMS_Simulator(cfg)
    mine.load_state_dict(ref.state_dict())
    mine = mine.cuda()
    mine.process.precision = "bf16"
    gdata = (data[0].cuda(), data[1].cuda(), data[2].cuda(), [g.cuda() for g in m_gs], [i.cuda() for i in m_ids])
    pred = mine(gdata, True, False)
    loss = eng.masked_rmse(pred, gdata[1], gdata[2])
    loss.backward()
    assert rel_err(pred.detach().cpu(), pred_ref.detach()) < 3e-2
    assert abs(float(loss) - float(loss_ref)) < 1e-2 * abs(float(loss_ref))
    got = {k: p.grad.cpu() for k, p in mine.named_parameters() if p.grad is not None}
    assert set(got) == set(want)
    # a 300-node mesh at B=2 leaves ~40 nodes at the bottom level: few rows per weight gradient, little averaging of the
    # bf16 rounding noise (measured worst 0.16 / cosine 0.986 in bottom_gmp; the full-size test below is the tight one)
    _grads_close(got, want, "del300 L=3 D=128 bf16", l2_tol=0.25, cos_tol=0.97)
    # fused step == autograd step in this precision too
    auto = {k: v.clone() for k, v in got.items()}
    mine.zero_grad(set_to_none=True)
    grads = eng.GradBuckets(list(mine.parameters()))
    step = eng.FusedStep(mine, grads)
    l2 = step(gdata, True)
    assert abs(float(l2) - float(loss)) < 1e-6 * abs(float(loss))
    for k, p in mine.named_parameters():   # a 1e-7 difference in the loss gradient moves bf16 roundings: 2^-9 steps, not 2^-24
        if p.requires_grad:
            assert rel_err(p.grad.cpu(), auto[k]) < 5e-3, k


def test_bf16_airfoil_full_size_vs_fp32_engine(eng):
    """BASELINE configs[2] (airfoil B=8, 5 levels, D=128, bf16): same model, same batch, bf16 precision against the fp32
    engine (itself pinned to the oracle by tests/test_hip_fullsize.py)."""
    from bench import build_workload, data_tuple, make_cfg
    wl = build_workload("airfoil", 8, "cuda")
    torch.manual_seed(0)
    sim = eng.BSMS_Simulator(make_cfg(wl["cfg"])).cuda()
    data = data_tuple(wl)
    sim(data, True, True)
    res = {}
    for prec in ("f32", "bf16"):
        sim.process.precision = prec
        sim.zero_grad(set_to_none=True)
        pred = sim(data, True, False)
        loss = eng.masked_rmse(pred, data[1], data[2])
        loss.backward()
        res[prec] = (pred.detach().clone(), float(loss), {k: p.grad.clone() for k, p in sim.named_parameters() if p.grad is not None})
    assert rel_err(res["bf16"][0], res["f32"][0]) < 3e-2
    assert abs(res["bf16"][1] - res["f32"][1]) < 1e-2 * abs(res["f32"][1])
    _grads_close(res["bf16"][2], res["f32"][2], "airfoil B=8 L=5 D=128 bf16 vs fp32 engine")


def _fused_step_both_precisions(eng, kind, batch):
    """One FusedStep (forward + masked RMSE + backward, no autograd: the path bench.py times) per precision on the same
    model and batch; returns {prec: (pred, loss, grads)}."""
    from bench import build_workload, data_tuple, make_cfg
    wl = build_workload(kind, batch, "cuda")
    torch.manual_seed(0)
    sim = eng.BSMS_Simulator(make_cfg(wl["cfg"])).cuda()
    data = data_tuple(wl)
    sim(data, True, True)
    grads = eng.GradBuckets(list(sim.parameters()))
    step = eng.FusedStep(sim, grads)
    res = {}
    for prec in ("f32", "bf16", "bf16_nodes"):
        sim.process.precision = prec
        grads.flat.zero_()
        loss = step(data, True)
        torch.cuda.synchronize()
        res[prec] = (step.prediction().detach().clone(), float(loss),
                     {k: p.grad.detach().clone() for k, p in sim.named_parameters() if p.grad is not None})
    return wl, res


def test_surface_b2_bf16_full_size(eng):
    """BASELINE configs[4] in its STATED precision: inflating-surface stand-in, 16384 nodes, 6 levels, D=256, pos_dim 3,
    B=2 (the per-GPU share of batch 16 over 8 GPUs), bf16 -- through the fused step, against the fp32 engine (itself
    pinned to the oracle at this size by tests/test_hip_fullsize.py::test_surface_b2_step_matches_oracle).  D = 256 takes
    the NB = 16 kernels and the deep one-plane weight ring: the LDS overflow fixed in round 3 showed up only at this size."""
    wl, res = _fused_step_both_precisions(eng, "surface", 2)
    assert wl["levels"][0][0] == 16384 and len(wl["levels"]) == 7 and wl["cfg"]["latent"] == 256 and wl["cfg"]["pos_dim"] == 3
    assert torch.isfinite(res["bf16"][0]).all()
    assert rel_err(res["bf16"][0], res["f32"][0]) < 3e-2
    assert abs(res["bf16"][1] - res["f32"][1]) < 1e-2 * abs(res["f32"][1])
    assert set(res["bf16"][2]) == set(res["f32"][2])
    _grads_close(res["bf16"][2], res["f32"][2], "surface B=2 L=6 D=256 p=3 bf16 vs fp32 engine (fused step)")
    # Round 6 ("What's weak" 1b): prediction and loss of BOTH bf16 precisions also against the INDEPENDENT CPU
    # emulation of the arithmetic (oracle/bf16_oracle.py) at full size, as the airfoil test does -- not only engine against engine
    for prec, node_level in (("bf16", False), ("bf16_nodes", True)):
        pred_e, loss_e = _emulated_prediction("surface", 2, node_level)
        e_pred, e_loss = rel_err(res[prec][0].cpu(), pred_e), abs(res[prec][1] - loss_e) / abs(loss_e)
        print(f"[surface B=2 {prec}] vs CPU emulation: prediction {e_pred:.2e}, loss {e_loss:.2e}")
        assert e_pred < 1e-2 and e_loss < 2e-3, (prec, e_pred, e_loss)


def _emulated_prediction(kind, batch, node_level):
    """Prediction and loss of the CPU emulation (oracle/bf16_oracle.py) on bench.py's workload and seed."""
    from bench import build_workload, data_tuple, make_cfg
    wl = build_workload(kind, batch, "cpu")
    torch.manual_seed(0)
    ref = ro.BSMS_Simulator(make_cfg(wl["cfg"]))
    data = data_tuple(wl)
    ref(data, True, True)
    emulate(ref, node_level=node_level)
    with torch.no_grad():
        pred = ref(data, True, False)
        return pred, float(ro.masked_rmse(pred, wl["target"], wl["mask"]))


def test_airfoil_b8_bf16_fused_step_full_size(eng):
    """configs[2] through the fused step as well (the autograd path is covered above).  Prediction and loss are also held
    against the INDEPENDENT CPU emulation of the precision (oracle/bf16_oracle.py) at full size -- not only against the
    engine's own fp32 run ("What's weak" 1b); gradients stay against the fp32 engine."""
    _, res = _fused_step_both_precisions(eng, "airfoil", 8)
    for prec, node_level in (("bf16", False), ("bf16_nodes", True)):
        pred_e, loss_e = _emulated_prediction("airfoil", 8, node_level)
        e_pred, e_loss = rel_err(res[prec][0].cpu(), pred_e), abs(res[prec][1] - loss_e) / abs(loss_e)
        print(f"[airfoil B=8 {prec}] vs CPU emulation: prediction {e_pred:.2e}, loss {e_loss:.2e}")
        assert e_pred < 1e-2 and e_loss < 2e-3, (prec, e_pred, e_loss)
    assert rel_err(res["bf16"][0], res["f32"][0]) < 3e-2
    assert abs(res["bf16"][1] - res["f32"][1]) < 1e-2 * abs(res["f32"][1])
    _grads_close(res["bf16"][2], res["f32"][2], "airfoil B=8 bf16 vs fp32 engine (fused step)")


def test_bf16_nodes_training_step_small(eng, graphs):
    """BSMS_BF16_NODES on the 300-node golden step: forward / loss within the bf16 tolerances of the fp32 oracle, every
    gradient finite and aligned with the fp32 one, fused step == autograd step."""
    z = load_golden("sim")
    es, ids = graphs.levels("del300")
    B = z.np("node_in").shape[0]
    cfg = ro.make_cfg(2, 128, 3, 3, 2)
    torch.manual_seed(1)
    ref = ro.BSMS_Simulator(cfg)
    m_gs, m_ids = [e.unsqueeze(0).repeat(B, 1, 1) for e in es], [i.unsqueeze(0).repeat(B, 1) for i in ids]
    data = (z.t("node_in"), z.t("tar"), z.t("mask"), m_gs, m_ids)
    ref(data, True, True)
    pred_ref = ref(data, True, False)
    loss_ref = ro.masked_rmse(pred_ref, data[1], data[2])
    loss_ref.backward()
    want = {k: p.grad for k, p in ref.named_parameters() if p.grad is not None}
    mine = eng.BSMS_Simulator(cfg)
    mine.load_state_dict(ref.state_dict())
    mine = mine.cuda()
    mine.process.precision = "bf16_nodes"
    gdata = (data[0].cuda(), data[1].cuda(), data[2].cuda(), [g.cuda() for g in m_gs], [i.cuda() for i in m_ids])
    pred = mine(gdata, True, False)
    loss = eng.masked_rmse(pred, gdata[1], gdata[2])
    loss.backward()
    assert rel_err(pred.detach().cpu(), pred_ref.detach()) < 4e-2
    assert abs(float(loss) - float(loss_ref)) < 2e-2 * abs(float(loss_ref))
    got = {k: p.grad.cpu() for k, p in mine.named_parameters() if p.grad is not None}
    assert set(got) == set(want)
    _grads_close(got, want, "del300 L=3 D=128 bf16_nodes", l2_tol=0.35, cos_tol=0.94)
    auto = {k: v.clone() for k, v in got.items()}
    mine.zero_grad(set_to_none=True)
    grads = eng.GradBuckets(list(mine.parameters()))
    step = eng.FusedStep(mine, grads)
    l2 = step(gdata, True)
    assert abs(float(l2) - float(loss)) < 1e-6 * abs(float(loss))
    for k, p in mine.named_parameters():
        if p.requires_grad:
            assert rel_err(p.grad.cpu(), auto[k]) < 5e-3, k


def test_bf16_nodes_full_size_vs_fp32_engine(eng):
    """BSMS_BF16_NODES at the sizes of BASELINE configs[2] and [4] through the fused step, against the fp32 engine.  Twice the
    bf16 Linears per block of the edge-only precision: the gradient tolerance is stated for THIS mode (relative L2 8e-2,
    cosine 0.996); prediction and loss keep the tolerances of the edge-only precision."""
    for kind, batch in (("airfoil", 8), ("surface", 2)):
        _, res = _fused_step_both_precisions(eng, kind, batch)
        assert torch.isfinite(res["bf16_nodes"][0]).all()
        assert rel_err(res["bf16_nodes"][0], res["f32"][0]) < 3e-2, kind
        assert abs(res["bf16_nodes"][1] - res["f32"][1]) < 1e-2 * abs(res["f32"][1]), kind
        assert set(res["bf16_nodes"][2]) == set(res["f32"][2])
        _grads_close(res["bf16_nodes"][2], res["f32"][2], f"{kind} B={batch} bf16_nodes vs fp32 engine (fused step)", l2_tol=8e-2, cos_tol=0.996)
