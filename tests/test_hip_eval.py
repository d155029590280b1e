"""GPU: on-device evaluation -- the masked error sums kernel (csrc/errsum.hip) against its NumPy fp64 restatement
(test_eval_host.np_error_sums), `Trainer.get_error` against the reference's figures (tests/golden/eval_err.npz) and against the
formula evaluated on the host, and `rollout_bank` (batched rollouts of a TrajectoryBank with the statistics taken on the device)
against `rollout_dataset` over the bank's one-at-a-time materialised trajectories."""
import numpy as np
import pytest
import torch

from conftest import load_golden, rel_err
from test_datapipe import cfg as make_cfg, synthetic_traj
from test_eval_host import CASES, REL_TOL, RMSE_TOL, np_error_sums, rel
from test_hip_databank import OPT, model_cfg, same_mesh_trajs

pytestmark = pytest.mark.gpu

SUM_TOL = 1e-12         # fp64 sums of at most 5000 non-negative terms taken in another order
FWD_TOL = 1e-5          # the project's forward tolerance (tests/test_hip_parity.py)


@pytest.fixture(scope="module")
def eng():
    import bsms_gnn_amd as eng
    return eng


def np_mean_std(sums, n, relative):
    """eval.error_mean_std restated in NumPy fp64."""
    c = (sums.shape[1] - 1) // 3
    M, SE, AE, TT = sums[:, :1], sums[:, 1:1 + c], sums[:, 1 + c:1 + 2 * c], sums[:, 1 + 2 * c:]
    scale = np.sqrt(TT / (M + 1e-6)) + 1e-6 if relative else np.ones_like(TT)
    mean = (AE / scale).sum(0) / (sums.shape[0] * n)
    e2 = (SE / scale ** 2).sum(0) / (sums.shape[0] * n)
    return mean, np.sqrt(np.maximum(e2 - mean ** 2, 0.0))


def segments(S, n, C, seed):
    """pred as the MIDDLE column block of a wider [S, 3, n, C] tensor (segments 3 n rows apart, as rollout_bank reads its
    results), a contiguous target, and 0/1 masks per segment."""
    rng = np.random.default_rng(seed)
    wide = torch.tensor(rng.standard_normal((S, 3, n, C)).astype(np.float32)).cuda()
    target = torch.tensor((rng.standard_normal((S, n, C)) * 3).astype(np.float32)).cuda()
    mask = torch.tensor((rng.random((S, n)) < 0.7).astype(np.float32)).cuda()
    return wide, wide[:, 1], target, mask


@pytest.mark.parametrize("S", [1, 70])
@pytest.mark.parametrize("C", [1, 3, 8])
@pytest.mark.parametrize("n", [1, 255, 256, 257, 5000])
def test_error_sums_against_numpy_fp64(eng, n, C, S):
    wide, pred, target, mask = segments(S, n, C, seed=1000 * n + 10 * C + S)
    assert pred.stride(0) == 3 * n * C and pred.data_ptr() != wide.data_ptr()
    p, t, m = pred.cpu().numpy(), target.cpu().numpy(), mask.cpu().numpy()
    for what, got, want in (
            ("mask per segment", eng.error_sums(pred, target, mask, n), np_error_sums(p, t, m)),
            ("explicit strides", eng.error_sums(pred, target, mask, n, pred_stride=3 * n, target_stride=n, mask_stride=n), np_error_sums(p, t, m)),
            ("one mask, stride 0", eng.error_sums(pred, target, mask[0], n, mask_stride=0), np_error_sums(p, t, m[0])),
            ("expanded mask", eng.error_sums(pred, target, mask[:1].expand(S, n), n), np_error_sums(p, t, m[0])),
            ("contiguous pred", eng.error_sums(pred.contiguous(), target, mask.unsqueeze(-1), n), np_error_sums(p, t, m))):
        assert got.dtype == torch.float64 and got.shape == (S, 1 + 3 * C) and got.is_cuda, what
        err = rel(got.cpu().numpy(), want)
        assert err <= SUM_TOL, (what, err)
    assert torch.equal(wide[:, 1], pred) and bool((wide[:, 0] != wide[:, 2]).any())


def test_error_sums_edge_cases(eng):
    from bsms_gnn_amd import _abi
    _, pred, target, mask = segments(4, 300, 3, seed=5)
    got = eng.error_sums(pred, target, torch.zeros_like(mask), 300)                 # an all-zero mask
    want = np_error_sums(pred.cpu().numpy(), target.cpu().numpy(), np.zeros((4, 300), np.float32))
    assert bool((got == 0).all()) and not want.any()
    # masks other than 0/1 weight all four sums
    soft = torch.rand(4, 300, device="cuda")
    err = rel(eng.error_sums(pred, target, soft, 300).cpu().numpy(), np_error_sums(pred.cpu().numpy(), target.cpu().numpy(), soft.cpu().numpy()))
    assert err <= SUM_TOL, err
    # seg_rows = 0 writes zeros (at the C ABI, into a buffer that held something else); S = 0 touches nothing
    sums = torch.ones(3, 7, device="cuda", dtype=torch.float64)
    s = torch.cuda.current_stream().cuda_stream
    assert _abi.lib().bsms_error_sums(None, None, None, 3, 0, 2, 0, 0, 0, sums.data_ptr(), None, s) == 0
    assert bool((sums == 0).all())
    sums.fill_(1.0)
    assert _abi.lib().bsms_error_sums(None, None, None, 0, 5, 2, 5, 5, 5, sums.data_ptr(), None, s) == 0
    assert bool((sums == 1).all())
    empty = eng.error_sums(torch.zeros(3, 0, 2, device="cuda"), torch.zeros(3, 0, 2, device="cuda"), torch.zeros(3, 0, device="cuda"), 0)
    assert empty.shape == (3, 7) and bool((empty == 0).all())
    # the wrapper refuses what it cannot read as segments, before anything is launched
    with pytest.raises(ValueError):
        eng.error_sums(pred.transpose(1, 2), target, mask, 300)
    with pytest.raises(ValueError):
        eng.error_sums(pred, target, mask, 300, pred_stride=10 ** 6)                # reaches past the storage
    with pytest.raises(eng._abi.BsmsError):
        eng.error_sums(torch.zeros(2, 5, 9, device="cuda"), torch.zeros(2, 5, 9, device="cuda"), torch.ones(2, 5, device="cuda"), 5)


def test_error_sums_are_bit_identical(eng):
    """Run to run, and whatever else is in the launch: segment 3 of 70 == the same rows alone, from another layout."""
    _, pred, target, mask = segments(70, 5000, 3, seed=11)
    a, b = eng.error_sums(pred, target, mask, 5000), eng.error_sums(pred, target, mask, 5000)
    assert torch.equal(a, b)
    alone = eng.error_sums(pred[3:4].contiguous(), target[3:4].clone(), mask[3].clone(), 5000)
    assert alone.shape == (1, 10) and torch.equal(alone[0], a[3])
    shared = eng.error_sums(pred, target, mask[3], 5000, mask_stride=0)
    assert torch.equal(shared[3], a[3]) and not torch.equal(shared[4], a[4])


def test_error_sums_capture_into_a_graph(eng):
    _, pred, target, mask = segments(6, 1500, 3, seed=12)
    eager = eng.error_sums(pred, target, mask, 1500)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                       # warm-up outside capture, as rollout._Stepper does
        eng.error_sums(pred, target, mask, 1500)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = eng.error_sums(pred, target, mask, 1500)
    out.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager)


@pytest.mark.parametrize("case", CASES)
def test_fixture_on_the_gpu(eng, case):
    z = load_golden("eval_err")
    pred, target, mask = z.t(f"{case}/pred").cuda(), z.t(f"{case}/target").cuda(), z.t(f"{case}/mask").cuda()
    sums = eng.error_sums(pred, target, mask, pred.shape[1])
    assert rel(sums.cpu().numpy(), np_error_sums(pred.cpu().numpy(), target.cpu().numpy(), mask.cpu().numpy()[..., 0])) <= SUM_TOL
    for relative, tag in ((True, "rel"), (False, "abs")):
        mean, std = eng.error_mean_std(sums, pred.shape[1], relative=relative)
        assert mean.is_cuda and mean.dtype == torch.float64
        e_mean, e_std = rel(mean.cpu().numpy(), z.np(f"{case}/{tag}/mean")), rel(std.cpu().numpy(), z.np(f"{case}/{tag}/std"))
        print(f"[get_error figures vs reference] {case} relative={relative}: mean {e_mean:.2e} std {e_std:.2e} (bound {REL_TOL:.0e})")
        assert e_mean <= REL_TOL and e_std <= REL_TOL


def check_get_error(tr, data, pred_shape):
    """get_error of `data` against the sums formula in NumPy fp64 on tr.get_pred(data); returns the relative=True figures."""
    with torch.no_grad():
        pred = tr.get_pred(data)
    tar, mask = tr.get_label_mask(data)
    assert tuple(pred.shape) == pred_shape
    S, n, c = pred_shape
    sums = np_error_sums(pred.cpu().numpy(), tar.cpu().numpy().reshape(S, n, c), mask.cpu().numpy().reshape(S, n))
    out = {}
    for relative in (True, False):
        mean, std = tr.get_error(data, relative=relative)
        assert isinstance(mean, np.ndarray) and mean.dtype == std.dtype == np.float32 and mean.shape == std.shape == (c,)
        want_mean, want_std = np_mean_std(sums, n, relative)
        e_mean, e_std = rel(mean, want_mean), rel(std, want_std)
        print(f"[Trainer.get_error vs NumPy fp64] {pred_shape} relative={relative}: mean {e_mean:.2e} std {e_std:.2e} (bound {REL_TOL:.0e})")
        assert np.isfinite(mean).all() and np.isfinite(std).all() and e_mean <= REL_TOL and e_std <= REL_TOL
        out[relative] = mean
    assert not np.allclose(out[True], out[False])
    return out[True]


def test_trainer_get_error_consistent_mesh(eng):
    bank = eng.TrajectoryBank(make_cfg(True), dataset="airfoil", seed=3)
    for t in same_mesh_trajs(120, 6, 3, seed=9):
        bank.add(t)
    torch.manual_seed(0)
    mcfg = model_cfg(True)
    tr = eng.Trainer(eng.BSMS_Simulator(mcfg), mcfg, OPT)
    data = bank.batch([(0, 2), (1, 1), (2, 4)], train=False)
    warm = check_get_error(tr, data, (3, 120, 3))                             # warm-up: the prediction is zeros, as in the reference
    with torch.no_grad():
        assert not bool(tr.get_pred(data).any())
    tr.iter(bank.batch([(0, 0), (1, 0), (2, 0)], train=False))                # the warm-up step
    assert tr.iter(bank.batch([(0, 1), (1, 2), (2, 3)], train=False)) is not None
    trained = check_get_error(tr, data, (3, 120, 3))
    assert not np.allclose(warm, trained)


def test_trainer_get_error_variable_meshes(eng):
    """The block-diagonal batch is ONE segment of sum N rows (the reference sees it as [1, sum N, C])."""
    torch.manual_seed(0)
    mcfg = model_cfg(False)
    tr = eng.Trainer(eng.BSMS_Simulator(mcfg), mcfg, OPT)
    bank = eng.TrajectoryBank(make_cfg(False), dataset="cylinder_flow", process=tr.model.process)
    for t in (synthetic_traj(100, 4, 1), synthetic_traj(140, 4, 2), synthetic_traj(90, 5, 3)):
        bank.add(t)
    tr.iter(bank.batch([(0, 0), (1, 0), (2, 0)], train=False))
    assert tr.iter(bank.batch([(0, 1), (1, 2), (2, 3)], train=False)) is not None
    check_get_error(tr, bank.batch([(2, 0), (0, 2), (1, 1)], train=False), (1, 330, 3))


def scaled(traj, factor):
    """The trajectory with its fields multiplied by `factor`: trajectories of different magnitudes have different RMSEs, so the
    standard deviations of the accumulators are of the order of their means and a relative bound on them means something."""
    return dict(traj, velocity=(traj["velocity"] * factor).astype(np.float32), density=(traj["density"] * factor).astype(np.float32))


def summaries_rel(a, b):
    """Worst relative difference between two RolloutErrors.summary() dicts; `equal`: bit for bit."""
    worst, equal = 0.0, True
    for k in ("all", "channel", "time"):
        for x, y in zip(a[k], b[k]):
            assert bool(torch.isfinite(x).all()) and x.shape == y.shape
            worst = max(worst, rel(x.cpu().numpy(), y.cpu().numpy()))
            equal = equal and torch.equal(x, y)
    return worst, equal


class SumsRecorder:
    """Stands in for RolloutErrors where trajectories of DIFFERENT lengths go through one rollout_bank call: the per-time
    accumulator of the reference's driver has the size of one T - 1 and cannot take another (nor can rollout_dataset's)."""

    def __init__(self):
        self.sums = []

    def add_sums(self, sums):
        self.sums.append(sums.clone())


def test_rollout_bank_consistent_mesh(eng):
    trajs = [scaled(t, f) for t, f in zip(same_mesh_trajs(120, 6, 4, seed=9), (1.0, 3.0, 0.3, 10.0))]
    bank = eng.TrajectoryBank(make_cfg(True), dataset="airfoil")
    for t in trajs:
        bank.add(t)
    torch.manual_seed(0)
    mcfg = model_cfg(True)
    tr = eng.Trainer(eng.BSMS_Simulator(mcfg), mcfg, OPT)
    tr.iter(bank.batch([(k, 0) for k in range(4)], train=False))              # warm-up: normaliser statistics
    tr.iter(bank.batch([(k, 1) for k in range(4)], train=False))
    e4, r4 = eng.rollout_bank(tr, bank, batch=4, keep_results=True)
    e1, r1 = eng.rollout_bank(tr, bank, batch=1, keep_results=True)
    e3, r3 = eng.rollout_bank(tr, bank, batch=3, keep_results=True)           # groups of 3 + 1
    assert len(r4) == len(r1) == len(r3) == 4 and all(r.shape == (5, 120, 3) and r.is_cuda for r in r4)
    for a, b, c in zip(r4, r1, r3):
        assert torch.equal(a, b) and torch.equal(a, c) and bool(torch.isfinite(a).all())
    assert summaries_rel(e4.summary(), e1.summary())[1] and summaries_rel(e4.summary(), e3.summary())[1]
    assert float(e4.all._num_accumulations) == 4
    ref = eng.rollout_dataset(tr, bank.rollouts(range(4))).summary()
    err = summaries_rel(e4.summary(), ref)[0]
    print(f"[rollout_bank vs rollout_dataset] consistent mesh, summary: {err:.2e} (bound {RMSE_TOL:.0e})")
    assert err <= RMSE_TOL
    eg, rg = eng.rollout_bank(tr, bank, batch=4, use_graph=True, keep_results=True)
    assert all(torch.equal(a, b) for a, b in zip(rg, r4)) and summaries_rel(eg.summary(), e4.summary())[1]
    # a custom order: the accumulators are fed in that order, whatever the grouping
    order = [2, 0, 3, 1]
    eo, ro = eng.rollout_bank(tr, bank, indices=order, batch=4, keep_results=True)
    assert all(torch.equal(ro[j], r4[i]) for j, i in enumerate(order))
    assert summaries_rel(eo.summary(), eng.rollout_bank(tr, bank, indices=order, batch=1).summary())[1]
    err = summaries_rel(eo.summary(), eng.rollout_dataset(tr, bank.rollouts(order)).summary())[0]
    print(f"[rollout_bank vs rollout_dataset] consistent mesh, order {order}: {err:.2e} (bound {RMSE_TOL:.0e})")
    assert err <= RMSE_TOL
    # the accumulators can be carried on
    more = eng.rollout_bank(tr, bank, indices=[1], errors=eo)
    assert more is eo and float(eo.all._num_accumulations) == 5


def test_rollout_bank_variable_meshes(eng):
    """Meshes of 100 / 140 / 90 nodes with T = 5 / 5 / 6: batch=3 advances the first two as one block-diagonal graph and the
    third alone (the grouping splits where T changes).  A trajectory advanced inside a union goes through other launch shapes
    than alone, so the comparison with batch=1 is held to the project's forward tolerance, not to bit-equality.
    One RolloutErrors cannot take T - 1 = 4 and then 5 (the per-time accumulator of the reference's driver has one size, and
    rollout_dataset fails on such a set in the same way): the three go through ONE rollout_bank call with their sums recorded
    per trajectory, and the accumulated statistics are compared on the T = 5 pair."""
    torch.manual_seed(0)
    mcfg = model_cfg(False)
    tr = eng.Trainer(eng.BSMS_Simulator(mcfg), mcfg, OPT)
    bank = eng.TrajectoryBank(make_cfg(False), dataset="cylinder_flow", process=tr.model.process)
    for t in (scaled(synthetic_traj(100, 5, 1), 1.0), scaled(synthetic_traj(140, 5, 2), 4.0), scaled(synthetic_traj(90, 6, 3), 0.3)):
        bank.add(t)
    tr.iter(bank.batch([(0, 0), (1, 0), (2, 0)], train=False))
    tr.iter(bank.batch([(0, 1), (1, 2), (2, 3)], train=False))
    # all three in one call: the sums are recorded per trajectory (one RolloutErrors cannot hold T - 1 = 4 and 5, see SumsRecorder)
    s3, s1 = SumsRecorder(), SumsRecorder()
    _, r3 = eng.rollout_bank(tr, bank, batch=3, keep_results=True, errors=s3)
    _, r1 = eng.rollout_bank(tr, bank, batch=1, keep_results=True, errors=s1)
    assert [tuple(r.shape) for r in r3] == [tuple(r.shape) for r in r1] == [(4, 100, 3), (4, 140, 3), (5, 90, 3)]
    assert [tuple(s.shape) for s in s3.sums] == [tuple(s.shape) for s in s1.sums] == [(4, 10), (4, 10), (5, 10)]
    assert r3[0].data_ptr() != r3[1].data_ptr() and r3[0].stride(0) == 240 * 3 and r3[2].stride(0) == 90 * 3   # 100 + 140 together, 90 alone
    errs = [rel_err(a, b) for a, b in zip(r3, r1)]
    errs_s = [rel(a.cpu().numpy(), b.cpu().numpy()) for a, b in zip(s3.sums, s1.sums)]
    bit_equal = all(torch.equal(a, b) for a, b in zip(r3, r1))
    print(f"[rollout_bank variable meshes] batch=3 vs batch=1: results {errs} (bit-equal: {bit_equal}), sums {errs_s}; bound {FWD_TOL:.0e}")
    assert all(bool(torch.isfinite(r).all()) for r in r3) and max(errs) <= FWD_TOL
    assert torch.equal(r3[2], r1[2]) and torch.equal(s3.sums[2], s1.sums[2])  # the third trajectory is alone in its group either way
    for k, (res, sums) in enumerate(zip(r1, s1.sums)):                        # the targets really are the bank's state[1:], the mask frame 0's
        _, tar, mask, *_ = bank.trajectory(k)
        assert rel(sums.cpu().numpy(), np_error_sums(res.cpu().numpy(), tar.cpu().numpy(), mask[0, :, 0].cpu().numpy())) <= SUM_TOL, k
        for got, want in zip(eng.RolloutErrors().add_sums(sums), eng.rollout_errors(res, tar, mask)):     # what rollout_dataset feeds
            assert got.shape == want.shape and rel(got.cpu().numpy(), want.cpu().numpy()) <= RMSE_TOL, k
    with pytest.raises(ValueError):
        eng.rollout_bank(tr, bank, batch=3)                                   # T - 1 = 5 into accumulators started with 4: refused, by name
    # the statistics, per length: the pair of T = 5 grouped and one at a time, and the trajectory of T = 6
    pair3, pair1 = eng.rollout_bank(tr, bank, indices=[0, 1], batch=3).summary(), eng.rollout_bank(tr, bank, indices=[0, 1], batch=1).summary()
    err_s = summaries_rel(pair3, pair1)[0]
    print(f"[rollout_bank variable meshes] summary of the T = 5 pair, batch=3 vs batch=1: {err_s:.2e} (bound {FWD_TOL:.0e})")
    assert err_s <= FWD_TOL
    err = summaries_rel(pair1, eng.rollout_dataset(tr, bank.rollouts([0, 1])).summary())[0]
    print(f"[rollout_bank vs rollout_dataset] variable meshes, summary of the T = 5 pair: {err:.2e} (bound {RMSE_TOL:.0e})")
    assert err <= RMSE_TOL
