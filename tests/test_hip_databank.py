"""GPU: the device-resident trajectory bank (bsms_gnn_amd/databank.py over csrc/batch.hip) against the host data path it replaces
(datapipe.proc_data + the collates + the upload) and against the NumPy restatement of its noise contract
(tests/test_databank_host.py).  Small trajectories come from test_datapipe.synthetic_traj, the airfoil-size one from bench.py's
mesh generator."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from test_databank_host import DRAW, SEED, check_noise_statistics, normals
from test_datapipe import cfg as make_cfg, synthetic_traj

pytestmark = pytest.mark.gpu

NOISE_LEVEL = [10, 10, 0.01]        # what test_datapipe.cfg sets; gamma = 0.8 below
OPT = SimpleNamespace(peak_lr=1e-3, weight_decay=1e-4, warmup_steps=1, decay_steps=50, gnorm_clip=1.0)


@pytest.fixture(scope="module")
def eng():
    import bsms_gnn_amd as eng
    return eng


def same_mesh_trajs(n, T, count, seed, moving=()):
    """`count` trajectories on ONE mesh with different fields; those listed in `moving` have node positions that change over time."""
    base = synthetic_traj(n, T, seed)
    out = []
    for k in range(count):
        rng = np.random.default_rng(1000 * seed + k)
        tr = dict(base, velocity=rng.standard_normal((T, n, 2)).astype(np.float32), density=rng.standard_normal((T, n, 1)).astype(np.float32))
        if k in moving:
            tr["mesh_pos"] = (base["mesh_pos"] + 1e-3 * np.arange(T, dtype=np.float32)[:, None, None]).astype(np.float32)
        out.append(tr)
    return out


def airfoil_traj(T, seed=0):
    """One trajectory on the bench workload's airfoil mesh (5233 nodes), node types drawn like synthetic_traj's."""
    import bench
    pts, cells = bench.mesh_points("airfoil")
    n = pts.shape[0]
    rng = np.random.default_rng(seed)
    return {"cells": np.repeat(cells[None], T, 0), "mesh_pos": np.repeat(pts.astype(np.float32)[None], T, 0),
            "node_type": np.repeat(rng.choice((0, 0, 0, 4, 5), (1, n, 1)).astype(np.float32), T, 0),
            "velocity": rng.standard_normal((T, n, 2)).astype(np.float32), "density": rng.standard_normal((T, n, 1)).astype(np.float32)}


def model_cfg(consistent, depth=2):
    return SimpleNamespace(out_dim=3, latent_dim=32, hidden_layer=2, unet_depth=depth, pos_dim=2, consistent_mesh=consistent, accumulation_steps=1)


def host_samples(dp, dcfg, trajs, picks, dataset):
    readers = {si: dp.SingleTrajReader(dcfg, trajs[si]) for si in {si for si, _ in picks}}
    return [(*dp.proc_data(dcfg, readers[si][ti], dp.MASKS[dataset], train=False), readers[si].m_gs, readers[si].m_ids) for si, ti in picks]


def test_consistent_mesh_batches_equal_the_host_collate(eng):
    import bsms_gnn_amd.datapipe as dp
    from bsms_gnn_amd.graph import LevelPlan
    dcfg = make_cfg(True)
    trajs = same_mesh_trajs(120, 6, 3, seed=9, moving=(2,))
    bank = eng.TrajectoryBank(dcfg, dataset="airfoil", seed=3)
    resident = []
    for k, t in enumerate(trajs):
        assert bank.add(t) == k
        resident.append(bank.bytes_resident)
    assert len(bank) == 3 and bank.lengths == [5, 5, 5]
    state_bytes = trajs[0]["velocity"].nbytes + trajs[0]["density"].nbytes
    assert resident[0] > state_bytes                                                       # + the hierarchy, once
    assert resident[1] - resident[0] == state_bytes + 120 * 2 * 4 + 120 * 4               # static positions / types: one frame each
    assert resident[2] - resident[1] == state_bytes + trajs[2]["mesh_pos"].nbytes + 120 * 4   # moving positions: every frame
    with pytest.raises(eng._abi.BsmsError):
        eng.TrajectoryBank(dcfg, max_bytes=1000).add(trajs[0])
    torch.manual_seed(0)
    mcfg = model_cfg(True)
    tr = eng.Trainer(eng.BSMS_Simulator(mcfg), mcfg, OPT)
    tr.iter(bank.batch([(0, 0), (1, 0), (2, 0), (0, 2)], train=False))        # warm-up step: statistics only, no plan is needed yet
    built = []
    for picks in ([(0, 1), (2, 0), (1, 3), (0, 0)], [(2, 4), (2, 1), (1, 0), (0, 3)], [(1, 1), (1, 2), (2, 3), (0, 4)]):
        got = bank.batch(picks, train=False)
        want = dp.collate_consistent(host_samples(dp, dcfg, trajs, picks, "airfoil"))
        for name, a, b in zip(("node_in", "node_tar", "node_mask"), got, want):
            assert a.is_cuda and a.shape == b.shape and torch.equal(a.cpu(), b), name
        assert len(got[3]) == len(want[3]) == 3 and len(got[4]) == len(want[4]) == 2
        for a, b in zip([*got[3], *got[4]], [*want[3], *want[4]]):
            assert a.is_cuda and a.shape == b.shape and a.stride(0) == 0 and torch.equal(a.cpu(), b)
        tr.iter(got)
        built.append(LevelPlan.constructed)
    assert built[1] == built[0] and built[2] == built[0], built          # the plans of the shared hierarchy are built once
    assert torch.isfinite(tr.get_loss(bank.sample(4, train=False))) and tr.get_pred(bank.sample(4)).shape == (4, 120, 3)
    with pytest.raises(IndexError):
        bank.batch([(0, 5)])


def test_variable_mesh_batches_equal_meshbank_collate(eng):
    import bsms_gnn_amd.datapipe as dp
    dcfg = make_cfg(False)
    trajs = [synthetic_traj(100, 4, 1), synthetic_traj(140, 4, 2), synthetic_traj(90, 5, 3)]
    trajs[1]["mesh_pos"] = (trajs[1]["mesh_pos"] + 1e-3 * np.arange(4, dtype=np.float32)[:, None, None]).astype(np.float32)
    torch.manual_seed(0)
    mcfg = model_cfg(False)
    tr = eng.Trainer(eng.BSMS_Simulator(mcfg), mcfg, OPT)
    bank = eng.TrajectoryBank(dcfg, dataset="cylinder_flow", process=tr.model.process)
    for t in trajs:
        bank.add(t)
    ref_bank = eng.MeshBank(tr.model.process, "cuda")
    for picks in ([(0, 0), (1, 2), (2, 3), (1, 0)], [(2, 0), (2, 1), (0, 2)]):
        got = bank.batch(picks, train=False)
        want = ref_bank.collate([dp.pack_levels(*s) for s in host_samples(dp, dcfg, trajs, picks, "cylinder_flow")])
        assert len(got) == len(want) == 3
        for lvl, (a, b) in enumerate(zip(got, want)):
            assert a.num_nodes == b.num_nodes and torch.equal(a.edge_index, b.edge_index), lvl
            assert (a.face is None) == (b.face is None) and (a.face is None or torch.equal(a.face, b.face)), lvl
            for name in ("x", "y", "mask"):
                u, v = getattr(a, name), getattr(b, name)
                assert (u is None) == (v is None) == (lvl > 0), (lvl, name)
                assert u is None or (u.shape == v.shape and torch.equal(u, v)), (lvl, name)
        tr.iter(got)
    assert torch.isfinite(tr.get_loss(bank.sample(3, train=False)))
    with pytest.raises(ValueError):
        eng.TrajectoryBank(dcfg, dataset="cylinder_flow")               # variable meshes need the model's BSGMP


def check_noisy_batch(bank, picks, draw, seed, std):
    """The contract of a train=True batch against the clean batch and the fp64 restatement; returns (noise [R,C], mask [R]) on the host."""
    (noisy_in, noisy_tar, mask, *_), noise = bank.batch(picks, train=True, draw=draw, return_noise=True)
    clean_in, clean_tar, clean_mask, *_ = bank.batch(picks, train=False)
    n_c = noise.shape[-1]
    noisy_in, noisy_tar, mask, noise, clean_in, clean_tar = (t.cpu().reshape(-1, t.shape[-1]) for t in (noisy_in, noisy_tar, mask, noise, clean_in, clean_tar))
    assert torch.equal(mask, clean_mask.cpu().reshape(-1, 1))
    assert torch.equal(noisy_in[:, :n_c], clean_in[:, :n_c] + noise)
    assert torch.equal(noisy_tar, clean_tar + torch.tensor(0.2, dtype=torch.float32) * noise)
    assert torch.equal(noisy_in[:, n_c:], clean_in[:, n_c:])                       # positions and node type untouched
    dead = mask[:, 0] == 0
    assert 0 < int(dead.sum()) < len(dead) and bool((noise[dead] == 0).all())       # Dirichlet nodes stay clean
    want = normals(noise.shape[0], n_c, seed, draw) * np.asarray(std, np.float32).astype(np.float64)
    err = np.abs(noise.numpy().astype(np.float64) - want)[~dead.numpy()] / np.asarray(std, np.float64)
    print(f"[noise vs fp64 restatement] {noise.shape[0]} rows: worst |noise - std z| / std per channel {err.max(0)} (bound 1e-5)")
    assert (err <= 1e-5).all()
    return noise.numpy(), mask[:, 0].numpy()


@pytest.fixture(scope="module")
def airfoil_bank(eng):
    dcfg = make_cfg(True, depth=5, gamma=0.8)
    bank = eng.TrajectoryBank(dcfg, dataset="airfoil", seed=SEED)
    bank.add(airfoil_traj(9))
    return bank


def test_training_noise_follows_the_contract(eng, airfoil_bank):
    """noise_level [10, 10, 0.01], gamma 0.8, B = 8 at airfoil size."""
    assert list(airfoil_bank.cfg.noise_level) == NOISE_LEVEL and airfoil_bank.cfg.noise_gamma == 0.8
    noise, mask = check_noisy_batch(airfoil_bank, [(0, t) for t in range(8)], DRAW, SEED, NOISE_LEVEL)
    assert noise.shape == (8 * 5233, 3)
    # a cylinder bank keeps type 5 (outflow) nodes noisy as well
    dcfg = make_cfg(False, gamma=0.8)
    torch.manual_seed(0)
    mcfg = model_cfg(False)
    sim = eng.BSMS_Simulator(mcfg).cuda()
    cyl = eng.TrajectoryBank(dcfg, dataset="cylinder_flow", process=sim.process, seed=SEED)
    traj = synthetic_traj(150, 4, 4)
    cyl.add(traj)
    levels, cyl_noise = cyl.batch([(0, 1)], train=True, draw=DRAW, return_noise=True)
    types = traj["node_type"][1, :, 0]
    assert torch.equal(levels[0].mask.cpu()[:, 0], torch.tensor((types == 0) | (types == 5)).float())
    cyl_noise = cyl_noise.cpu().numpy()
    assert (types == 5).any() and (types == 4).any() and (cyl_noise[types == 5] != 0).all() and (cyl_noise[types == 4] == 0).all()


def test_noise_does_not_depend_on_chunking_and_is_deterministic(eng):
    """70 samples cross the 64-sample launch: every row still gets the noise of its batch-global row index."""
    dcfg = make_cfg(True, gamma=0.8)
    traj = same_mesh_trajs(100, 80, 1, seed=5)[0]
    bank = eng.TrajectoryBank(dcfg, dataset="airfoil", seed=SEED)
    bank.add(traj)
    picks = [(0, (7 * k) % 79) for k in range(70)]
    noise, _ = check_noisy_batch(bank, picks, DRAW, SEED, NOISE_LEVEL)
    clean = bank.batch(picks, train=False)
    assert torch.equal(clean[0][:, :, :2].cpu(), torch.tensor(traj["velocity"][[t for _, t in picks]]))     # rows past the first launch too
    again = bank.batch(picks, train=True, draw=DRAW, return_noise=True)
    assert np.array_equal(again[1].cpu().numpy().reshape(-1, 3), noise)
    # the first 3 samples alone: the same rows get the same noise (no dependence on the batch around them)
    head = bank.batch(picks[:3], train=True, draw=DRAW, return_noise=True)[1].cpu().numpy().reshape(-1, 3)
    assert np.array_equal(head, noise[:300])
    other_draw = bank.batch(picks, train=True, draw=DRAW + 1, return_noise=True)[1].cpu().numpy().reshape(-1, 3)
    live = noise[:, 0] != 0
    assert live.any() and (other_draw[live] != noise[live]).mean() > 0.99
    reseeded = eng.TrajectoryBank(dcfg, dataset="airfoil", seed=SEED + 1)
    reseeded.add(traj)
    other_seed = reseeded.batch(picks, train=True, draw=DRAW, return_noise=True)[1].cpu().numpy().reshape(-1, 3)
    assert (other_seed[live] != noise[live]).mean() > 0.99
    # draw=None: the running batch counter -- two consecutive samples differ, and restart from 0 on a fresh bank
    a, b = bank.sample(4, return_noise=True)[1], bank.sample(4, return_noise=True)[1]
    assert not torch.equal(a, b)


def test_noise_statistics_at_airfoil_size(eng, airfoil_bank):
    """Per channel over the unmasked rows of a B = 8 airfoil batch: mean, standard deviation, kurtosis, lag-1 correlation along the
    rows and correlation between channels, each within five standard errors (test_databank_host.check_noise_statistics)."""
    _, noise = airfoil_bank.batch([(0, t) for t in range(8)], train=True, draw=DRAW, return_noise=True)
    mask = airfoil_bank.batch([(0, t) for t in range(8)], train=False)[2].cpu().reshape(-1).numpy()
    noise = noise.cpu().numpy().reshape(-1, 3).astype(np.float64)
    live = noise[mask == 1] / np.asarray(NOISE_LEVEL, np.float32).astype(np.float64)
    assert 20000 < len(live) < 8 * 5233
    check_noise_statistics(live, " kernel")


@pytest.mark.parametrize("consistent", [True, False])
def test_training_through_the_bank_equals_the_host_loader(eng, consistent):
    """Noise off: warm-up + three optimisation steps fed by bank.sample(8) and by the host loader in the same order give the same
    losses and parameters bit for bit (bit-equal batches into a deterministic engine)."""
    import bsms_gnn_amd.datapipe as dp
    dataset = "airfoil" if consistent else "cylinder_flow"
    dcfg = make_cfg(consistent)
    trajs = same_mesh_trajs(120, 13, 3, seed=7) if consistent else [synthetic_traj(100, 13, 1), synthetic_traj(140, 13, 2), synthetic_traj(90, 13, 3)]
    mcfg = model_cfg(consistent)
    torch.manual_seed(0)
    first = eng.BSMS_Simulator(mcfg)
    second = eng.BSMS_Simulator(mcfg)
    second.load_state_dict(first.state_dict())
    tr_bank, tr_host = eng.Trainer(first, mcfg, OPT), eng.Trainer(second, mcfg, OPT)
    bank = eng.TrajectoryBank(dcfg, dataset=dataset, seed=11, process=None if consistent else tr_bank.model.process)
    for t in trajs:
        bank.add(t)
    loader = iter(dp.make_loader(dp.TrajectoryDataset(dcfg, trajs, dataset=dataset, mode="valid", seed=11), 8))
    for step in range(4):
        loss_bank, loss_host = tr_bank.iter(bank.sample(8, train=False)), tr_host.iter(next(loader))
        assert (loss_bank is None) == (loss_host is None) == (step == 0)
        if step:
            assert torch.isfinite(loss_bank) and torch.equal(loss_bank, loss_host), (step, float(loss_bank), float(loss_host))
    assert tr_bank.train_step == 4
    assert torch.equal(tr_bank.optimizer.flat_p, tr_host.optimizer.flat_p)
    for (k, a), (_, b) in zip(tr_bank.model.state_dict().items(), tr_host.model.state_dict().items()):
        assert torch.equal(a, b), k


def test_rollout_through_the_bank(eng):
    import bsms_gnn_amd.datapipe as dp
    dcfg = make_cfg(True)
    trajs = same_mesh_trajs(120, 6, 3, seed=9)
    bank = eng.TrajectoryBank(dcfg, dataset="airfoil")
    for t in trajs:
        bank.add(t)
    order = list(range(3))
    np.random.default_rng(4).shuffle(order)                       # the order TrajectoryDataset(seed=4) visits the trajectories in
    yields = list(dp.TrajectoryDataset(dcfg, trajs, dataset="airfoil", mode="rollout", seed=4))
    for si, want in zip(order, yields):
        got = bank.trajectory(si)
        assert got[0].shape == (5, 120, 6) and got[1].shape == (5, 120, 3) and got[2].shape == (5, 120, 1)
        for a, b in zip(got[:3], want[:3]):
            assert torch.equal(a.cpu(), b)
        for a, b in zip([*got[3], *got[4]], [*want[3], *want[4]]):
            assert torch.equal(a.cpu(), b)
    torch.manual_seed(0)
    mcfg = model_cfg(True)
    tr = eng.Trainer(eng.BSMS_Simulator(mcfg), mcfg, OPT)
    tr.iter(bank.batch([(0, 0), (1, 1), (2, 2)], train=False))                 # warm-up: normaliser statistics
    host = eng.rollout_dataset(tr, dp.make_loader(dp.TrajectoryDataset(dcfg, trajs, dataset="airfoil", mode="rollout", seed=4), 1)).summary()
    dev = eng.rollout_dataset(tr, bank.rollouts(order)).summary()
    for k in ("all", "channel", "time"):
        for a, b in zip(dev[k], host[k]):
            assert bool(torch.isfinite(a).all()) and torch.equal(a, b), k
