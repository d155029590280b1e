"""GPU: the dataset statistics -- bsms_moment_sums / bsms_moment_fold of libbsms_hip_stats.so (csrc/stats/moments.hip)
against NumPy fp64 at the edges of the kernel's decomposition, and the layers above them: TrajectoryBank.moments, fit_normalizers,
Trainer.fit_normalizers.

The decomposition's constants (csrc/stats/moments.hip), each with the value below, at and above it in the size lists:
  64 lanes of a wave, kThreads = 256 elements between a thread's own, kSlab = 1024 elements of a frame per block  (n * C)
  kFrameChunk = 32 frame pairs per block                                                                           (frames)
  kEntries = 64 table entries per launch                                                                           (S)
  the piece capacity of the work area (a launch closes early when the next entry's pieces do not fit)              (test_launches_close...)
  kMaxBlocksPerLaunch = 2^20 pieces per dispatch                                                                   (test_more_pieces...)"""
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from conftest import ROOT
from test_datapipe import cfg as make_cfg, synthetic_traj

pytestmark = pytest.mark.gpu

NS = [1, 63, 64, 65, 255, 256, 257, 341, 342, 1023, 1024, 1025, 4097]      # n * C crosses 64 / 256 / 1024 for C = 1, 3 and 4
NS_C8 = [1, 7, 8, 9, 31, 32, 33, 127, 128, 129, 257, 4097]                 # ... and for C = 8
FRAMES = [1, 2, 3, 17, 31, 32, 33, 65]
FRAME0 = [0, 2]
VALID = {1: (0.0,), 2: (0.0, 5.0), 4: (0.0, 5.0, 4.0, 9.0)}
CASES = [(1, 1), (3, 2), (4, 4), (8, 2), (3, 1), (2, 4)]                   # (C, n_valid)
EPS = 2.0 ** -53
OPT = SimpleNamespace(peak_lr=1e-3, weight_decay=1e-4, warmup_steps=1, decay_steps=50, gnorm_clip=1.0)


@pytest.fixture(scope="module")
def eng():
    import bsms_gnn_amd as eng
    return eng


# ------------------------------------------------------------------------------------------------ the NumPy reference
def np_row(state, typ, frame0, frames, valid):
    """(row, A): the row of bsms_moment_sums in NumPy fp64 (d by the fp32 subtraction) and, per column, the sum of the absolute
    values of its terms."""
    T, n, C = state.shape
    x = state[frame0:frame0 + frames].astype(np.float64).reshape(-1, C)
    d = (state[frame0 + 1:frame0 + frames + 1] - state[frame0:frame0 + frames]).astype(np.float64).reshape(-1, C)
    ty = (typ[frame0:frame0 + frames] if typ.ndim == 2 else np.broadcast_to(typ, (frames, n))).astype(np.float64).reshape(-1)
    m = np.isin(ty, np.asarray(valid, dtype=np.float64)).astype(np.float64)
    row = np.concatenate([[frames * n, m.sum()], x.sum(0), [ty.sum()], (x * x).sum(0), [(ty * ty).sum()], d.sum(0), (d * d).sum(0)])
    A = np.concatenate([[0.0, 0.0], np.abs(x).sum(0), [np.abs(ty).sum()], (x * x).sum(0), [(ty * ty).sum()], np.abs(d).sum(0), (d * d).sum(0)])
    return row, A


def within_bound(got, row, A):
    """Worst |got - ref| / ((R + 16) 2^-53 A) over the columns (R and M exact); inf on a violation where A == 0."""
    assert got[0] == row[0] and got[1] == row[1], (got[:2], row[:2])
    bound = (row[0] + 16.0) * EPS * A[2:]
    err = np.abs(got[2:] - row[2:])
    if np.any((bound == 0) & (err > 0)):
        return np.inf
    return float(np.max(np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), 0.0))) if err.size else 0.0


def make_entries(shapes, C, integer, seed):
    """Host trajectories for `shapes` = [(n, frames, frame0, per_frame_type)]: T = frame0 + frames + 1 frames each."""
    rng = np.random.default_rng(seed)
    scale = (10.0 ** np.linspace(-2, 3, C)).astype(np.float32) if C > 1 else np.asarray([3.0], np.float32)    # five decades
    out = []
    for n, frames, frame0, per_frame in shapes:
        T = frame0 + frames + 1
        if integer:
            state = rng.integers(-8, 9, (T, n, C)).astype(np.float32)
        else:
            walk = np.cumsum(rng.standard_normal((T, n, C)) * 0.1, axis=0) + rng.standard_normal((1, n, C))
            state = ((walk + 10.0 * rng.random(C)) * scale).astype(np.float32)                                # means up to 10x the spread
        typ = rng.choice((0.0, 0.0, 0.0, 4.0, 5.0, 6.0, 9.0), (T, n) if per_frame else (n,)).astype(np.float32)
        out.append((state, typ, frame0, frames))
    return out


def upload(entries):
    """One flat device buffer for all states and one for all types; the entries are views at 4-byte granularity (frames that are not
    16-byte aligned, trajectories that start anywhere)."""
    flat_s = torch.from_numpy(np.concatenate([np.zeros(1, np.float32)] + [e[0].reshape(-1) for e in entries])).cuda()
    flat_t = torch.from_numpy(np.concatenate([np.zeros(3, np.float32)] + [e[1].reshape(-1) for e in entries])).cuda()
    table, so, to = [], 1, 3
    for state, typ, frame0, frames in entries:
        s = flat_s[so:so + state.size].view(state.shape)
        t = flat_t[to:to + typ.size].view(typ.shape)
        so, to = so + state.size, to + typ.size
        table.append((s, t, frame0, frames))
    return table


def size_list(C):
    ns = NS_C8 if C == 8 else NS
    shapes = [(n, f, f0, (i + j + k) % 2 == 1) for i, n in enumerate(ns) for j, f in enumerate(FRAMES) for k, f0 in enumerate(FRAME0)]
    shapes += [(n, f, 0, (i + j) % 2 == 0) for i, n in enumerate(ns) for j, f in enumerate(FRAMES)]           # the other type layout
    return shapes


@pytest.mark.parametrize("C,n_valid", CASES)
def test_integer_data_is_bit_equal_to_numpy(eng, C, n_valid):
    entries = make_entries(size_list(C), C, True, seed=100 + C)
    got = eng.moment_sums(upload(entries), C, VALID[n_valid]).cpu().numpy()
    assert got.shape == (len(entries), 4 * C + 4)
    for k, (state, typ, frame0, frames) in enumerate(entries):
        row, _ = np_row(state, typ, frame0, frames, VALID[n_valid])
        assert np.array_equal(got[k], row), (k, state.shape, frame0, frames, typ.ndim, got[k], row)


@pytest.mark.parametrize("C,n_valid", CASES)
def test_real_data_within_the_summation_bound(eng, C, n_valid):
    entries = make_entries(size_list(C), C, False, seed=200 + C)
    got = eng.moment_sums(upload(entries), C, VALID[n_valid]).cpu().numpy()
    worst = 0.0
    for k, (state, typ, frame0, frames) in enumerate(entries):
        row, A = np_row(state, typ, frame0, frames, VALID[n_valid])
        worst = max(worst, within_bound(got[k], row, A))
    print(f"[moment parity] C={C} n_valid={n_valid}: {len(entries)} entries, worst |got - ref| / ((R + 16) 2^-53 A) = {worst:.3e}")
    assert worst <= 1.0


def tiny_and_large(S, C, integer, seed):
    """S entries: tiny trajectories (T = 2, n = 3), one large one, and an entry of zero rows in the middle."""
    shapes = [(3, 1, 0, k % 2 == 0) for k in range(S)]
    if S > 1:
        shapes[S // 3] = (4097, 65, 2, True)
        shapes[S // 2] = (0, 5, 0, False) if S % 2 else (7, 0, 1, False)
    return make_entries(shapes, C, integer, seed)


@pytest.mark.parametrize("S", [0, 1, 63, 64, 65, 130])
def test_table_sizes(eng, S):
    C, valid = 3, VALID[2]
    for integer in (True, False):
        entries = tiny_and_large(S, C, integer, seed=300 + S)
        got = eng.moment_sums(upload(entries) if S else [], C, valid)
        assert tuple(got.shape) == (S, 16) and got.dtype == torch.float64 and got.is_cuda
        got = got.cpu().numpy()
        for k, (state, typ, frame0, frames) in enumerate(entries):
            row, A = np_row(state, typ, frame0, frames, valid)
            if state.shape[1] * frames == 0:
                assert np.array_equal(got[k], np.zeros(16)), k
            elif integer:
                assert np.array_equal(got[k], row), k
            else:
                assert within_bound(got[k], row, A) <= 1.0, k


def test_launches_close_when_the_work_area_is_full(eng):
    """Three entries of n = 1 and 200000 frame pairs: 6250 pieces each against a work area of 7864 (bsms_moment_work_bytes of the
    table's largest entry), so every entry gets a launch pair of its own and the area is reused in stream order."""
    C, frames = 1, 200000
    X = eng._abi.stats()
    assert X.bsms_moment_work_bytes(frames) // (35 * 8) < 2 * -(-frames // 32)
    entries = make_entries([(1, frames, 0, False), (1, frames, 1, True), (1, frames, 0, False)], C, True, seed=7)
    got = eng.moment_sums(upload(entries), C, VALID[1]).cpu().numpy()
    for k, (state, typ, frame0, fr) in enumerate(entries):
        assert np.array_equal(got[k], np_row(state, typ, frame0, fr, VALID[1])[0]), k


def test_more_pieces_than_one_dispatch_takes(eng):
    """n = 1, 32 (2^20 + 1) + 5 frame pairs: 2^20 + 2 pieces, cut into two dispatches of k_moment_pieces; integer data, exact sums by
    torch in fp64 on the device.  The work area of such a table (0.4 GB) is dropped again afterwards."""
    from bsms_gnn_amd import ops
    frames = 32 * ((1 << 20) + 1) + 5
    state = (torch.arange(frames + 1, device="cuda", dtype=torch.int32) % 7 - 3).float().view(frames + 1, 1, 1)
    state[-40:] += 2.0                                                        # the last two pieces differ from the pattern
    typ = torch.zeros(1, device="cuda")
    got = eng.moment_sums([(state, typ, 0, frames)], 1, (0.0,))[0]
    x, d = state[:-1, 0, 0].double(), (state[1:, 0, 0] - state[:-1, 0, 0]).double()
    want = torch.stack([torch.tensor(float(frames), device="cuda", dtype=torch.float64), torch.tensor(float(frames), device="cuda", dtype=torch.float64),
                        x.sum(), torch.zeros((), device="cuda", dtype=torch.float64), (x * x).sum(), torch.zeros((), device="cuda", dtype=torch.float64),
                        d.sum(), (d * d).sum()])
    ops._WORK.clear()
    assert torch.equal(got, want), (got, want)


def test_rows_are_bit_identical_whatever_surrounds_them(eng):
    C, valid = 3, VALID[2]
    probe = make_entries([(1025, 33, 2, True)], C, False, seed=41)[0]
    others = make_entries([(3 + k % 5, 1 + k % 3, 0, k % 2 == 0) for k in range(129)], C, False, seed=42)
    alone_table = upload([probe])
    alone = eng.moment_sums(alone_table, C, valid)
    assert torch.equal(alone, eng.moment_sums(alone_table, C, valid))                      # run to run
    for pos in (0, 63, 64, 129):
        entries = others[:pos] + [probe] + others[pos:]
        assert len(entries) == 130
        got = eng.moment_sums(upload(entries), C, valid)
        assert torch.equal(got[pos], alone[0]), pos
    # a NaN-filled work area, NaN in `sums` before the call (overwritten, never added to), sentinels behind `sums`
    from bsms_gnn_amd import ops
    work = ops._workspace(alone.device, eng._abi.stats().bsms_moment_work_bytes(1025 * 33))
    work[:work.numel() // 8 * 8].view(torch.float64).fill_(float("nan"))
    buf = torch.full((2 * 16 + 8,), float("nan"), device="cuda", dtype=torch.float64)
    buf[32:] = -12345.0
    entries = [probe, others[0]]
    got = eng.moment_sums(upload(entries), C, valid, out=buf[:32].view(2, 16))
    assert torch.equal(got[0], alone[0]) and bool(torch.isfinite(got).all())
    assert bool((buf[32:] == -12345.0).all())
    assert ops._workspace(alone.device, 1).data_ptr() == work.data_ptr()                   # the call used the area that was filled


def np_fold(rows):
    out = np.zeros(rows.shape[1])
    for r in rows:                                                                         # left to right, fp64
        out = out + r
    return out


@pytest.mark.parametrize("S", [0, 1, 2, 70])
def test_fold_is_the_left_to_right_sum(eng, S):
    rng = np.random.default_rng(S)
    rows = rng.standard_normal((S, 16)) * 10.0 ** rng.integers(-3, 6, (S, 16))
    out = torch.full((16,), float("nan"), device="cuda", dtype=torch.float64)
    got = eng.moment_fold(torch.from_numpy(rows).cuda(), out=out)
    assert got.data_ptr() == out.data_ptr() and np.array_equal(got.cpu().numpy(), np_fold(rows))
    wide = rng.standard_normal((S, 130))                                                   # more columns than one block of the fold
    assert np.array_equal(eng.moment_fold(torch.from_numpy(wide).cuda()).cpu().numpy(), np_fold(wide))


def test_sums_and_fold_capture_into_a_graph(eng):
    C, valid = 3, VALID[2]
    table = upload(tiny_and_large(70, C, False, seed=51))
    eager = eng.moment_sums(table, C, valid)
    eager_total = eng.moment_fold(eager)
    sums = torch.empty_like(eager)
    total = torch.empty_like(eager_total)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                                                          # warm-up outside capture: the workspace of the stream
        eng.moment_sums(table, C, valid, out=sums)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        eng.moment_sums(table, C, valid, out=sums)
        eng.moment_fold(sums, out=total)
    for _ in range(2):
        sums.fill_(float("nan"))
        total.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(sums, eager) and torch.equal(total, eager_total)


def test_python_surface_refuses_what_the_entries_cannot_take(eng):
    state, typ = torch.zeros(4, 5, 3, device="cuda"), torch.zeros(5, device="cuda")
    with pytest.raises(ValueError):
        eng.moment_sums([(state, typ, 0, 4)], 3, (0.0,))                                   # frame 4 has no successor
    with pytest.raises(ValueError):
        eng.moment_sums([(state, torch.zeros(6, device="cuda"), 0, 3)], 3, (0.0,))
    with pytest.raises(ValueError):
        eng.moment_sums([(state, typ, 0, 3)], 2, (0.0,))
    with pytest.raises(eng._abi.BsmsError):
        eng.moment_sums([(state.cpu(), typ, 0, 3)], 3, (0.0,))
    with pytest.raises(eng._abi.BsmsError):
        eng.moment_sums([(state, typ, 0, 3)], 3, (0.0, 1.0, 2.0, 3.0, 4.0))               # n_valid = 5: the library's refusal
    with pytest.raises(eng._abi.BsmsError):
        eng.moment_fold(torch.zeros(3, 16))


# ------------------------------------------------------------------------------------------------ the layers above
def spread_fields(tr, seed):
    """The fields of a synthetic trajectory replaced by data whose per-channel spread is at least a tenth of its mean: state
    randn * (1, 0.3, 20) + (0.5, -0.2, 10), drifting over the frames (the deltas have a mean of their own)."""
    rng = np.random.default_rng(seed)
    T, n = tr["velocity"].shape[:2]
    state = rng.standard_normal((1, n, 3)) * np.asarray([1.0, 0.3, 20.0]) + np.asarray([0.5, -0.2, 10.0])
    state = state + np.cumsum(rng.standard_normal((T, n, 3)) * np.asarray([0.05, 0.02, 1.0]) + np.asarray([0.02, -0.01, 0.5]), axis=0)
    return dict(tr, velocity=state[..., :2].astype(np.float32), density=state[..., 2:].astype(np.float32))


def consistent_trajs(n=257, lengths=(4, 5, 9), seed=3, per_frame_type=()):
    base = synthetic_traj(n, max(lengths), seed)
    out = []
    for k, T in enumerate(lengths):
        tr = spread_fields({key: v[:T] for key, v in base.items()}, 10 * seed + k)
        if k in per_frame_type:
            tr["node_type"] = np.random.default_rng(k).choice((0.0, 4.0, 5.0), (T, n, 1)).astype(np.float32)
        out.append(tr)
    return out


def variable_trajs():
    return [spread_fields(synthetic_traj(n, T, seed), 70 + seed) for n, T, seed in ((100, 4, 1), (140, 6, 2), (90, 5, 3))]


def host_state(tr):
    return np.concatenate([tr["velocity"], tr["density"]], axis=-1)


def host_type(tr):
    typ = tr["node_type"][..., 0]
    return typ[0] if bool((typ == typ[:1]).all()) else typ


def host_rows(trajs, valid):
    rows = [np_row(host_state(tr), host_type(tr), 0, tr["velocity"].shape[0] - 1, valid) for tr in trajs]
    return np.stack([r for r, _ in rows]), np.stack([a for _, a in rows])


def model_cfg(consistent, accumulation_steps=3, depth=2):
    return SimpleNamespace(out_dim=3, latent_dim=32, hidden_layer=2, unet_depth=depth, pos_dim=2, consistent_mesh=consistent,
                           accumulation_steps=accumulation_steps)


def new_model(eng, mcfg, seed=0):
    torch.manual_seed(seed)
    return eng.BSMS_Simulator(mcfg).cuda()


@pytest.fixture(scope="module")
def consistent(eng):
    trajs = consistent_trajs(per_frame_type=(1,))
    bank = eng.TrajectoryBank(make_cfg(True, gamma=0.8), dataset="cylinder_flow", seed=3, horizon=2)
    for tr in trajs:
        bank.add(tr)
    return trajs, bank, VALID[2]


def test_bank_moments_against_numpy(eng, consistent):
    trajs, bank, valid = consistent
    mom = bank.moments()
    assert mom.per_trajectory.shape == (3, 16) and mom.total.shape == (16,) and mom.total.is_cuda
    rows, A = host_rows(trajs, valid)                                                      # every pair (t, t+1), whatever the horizon
    assert [int(r[0]) for r in rows] == [3 * 257, 4 * 257, 8 * 257]
    got = mom.per_trajectory.cpu().numpy()
    for k in range(3):
        assert within_bound(got[k], rows[k], A[k]) <= 1.0, k
    assert np.array_equal(mom.total.cpu().numpy(), np_fold(got))
    assert within_bound(mom.total.cpu().numpy(), rows.sum(0), A.sum(0)) <= 1.0
    assert float(mom.rows) == 15 * 257 and float(mom.masked) == rows[:, 1].sum()
    # subsets and their order: a trajectory's row is its own
    for indices in ([2], [2, 0], [1, 1, 0], [0, 1, 2][::-1]):
        sub = bank.moments(indices)
        assert torch.equal(sub.per_trajectory, mom.per_trajectory[indices]), indices
        assert np.array_equal(sub.total.cpu().numpy(), np_fold(got[indices]))
    empty = bank.moments([])
    assert empty.per_trajectory.shape == (0, 16) and bool((empty.total == 0).all())
    with pytest.raises(ValueError, match="no rows"):
        empty.normalizer_stats()
    with pytest.raises(IndexError):
        bank.moments([3])


def test_variable_mesh_bank_moments_against_numpy(eng):
    trajs = variable_trajs()
    mcfg = model_cfg(False)
    model = new_model(eng, mcfg)
    bank = eng.TrajectoryBank(make_cfg(False), dataset="airfoil", process=model.process)
    for tr in trajs:
        bank.add(tr)
    mom = bank.moments()
    rows, A = host_rows(trajs, VALID[1])
    got = mom.per_trajectory.cpu().numpy()
    for k in range(3):
        assert within_bound(got[k], rows[k], A[k]) <= 1.0, k
    assert float(mom.rows) == 3 * 100 + 5 * 140 + 4 * 90
    assert torch.equal(bank.moments([1]).per_trajectory[0], mom.per_trajectory[1])


def oracle_stats(trajs):
    """oracle.bsms_oracle.Normalizer fed ALL pairs as one accumulate call: inputs [state_t | type], deltas by the fp32 subtraction."""
    from oracle import bsms_oracle as ro
    ins, deltas = [], []
    for tr in trajs:
        state, typ = torch.from_numpy(host_state(tr)), torch.from_numpy(tr["node_type"])
        ins.append(torch.cat([state[:-1], typ[:-1]], -1).reshape(-1, 4))
        deltas.append((state[1:] - state[:-1]).reshape(-1, 3))
    n_in, n_out = ro.Normalizer(4, max_accumulations=5e5), ro.Normalizer(3, max_accumulations=5e5)
    n_in(torch.cat(ins), accumulate=True)
    n_out(torch.cat(deltas), accumulate=True)
    return n_in, n_out


def test_fit_without_noise_matches_the_cpu_oracle(eng, consistent):
    trajs, bank, _ = consistent
    trajs = [dict(tr) for tr in trajs]
    model = new_model(eng, model_cfg(True))
    eng.fit_normalizers(model, bank, noise="none")
    for name, got, ref in zip(("in", "out"), (model._inputNormalizer, model._targetNormalizer), oracle_stats(trajs)):
        mean, std = got.mean().cpu().numpy(), got.std_with_epsilon().cpu().numpy()
        r_mean, r_std = ref._E_data.numpy(), ref.std_with_epsilon().numpy()
        for c in range(mean.size):
            if name == "in" and c == 3 and r_std[c] < 1e-6:
                continue
            e_mean, e_std = abs(mean[c] - r_mean[c]) / max(abs(r_mean[c]), r_std[c]), abs(std[c] - r_std[c]) / r_std[c]
            print(f"[fit vs oracle] {name}[{c}]: mean {e_mean:.2e} std {e_std:.2e} (budget 1e-5)")
            assert e_mean <= 1e-5 and e_std <= 1e-5, (name, c)
        assert got.synced and float(got._num_accumulations) == float(got._max_accumulations) and float(got._acc_weight) == 15 * 257 / got.unit


def test_fit_with_expected_noise_is_the_closed_form_of_the_numpy_sums(eng, consistent):
    from test_moments_host import numpy_stats
    trajs, bank, valid = consistent
    rows, _ = host_rows(trajs, valid)
    model = new_model(eng, model_cfg(True))
    mom = eng.fit_normalizers(model, bank, noise="expected")
    assert isinstance(mom, eng.Moments)
    want = numpy_stats(rows.sum(0), 3, bank.cfg.noise_level, bank.cfg.noise_gamma)
    got = (model._inputNormalizer._E_data, model._inputNormalizer._E_data_squared, model._targetNormalizer._E_data, model._targetNormalizer._E_data_squared)
    for name, g, w in zip(("in_mean", "in_meansq", "out_mean", "out_meansq"), got, want):
        err = np.abs(g.cpu().numpy() - w) / np.abs(w)
        assert err.max() <= 1e-12, (name, err)
    noisy_meansq = got[1].clone()
    eng.fit_normalizers(model, bank, noise="none")
    assert bool((noisy_meansq[:3] > model._inputNormalizer._E_data_squared[:3]).all())
    # a bank without noise: "expected" is bit-equal to "none"
    quiet_cfg = make_cfg(True, gamma=0.8)
    quiet_cfg.noise_level = [0, 0, 0]
    quiet = eng.TrajectoryBank(quiet_cfg, dataset="cylinder_flow")
    for tr in trajs:
        quiet.add(tr)
    a, b = new_model(eng, model_cfg(True)), new_model(eng, model_cfg(True))
    eng.fit_normalizers(a, quiet, noise="expected")
    eng.fit_normalizers(b, quiet, noise="none")
    for na, nb in ((a._inputNormalizer, b._inputNormalizer), (a._targetNormalizer, b._targetNormalizer)):
        assert torch.equal(na._E_data, nb._E_data) and torch.equal(na._E_data_squared, nb._E_data_squared)
    assert torch.equal(b._inputNormalizer._E_data, model._inputNormalizer._E_data)          # ... and to the noisy bank's "none"
    with pytest.raises(ValueError, match="augment"):
        eng.fit_normalizers(a, eng.TrajectoryBank(quiet_cfg, dataset="cylinder_flow", augment=eng.Augment()))


def stat_tensors(model):
    return [t for n in (model._inputNormalizer, model._targetNormalizer) for t in (n._E_data, n._E_data_squared)]


def test_fits_are_in_place_for_a_fused_step_and_a_captured_rollout(eng, consistent):
    from bsms_gnn_amd.rollout import _Stepper
    _, bank, _ = consistent
    mcfg = model_cfg(True)
    model = new_model(eng, mcfg)
    eng.fit_normalizers(model, bank, indices=[0, 1])
    ptrs = [t.data_ptr() for t in stat_tensors(model)]
    first = [t.clone() for t in stat_tensors(model)]
    data = bank.batch([(0, 0), (1, 2), (2, 5)], train=True, draw=4, horizon=1)
    one = bank.batch([(2, 1)], train=False, horizon=1)
    old_step = eng.DataParallel(model)
    old_step.step_loss_backward(data, True)
    old_roll = _Stepper(model, one[0], one[2], one[3], one[4], 3, True)
    old_roll.step()
    eng.fit_normalizers(model, bank, indices=[2])                                          # other statistics, the same tensors
    assert ptrs == [t.data_ptr() for t in stat_tensors(model)]
    assert not any(torch.equal(a, b) for a, b in zip(first, stat_tensors(model)))
    loss_old = old_step.step_loss_backward(data, True).clone()
    grads_old = old_step.grads.flat.clone()
    old_roll.cur.copy_(old_roll.ic)
    pred_old = old_roll.step().clone()
    new_roll = _Stepper(model, one[0], one[2], one[3], one[4], 3, True)
    assert torch.equal(new_roll.step(), pred_old)
    new_step = eng.DataParallel(model)
    assert torch.equal(new_step.step_loss_backward(data, True), loss_old) and torch.equal(new_step.grads.flat, grads_old)
    assert bool(torch.isfinite(loss_old)) and bool(torch.isfinite(pred_old).all())


def test_trainer_fit_trains_from_the_first_iter(eng, consistent, tmp_path):
    _, bank, _ = consistent
    mcfg = model_cfg(True, accumulation_steps=3)
    tr = eng.Trainer(new_model(eng, mcfg, seed=5), mcfg, OPT)
    assert tr._warming_up()
    mom = tr.fit_normalizers(bank)
    assert isinstance(mom, eng.Moments) and not tr._warming_up() and tr._synced and tr.train_step == 0
    fitted = [t.clone() for t in stat_tensors(tr.model)]
    # the twin: the same initial parameters, the statistics loaded through the state_dict, no warm-up configured
    zero_cfg = model_cfg(True, accumulation_steps=0)
    twin = eng.Trainer(new_model(eng, zero_cfg, seed=5), zero_cfg, OPT)
    twin.model.load_state_dict(tr.model.state_dict())
    for t in (tr, twin):
        t.lr_scheduler.last_epoch = 1            # the schedule's first epoch has factor 0: start behind it, so that the step moves the parameters
    data = bank.batch([(0, 0), (1, 1), (2, 3), (2, 6)], train=True, draw=9, horizon=1)
    before = tr.optimizer.flat_p.clone()
    loss = tr.iter(data)
    assert loss is not None and bool(torch.isfinite(loss)) and tr.train_step == 1
    assert not torch.equal(tr.optimizer.flat_p, before)                                    # trained at train_step == 0
    assert torch.equal(twin.iter(data), loss) and torch.equal(twin.optimizer.flat_p, tr.optimizer.flat_p)
    # a later warm-up style call accumulates nothing
    with torch.no_grad():
        tr.model(data, True, True)
    assert all(torch.equal(a, b) for a, b in zip(fitted, stat_tensors(tr.model)))
    # save / restore carry the statistics in the state_dict
    tr.save(str(tmp_path))
    other = eng.Trainer(new_model(eng, mcfg, seed=6), mcfg, OPT)
    other.restore(str(tmp_path), 1)
    assert all(torch.equal(a, b) for a, b in zip(fitted, stat_tensors(other.model)))
    assert float(other.model._inputNormalizer._num_accumulations) == float(other.model._inputNormalizer._max_accumulations)


def test_a_trainer_that_never_fits_does_not_touch_the_new_code(eng, consistent, monkeypatch):
    from bsms_gnn_amd import _abi, databank, ops, trainer
    _, bank, _ = consistent
    mcfg = model_cfg(True, accumulation_steps=2)
    batches = [bank.batch(p, train=True, draw=k, horizon=1) for k, p in enumerate(([(0, 0), (1, 1)], [(2, 2), (2, 5)], [(1, 0), (0, 2)]))]

    def run():
        tr = eng.Trainer(new_model(eng, mcfg, seed=8), mcfg, OPT)
        losses = [tr.iter(b) for b in batches]
        assert losses[0] is None and losses[1] is None and losses[2] is not None
        return [t.clone() for t in stat_tensors(tr.model)], losses[2].clone()

    monkeypatch.setattr(_abi, "_stats", None)                                              # as in a process that has not asked for statistics
    stats, loss = run()
    assert _abi._stats is None                                                             # the default route never loads libbsms_hip_stats.so

    def refuse(*a, **k):
        raise AssertionError("the default route reached the dataset statistics")

    for owner, name in ((_abi, "stats"), (ops, "moment_sums"), (ops, "moment_fold"), (databank, "fit_normalizers"), (databank.TrajectoryBank, "moments"),
                        (databank.Moments, "normalizer_stats"), (databank.Moments, "all_reduce"), (trainer.Trainer, "fit_normalizers")):
        monkeypatch.setattr(owner, name, refuse)
    stats2, loss2 = run()
    assert torch.equal(loss, loss2) and all(torch.equal(a, b) for a, b in zip(stats, stats2))
    assert _abi._stats is None


# ------------------------------------------------------------------------------------------------ two ranks
DP_LENGTHS = (3, 6, 4, 9)


def _fit_worker(rank, world, port, out_path):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    torch.cuda.set_device(0)
    import bsms_gnn_amd as eng
    from test_hip_moments import DP_LENGTHS, consistent_trajs, model_cfg, new_model, stat_tensors
    bank = eng.TrajectoryBank(make_cfg(True, gamma=0.8), dataset="cylinder_flow", seed=3)
    mine = bank.add_sharded(consistent_trajs(n=130, lengths=DP_LENGTHS, seed=4))
    model = new_model(eng, model_cfg(True), seed=20 + rank)
    mom = eng.fit_normalizers(model, bank, noise="expected")
    torch.cuda.synchronize()
    torch.save({"mine": mine, "total": mom.total.cpu(), "per": mom.per_trajectory.cpu(), "stats": [t.cpu() for t in stat_tensors(model)],
                "weight": model._inputNormalizer._acc_weight.cpu()}, f"{out_path}.{rank}")
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.timeout(300)
def test_two_ranks_fit_identical_statistics(eng, tmp_path):
    port = 29700 + os.getpid() % 200
    out = str(tmp_path / "fit")
    mp.start_processes(_fit_worker, args=(2, port, out), nprocs=2, join=True, start_method="spawn")
    r0, r1 = torch.load(out + ".0"), torch.load(out + ".1")
    assert r0["mine"] == [0, 1] and r1["mine"] == [0, 1] and r0["per"].shape == r1["per"].shape == (2, 16)
    assert not torch.equal(r0["per"], r1["per"])                                           # different shards ...
    assert torch.equal(r0["total"], r1["total"]) and torch.equal(r0["weight"], r1["weight"])
    assert all(torch.equal(a, b) for a, b in zip(r0["stats"], r1["stats"]))               # ... identical statistics, bit for bit
    trajs = consistent_trajs(n=130, lengths=DP_LENGTHS, seed=4)
    rows, A = host_rows(trajs, VALID[2])
    assert within_bound(r0["total"].numpy(), rows.sum(0), A.sum(0)) <= 1.0                 # the all-reduce is one more order of fp64 sums
    bank = eng.TrajectoryBank(make_cfg(True, gamma=0.8), dataset="cylinder_flow", seed=3)
    for tr in trajs:
        bank.add(tr)
    single = bank.moments()
    assert within_bound(single.total.cpu().numpy(), rows.sum(0), A.sum(0)) <= 1.0
    assert torch.equal(torch.cat([r0["per"], r1["per"]]), single.per_trajectory.cpu())     # a trajectory's row does not know its rank
    assert float(r0["weight"]) == sum(T - 1 for T in DP_LENGTHS) * 130 / 10 ** 6
