"""GPU: frame augmentation -- bsms_batch_assemble_xf and bsms_rows_transform through the C ABI on raw tensors, bit for bit against
the torch-fp32 restatement of tests/test_augment_host.py (every product and every sum a separate op) built on the PLAIN entry's
outputs; then TrajectoryBank(augment=), transform_rows, eval.equivariance_error and the Trainer on small Delaunay meshes."""
import ctypes as C
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from test_augment_host import EPS, restate_rows
from test_datapipe import cfg as make_cfg, synthetic_traj

pytestmark = pytest.mark.gpu

SEED, DRAW, GAMMA = 0x1234ABCD5678, 7, 0.8
STD = [10, 10, 0.01, 0.5, 2, 2, 0.1, 1]
PAD = 5                                             # sentinel rows behind every output
LAYOUTS = {"airfoil": (2, 3, (0,)), "scalar_first_3d": (3, 4, (1,)), "two_groups": (2, 8, (0, 4))}        # p, C, groups
SIZES = {"edges": [1, 255, 0, 256, 257, 700],       # block edges of the 256-row blocks, a 0-row sample in the middle
         "chunks": [(37 * k + 5) % 301 for k in range(70)]}      # 70 samples of <= 300 rows: more than one launch at any chunk size < 70
OPT = SimpleNamespace(peak_lr=1e-3, weight_decay=1e-4, warmup_steps=1, decay_steps=50, gnorm_clip=1.0)


@pytest.fixture(scope="module")
def eng():
    import bsms_gnn_amd as eng
    return eng


class Raw:
    """Per-sample device tensors and the host table of one batch, and the two assembly entries on them."""

    def __init__(self, eng, sizes, p, n_c, seed=0):
        from bsms_gnn_amd.databank import _Sample
        rng = np.random.default_rng(seed)
        self.L, self.check = eng._abi.lib(), eng._abi.check
        self.sizes, self.p, self.C, self.R = list(sizes), p, n_c, int(sum(sizes))
        self.keep, self.table = [], (_Sample * len(sizes))()
        for k, n in enumerate(sizes):
            t = [torch.tensor(rng.standard_normal((n, w)).astype(np.float32)).cuda() for w in (n_c, n_c, p)]
            t.append(torch.tensor(rng.choice((0, 0, 0, 4, 5), (n,)).astype(np.float32)).cuda())
            self.keep.append(t)
            s = self.table[k]
            s.state_in, s.state_tar, s.pos, s.type, s.n = (*[v.data_ptr() if n else None for v in t], n)
        self.std = (C.c_float * n_c)(*STD[:n_c])
        self.valid = (C.c_float * 1)(0.0)

    def assemble(self, xf=None, groups=(), noisy=False, draw=DRAW):
        """(node_in, node_tar, node_mask, noise_out) [R, .] of the plain entry (xf None) or the transforming one; the outputs start
        as NaN and the PAD rows behind them must stay NaN."""
        outs = [torch.full((self.R + PAD, w), float("nan"), device="cuda") for w in (self.C + self.p + 1, self.C, 1, self.C)]
        ptrs = [o.data_ptr() for o in outs]
        stream = torch.cuda.current_stream().cuda_stream
        std = C.addressof(self.std) if noisy else None
        if xf is None:
            self.check(self.L.bsms_batch_assemble(C.addressof(self.table), len(self.sizes), self.C, self.p, std, GAMMA, C.addressof(self.valid), len(self.valid),
                                                  SEED, draw, *ptrs, stream), "bsms_batch_assemble")
        else:
            xf = np.ascontiguousarray(xf, np.float32)
            assert xf.shape == (len(self.sizes), self.p, self.p)
            first = (C.c_int32 * max(len(groups), 1))(*groups)
            self.check(self.L.bsms_batch_assemble_xf(C.addressof(self.table), len(self.sizes), self.C, self.p, xf.ctypes.data, C.addressof(first),
                                                     len(groups), std, GAMMA, C.addressof(self.valid), len(self.valid), SEED, draw, *ptrs, stream),
                       "bsms_batch_assemble_xf")
        outs = [o.cpu() for o in outs]
        for o in outs:
            assert bool(torch.isnan(o[self.R:]).all()), "rows behind the batch were written"
            assert not bool(torch.isnan(o[:self.R]).any()), "rows of the batch were left unwritten"
        return [o[:self.R] for o in outs]

    def restated(self, xf, groups):
        """y_in [R, C+p+1], y_tar [R, C] on the host: the restatement applied to the plain entry's noise-free outputs (the position
        columns of node_in are one more group)."""
        clean_in, clean_tar, mask, _ = self.assemble()
        return restate_rows(clean_in, self.sizes, xf, [*groups, self.C]), restate_rows(clean_tar, self.sizes, xf, groups), mask


def any_matrices(n, p, seed):
    """Not orthogonal on purpose: the kernel applies what it is given, and generic entries exercise every rounding."""
    return np.random.default_rng(seed).standard_normal((n, p, p)).astype(np.float32)


@pytest.fixture(scope="module")
def raws(eng):
    cache = {}

    def get(layout, sizes):
        if (layout, sizes) not in cache:
            p, n_c, _ = LAYOUTS[layout]
            cache[layout, sizes] = Raw(eng, SIZES[sizes], p, n_c, seed=len(cache))
        return cache[layout, sizes]
    return get


# ------------------------------------------------------------------------------------------------ 1: bsms_batch_assemble_xf
@pytest.mark.parametrize("sizes", list(SIZES))
@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_assemble_xf_is_the_restatement_bit_for_bit(raws, layout, sizes):
    raw = raws(layout, sizes)
    p, n_c, groups = LAYOUTS[layout]
    xf = any_matrices(len(raw.sizes), p, 3)
    y_in, y_tar, mask = raw.restated(xf, groups)
    got = raw.assemble(xf, groups)
    assert torch.equal(got[0], y_in) and torch.equal(got[1], y_tar) and torch.equal(got[2], mask)
    assert bool((got[3] == 0).all())                                                   # noise_out without noise: zeros
    turned = [c for f in groups for c in range(f, f + p)]
    still = [c for c in range(n_c) if c not in turned]
    clean = raw.assemble()
    assert torch.equal(got[0][:, still], clean[0][:, still]) and torch.equal(got[0][:, -1], clean[0][:, -1])     # scalars, node type: copies
    assert not torch.equal(got[0][:, turned], clean[0][:, turned]) and not torch.equal(got[0][:, n_c:n_c + p], clean[0][:, n_c:n_c + p])
    # with noise: the plain entry's noise, added after the transform
    plain = raw.assemble(noisy=True)
    noisy = raw.assemble(xf, groups, noisy=True)
    noise = plain[3]
    assert float(noise.abs().max()) > 0 and torch.equal(noisy[3], noise)
    assert bool((noise[mask[:, 0] == 0] == 0).all())
    g = torch.tensor(np.float32(1.0 - GAMMA))
    assert torch.equal(noisy[0][:, :n_c], y_in[:, :n_c] + noise) and torch.equal(noisy[0][:, n_c:], y_in[:, n_c:])
    assert torch.equal(noisy[1], y_tar + g * noise) and torch.equal(noisy[2], mask)
    # two runs, and another draw
    again = raw.assemble(xf, groups, noisy=True)
    assert all(torch.equal(a, b) for a, b in zip(noisy, again))
    assert not torch.equal(raw.assemble(xf, groups, noisy=True, draw=DRAW + 1)[3], noise)


@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_identity_matrices_reproduce_the_plain_entry(raws, layout):
    raw = raws(layout, "chunks")
    p, _, groups = LAYOUTS[layout]
    eye = np.tile(np.eye(p, dtype=np.float32), (len(raw.sizes), 1, 1))
    for noisy in (False, True):
        for a, b in zip(raw.assemble(eye, groups, noisy=noisy), raw.assemble(noisy=noisy)):
            assert torch.equal(a, b)


def test_result_does_not_depend_on_the_chunking(raws, eng):
    """Samples 60 .. 69 of the 70 lie behind the first launch at any chunk size up to 60; on their own they are one launch.  Rows and
    matrices must line up the same way (the noise is keyed by the batch-global row, so this half is compared without it)."""
    raw = raws("airfoil", "chunks")
    p, n_c, groups = LAYOUTS["airfoil"]
    xf = any_matrices(70, p, 3)
    full = raw.assemble(xf, groups)
    tail = Raw(eng, raw.sizes[60:], p, n_c)
    tail.keep = raw.keep[60:]
    for k in range(10):
        for name in ("state_in", "state_tar", "pos", "type"):
            setattr(tail.table[k], name, getattr(raw.table[60 + k], name))
    part = tail.assemble(xf[60:], groups)
    row0 = sum(raw.sizes[:60])
    for a, b in zip(full, part):
        assert torch.equal(a[row0:], b)


@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_rigid_transforms_preserve_norms_and_distances(raws, eng, layout):
    """Orthogonal matrices (Augment.sample, with reflections).  Bound: 4 p 2^-24 of the vector's 1-norm -- every component of
    fl(Q v) is within p 2^-24 sum_b |Q_ab| |v_b| <= p 2^-24 |v|_1 of the exact product, and the fp32 matrix is orthogonal to
    8 * 2^-24 (tests/test_augment_host.py); a distance moves by at most the bound of its two end points."""
    raw = raws(layout, "edges")
    p, n_c, groups = LAYOUTS[layout]
    xf = eng.Augment(reflect=True).sample(p, len(raw.sizes), SEED, DRAW)
    clean, got = raw.assemble(), raw.assemble(xf, groups)
    bound = 4 * p * EPS
    for name, a, b, firsts in (("node_in", clean[0], got[0], [*groups, n_c]), ("node_tar", clean[1], got[1], groups)):
        for f in firsts:
            v, y = a[:, f:f + p].double(), b[:, f:f + p].double()
            err = (y.norm(dim=1) - v.norm(dim=1)).abs() / v.abs().sum(1)
            print(f"[rigid {layout}] {name} group {f}: worst |norm change| / |v|_1 = {float(err.max()):.2e} (bound {bound:.2e})")
            assert float(err.max()) <= bound
    row0 = sum(raw.sizes[:5])                                                          # the 700-row sample: its rows 0 .. 63
    x, y = clean[0][row0:row0 + 64, n_c:n_c + p].double(), got[0][row0:row0 + 64, n_c:n_c + p].double()
    one = x.abs().sum(1)
    err = (torch.cdist(y, y) - torch.cdist(x, x)).abs() / (one[:, None] + one[None, :])
    print(f"[rigid {layout}] position distances: worst change / (|x_i|_1 + |x_j|_1) = {float(err.max()):.2e} (bound {bound:.2e})")
    assert float(err.max()) <= bound


# ------------------------------------------------------------------------------------------------ 2: bsms_rows_transform
def rows_transform(eng, x, out, frames, per_frame, width, rows, xf, groups, transpose=False):
    xf = np.ascontiguousarray(xf, np.float32)
    table, first = (C.c_int64 * len(rows))(*rows), (C.c_int32 * max(len(groups), 1))(*groups)
    eng._abi.check(eng._abi.lib().bsms_rows_transform(x.data_ptr(), out.data_ptr(), frames, per_frame, width, C.addressof(table), len(rows),
                                                      xf.shape[1], xf.ctypes.data, int(transpose), C.addressof(first), len(groups),
                                                      torch.cuda.current_stream().cuda_stream), "bsms_rows_transform")


@pytest.mark.parametrize("frames", [1, 3])
@pytest.mark.parametrize("sizes", list(SIZES))
@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_rows_transform_is_the_restatement_bit_for_bit(eng, layout, sizes, frames):
    p, n_c, groups = LAYOUTS[layout]
    rows = SIZES[sizes]
    total, per_frame = sum(rows), sum(rows) + PAD                                       # PAD rows of every frame lie outside the table
    xf = any_matrices(len(rows), p, 11)
    x = torch.tensor(np.random.default_rng(5).standard_normal((frames + 1, per_frame, n_c)).astype(np.float32)).cuda()    # + a frame not passed
    host = x.cpu()
    for transpose in (False, True):
        want = torch.stack([restate_rows(host[j], rows, xf, groups, transpose) for j in range(frames)])
        out = torch.full_like(x, float("nan"))
        rows_transform(eng, x, out, frames, per_frame, n_c, rows, xf, groups, transpose)
        got = out.cpu()
        assert torch.equal(got[:frames, :total], want[:, :total])
        assert bool(torch.isnan(got[:frames, total:]).all()) and bool(torch.isnan(got[frames]).all())       # rows / frames outside: untouched
        assert torch.equal(x.cpu(), host)                                               # out of place: the input is read only
        again = torch.full_like(x, float("nan"))
        rows_transform(eng, x, again, frames, per_frame, n_c, rows, xf, groups, transpose)
        assert torch.equal(again.cpu()[:frames, :total], got[:frames, :total])
        inplace = x.clone()
        rows_transform(eng, inplace, inplace, frames, per_frame, n_c, rows, xf, groups, transpose)
        got = inplace.cpu()
        assert torch.equal(got[:frames, :total], want[:, :total])
        assert torch.equal(got[:frames, total:], host[:frames, total:]) and torch.equal(got[frames], host[frames])


@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_transpose_undoes_a_rigid_transform(eng, layout):
    """Q^T (Q v) = v within 16 * 2^-24 |v|_1: two applications of p <= 3 rounded products and sums, 2 * p * 2^-24 |v|_1 <= 6 * 2^-24,
    plus the orthogonality defect 8 * 2^-24 of the fp32 matrix."""
    p, n_c, groups = LAYOUTS[layout]
    rows = SIZES["edges"]
    xf = eng.Augment(reflect=True).sample(p, len(rows), SEED, DRAW + 1)
    x = torch.tensor(np.random.default_rng(6).standard_normal((2, sum(rows), n_c)).astype(np.float32)).cuda()
    y = eng.transform_rows(x, rows, xf, groups)
    back = eng.transform_rows(y, rows, torch.tensor(xf).cuda(), groups, inverse=True)
    assert not torch.equal(y, x) and y.data_ptr() != x.data_ptr()
    for f in groups:
        v = x[..., f:f + p].double()
        err = (back[..., f:f + p].double() - v).abs().amax(-1) / v.abs().sum(-1)
        print(f"[transpose {layout}] group {f}: worst |Q^T Q v - v| / |v|_1 = {float(err.max()):.2e} (bound {16 * EPS:.2e})")
        assert float(err.max()) <= 16 * EPS
    still = [c for c in range(n_c) if not any(f <= c < f + p for f in groups)]
    assert torch.equal(back[..., still], x[..., still])


def test_transform_rows_reads_its_shapes(eng):
    """[R,C], [B,N,C] and [F,R,C]; an int or a table of row counts; in place through out=."""
    p, n_c, groups = LAYOUTS["airfoil"]
    xf = any_matrices(4, p, 2)
    x = torch.tensor(np.random.default_rng(8).standard_normal((4, 90, n_c)).astype(np.float32)).cuda()
    want = restate_rows(x.cpu().reshape(-1, n_c), [90] * 4, xf, groups)
    assert torch.equal(eng.transform_rows(x, 90, xf, groups).cpu().reshape(-1, n_c), want)                      # [B,N,C]
    assert torch.equal(eng.transform_rows(x.reshape(-1, n_c), [90] * 4, xf, groups).cpu(), want)                 # [R,C]
    frames = x.reshape(2, 180, n_c)                                                                              # [F,R,C]: two samples per frame
    got = eng.transform_rows(frames, [90, 90], xf[:2], groups).cpu()
    assert all(torch.equal(got[j], restate_rows(frames[j].cpu(), [90, 90], xf[:2], groups)) for j in range(2))
    short = eng.transform_rows(x.reshape(-1, n_c), [50, 0, 20], xf[:3], groups).cpu()                            # rows past the table: kept
    assert torch.equal(short, restate_rows(x.cpu().reshape(-1, n_c), [50, 0, 20], xf[:3], groups))
    y = x.clone()
    assert eng.transform_rows(y, 90, xf, groups, out=y) is y and torch.equal(y.cpu().reshape(-1, n_c), want)
    with pytest.raises(ValueError):
        eng.transform_rows(x, 91, xf, groups)
    with pytest.raises(ValueError):
        eng.transform_rows(x, [90] * 3, xf, groups)
    with pytest.raises(eng._abi.BsmsError):
        eng.transform_rows(x, 90, xf, (2,))                                                                      # the group overruns C = 3


# ------------------------------------------------------------------------------------------------ 3: the bank
def field_trajs(n, T, count, seed):
    """`count` trajectories on ONE Delaunay mesh of `n` nodes with different fields."""
    base = synthetic_traj(n, T, seed)
    out = []
    for k in range(count):
        rng = np.random.default_rng(1000 * seed + k)
        out.append(dict(base, velocity=rng.standard_normal((T, n, 2)).astype(np.float32), density=rng.standard_normal((T, n, 1)).astype(np.float32)))
    return out


def model_cfg(consistent, warmup=1):
    return SimpleNamespace(out_dim=3, latent_dim=32, hidden_layer=2, unet_depth=2, pos_dim=2, consistent_mesh=consistent, accumulation_steps=warmup)


def node_tensors(batch, consistent):
    """(node_in, node_tar, node_mask) flattened to rows."""
    t = batch[:3] if consistent else (batch[0].x, batch[0].y, batch[0].mask)
    return [v.reshape(-1, v.shape[-1]) for v in t]


@pytest.fixture(scope="module")
def banks(eng):
    """Per mesh case: (trajectories, a bank with Augment(reflect=True), a bank without, a horizon-3 bank of each kind), same seed."""
    cache = {}

    def get(consistent):
        if consistent not in cache:
            dcfg = make_cfg(consistent, gamma=GAMMA)
            trajs = field_trajs(300, 7, 2, seed=4) if consistent else [synthetic_traj(300, 7, 1), synthetic_traj(260, 7, 2)]
            process = None if consistent else eng.BSMS_Simulator(model_cfg(False)).cuda().process
            kw = dict(dataset="airfoil" if consistent else "cylinder_flow", seed=SEED, process=process)
            aug = eng.Augment(reflect=True)
            made = [eng.TrajectoryBank(dcfg, augment=aug, **kw), eng.TrajectoryBank(dcfg, **kw),
                    eng.TrajectoryBank(dcfg, augment=aug, horizon=3, **kw), eng.TrajectoryBank(dcfg, horizon=3, **kw)]
            for b in made:
                for t in trajs:
                    b.add(t)
            cache[consistent] = (trajs, *made)
        return cache[consistent]
    return get


PICKS = [(0, 3), (1, 0), (1, 3), (0, 1)]


@pytest.mark.parametrize("consistent", [True, False])
def test_bank_draws_applies_and_reports_its_transforms(eng, banks, consistent):
    trajs, aug, plain, _, _ = banks(consistent)
    assert aug.vector_groups == (0,) and aug.fields == {"velocity": (0, 2), "density": (2, 1)}
    rows = [trajs[si]["velocity"].shape[1] for si, _ in PICKS]
    batch, noise, xf = aug.batch(PICKS, draw=DRAW, return_noise=True, return_transforms=True)
    assert isinstance(xf, np.ndarray) and np.array_equal(xf, eng.Augment(reflect=True).sample(2, 4, SEED, DRAW))
    got = node_tensors(batch, consistent)
    again = node_tensors(aug.batch(PICKS, draw=DRAW), consistent)
    other = node_tensors(aug.batch(PICKS, draw=DRAW + 1), consistent)
    assert all(torch.equal(a, b) for a, b in zip(got, again))
    assert not torch.equal(got[0], other[0]) and not torch.equal(got[0][:, 3:5], other[0][:, 3:5])        # other noise AND other frames
    # the contract, from the un-augmented clean batch: transform, then the plain bank's noise of the same draw
    clean = node_tensors(plain.batch(PICKS, train=False), consistent)
    plain_batch, plain_noise = plain.batch(PICKS, draw=DRAW, return_noise=True)
    assert torch.equal(noise, plain_noise)
    noise = noise.reshape(-1, 3).cpu()
    y_in, y_tar = restate_rows(clean[0].cpu(), rows, xf, [0, 3]), restate_rows(clean[1].cpu(), rows, xf, [0])
    assert torch.equal(got[0].cpu()[:, :3], y_in[:, :3] + noise) and torch.equal(got[0].cpu()[:, 3:], y_in[:, 3:])
    assert torch.equal(got[1].cpu(), y_tar + torch.tensor(np.float32(1.0 - GAMMA)) * noise) and torch.equal(got[2], clean[2])
    # evaluation batches stay in the data's frame; explicit matrices are applied whatever `train` says, by either bank
    for a, b in zip(node_tensors(aug.batch(PICKS, train=False), consistent), clean):
        assert torch.equal(a, b)
    assert aug.batch(PICKS, train=False, return_transforms=True)[1] is None
    for bank, matrices in ((aug, xf), (plain, torch.tensor(xf).cuda()), (plain, xf.astype(np.float64))):
        for a, b in zip(node_tensors(bank.batch(PICKS, draw=DRAW, transforms=matrices), consistent), got):
            assert torch.equal(a, b)
    turned = node_tensors(plain.batch(PICKS, train=False, transforms=xf), consistent)
    assert torch.equal(turned[0].cpu(), y_in) and torch.equal(turned[1].cpu(), y_tar)
    with pytest.raises(ValueError):
        plain.batch(PICKS, transforms=xf[:3])
    # draw=None: the running counter selects noise and frames alike
    first, second = aug.batch(PICKS, return_transforms=True)[1], aug.batch(PICKS, return_transforms=True)[1]
    assert not np.array_equal(first, second)


@pytest.mark.parametrize("consistent", [True, False])
def test_bank_without_augment_makes_the_plain_entrys_batches(eng, banks, consistent):
    """What the bank gave before the feature, restated through bsms_batch_assemble on tensors uploaded here."""
    trajs, _, plain, _, _ = banks(consistent)
    raw = Raw(eng, [trajs[si]["velocity"].shape[1] for si, _ in PICKS], 2, 3)
    raw.keep = []
    for k, (si, ti) in enumerate(PICKS):
        tr = trajs[si]
        state = np.concatenate([tr["velocity"], tr["density"]], -1)
        t = [torch.tensor(np.ascontiguousarray(a)).cuda() for a in (state[ti], state[ti + 1], tr["mesh_pos"][ti], tr["node_type"][ti, :, 0])]
        raw.keep.append(t)
        s = raw.table[k]
        s.state_in, s.state_tar, s.pos, s.type = (v.data_ptr() for v in t)
    raw.std = (C.c_float * 3)(*[float(v) for v in plain.cfg.noise_level])
    codes = (0.0,) if consistent else (0.0, 5.0)                                        # the airfoil / cylinder banks of the fixture
    raw.valid = (C.c_float * len(codes))(*codes)
    for noisy in (False, True):
        want = raw.assemble(noisy=noisy)
        batch, noise = plain.batch(PICKS, train=noisy, draw=DRAW, return_noise=True)
        assert all(torch.equal(a.cpu(), b) for a, b in zip([*node_tensors(batch, consistent), noise.reshape(-1, 3)], want))


@pytest.mark.parametrize("consistent", [True, False])
def test_bank_horizon_transforms_the_later_targets(eng, banks, consistent):
    trajs, aug, _, aug3, plain3 = banks(consistent)
    rows = [trajs[si]["velocity"].shape[1] for si, _ in PICKS]
    batch, later, xf = aug3.batch(PICKS, draw=DRAW, return_transforms=True)
    _, later_plain = plain3.batch(PICKS, draw=DRAW)
    assert later.shape == later_plain.shape and later.shape[0] == 2 and not torch.equal(later, later_plain)
    want = eng.transform_rows(later_plain.reshape(2, -1, 3), rows, xf, aug3.vector_groups)
    assert torch.equal(later.reshape(2, -1, 3), want)
    assert torch.equal(want.cpu(), torch.stack([restate_rows(later_plain.reshape(2, -1, 3)[j].cpu(), rows, xf, [0]) for j in range(2)]))
    for a, b in zip(node_tensors(batch, consistent), node_tensors(aug.batch(PICKS, draw=DRAW), consistent)):
        assert torch.equal(a, b)                                                        # the first step is the horizon-1 batch


def test_bank_refuses_fields_that_are_no_vectors(eng):
    dcfg = make_cfg(True)
    bank = eng.TrajectoryBank(dcfg, augment=eng.Augment(vector_fields=("density",)))
    with pytest.raises(ValueError):
        bank.add(synthetic_traj(60, 3, 0))                                              # 1 component, 2-D positions
    dcfg = make_cfg(True)
    dcfg.augment_reflect = True
    assert eng.TrajectoryBank(dcfg).augment == eng.Augment(rotate=False, reflect=True)


# ------------------------------------------------------------------------------------------------ 4: equivariance, training
@pytest.mark.parametrize("consistent", [True, False])
def test_equivariance_error(eng, banks, consistent):
    trajs, _, plain, _, _ = banks(consistent)
    torch.manual_seed(0)
    mcfg = model_cfg(consistent)
    tr = eng.Trainer(eng.BSMS_Simulator(mcfg), mcfg, OPT)
    tr.iter(plain.batch(PICKS, train=False))                                            # warm-up: normaliser statistics
    batch = plain.batch(PICKS, train=False)
    rows = None if consistent else [trajs[si]["velocity"].shape[1] for si, _ in PICKS]
    eye = np.tile(np.eye(2, dtype=np.float32), (4, 1, 1))
    zero = eng.equivariance_error(tr, batch, eye, plain.vector_groups, rows_per_sample=rows)
    assert zero.shape == (3,) and zero.dtype == torch.float64 and bool((zero == 0).all())
    quarter = np.tile(np.array([[0, -1], [1, 0]], np.float32), (4, 1, 1))
    err = eng.equivariance_error(tr, batch, quarter, plain.vector_groups, rows_per_sample=rows)
    print(f"[equivariance {'consistent' if consistent else 'variable'}] 90 degrees, fresh model: {err.tolist()}")
    assert bool(torch.isfinite(err).all()) and bool((err > 0).all())


def test_trainer_on_augmented_batches(eng):
    """Six bank batches, three of them warm-up: finite losses, bit-equal between two runs with the same seeds, different from the
    run without augmentation."""
    dcfg = make_cfg(True, gamma=GAMMA)
    dcfg.noise_level = [0.02, 0.02, 0.01]
    trajs = field_trajs(300, 9, 2, seed=6)

    def run(augment):
        torch.manual_seed(0)
        mcfg = model_cfg(True, warmup=3)
        tr = eng.Trainer(eng.BSMS_Simulator(mcfg), mcfg, OPT)
        bank = eng.TrajectoryBank(dcfg, seed=3, augment=augment)
        for t in trajs:
            bank.add(t)
        losses = [tr.iter(bank.sample(4)) for _ in range(6)]
        assert all(v is None for v in losses[:3])
        return torch.stack(losses[3:]).cpu(), tr.optimizer.flat_p.clone()

    aug = eng.Augment(reflect=True)
    (a, pa), (b, pb), (c, pc) = run(aug), run(aug), run(None)
    print(f"[trainer] losses with augmentation {a.tolist()}, without {c.tolist()}")
    assert bool(torch.isfinite(a).all()) and torch.equal(a, b) and torch.equal(pa, pb)
    assert not torch.equal(a, c) and not torch.equal(pa, pc)
