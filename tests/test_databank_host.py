"""CPU: the host side of the device-resident trajectory bank (bsms_gnn_amd/databank.py, include/bsms_hip.h: bsms_batch_assemble).

  * the noise contract restated in NumPy (Philox4x32-10 + Box-Muller in fp64) reproduces the published known answers of
    Philox4x32-10, and its normals pass -- at the seed / draw values and the size the GPU tests use -- the statistical
    bounds the GPU tests apply to the kernel's noise, so those bounds can be met;
  * bsms_batch_assemble validates its arguments before any device call;
  * the sampler's default order is datapipe.TrajectoryDataset's.
tests/test_hip_databank.py imports the restatement from here."""
import ctypes as C

import numpy as np
import pytest
import torch

from test_datapipe import cfg as make_cfg, synthetic_traj

SEED, DRAW = 0x1234ABCD5678, 7          # what the GPU tests pass as (seed, draw)
AIRFOIL_ROWS, AIRFOIL_C = 8 * 5233, 3
M32 = np.uint64(0xFFFFFFFF)


def philox4x32_10(ctr, key):
    """ctr: 4 uint32 arrays (or scalars), key: 2 uint32 scalars -> 4 uint32 arrays."""
    c = [np.asarray(v, dtype=np.uint64) & M32 for v in ctr]
    c = list(np.broadcast_arrays(*c))
    k0, k1 = np.uint64(key[0]), np.uint64(key[1])
    for _ in range(10):
        m0, m1 = np.uint64(0xD2511F53) * c[0], np.uint64(0xCD9E8D57) * c[2]
        c = [(m1 >> np.uint64(32)) ^ c[1] ^ k0, m1 & M32, (m0 >> np.uint64(32)) ^ c[3] ^ k1, m0 & M32]
        k0, k1 = (k0 + np.uint64(0x9E3779B9)) & M32, (k1 + np.uint64(0xBB67AE85)) & M32
    return [v.astype(np.uint32) for v in c]


def normals(rows, channels, seed, draw, row0=0):
    """z [rows, channels] in fp64: the standard normals of the noise contract for batch-global rows row0 .. row0 + rows - 1."""
    r = np.arange(row0, row0 + rows, dtype=np.uint64)
    out = np.empty((rows, channels), np.float64)
    for q in range((channels + 3) // 4):
        x = philox4x32_10((r, q, draw & 0xFFFFFFFF, draw >> 32), (seed & 0xFFFFFFFF, seed >> 32))
        u = [((v >> np.uint32(8)).astype(np.float64) + 0.5) * 2.0 ** -24 for v in x]
        z = []
        for a, b in ((u[0], u[1]), (u[2], u[3])):
            rad = np.sqrt(-2.0 * np.log(a))
            z += [rad * np.cos(2.0 * np.pi * b), rad * np.sin(2.0 * np.pi * b)]
        for j in range(4):
            if 4 * q + j < channels:
                out[:, 4 * q + j] = z[j]
    return out


def check_noise_statistics(z, label=""):
    """z [n, C]: samples that should be iid N(0, 1) (the caller divides by std_c).  Five-sigma bounds of the sampling
    distributions: mean ~ 1/sqrt(n), std ~ 1/sqrt(2n), kurtosis ~ sqrt(24/n), correlations ~ 1/sqrt(n)."""
    z = np.asarray(z, np.float64)
    n, ch = z.shape
    for c in range(ch):
        v = z[:, c]
        mean, std = v.mean(), v.std()
        kurt = ((v - mean) ** 4).mean() / std ** 4
        lag1 = np.corrcoef(v[:-1], v[1:])[0, 1]
        print(f"[noise statistics{label}] channel {c}: n {n} mean {mean:+.2e} (bound {5 / np.sqrt(n):.2e}) std-1 {std - 1:+.2e} "
              f"(bound {5 / np.sqrt(2 * n):.2e}) kurtosis-3 {kurt - 3:+.2e} (bound {5 * np.sqrt(24 / n):.2e}) lag-1 {lag1:+.2e}")
        assert abs(mean) <= 5 / np.sqrt(n)
        assert abs(std - 1) <= 5 / np.sqrt(2 * n)
        assert abs(kurt - 3) <= 5 * np.sqrt(24 / n)
        assert abs(lag1) <= 5 / np.sqrt(n)
        for d in range(c + 1, ch):
            cross = np.corrcoef(v, z[:, d])[0, 1]
            print(f"[noise statistics{label}] channels {c},{d}: correlation {cross:+.2e} (bound {5 / np.sqrt(n):.2e})")
            assert abs(cross) <= 5 / np.sqrt(n)


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__
    __graft_entry__.build()
    from bsms_gnn_amd import _abi
    return _abi.lib()


def test_philox_known_answers():
    kat = [((0, 0, 0, 0), (0, 0), (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)),
           ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)),
           ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0), (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1))]
    for ctr, key, want in kat:
        got = tuple(int(v) for v in philox4x32_10(ctr, key))
        assert got == want, ([hex(v) for v in got], [hex(v) for v in want])
    # vectorised over the first counter word as `normals` uses it
    rows = philox4x32_10((np.array([0, 0x243F6A88], np.uint64), np.array([0, 0x85A308D3], np.uint64), np.array([0, 0x13198A2E], np.uint64),
                          np.array([0, 0x03707344], np.uint64)), (0, 0))
    assert tuple(int(v[0]) for v in rows) == kat[0][2]


def test_restatement_statistics_at_airfoil_size():
    z = normals(AIRFOIL_ROWS, AIRFOIL_C, SEED, DRAW)
    assert np.isfinite(z).all() and np.abs(z).max() <= 5.9
    check_noise_statistics(z, " fp64 restatement")
    assert not np.array_equal(z, normals(AIRFOIL_ROWS, AIRFOIL_C, SEED, DRAW + 1))
    assert not np.array_equal(z, normals(AIRFOIL_ROWS, AIRFOIL_C, SEED + 1, DRAW))
    np.testing.assert_array_equal(z[1000:1100], normals(100, AIRFOIL_C, SEED, DRAW, row0=1000))     # a row's noise depends on the row alone


def test_symbol_bound(lib):
    from bsms_gnn_amd import _abi
    assert "bsms_batch_assemble" in _abi.SIGNATURES
    assert lib.bsms_batch_assemble.argtypes == _abi.SIGNATURES["bsms_batch_assemble"][1]
    assert lib.bsms_abi_version() == 4


def test_argument_validation(lib):
    """Return codes of the envelope, checked before any device call (no GPU here): pointers are never dereferenced on the device."""
    from bsms_gnn_amd.databank import _Sample
    OK, INVALID, UNSUPPORTED = 0, -1, -3
    table = (_Sample * 2)()
    buf = np.zeros(64, np.float32)
    for s in table:
        s.state_in = s.state_tar = s.pos = s.type = buf.ctypes.data
        s.n = 0                                             # zero rows: even a valid call launches nothing
    std = (C.c_float * 8)(*[1.0] * 8)
    valid = (C.c_float * 4)(0.0, 5.0, 0.0, 0.0)
    out = buf.ctypes.data

    def call(samples=C.addressof(table), n=2, ch=3, p=2, noise=C.addressof(std), codes=C.addressof(valid), nv=1, node_in=out,
             node_tar=out, mask=out, noise_out=None):
        return lib.bsms_batch_assemble(samples, n, ch, p, noise, 0.8, codes, nv, SEED, DRAW, node_in, node_tar, mask, noise_out, None)

    assert call() == OK
    assert call(noise=None) == OK and call(noise_out=out) == OK
    for ch in (0, 9, -1):
        assert call(ch=ch) == UNSUPPORTED
    for ch in (1, 8):
        assert call(ch=ch) == OK
    for p in (0, 8):
        assert call(p=p) == UNSUPPORTED
    for p in (1, 7):
        assert call(p=p) == OK
    for nv in (0, 5):
        assert call(nv=nv) == UNSUPPORTED
    for nv in (1, 4):
        assert call(nv=nv) == OK
    assert call(n=0, samples=None, codes=None, node_in=None, node_tar=None, mask=None) == OK      # nothing to do: no launch, nothing read
    assert call(n=0, ch=9) == UNSUPPORTED                                                           # the envelope is checked first
    for kw in (dict(samples=None), dict(codes=None), dict(node_in=None), dict(node_tar=None), dict(mask=None)):
        assert call(**kw) == INVALID, kw
    table[1].n = 5
    table[1].pos = None
    assert call() == INVALID                                # a sample with rows and a null field
    table[1].pos = buf.ctypes.data
    table[1].n = -1
    assert call() == UNSUPPORTED
    table[1].n = 1 << 40
    assert call() == UNSUPPORTED


@pytest.mark.parametrize("seed", [0, 5])
def test_sampler_order_is_the_datasets(lib, seed):
    """`epoch_picks` (behind TrajectoryBank.sample) against the (trajectory, frame) sequence datapipe.TrajectoryDataset yields for the
    same seed and lengths, over two epochs (the generator carries on).  Frames are recognised by a marker in the density field."""
    import bsms_gnn_amd.datapipe as dp
    from bsms_gnn_amd.databank import epoch_picks
    lengths, trajs = [5, 3, 7, 4], []
    for si, n_frames in enumerate(lengths):
        tr = synthetic_traj(40, n_frames + 1, 10 + si)
        tr["density"] = np.broadcast_to((100.0 * si + np.arange(n_frames + 1, dtype=np.float32))[:, None, None], tr["density"].shape).copy()
        trajs.append(tr)
    ds = dp.TrajectoryDataset(make_cfg(True), trajs, mode="valid", seed=seed)
    rng = np.random.default_rng(seed)
    for _ in range(2):
        seen = [divmod(int(node_in[0, 2]), 100) for node_in, *_ in ds]
        assert len(seen) == sum(lengths)
        assert epoch_picks(rng, lengths) == seen
    pairs = epoch_picks(np.random.default_rng(seed), lengths, order="global")
    assert sorted(pairs) == [(si, ti) for si, n in enumerate(lengths) for ti in range(n)] and pairs != sorted(pairs)
