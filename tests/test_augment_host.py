"""CPU: the host side of frame augmentation (bsms_gnn_amd/databank.py: Augment, include/bsms_hip.h: bsms_batch_assemble_xf,
bsms_rows_transform).

  * both entries are declared, exported and bound;
  * they refuse what the header says they refuse, in the documented order and before any device call (there is no GPU here:
    a device call would fail with BSMS_E_HIP, a dereferenced device pointer would crash);
  * Augment.sample gives orthogonal matrices of the right determinant and angle, as a function of (seed, draw, k) alone;
  * Augment / from_cfg / TrajectoryBank(augment=) validate their arguments.
tests/test_hip_augment.py imports the torch restatement of the transform from here."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT
from test_datapipe import cfg as make_cfg

OK, INVALID, UNSUPPORTED = 0, -1, -3
SEED, DRAW = 0x1234ABCD5678, 7
EPS = 2.0 ** -24


def restate(v, q):
    """Q v in the entry's arithmetic, as separate fp32 torch ops: v [R, p], q [R, p, p] (one matrix per row), every product and
    every sum its own rounding, b ascending."""
    p = v.shape[-1]
    cols = []
    for a in range(p):
        acc = q[:, a, 0] * v[:, 0]
        for b in range(1, p):
            t = q[:, a, b] * v[:, b]
            acc = acc + t
        cols.append(acc)
    return torch.stack(cols, -1)


def restate_rows(x, rows, xf, groups, transpose=False):
    """x [R, C] (fp32, any device) with the first sum(rows) rows cut into segments: every group [f, f+p) becomes Q v."""
    xf = torch.as_tensor(xf, dtype=torch.float32, device=x.device)
    if transpose:
        xf = xf.transpose(1, 2)
    p, total = xf.shape[-1], int(sum(rows))
    q = torch.repeat_interleave(xf, torch.as_tensor(list(rows), device=x.device), dim=0)     # [total, p, p]
    out = x.clone()
    for f in groups:
        out[:total, f:f + p] = restate(x[:total, f:f + p], q)
    return out


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__
    __graft_entry__.build()
    from bsms_gnn_amd import _abi
    return _abi.lib()


def test_both_entries_are_declared_exported_and_bound(lib):
    from bsms_gnn_amd import _abi
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "bsms_hip.h")).read(), flags=re.S)
    raw = C.CDLL(_abi.LIB_PATH)
    for name, nargs in (("bsms_batch_assemble_xf", 18), ("bsms_rows_transform", 13)):
        m = re.search(name + r"\s*\(([^;]*)\)\s*;", text)
        assert m, f"{name} is not declared in include/bsms_hip.h"
        assert len(m.group(1).split(",")) == len(_abi.SIGNATURES[name][1]) == nargs
        assert hasattr(raw, name) and getattr(lib, name).argtypes == _abi.SIGNATURES[name][1]
    assert lib.bsms_abi_version() == 4


def test_batch_assemble_xf_refusals(lib):
    from bsms_gnn_amd.databank import _Sample
    table = (_Sample * 2)()
    buf = np.zeros(64, np.float32)
    for s in table:
        s.state_in = s.state_tar = s.pos = s.type = buf.ctypes.data
        s.n = 0                                             # zero rows: a valid call launches nothing
    std = (C.c_float * 8)(*[1.0] * 8)
    valid = (C.c_float * 4)(0.0, 5.0, 0.0, 0.0)
    xf = np.tile(np.eye(3, dtype=np.float32), (2, 1, 1))
    out = buf.ctypes.data

    def groups(*first):
        return (C.c_int32 * max(len(first), 1))(*first), len(first)

    def call(samples=C.addressof(table), n=2, ch=3, p=2, mats=xf.ctypes.data, vec=groups(0), noise=C.addressof(std), codes=C.addressof(valid),
             nv=1, node_in=out, node_tar=out, mask=out, noise_out=None, n_vec=None, vec_ptr=True):
        first, count = vec
        return lib.bsms_batch_assemble_xf(samples, n, ch, p, mats, C.addressof(first) if vec_ptr else None, count if n_vec is None else n_vec,
                                          noise, 0.8, codes, nv, SEED, DRAW, node_in, node_tar, mask, noise_out, None)

    assert call() == OK and call(noise=None) == OK and call(noise_out=out) == OK
    assert call(vec=groups()) == OK and call(vec=groups(), vec_ptr=False) == OK             # no vector field: only the positions turn
    # 1: the envelope
    for ch in (0, 9, -1):
        assert call(ch=ch, vec=groups()) == UNSUPPORTED
    for p in (1, 4, 0, 7):
        assert call(p=p) == UNSUPPORTED
    for nv in (0, 5):
        assert call(nv=nv) == UNSUPPORTED
    for n_vec in (-1, 5):
        assert call(n_vec=n_vec) == UNSUPPORTED
    assert call(ch=8, p=3, vec=groups(0, 3)) == OK and call(ch=8, vec=groups(0, 2, 4, 6)) == OK and call(ch=2) == OK
    assert call(ch=9, vec=groups(8)) == UNSUPPORTED and call(ch=9, n=-1) == UNSUPPORTED     # ... comes before everything else
    # 2: the sample count
    assert call(n=-1) == INVALID and call(n=-1, vec=groups(2)) == INVALID
    # 3: the groups -- also for an empty batch
    assert call(vec_ptr=False) == INVALID                                                   # n_vec = 1 without a table
    for bad in (groups(2), groups(-1), groups(0, 1), groups(1, 0), groups(0, 0)):           # overruns C = 3, negative, overlaps
        assert call(vec=bad) == INVALID and call(vec=bad, n=0) == INVALID, list(bad[0])
    assert call(ch=4, p=3, vec=groups(2)) == INVALID and call(ch=4, p=3, vec=groups(1)) == OK
    assert call(ch=8, vec=groups(0, 2, 5, 6)) == INVALID and call(ch=8, p=3, vec=groups(0, 3, 6)) == INVALID
    # 4: nothing to do
    assert call(n=0, samples=None, mats=None, codes=None, node_in=None, node_tar=None, mask=None) == OK
    # 5: null pointers
    for kw in (dict(samples=None), dict(mats=None), dict(codes=None), dict(node_in=None), dict(node_tar=None), dict(mask=None)):
        assert call(**kw) == INVALID, kw
    # 6: the samples
    table[1].n = 5
    table[1].pos = None
    assert call() == INVALID
    table[1].pos = buf.ctypes.data
    table[1].n = -1
    assert call() == UNSUPPORTED
    table[1].n = 1 << 40
    assert call() == UNSUPPORTED


def test_rows_transform_refusals(lib):
    buf = np.zeros(64, np.float32)
    xf = np.tile(np.eye(3, dtype=np.float32), (2, 1, 1))
    rows = (C.c_int64 * 2)(0, 0)
    ptr = buf.ctypes.data

    def groups(*first):
        return (C.c_int32 * max(len(first), 1))(*first), len(first)

    def call(x=ptr, out=ptr, F=1, R=4, ch=3, table=C.addressof(rows), n=2, p=2, mats=xf.ctypes.data, transpose=0, vec=groups(0), n_vec=None,
             vec_ptr=True):
        first, count = vec
        return lib.bsms_rows_transform(x, out, F, R, ch, table, n, p, mats, transpose, C.addressof(first) if vec_ptr else None,
                                       count if n_vec is None else n_vec, None)

    assert call() == OK and call(transpose=1) == OK and call(vec=groups()) == OK and call(F=65535) == OK     # 0-row segments: no launch
    for ch in (0, 17, -1):
        assert call(ch=ch, vec=groups()) == UNSUPPORTED
    assert call(ch=16, vec=groups(14)) == OK and call(ch=12, p=3, vec=groups(0, 8)) == OK                   # node_in rows: C + p + 1
    for p in (1, 4):
        assert call(p=p) == UNSUPPORTED
    for n_vec in (-1, 5):
        assert call(n_vec=n_vec) == UNSUPPORTED
    assert call(F=65536) == UNSUPPORTED and call(F=65536, n=-1) == UNSUPPORTED
    assert call(n=-1) == INVALID and call(F=-1) == INVALID and call(R=-1) == INVALID
    assert call(vec_ptr=False) == INVALID
    for bad in (groups(2), groups(-1), groups(0, 1), groups(0, 0)):
        assert call(vec=bad) == INVALID and call(vec=bad, n=0) == INVALID and call(vec=bad, F=0) == INVALID, list(bad[0])
    assert call(n=0, x=None, out=None, table=None, mats=None) == OK and call(F=0, x=None, out=None, table=None, mats=None) == OK
    for kw in (dict(x=None), dict(out=None), dict(table=None), dict(mats=None)):
        assert call(**kw) == INVALID, kw
    rows[0] = -1
    assert call() == UNSUPPORTED
    rows[0] = 1 << 40
    assert call() == UNSUPPORTED
    rows[0], rows[1] = 3, 2
    assert call(R=4) == INVALID                             # five rows in the table, four in a frame


@pytest.mark.parametrize("p", [2, 3])
def test_sampled_transforms_are_rigid(lib, p):
    """|Q^T Q - I| <= 8 * 2^-24 per entry: an entry of the exactly orthogonal fp64 matrix has magnitude <= 1 and is rounded to fp32
    with an error <= 2^-25; an entry of Q^T Q sums p <= 3 products of two such entries, so it moves by at most
    3 * (2 * 2^-25 + 2^-50) < 4 * 2^-24, and the fp64 evaluation of the formulas is itself orthogonal to ~1e-15."""
    from bsms_gnn_amd import Augment
    eye = np.eye(p)
    for max_angle in (math.pi, 0.5):
        aug = Augment(max_angle=max_angle)
        q = aug.sample(p, 64, SEED, DRAW)
        assert q.shape == (64, p, p) and q.dtype == np.float32 and q.flags.c_contiguous
        q64 = q.astype(np.float64)
        defect = np.abs(np.einsum("nba,nbc->nac", q64, q64) - eye).max()
        print(f"[augment p={p} max_angle={max_angle:.2f}] orthogonality defect {defect:.2e} (bound {8 * EPS:.2e})")
        assert defect <= 8 * EPS
        assert np.abs(np.linalg.det(q64) - 1.0).max() <= 1e-6                         # proper rotations without `reflect`
        # the angle from the antisymmetric part and the trace: atan2 of two numbers each within 3 * 2^-25 of (sin, cos)
        if p == 2:
            angle = np.arctan2(q64[:, 1, 0], q64[:, 0, 0])
        else:
            vee = 0.5 * np.stack([q64[:, 2, 1] - q64[:, 1, 2], q64[:, 0, 2] - q64[:, 2, 0], q64[:, 1, 0] - q64[:, 0, 1]], -1)
            angle = np.arctan2(np.linalg.norm(vee, axis=-1), 0.5 * (np.trace(q64, axis1=1, axis2=2) - 1.0))
        assert np.abs(angle).max() <= max_angle + 1e-6
        assert np.abs(angle).max() > 0.5 * max_angle                                   # ... and the range is used
    both = Augment(reflect=True).sample(p, 64, SEED, DRAW)
    det = np.linalg.det(both.astype(np.float64))
    assert np.abs(np.abs(det) - 1.0).max() <= 1e-6 and (det > 0).any() and (det < 0).any()
    assert np.abs(np.einsum("nba,nbc->nac", both.astype(np.float64), both.astype(np.float64)) - eye).max() <= 8 * EPS
    # a reflection alone: identity or diag(-1, 1, ..)
    flips = Augment(rotate=False, reflect=True).sample(p, 64, SEED, DRAW)
    assert all(np.array_equal(m, np.eye(p, dtype=np.float32)) or np.array_equal(m, np.diag([-1.0] + [1.0] * (p - 1)).astype(np.float32)) for m in flips)
    assert np.array_equal(np.linalg.det(flips.astype(np.float64)) < 0, det < 0)        # the same samples are reflected


@pytest.mark.parametrize("p", [2, 3])
def test_sampled_transforms_depend_on_seed_draw_and_position_only(lib, p):
    from bsms_gnn_amd import Augment
    aug = Augment(reflect=True)
    a = aug.sample(p, 8, SEED, DRAW)
    assert np.array_equal(a, aug.sample(p, 8, SEED, DRAW))
    assert not np.array_equal(a, aug.sample(p, 8, SEED, DRAW + 1)) and not np.array_equal(a, aug.sample(p, 8, SEED + 1, DRAW))
    assert np.array_equal(a, aug.sample(p, 48, SEED, DRAW)[:8])                        # sample k of 8 is sample k of 48
    assert np.array_equal(aug.sample(p, 3, (1 << 64) - 1, (1 << 64) - 1), aug.sample(p, 3, -1, -1))      # 64-bit seeds and draws, like the noise


def test_augment_validation_and_from_cfg(lib):
    from bsms_gnn_amd import Augment, TrajectoryBank
    for bad in (0.0, -1.0, math.pi + 1e-6, float("nan")):
        with pytest.raises(ValueError):
            Augment(max_angle=bad)
    Augment(max_angle=math.pi), Augment(max_angle=1e-3)
    for bad in (("velocity", 3), (None,), "velocity"):
        with pytest.raises(ValueError):
            Augment(vector_fields=bad)
    aug = Augment()
    assert (aug.rotate, aug.max_angle, aug.reflect, aug.vector_fields) == (True, math.pi, False, ("velocity",))
    with pytest.raises(Exception):
        aug.reflect = True                                                             # frozen
    with pytest.raises(ValueError):
        aug.sample(4, 2, 0, 0)
    assert Augment(vector_fields=["velocity", "momentum"]).vector_fields == ("velocity", "momentum")
    cfg = make_cfg(True)
    assert Augment.from_cfg(cfg) is None                                               # a config without the keys: as today
    cfg.augment_max_angle, cfg.vector_fields = 0.25, ["velocity"]
    assert Augment.from_cfg(cfg) is None                                               # neither rotate nor reflect asked for
    cfg.augment_rotate = True
    assert Augment.from_cfg(cfg) == Augment(max_angle=0.25)
    cfg.augment_rotate, cfg.augment_reflect = False, True
    assert Augment.from_cfg(cfg) == Augment(rotate=False, reflect=True, max_angle=0.25)
    cfg.augment_max_angle = 4.0
    with pytest.raises(ValueError):
        Augment.from_cfg(cfg)
    # the bank checks the names against cfg.output_field_names before it looks for a device
    for names in (("pressure",), ("velocity", "velocity")):
        with pytest.raises(ValueError):
            TrajectoryBank(make_cfg(True), augment=Augment(vector_fields=names))
    with pytest.raises(ValueError):
        TrajectoryBank(make_cfg(True), augment="rotate")
    cfg = make_cfg(True)
    cfg.augment_rotate, cfg.vector_fields = True, ["pressure"]
    with pytest.raises(ValueError):
        TrajectoryBank(cfg)                                                            # augment=None falls back to from_cfg


def test_restatement_is_plain_fp32_arithmetic():
    """The torch restatement the GPU tests compare against: separate roundings (it differs from an FMA evaluation), identity and
    transpose behave."""
    rng = np.random.default_rng(0)
    v = torch.tensor(rng.standard_normal((4096, 3)).astype(np.float32))
    q = torch.tensor(rng.standard_normal((4096, 3, 3)).astype(np.float32))
    y = restate(v, q)
    exact = torch.einsum("rab,rb->ra", q.double(), v.double())
    bound = 4 * EPS * torch.einsum("rab,rb->ra", q.double().abs(), v.double().abs())   # p products and p - 1 sums, each within 2^-24 (1 + 2^-24) sum |q||v|
    assert bool(((y.double() - exact).abs() <= bound).all())
    fused = torch.einsum("rab,rb->ra", q.double(), v.double()).float()                 # one rounding: what an FMA chain approaches
    assert not torch.equal(y, fused)
    x = torch.tensor(rng.standard_normal((10, 4)).astype(np.float32))
    eye = np.tile(np.eye(3, dtype=np.float32), (2, 1, 1))
    assert torch.equal(restate_rows(x, [3, 5], eye, [1]), x)
    m = rng.standard_normal((2, 3, 3)).astype(np.float32)
    assert torch.equal(restate_rows(x, [3, 5], m, [1], transpose=True), restate_rows(x, [3, 5], m.transpose(0, 2, 1).copy(), [1]))
    assert torch.equal(restate_rows(x, [3, 5], m, [1])[8:], x[8:])                     # rows past the table
