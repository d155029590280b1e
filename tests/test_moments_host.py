"""Host (no GPU): the dataset statistics' third shared library (include/bsms_hip_stats.h, libbsms_hip_stats.so, _abi.STATS_SIGNATURES)
-- what it declares, exports and binds, and the order in which bsms_moment_sums / bsms_moment_fold refuse their arguments -- and the
closed form of `Moments.normalizer_stats` on CPU tensors against a NumPy fp64 restatement."""
import ctypes as C
import os
import re
import subprocess
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from conftest import ROOT

ENTRIES = {"bsms_moment_work_bytes": 1, "bsms_moment_sums": 8, "bsms_moment_fold": 5}


@pytest.fixture(scope="module")
def eng():
    import bsms_gnn_amd as eng
    return eng


def declared(text, name):
    decl = re.search(r"\b" + name + r"\s*\(([^;]*)\)\s*;", text)
    return None if decl is None else len([a for a in decl.group(1).split(",") if a.strip() not in ("", "void")])


def test_the_third_library_declares_exports_and_binds_the_same_entries(eng):
    _abi = eng._abi
    strip = lambda path: re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", path)).read(), flags=re.S)
    text, ext_text, stats_text = strip("bsms_hip.h"), strip("bsms_hip_ext.h"), strip("bsms_hip_stats.h")
    names = set(re.findall(r"\b(bsms_[a-z0-9_]+)\s*\(", stats_text))
    out = subprocess.run(["nm", "-D", "--defined-only", _abi.STATS_LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if ln.split() and ln.split()[-1].startswith("bsms_") and ln.split()[-2] in ("T", "t", "W")}
    assert names == set(ENTRIES) == set(_abi.STATS_SIGNATURES) == exported
    raw = C.CDLL(_abi.LIB_PATH), C.CDLL(_abi.EXT_LIB_PATH)
    for name, nargs in ENTRIES.items():
        assert declared(stats_text, name) == nargs and len(_abi.STATS_SIGNATURES[name][1]) == nargs, name
        assert declared(text, name) is None and declared(ext_text, name) is None, name
        assert name not in _abi.SIGNATURES and name not in _abi.EXT_SIGNATURES, name
        assert not any(hasattr(r, name) for r in raw), name
    assert os.path.basename(_abi.STATS_LIB_PATH) == "libbsms_hip_stats.so"
    assert C.sizeof(_abi.MomentTraj) == 48 and [f[0] for f in _abi.MomentTraj._fields_] == ["state", "type", "n", "frame0", "frames", "type_stride"]
    for doc in ("INTEGRATION.md", "README.md", "DESIGN.md"):
        body = open(os.path.join(ROOT, doc)).read()
        assert "bsms_moment_sums" in body and "bsms_hip_stats" in body, doc


def test_refusal_order_without_gpu(eng):
    L, X = eng._abi.lib(), eng._abi.stats()
    one = C.c_double(0.0)
    ptr = C.addressof(one)                               # a non-null pointer that is never dereferenced: every call below fails first
    table = (eng._abi.MomentTraj * 2)()

    def entry(k, n=5, frame0=0, frames=2, stride=0, state=ptr, typ=ptr):
        e = table[k]
        e.state, e.type, e.n, e.frame0, e.frames, e.type_stride = state, typ, n, frame0, frames, stride

    def sums(S=2, Cn=3, n_valid=1, trajs=C.addressof(table), valid=ptr, out=ptr, work=ptr):
        return X.bsms_moment_sums(trajs, S, Cn, valid, n_valid, out, work, None)

    entry(0), entry(1)
    UNSUPPORTED, INVALID, SHAPE = -3, -1, -2
    # 1. C and n_valid before anything else
    assert sums(Cn=0) == UNSUPPORTED and sums(Cn=9) == UNSUPPORTED and b"C in 1..8" in L.bsms_last_error()
    assert sums(n_valid=0) == UNSUPPORTED and sums(n_valid=5) == UNSUPPORTED
    assert sums(Cn=9, S=-1, trajs=None, valid=None, out=None, work=None) == UNSUPPORTED
    assert sums(n_valid=5, S=-1, trajs=None) == UNSUPPORTED
    # 2. S < 0 before the pointers; 3. S == 0 is fine with nothing behind the pointers
    assert sums(S=-1, trajs=None, valid=None, out=None, work=None) == INVALID and b"S=-1" in L.bsms_last_error()
    assert sums(S=0, trajs=None, valid=None, out=None, work=None) == 0
    # 4. null pointers before the entries are looked at
    entry(1, stride=3)
    for kw in (dict(trajs=None), dict(valid=None), dict(out=None), dict(work=None)):
        assert sums(**kw) == INVALID and b"null argument" in L.bsms_last_error(), kw
    # 5. per entry, in table order: signs, type_stride, null fields, then the row count
    assert sums() == INVALID and b"entry 1 has type_stride=3" in L.bsms_last_error()
    entry(1, stride=5)
    entry(0, n=-1)
    assert sums() == INVALID and b"entry 0 has n=-1" in L.bsms_last_error()
    entry(0, frame0=-2)
    assert sums() == INVALID and b"frame0=-2" in L.bsms_last_error()
    entry(0, frames=-3)
    assert sums() == INVALID and b"frames=-3" in L.bsms_last_error()
    entry(0, frames=-3, stride=4)
    assert sums() == INVALID and b"frames=-3" in L.bsms_last_error()                  # a negative field before the stride
    entry(0, state=None)
    assert sums() == INVALID and b"entry 0 has a null field" in L.bsms_last_error()
    entry(0, typ=None)
    assert sums() == INVALID and b"entry 0 has a null field" in L.bsms_last_error()
    entry(0, n=1 << 20, frames=1 << 20)
    assert sums() == SHAPE and b"below 2^40" in L.bsms_last_error()
    entry(0, n=1 << 20, frames=1 << 20, stride=7)
    assert sums() == INVALID                                                          # the stride before the row count
    entry(0, n=1 << 20, frames=1 << 20, stride=1 << 20, state=None)
    assert sums() == INVALID and b"null field" in L.bsms_last_error()                 # a null field before the row count
    # the fold: W, then S, then the pointers
    fold = lambda S=3, W=16, s=ptr, out=ptr: X.bsms_moment_fold(s, S, W, out, None)
    assert fold(W=0) == UNSUPPORTED and fold(W=65537, S=-1, s=None, out=None) == UNSUPPORTED
    assert fold(S=-1, s=None, out=None) == INVALID
    assert fold(s=None) == INVALID and fold(out=None) == INVALID and fold(S=0, s=None, out=None) == INVALID
    # the work area: does not know S, grows with the rows of ONE entry, and covers the pieces of every shape with that many rows
    wb = X.bsms_moment_work_bytes
    assert wb(0) == wb(-5) == wb(1000) > 0 and wb(1 << 30) > wb(1 << 20) > wb(1000)
    for n, frames in ((1, 1 << 20), (1 << 20, 1), (1 << 10, 1 << 10), (5233, 100), (131073, 8), (127, 8257)):
        pieces = -(-n * 8 // 1024) * -(-frames // 32)                                  # C = 8: slabs x frame chunks (the header)
        assert wb(n * frames) >= pieces * 35 * 8, (n, frames)


def numpy_stats(total, Cn, noise_std=None, gamma=0.0):
    """The closed form of the issue, restated in NumPy fp64."""
    t = np.asarray(total, dtype=np.float64)
    R, M = t[0], t[1]
    SX, ST, QX, QT = t[2:2 + Cn], t[2 + Cn], t[3 + Cn:3 + 2 * Cn], t[3 + 2 * Cn]
    SD, QD = t[4 + 2 * Cn:4 + 3 * Cn], t[4 + 3 * Cn:4 + 4 * Cn]
    var = np.zeros(Cn) if noise_std is None else np.asarray(noise_std, dtype=np.float32).astype(np.float64) ** 2
    in_mean = np.concatenate([SX, [ST]]) / R
    in_meansq = np.concatenate([QX / R + var * M / R, [QT / R]])
    return in_mean, in_meansq, SD / R, QD / R + gamma ** 2 * var * M / R


def synthetic_total(Cn, rows, masked, seed):
    """A plausible total row: moments of `rows` samples with means up to 10x the spread."""
    rng = np.random.default_rng(seed)
    mean, std = rng.standard_normal(2 * Cn + 1) * 10.0, np.abs(rng.standard_normal(2 * Cn + 1)) + 0.1
    s1, s2 = rows * mean, rows * (mean ** 2 + std ** 2)
    return np.concatenate([[rows, masked], s1[:Cn], s1[2 * Cn:], s2[:Cn], s2[2 * Cn:], s1[Cn:2 * Cn], s2[Cn:2 * Cn]])


@pytest.mark.parametrize("Cn", [1, 3, 8])
def test_normalizer_stats_equal_the_numpy_closed_form(eng, Cn):
    rows = 123457
    for masked in (0, 100000, rows):                                                   # M = 0: the noise terms vanish
        total = synthetic_total(Cn, rows, masked, seed=Cn)
        mom = eng.Moments(None, torch.from_numpy(total.copy()), Cn)
        assert float(mom.rows) == rows and float(mom.masked) == masked
        assert np.array_equal(mom.sum_state.numpy(), total[2:2 + Cn]) and np.array_equal(mom.sumsq_delta.numpy(), total[4 + 3 * Cn:])
        assert float(mom.sum_type) == total[2 + Cn] and float(mom.sumsq_type) == total[3 + 2 * Cn]
        assert np.array_equal(mom.sumsq_state.numpy(), total[3 + Cn:3 + 2 * Cn]) and np.array_equal(mom.sum_delta.numpy(), total[4 + 2 * Cn:4 + 3 * Cn])
        per_channel = [10.0 ** (k - 3) * 0.3 for k in range(Cn)]                       # per-channel sigma, not exact in fp32
        for std, gamma in ((None, 0.0), (per_channel, 0.0), (per_channel, 1.0), (per_channel, 0.8), ([0.0] * Cn, 1.0)):
            got = mom.normalizer_stats(std, gamma)
            want = numpy_stats(total, Cn, std, gamma)
            assert [tuple(g.shape) for g in got] == [(Cn + 1,), (Cn + 1,), (Cn,), (Cn,)]
            for name, g, w in zip(("in_mean", "in_meansq", "out_mean", "out_meansq"), got, want):
                assert g.dtype == torch.float64
                err = np.abs(g.numpy() - w) / np.abs(w)
                assert err.max() <= 1e-15, (name, masked, gamma, err.max())
        clean = mom.normalizer_stats()
        zero = mom.normalizer_stats([0.0] * Cn, 0.7)
        assert all(torch.equal(a, b) for a, b in zip(clean, zero))                     # sigma = 0: bit-equal to no noise at all
        if masked == 0:
            noisy = mom.normalizer_stats(per_channel, 1.0)
            assert all(torch.equal(a, b) for a, b in zip(clean, noisy))
        elif masked:
            noisy = mom.normalizer_stats(per_channel, 1.0)
            assert bool((noisy[1][:Cn] > clean[1][:Cn]).all()) and bool((noisy[3] > clean[3]).all())
            assert torch.equal(noisy[1][Cn:], clean[1][Cn:]) and torch.equal(noisy[0], clean[0]) and torch.equal(noisy[2], clean[2])
            assert torch.equal(mom.normalizer_stats(per_channel, 0.0)[3], clean[3])    # gamma = 0: the targets carry no noise


def test_normalizer_stats_refuse_an_empty_total_and_a_wrong_width(eng):
    with pytest.raises(ValueError, match="no rows"):
        eng.Moments(None, torch.zeros(16, dtype=torch.float64), 3).normalizer_stats()
    with pytest.raises(ValueError, match="no rows"):
        eng.Moments(torch.zeros(0, 16, dtype=torch.float64), torch.zeros(16, dtype=torch.float64), 3, rows_known=0).normalizer_stats([1, 1, 1])
    with pytest.raises(ValueError):
        eng.Moments(None, torch.zeros(15, dtype=torch.float64), 3)
    with pytest.raises(ValueError):
        eng.Moments(None, torch.zeros(16, dtype=torch.float32), 3)
    mom = eng.Moments(None, torch.from_numpy(synthetic_total(3, 10, 5, 0)), 3)
    with pytest.raises(ValueError, match="noise_std"):
        mom.normalizer_stats([0.1, 0.2])
    assert mom.all_reduce() is mom                                                     # no process group: a no-op


def test_fit_normalizers_refusals_come_before_any_work(eng):
    class Bank:
        cfg = SimpleNamespace(noise_level=[1.0], noise_gamma=0.5)

        def __init__(self, augment):
            self.augment, self.asked = augment, 0

        def moments(self, indices=None):
            self.asked += 1
            raise AssertionError("the refusal comes first")

    plain, augmented = Bank(None), Bank(eng.Augment())
    with pytest.raises(ValueError, match="noise must be"):
        eng.fit_normalizers(None, plain, noise="sampled")
    with pytest.raises(ValueError, match="noise must be"):
        eng.fit_normalizers(None, augmented, noise=None, ignore_augment=True)
    with pytest.raises(ValueError, match="augment"):
        eng.fit_normalizers(None, augmented)
    with pytest.raises(ValueError, match="augment"):
        eng.fit_normalizers(None, augmented, noise="none")
    assert plain.asked == augmented.asked == 0
    with pytest.raises(AssertionError):                                                # ignore_augment lets the call through
        eng.fit_normalizers(None, augmented, ignore_augment=True)
    assert augmented.asked == 1


def test_fit_normalizers_writes_in_place_from_host_moments(eng):
    """The write itself needs no device: a stand-in bank that hands out CPU moments."""
    Cn, rows, masked = 2, 1000, 600
    total = synthetic_total(Cn, rows, masked, seed=5)

    class Bank:
        augment = None
        cfg = SimpleNamespace(noise_level=[0.5, 0.02], noise_gamma=0.8)

        def moments(self, indices=None):
            return eng.Moments(None, torch.from_numpy(total.copy()), Cn)

    model = SimpleNamespace(_inputNormalizer=eng.Normalizer(Cn + 1, max_accumulations=5e5), _targetNormalizer=eng.Normalizer(Cn, max_accumulations=5e5))
    norms = (model._inputNormalizer, model._targetNormalizer)
    ptrs = [t.data_ptr() for n in norms for t in (n._E_data, n._E_data_squared, n._acc_weight, n._num_accumulations)]
    for noise, args in (("none", (None, 0.0)), ("expected", ([0.5, 0.02], 0.8))):
        eng.fit_normalizers(model, Bank(), noise=noise)
        want = numpy_stats(total, Cn, *args)
        for n, mean, meansq in ((norms[0], want[0], want[1]), (norms[1], want[2], want[3])):
            assert np.abs(n._E_data.numpy() - mean).max() <= 1e-15 * np.abs(mean).max()
            assert np.abs(n._E_data_squared.numpy() - meansq).max() <= 1e-15 * np.abs(meansq).max()
            assert float(n._acc_weight) == rows / n.unit and float(n._num_accumulations) == 5e5 and n.synced
    assert ptrs == [t.data_ptr() for n in norms for t in (n._E_data, n._E_data_squared, n._acc_weight, n._num_accumulations)]
    before = [n._E_data.clone() for n in norms]
    norms[0](torch.randn(7, Cn + 1), accumulate=True)                                  # saturated: a later accumulating call changes nothing
    assert torch.equal(norms[0]._E_data, before[0])
