"""Host (no GPU): the fifth companion library's declarations / bindings / exports (include/bsms_hip_diffop.h) and the
pinned surfaces of the five other libraries; the node -> triangle incidence of `diffop.incidence` against a plain Python loop; every
refusal of `MeshGradient` and of the entries, raised before a device call; that nothing on the default path loads the library; and the
evaluation figures `cell_error_mean_std` / `divergence_rms` against NumPy.  The meshes of the GPU tests (tests/test_hip_diffop.py) are
built here."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT
from test_sample_host import declared, exports, lattice, split_quads

ENTRIES = {"bsms_cell_gradient": 13, "bsms_node_gradient": 17, "bsms_cell_gradient_work_bytes": 2, "bsms_cell_gradient_sums": 20,
           "bsms_cell_gradient_bwd": 25}


@pytest.fixture(scope="module")
def eng():
    import bsms_gnn_amd as eng
    return eng


# ------------------------------------------------------------------------------------------------------ meshes
def fan(spokes=72):
    """A hub (node 0) of `spokes` triangles around it, every second one clockwise, on a ring of radius-2 nodes with dyadic
    coordinates; nodes spokes + 1 and spokes + 2 lie in no triangle."""
    ang = 2 * np.pi * np.arange(spokes) / spokes
    ring = np.rint(np.stack([2 * np.cos(ang), 2 * np.sin(ang)], -1) * 2.0 ** 10) / 2.0 ** 10
    pos = np.concatenate([[[0.0, 0.0]], ring, [[5.0, 5.0], [6.0, 5.0]]]).astype(np.float32)
    tris = np.array([[0, 1 + k, 1 + (k + 1) % spokes] for k in range(spokes)], dtype=np.int64)
    tris[1::2] = tris[1::2, ::-1]
    return pos, tris


def loop_incidence(tris, N):
    lists = [[] for _ in range(N)]
    for t, tri in enumerate(np.asarray(tris).reshape(-1, 3)):
        for n in tri:
            if t not in lists[n]:
                lists[n].append(t)
    return lists


def as_lists(ptr, tri):
    return [tri[ptr[n]:ptr[n + 1]].tolist() for n in range(len(ptr) - 1)]


@pytest.mark.parametrize("case", ["lattice", "fan", "orphans", "empty", "quads", "repeated"])
def test_the_incidence_is_the_plain_loop(eng, case):
    from bsms_gnn_amd.diffop import incidence
    if case == "lattice":
        pos, tris = lattice(7, 5, "tri", flip=True)
    elif case == "fan":
        pos, tris = fan(72)
    elif case == "orphans":
        pos, tris = np.zeros((9, 2), dtype=np.float32), np.array([[8, 1, 3], [3, 1, 6]])
    elif case == "empty":
        pos, tris = np.zeros((4, 2), dtype=np.float32), np.zeros((0, 3), dtype=np.int64)
    elif case == "quads":
        pos, quads = lattice(5, 4, "quad", flip=True)
        tris = split_quads(quads)
    else:
        pos, tris = np.zeros((5, 2), dtype=np.float32), np.array([[2, 2, 4], [0, 0, 0], [4, 1, 2]])
    ptr, tri = incidence(tris, len(pos))
    assert ptr.dtype == np.int32 and tri.dtype == np.int32 and ptr.shape == (len(pos) + 1,) and ptr[0] == 0 and ptr[-1] == len(tri)
    want = loop_incidence(tris, len(pos))
    assert as_lists(ptr, tri) == want
    assert all(l == sorted(set(l)) for l in want)                       # ascending, each pair once
    if case == "fan":
        assert len(want[0]) == 72 and want[73] == [] and want[74] == []
    if case == "quads":                                                 # the sampler's own split: cell k is the triangles 2k and 2k + 1
        from bsms_gnn_amd.sample import _triangles
        assert np.array_equal(_triangles(pos, quads, "quad"), tris)


# ------------------------------------------------------------------------------------------------------ refusals
def test_mesh_gradient_refuses_before_any_device_call(eng, monkeypatch):
    from bsms_gnn_amd import diffop
    monkeypatch.setattr(eng._abi, "diffop", lambda: pytest.fail("the library was loaded"))
    monkeypatch.setattr(torch.Tensor, "to", lambda *a, **k: pytest.fail("a tensor was moved"))
    pos, tris = lattice(3, 3, "tri")
    for bad_pos, cells, kind in ((pos, tris, "tet"), (pos, tris, "line"), (pos[:, :1], tris, "tri"), (np.zeros((9, 3), dtype=np.float32), tris, "tri"),
                                 (pos, tris[:, :2], "tri"), (pos, tris, "quad"), (pos, np.array([[0, 1, 9]]), "tri"), (pos, np.array([[0, -1, 2]]), "tri")):
        with pytest.raises(ValueError):
            diffop.MeshGradient(bad_pos, cells, kind, device="cuda")
    with pytest.raises(eng._abi.BsmsError):                             # a valid mesh, no GPU device
        diffop.MeshGradient(pos, tris, "tri", device="cpu")
    assert diffop.MeshGradient._check_fields is eng.MeshSampler._check_fields and diffop._sets is eng.sample._sets
    assert diffop._triangles is eng.sample._triangles                   # shared, not copied


def test_cell_gradient_loss_refuses_weights_without_a_pair(eng):
    x = torch.zeros(4, 2)
    with pytest.raises(ValueError):
        eng.cell_gradient_loss(None, x, x, div_weight=1.0)
    with pytest.raises(ValueError):
        eng.cell_gradient_loss(None, x, x, vort_weight=0.5)
    with pytest.raises(ValueError):
        eng.cell_gradient_loss(None, x, x, channel_weights=[1.0, 2.0, 3.0])


def test_entries_refuse_bad_arguments_without_a_gpu(eng):
    L, X = eng._abi.lib(), eng._abi.diffop()
    one = C.c_double(0.0)
    ptr = C.addressof(one)                              # a non-null pointer that is never dereferenced: every call below fails first
    INVALID, SHAPE, UNSUPPORTED = -1, -2, -3

    def cell(pos=ptr, stride=2, N=4, tris=ptr, T=2, f=ptr, S=2, Cn=3, set_stride=12, row_stride=3, out=ptr):
        return X.bsms_cell_gradient(pos, stride, N, tris, T, f, S, Cn, set_stride, row_stride, 0.0, out, None)

    def node(pos=ptr, stride=2, N=4, tris=ptr, T=2, ip=ptr, it=ptr, nnz=6, f=ptr, S=2, Cn=3, row_stride=3, out=ptr):
        return X.bsms_node_gradient(pos, stride, N, tris, T, ip, it, nnz, f, S, Cn, 12, row_stride, 0.0, 0, out, None)

    def sums(pos=ptr, stride=2, N=4, tris=ptr, T=2, p=ptr, prs=3, t=ptr, trs=3, m=None, ms=0, S=2, Cn=3, cu=-1, cv=-1, out=ptr, work=ptr):
        return X.bsms_cell_gradient_sums(pos, stride, N, tris, T, p, 12, prs, t, 12, trs, m, ms, S, Cn, cu, cv, out, work, None)

    def bwd(pos=ptr, stride=2, N=4, tris=ptr, T=2, ip=ptr, it=ptr, nnz=6, p=ptr, prs=3, t=ptr, trs=3, ms=0, S=2, Cn=3, cu=-1, cv=-1, coef=ptr,
            grad=ptr, gs=4):
        return X.bsms_cell_gradient_bwd(pos, stride, N, tris, T, ip, it, nnz, p, 12, prs, t, 12, trs, None, ms, S, Cn, cu, cv, coef, 0, grad, gs, None)

    for fn in (cell, node, sums, bwd):
        for kw, code, text in ((dict(Cn=0), UNSUPPORTED, b"C in 1..8"), (dict(Cn=9), UNSUPPORTED, b"C in 1..8"),
                               (dict(Cn=9, pos=None), UNSUPPORTED, b"C in 1..8"),          # C is checked before any pointer
                               (dict(N=-1), INVALID, b"N=-1"), (dict(T=-1), INVALID, b"T=-1"), (dict(stride=1), INVALID, b"pos_stride=1"),
                               (dict(N=1 << 31), SHAPE, b"2^31"), (dict(T=1 << 31), SHAPE, b"2^31"), (dict(pos=None), INVALID, b"null mesh"),
                               (dict(tris=None), INVALID, b"null mesh"), (dict(S=-1), INVALID, b"S=-1")):
            assert fn(**kw) == code and text in L.bsms_last_error(), (fn.__name__, kw)
    assert cell(row_stride=2) == INVALID and b"row_stride=2" in L.bsms_last_error()
    assert cell(out=None) == INVALID and cell(f=None) == INVALID and cell(S=0, out=None, f=None) == 0 and cell(T=0, tris=None, out=None) == 0
    assert node(row_stride=2) == INVALID and node(ip=None) == INVALID and node(it=None) == INVALID and node(nnz=-1) == INVALID
    assert node(out=None) == INVALID and node(f=None) == INVALID and node(S=0, out=None, f=None) == 0
    assert sums(prs=2) == INVALID and sums(trs=2) == INVALID and sums(ms=-1) == INVALID and sums(p=None) == INVALID and sums(t=None) == INVALID
    assert sums(cu=0, cv=0) == INVALID and b"velocity pair" in L.bsms_last_error()
    assert sums(cu=0, cv=3) == INVALID and sums(cu=3, cv=0) == INVALID and sums(cu=1, cv=-1) == INVALID
    assert sums(out=None) == INVALID and sums(work=None) == INVALID and sums(S=0, out=None, work=None) == 0
    assert bwd(prs=2) == INVALID and bwd(cu=2, cv=2) == INVALID and bwd(ip=None) == INVALID and bwd(gs=3) == INVALID and b"grad_stride=3" in L.bsms_last_error()
    assert bwd(coef=None) == INVALID and bwd(grad=None) == INVALID and bwd(S=0, coef=None, grad=None) == 0
    # the work area: S x pieces of 1024 triangles x (1 + 2 * 8 + 4) doubles, never nothing
    W = X.bsms_cell_gradient_work_bytes
    assert W(3, 2049) >= 3 * 3 * 21 * 8 and W(1, 0) >= 21 * 8 and W(0, 0) > 0 and W(-1, 5) == 0 and W(1, 1024) < W(1, 1025)


# ------------------------------------------------------------------------------------------------------ the library
def test_the_fifth_library_declares_exports_and_binds_the_same_entries(eng):
    _abi = eng._abi
    strip = lambda path: re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", path)).read(), flags=re.S)
    others = [strip(h) for h in ("bsms_hip.h", "bsms_hip_ext.h", "bsms_hip_stats.h", "bsms_hip_sample.h", "bsms_hip_query.h")]
    text = strip("bsms_hip_diffop.h")
    names = set(re.findall(r"\b(bsms_[a-z0-9_]+)\s*\(", text))
    assert names == set(ENTRIES) == set(_abi.DIFFOP_SIGNATURES) == exports(_abi.DIFFOP_LIB_PATH)
    raw = [C.CDLL(p) for p in (_abi.LIB_PATH, _abi.EXT_LIB_PATH, _abi.STATS_LIB_PATH, _abi.SAMPLE_LIB_PATH, _abi.QUERY_LIB_PATH)]
    taken = (_abi.SIGNATURES, _abi.EXT_SIGNATURES, _abi.STATS_SIGNATURES, _abi.SAMPLE_SIGNATURES, _abi.QUERY_SIGNATURES)
    for name, nargs in ENTRIES.items():
        assert declared(text, name) == nargs and len(_abi.DIFFOP_SIGNATURES[name][1]) == nargs, name
        assert all(declared(o, name) is None for o in others), name
        assert not any(name in sig for sig in taken) and not any(hasattr(r, name) for r in raw), name
    assert os.path.basename(_abi.DIFFOP_LIB_PATH) == "libbsms_hip_diffop.so"
    for doc in ("INTEGRATION.md", "README.md", "DESIGN.md"):
        body = open(os.path.join(ROOT, doc)).read()
        assert "bsms_cell_gradient_sums" in body and "bsms_hip_diffop" in body, doc


def test_the_other_libraries_export_exactly_what_they_did(eng):
    _abi = eng._abi
    assert len(exports(_abi.LIB_PATH)) == len(_abi.SIGNATURES) == 99 and exports(_abi.LIB_PATH) == set(_abi.SIGNATURES)
    assert _abi.lib().bsms_abi_version() == 4
    assert exports(_abi.EXT_LIB_PATH) == set(_abi.EXT_SIGNATURES) == {"bsms_edge_diff_fold", "bsms_sim_edge_objective_bwd"}
    assert exports(_abi.STATS_LIB_PATH) == set(_abi.STATS_SIGNATURES) == {"bsms_moment_work_bytes", "bsms_moment_sums", "bsms_moment_fold"}
    assert exports(_abi.SAMPLE_LIB_PATH) == set(_abi.SAMPLE_SIGNATURES) == {"bsms_raster_work_bytes", "bsms_raster_owner", "bsms_point_owner",
                                                                            "bsms_field_gather"}
    assert exports(_abi.QUERY_LIB_PATH) == set(_abi.QUERY_SIGNATURES) == {"bsms_chain_launch_query"}
    assert exports(_abi.DIFFOP_LIB_PATH) == set(ENTRIES)                # and the new one nothing beyond its header


def test_nothing_on_the_default_path_loads_the_library(eng):
    """`import bsms_gnn_amd`, a model and (where there is a device to put it on) a Trainer never touch libbsms_hip_diffop.so: in a
    fresh interpreter, so that what other tests loaded does not count."""
    code = ("import sys; sys.path.insert(0, %r)\n"
            "import torch\n"
            "import bsms_gnn_amd as eng\n"
            "from types import SimpleNamespace as NS\n"
            "assert eng._abi._diffop is None and eng.MeshGradient is not None and eng.cell_gradient_loss is not None\n"
            "mcfg = NS(out_dim=3, latent_dim=32, hidden_layer=2, unet_depth=1, pos_dim=2, consistent_mesh=True, accumulation_steps=1)\n"
            "opt = NS(peak_lr=1e-3, weight_decay=1e-4, warmup_steps=1, decay_steps=50, gnorm_clip=1.0)\n"
            "model = eng.BSMS_Simulator(mcfg)\n"
            "if torch.cuda.is_available():\n"                          # a Trainer puts its model on the device: only where there is one
            "    eng.Trainer(model, mcfg, opt)\n"
            "assert eng._abi._diffop is None\n"
            "assert 'libbsms_hip_diffop' not in open('/proc/self/maps').read()\n"
            "print('clean')\n") % ROOT
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True)
    assert r.returncode == 0 and "clean" in r.stdout, r.stderr


# ------------------------------------------------------------------------------------------------------ evaluation figures
def test_cell_error_and_divergence_figures_against_numpy(eng):
    C_ = 2
    rows = np.array([[2.0, 8.0, 18.0, 2.0, 8.0, 0.5, 4.5, 1.0, 3.0],            # A | GE0 GE1 | GT0 GT1 | DP DT WE WT
                     [4.0, 1.0, 4.0, 16.0, 1.0, 1.0, 0.25, 2.0, 5.0],
                     [1.0, 0.25, 9.0, 4.0, 36.0, 9.0, 0.0, 0.0, 1.0]])
    sums = torch.from_numpy(rows)
    A, GE, GT = rows[:, :1], rows[:, 1:1 + C_], rows[:, 1 + C_:1 + 2 * C_]
    for relative in (True, False):
        E = np.sqrt(GE / A) / (np.sqrt(GT / A) if relative else 1.0)
        mean, std = eng.cell_error_mean_std(sums, relative)
        assert mean.dtype == torch.float64 and np.allclose(mean.numpy(), E.mean(0), rtol=1e-15) and np.allclose(std.numpy(), E.std(0), rtol=1e-14)
    mean, _ = eng.cell_error_mean_std(sums[:1], relative=False)
    assert mean.tolist() == [2.0, 3.0]                                  # sqrt(8 / 2), sqrt(18 / 2)
    mean, std = eng.cell_error_mean_std(sums[:1])
    assert mean.tolist() == [2.0, 1.5] and std.tolist() == [0.0, 0.0]   # over sqrt(2 / 2), sqrt(8 / 2)
    dp, dt = eng.divergence_rms(sums)
    assert np.array_equal(dp.numpy(), np.sqrt(rows[:, 5] / rows[:, 0])) and np.array_equal(dt.numpy(), np.sqrt(rows[:, 6] / rows[:, 0]))
    assert dp.tolist() == [0.5, 0.5, 3.0] and dt.tolist() == [1.5, 0.25, 0.0]
    assert eng.cell_error_mean_std(sums.float())[0].dtype == torch.float64
    for bad in (torch.zeros(3, 6), torch.zeros(3, 5), torch.zeros(9)):
        with pytest.raises(ValueError):
            eng.cell_error_mean_std(bad)
        with pytest.raises(ValueError):
            eng.divergence_rms(bad)
