"""GPU: the cell-gradient library (libbsms_hip_diffop.so: bsms_cell_gradient, bsms_node_gradient, bsms_cell_gradient_sums,
bsms_cell_gradient_bwd) against `Ref`, a NumPy fp64 restatement of the contract of include/bsms_hip_diffop.h with the
same operation order, and the routes above it (MeshGradient, cell_gradient_loss, TrajectoryBank.gradient_ops, Trainer.get_cell_error).

Bounds.  With g the restatement's fp64 value before the rounding to fp32, |out - g| <= 2^-24 |g| + c 2^-53 B:
  cell gradient   B = (|f_a k_0| + |f_b k_1| + |f_c k_2|) / |A2|, c = 8: the two differences behind a normal and behind A2 (4), a product,
                  two sums and the quotient;
  node gradient   B = sum over the list of the triangles' (|f_a k_0| + ..) / sum |A2|, c = 8 + the list's length (one more addition per
                  entry in numerator and denominator);
  backward        B = 2 sum over the list of the terms with every product replaced by its absolute value, c = 32 + the list's length
                  (two gradients of 8, b_k 2, w 3, the dot product 3, the coefficient products 3, rounded up).
The device performs the restatement's operations in the restatement's order without contraction, so what is measured is the one fp32
rounding: the worst fraction of the bound is printed by the tests and recorded in profiles/diffop_parity.txt.
Sums: every term is non-negative, so |sum - ref| <= (T + 16) 2^-53 ref, the criterion of the edge-difference sums."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from test_datapipe import cfg as make_cfg
from test_diffop_host import fan
from test_hip_databank import OPT, model_cfg, same_mesh_trajs
from test_sample_host import lattice, split_quads

pytestmark = pytest.mark.gpu

U24, U53 = 2.0 ** -24, 2.0 ** -53
NAN = float("nan")
WORST = {}                                              # check -> the worst measured fraction of its bound


@pytest.fixture(scope="module")
def eng():
    import bsms_gnn_amd as eng
    return eng


def note(key, value):
    WORST[key] = max(WORST.get(key, 0.0), float(value))
    print(f"diffop parity: {key}: worst fraction of the bound {WORST[key]:.3g}")


def bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int64)


# ------------------------------------------------------------------------------------------------------ meshes
def lists_of(tris, N):
    """(ptr, tri) int32: per node the ascending triangles that name it, each once; nodes outside [0, N) are left out."""
    lists = [[] for _ in range(N)]
    for t, tri in enumerate(np.asarray(tris).reshape(-1, 3)):
        for n in dict.fromkeys(int(v) for v in tri):
            if 0 <= n < N:
                lists[n].append(t)
    ptr = np.concatenate([[0], np.cumsum([len(l) for l in lists])]).astype(np.int32)
    return ptr, np.array([t for l in lists for t in l], dtype=np.int32)


def mesh_of(T, kind="tri", seed=0, jitter=True):
    """A lattice of at least T triangles (every second cell clockwise), jittered by multiples of 2^-14, cut to its first T triangles:
    the nodes of the cells behind the cut lie in no triangle."""
    side = 3
    while 2 * (side - 1) * (side - 2) < T:
        side += 1
    pos, cells = lattice(side, side - 1, kind, flip=True)
    if jitter:
        rng = np.random.default_rng(seed)
        pos = (pos + np.rint(rng.uniform(-0.3, 0.3, pos.shape) * 2.0 ** 14) / 2.0 ** 14).astype(np.float32)
    tris = (split_quads(cells) if kind == "quad" else cells)[:T]
    return pos, tris.astype(np.int64)


def special_mesh():
    """The fan (a hub of degree 72, both orientations, two orphan nodes) and behind it: a zero-area triangle, one with a NaN and one
    with an infinite corner, one that names node N, one that names node -1, and a good one that shares nodes with the bad ones."""
    pos, tris = fan(72)
    n0 = len(pos)
    extra = np.array([[8, 8], [9, 9], [10, 10], [np.nan, 1], [np.inf, 2], [12, 8]], dtype=np.float32)
    pos = np.concatenate([pos, extra])
    N = len(pos)
    bad = np.array([[n0, n0 + 1, n0 + 2], [n0, n0 + 5, n0 + 3], [n0 + 4, n0, n0 + 5], [n0, n0 + 5, N], [-1, n0, n0 + 5], [n0, n0 + 5, n0 + 1]])
    return pos, np.concatenate([tris, bad]), np.arange(len(tris), len(tris) + 5)       # the last one is valid


def quantised(rng, shape, scale=4.0):
    """fp32 multiples of 2^-10 in (-scale, scale): sums and differences of a few of them are exact in fp32."""
    return (np.rint(rng.uniform(-scale, scale, shape) * 1024.0) / 1024.0).astype(np.float32)


# ------------------------------------------------------------------------------------------------------ the NumPy restatement
class Ref:
    def __init__(self, pos, tris, inc=None):
        self.pos = np.asarray(pos, dtype=np.float32).astype(np.float64).reshape(-1, 2)
        self.tris = np.asarray(tris, dtype=np.int64).reshape(-1, 3)
        self.N, self.T = len(self.pos), len(self.tris)
        self.ptr, self.tri = (np.asarray(a, dtype=np.int64) for a in (lists_of(self.tris, self.N) if inc is None else inc))
        inb = ((self.tris >= 0) & (self.tris < self.N)).all(1)
        self.safe = np.where(inb[:, None], self.tris, 0)
        with np.errstate(all="ignore"):
            (ax, ay), (bx, by), (cx, cy) = (self.pos[self.safe[:, k]].T for k in range(3)) if self.N else ((np.zeros((2, self.T)),) * 3)
            self.A2 = (bx - ax) * (cy - ay) - (by - ay) * (cx - ax)
            self.kx = np.stack([by - cy, cy - ay, ay - by], -1)         # [T, 3]
            self.ky = np.stack([cx - bx, ax - cx, bx - ax], -1)
            self.valid = inb & (self.A2 != 0) & np.isfinite(self.A2)
        self.A2v = np.where(self.valid, self.A2, 1.0)
        self.kxv, self.kyv = np.where(self.valid[:, None], self.kx, 0.0), np.where(self.valid[:, None], self.ky, 0.0)

    def corners(self, f):
        """f [S, N, C] fp32 -> fp64 [S, T, 3, C] (zeros on invalid triangles)."""
        f = np.asarray(f).astype(np.float64)
        if self.N == 0:
            return np.zeros((f.shape[0], self.T, 3, f.shape[2]))
        return np.where(self.valid[None, :, None, None], f[:, self.safe], 0.0)

    def normals(self, v):
        """v [S, T, 3, C] -> n [S, T, C, 2] = (nx, ny) in the contract's order, and the sums of the absolute products."""
        def one(k):
            k = k[None, :, :, None]
            return (v[:, :, 0] * k[:, :, 0] + v[:, :, 1] * k[:, :, 1]) + v[:, :, 2] * k[:, :, 2], np.abs(v * k).sum(2)
        (nx, mx), (ny, my) = one(self.kxv), one(self.kyv)
        return np.stack([nx, ny], -1), np.stack([mx, my], -1)

    def cell_gradient(self, f, fill):
        n, m = self.normals(self.corners(f))
        A = self.A2v[None, :, None, None]
        ok = self.valid[None, :, None, None]
        return np.where(ok, n / A, fill), m / np.abs(A), np.broadcast_to(ok, n.shape)

    def steps(self):
        """The walk of every node's list, position by position: (nodes, triangles, corner) of the entries that count."""
        deg = self.ptr[1:] - self.ptr[:-1]
        for j in range(int(deg.max()) if self.N else 0):
            nodes = np.nonzero(deg > j)[0]
            t = self.tri[self.ptr[nodes] + j]
            ok = (t >= 0) & (t < self.T)
            t = np.where(ok, t, 0)
            hit = self.tris[t] == nodes[:, None] if self.T else np.zeros((len(nodes), 3), dtype=bool)
            ok &= (self.valid[t] if self.T else False) & hit.any(1)
            yield nodes[ok], t[ok], hit[ok].argmax(1)

    def node_gradient(self, f, fill):
        S, C = f.shape[0], f.shape[2]
        n, m = self.normals(self.corners(f))
        sg = np.where(self.A2 > 0, 1.0, -1.0)[None, :, None, None]
        num, mag = np.zeros((S, self.N, C, 2)), np.zeros((S, self.N, C, 2))
        den, cnt = np.zeros(self.N), np.zeros(self.N, dtype=np.int64)
        for nodes, t, _ in self.steps():
            num[:, nodes] += (sg * n)[:, t]
            mag[:, nodes] += m[:, t]
            den[nodes] += np.abs(self.A2[t])
            cnt[nodes] += 1
        ok = np.broadcast_to((cnt > 0)[None, :, None, None], num.shape)
        d = np.where(cnt > 0, den, 1.0)[None, :, None, None]
        return np.where(ok, num / d, fill), mag / d, ok, cnt

    def weights(self, mask, S):
        """w [S, T] = mu * (|A2| * 0.5) on the valid triangles, 0 elsewhere."""
        mu = np.ones((S, self.T))
        if mask is not None:
            m = np.broadcast_to(np.asarray(mask).astype(np.float64).reshape(-1, self.N), (S, self.N))[:, self.safe] if self.N else np.ones((S, self.T, 3))
            mu = (m[:, :, 0] * m[:, :, 1]) * m[:, :, 2]
        return np.where(self.valid[None], mu * (np.abs(self.A2v) * 0.5)[None], 0.0)

    def gradients(self, pred, target, exact_d=False):
        p, t = np.asarray(pred), np.asarray(target)
        d = p.astype(np.float64) - t.astype(np.float64) if exact_d else (p - t).astype(np.float64)       # fl32(pred - target) otherwise
        A = self.A2v[None, :, None, None]
        out = []
        for f in (d, t, p):
            n, m = self.normals(self.corners(f))
            out += [n / A, m / np.abs(A)]
        return out                                      # Gd, |Gd|, Gt, |Gt|, Gp, |Gp|: [S, T, C, 2]

    def sums(self, pred, target, mask=None, velocity=None, exact_d=False):
        S, C = pred.shape[0], pred.shape[2]
        w = self.weights(mask, S)
        Gd, _, Gt, _, Gp, _ = self.gradients(pred, target, exact_d)
        sq = lambda G: w[:, :, None] * (G[..., 0] * G[..., 0] + G[..., 1] * G[..., 1])
        cols = [w.sum(1, keepdims=True), sq(Gd).sum(1), sq(Gt).sum(1)]
        if velocity is None:
            cols.append(np.zeros((S, 4)))
        else:
            cu, cv = velocity
            div = lambda G: G[:, :, cu, 0] + G[:, :, cv, 1]
            curl = lambda G: G[:, :, cv, 0] - G[:, :, cu, 1]
            cols.append(np.stack([(w * (x * x)).sum(1) for x in (div(Gp), div(Gt), curl(Gd), curl(Gt))], -1))
        return np.concatenate(cols, 1)

    def objective(self, pred, target, mask, coef, velocity):
        """J [S] in fp64 with d = pred - target exact."""
        s = self.sums(pred, target, mask, velocity, exact_d=True)
        C = pred.shape[2]
        return (coef[:, :C] * s[:, 1:1 + C]).sum(1) + coef[:, C] * s[:, 1 + 2 * C] + coef[:, C + 1] * s[:, 3 + 2 * C]

    def backward(self, pred, target, mask, coef, velocity=None):
        """(grad [S, N, C] in fp64 before its rounding, the bound's B, the lists' valid lengths)."""
        S, C = pred.shape[0], pred.shape[2]
        w = self.weights(mask, S)
        Gd, Md, _, _, Gp, Mp = self.gradients(pred, target)
        acc, mag, cnt = np.zeros((S, self.N, C)), np.zeros((S, self.N, C)), np.zeros(self.N, dtype=np.int64)
        kD, kW = coef[:, C][:, None], coef[:, C + 1][:, None]
        for nodes, t, k in self.steps():
            bx, by = (self.kx[t, k] / self.A2[t])[None], (self.ky[t, k] / self.A2[t])[None]
            wt = w[:, t]
            for c in range(C):
                acc[:, nodes, c] += (wt * coef[:, c][:, None]) * (Gd[:, t, c, 0] * bx + Gd[:, t, c, 1] * by)
                mag[:, nodes, c] += (wt * np.abs(coef[:, c])[:, None]) * (Md[:, t, c, 0] * np.abs(bx) + Md[:, t, c, 1] * np.abs(by))
            if velocity is not None:
                cu, cv = velocity
                divp, curld = Gp[:, t, cu, 0] + Gp[:, t, cv, 1], Gd[:, t, cv, 0] - Gd[:, t, cu, 1]
                mdiv, mcurl = Mp[:, t, cu, 0] + Mp[:, t, cv, 1], Md[:, t, cv, 0] + Md[:, t, cu, 1]
                acc[:, nodes, cu] += (wt * kD) * (divp * bx)
                acc[:, nodes, cv] += (wt * kD) * (divp * by)
                acc[:, nodes, cu] += (wt * kW) * (curld * (-by))
                acc[:, nodes, cv] += (wt * kW) * (curld * bx)
                for c, b in ((cu, by), (cv, bx)):
                    other = bx if c == cu else by
                    mag[:, nodes, c] += (wt * np.abs(kD)) * (mdiv * np.abs(other)) + (wt * np.abs(kW)) * (mcurl * np.abs(b))
            cnt[nodes] += 1
        return 2.0 * acc, 2.0 * mag, cnt


# ------------------------------------------------------------------------------------------------------ the raw entries
class Raw:
    """A mesh and its incidence on the device and the four entries called directly; fields are device views [S, N, C]."""

    def __init__(self, eng, pos, tris, inc=None):
        self.eng, self.X = eng, eng._abi.diffop()
        self.pos = torch.as_tensor(np.asarray(pos, dtype=np.float32)).reshape(-1, 2).cuda()
        self.tris = torch.as_tensor(np.asarray(tris, dtype=np.int32)).reshape(-1, 3).contiguous().cuda()
        self.N, self.T = self.pos.shape[0], self.tris.shape[0]
        ptr, tri = lists_of(np.asarray(tris), self.N) if inc is None else inc
        self.ptr, self.tri = torch.as_tensor(np.asarray(ptr, dtype=np.int32)).cuda(), torch.as_tensor(np.asarray(tri, dtype=np.int32)).cuda()
        self.nnz = int(self.tri.shape[0])

    def mesh(self):
        return self.pos.data_ptr() if self.N else None, 2, self.N, self.tris.data_ptr() if self.T else None, self.T

    def inc(self):
        return self.ptr.data_ptr(), self.tri.data_ptr() if self.nnz else None, self.nnz

    @staticmethod
    def view(f):
        S, N, Cn = f.shape
        assert Cn == 1 or f.stride(2) == 1
        return f.data_ptr(), int(f.stride(0)) if S > 1 else 0, int(f.stride(1)) if N > 1 else Cn

    def stream(self):
        return torch.cuda.current_stream().cuda_stream

    def cell(self, f, fill=NAN):
        S, _, Cn = f.shape
        out = torch.full((S, self.T, Cn, 2), 777.0, device="cuda")
        p, ss, rs = self.view(f)
        self.eng._abi.check(self.X.bsms_cell_gradient(*self.mesh(), p, S, Cn, ss, rs, fill, out.data_ptr(), self.stream()), "bsms_cell_gradient")
        return out

    def node(self, f, fill=NAN, long_list=0):
        S, _, Cn = f.shape
        out = torch.full((S, self.N, Cn, 2), 777.0, device="cuda")
        p, ss, rs = self.view(f)
        self.eng._abi.check(self.X.bsms_node_gradient(*self.mesh(), *self.inc(), p, S, Cn, ss, rs, fill, long_list, out.data_ptr(), self.stream()),
                            "bsms_node_gradient")
        return out

    def operands(self, pred, target, mask):
        (pp, pss, prs), (tp, tss, trs) = self.view(pred), self.view(target)
        ms = 0 if mask is None or mask.shape[0] == 1 else self.N
        return pp, pss, prs, tp, tss, trs, None if mask is None else mask.data_ptr(), ms

    def sums(self, pred, target, mask=None, velocity=None, poison=False):
        S, _, Cn = pred.shape
        cu, cv = (-1, -1) if velocity is None else velocity
        out = torch.full((S, 1 + 2 * Cn + 4), NAN if poison else 0.0, dtype=torch.float64, device="cuda")
        work = torch.full((self.X.bsms_cell_gradient_work_bytes(S, self.T) // 8,), NAN if poison else 0.0, dtype=torch.float64, device="cuda")
        self.eng._abi.check(self.X.bsms_cell_gradient_sums(*self.mesh(), *self.operands(pred, target, mask), S, Cn, cu, cv, out.data_ptr(),
                                                           work.data_ptr(), self.stream()), "bsms_cell_gradient_sums")
        return out

    def bwd(self, pred, target, mask, coef, velocity=None, out=None, accumulate=False):
        S, _, Cn = pred.shape
        cu, cv = (-1, -1) if velocity is None else velocity
        out = torch.full((S, self.N, Cn), 777.0, device="cuda") if out is None else out
        self.eng._abi.check(self.X.bsms_cell_gradient_bwd(*self.mesh(), *self.inc(), *self.operands(pred, target, mask), S, Cn, cu, cv,
                                                          coef.data_ptr(), int(accumulate), out.data_ptr(), self.N, self.stream()),
                            "bsms_cell_gradient_bwd")
        return out


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a)).cuda()


def within(out, ref, B, c, ok=None):
    """The worst |out - ref| / (2^-24 |ref| + c 2^-53 B) over the entries `ok` (0 where the bound is 0 and the value exact)."""
    out, ref = np.asarray(out, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    ok = np.ones(ref.shape, dtype=bool) if ok is None else ok
    err, bound = np.abs(out - ref)[ok], (U24 * np.abs(ref) + c * U53 * B)[ok]
    if err.size == 0:
        return 0.0
    assert not np.isnan(err).any()
    assert (err[bound == 0] == 0).all()
    return float(np.max(np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), 0.0)))


# ------------------------------------------------------------------------------------------------------ 1. exact cases
@pytest.mark.parametrize("kind", ["tri", "quad"])
def test_integer_lattices_are_bit_equal_to_the_restatement(eng, kind):
    pos, tris = mesh_of(200, kind, jitter=False)
    rng = np.random.default_rng(3)
    f = rng.integers(-9, 10, (3, len(pos), 3)).astype(np.float32)
    ref, raw = Ref(pos, tris), Raw(eng, pos, tris)
    g, _, ok = ref.cell_gradient(f, NAN)
    assert ok.all() and np.array_equal(raw.cell(dev(f)).cpu().numpy(), g.astype(np.float32))
    gn, _, okn, cnt = ref.node_gradient(f, -5.0)
    out = raw.node(dev(f), fill=-5.0).cpu().numpy()
    assert (cnt == 0).any() and (cnt > 0).any()                         # the nodes behind the cut are orphans
    assert np.array_equal(out, gn.astype(np.float32)) and (out[~okn] == -5.0).all()


def test_linear_rotation_and_constant_fields_are_exact(eng):
    pos, tris, bad = special_mesh()
    finite = np.where(np.isfinite(pos), pos, 0.0).astype(np.float64)
    x, y = finite[:, 0], finite[:, 1]
    alpha, beta, gamma = 0.75, -1.5, 2.0
    f = np.stack([alpha * x + beta * y + gamma, -y, x, np.full_like(x, 3.25)], -1)[None].astype(np.float32)      # [1, N, 4], exact in fp32
    f[0, ~np.isfinite(pos).all(1)] = 1.0
    ref, raw = Ref(pos, tris), Raw(eng, pos, tris)
    assert ref.valid.sum() == len(tris) - 5 and not ref.valid[bad].any() and (ref.A2[ref.valid] > 0).any() and (ref.A2[ref.valid] < 0).any()
    cell = raw.cell(dev(f), fill=-7.0).cpu().numpy()[0]
    node = raw.node(dev(f), fill=-7.0).cpu().numpy()[0]
    _, _, _, cnt = ref.node_gradient(f, -7.0)
    assert cnt[0] == 72 and (cnt == 0).sum() >= 4                        # the hub; the two orphans and the nodes of bad triangles only
    for out, ok in ((cell, ref.valid), (node, cnt > 0)):
        assert (out[~ok] == -7.0).all() and not (out[ok] == -7.0).any()  # fill lands there and nowhere else
        assert (out[ok, 0] == [alpha, beta]).all()                       # the plane's gradient on every valid triangle and node
        assert (out[ok, 1] == [0.0, -1.0]).all() and (out[ok, 2] == [1.0, 0.0]).all() and (out[ok, 3] == 0.0).all()
    ops_f = dev(f)[..., 1:3]                                             # (u, v) = (-y, x): divergence 0, vorticity 2
    mg = eng.MeshGradient(pos[:75], tris[:72], "tri")
    div, vort = mg.divergence(ops_f[:, :75]).cpu().numpy()[0, :, 0], mg.vorticity(ops_f[:, :75]).cpu().numpy()[0, :, 0]
    assert div.shape == (75,) and (div[:73] == 0.0).all() and (vort[:73] == 2.0).all() and np.isnan(div[73:]).all() and np.isnan(vort[73:]).all()
    # a wrong list: entries outside [0, T) and triangles that do not contain the node are skipped
    ptr, tri = lists_of(tris, len(pos))
    lo, hi = ptr[1], ptr[2]
    wrong = np.concatenate([tri[:lo], [-3, len(tris) + 5, 40], tri[lo:]]).astype(np.int32)       # triangle 40 does not contain node 1
    wptr = ptr.copy()
    wptr[2:] += 3
    assert 1 not in tris[40] and hi > lo
    again = Raw(eng, pos, tris, (wptr, wrong)).node(dev(f), fill=-7.0).cpu().numpy()[0]
    assert np.array_equal(again, node)


# ------------------------------------------------------------------------------------------------------ 2. real data
CASES = [(0, 1, 1), (1, 3, 3), (2, 1, 8), (255, 3, 1), (256, 1, 3), (257, 3, 8), (1024, 37, 1), (1025, 1, 8), (2049, 3, 3), (300, 37, 8)]


@pytest.mark.parametrize("T,S,Cn", CASES)
def test_gradients_against_the_restatement(eng, T, S, Cn):
    pos, tris = mesh_of(T, "quad" if T % 2 == 0 else "tri", seed=T)
    rng = np.random.default_rng(T + 1)
    f = rng.standard_normal((S, len(pos), Cn)).astype(np.float32)
    ref, raw = Ref(pos, tris), Raw(eng, pos, tris)
    g, B, ok = ref.cell_gradient(f, NAN)
    out = raw.cell(dev(f)).cpu().numpy()
    assert out.shape == (S, T, Cn, 2) and ok.all()
    note("cell_gradient", within(out, g, B, 8))
    gn, Bn, okn, cnt = ref.node_gradient(f, NAN)
    outn = raw.node(dev(f)).cpu().numpy()
    assert np.isnan(outn[~okn]).all()
    frac = within(outn, gn, Bn, (8 + cnt)[None, :, None, None], okn)
    note("node_gradient", frac)
    assert WORST["cell_gradient"] < 1 and frac < 1
    assert np.array_equal(bits(raw.node(dev(f))).cpu().numpy(), bits(torch.from_numpy(outn)).numpy())      # run to run


def test_the_hub_and_the_special_triangles(eng):
    pos, tris, bad = special_mesh()
    rng = np.random.default_rng(5)
    ref, raw = Ref(pos, tris), Raw(eng, pos, tris)
    for S, Cn in ((1, 1), (3, 3), (37, 8)):
        f = rng.standard_normal((S, len(pos), Cn)).astype(np.float32)
        g, B, ok = ref.cell_gradient(f, NAN)
        out = raw.cell(dev(f)).cpu().numpy()
        assert np.isnan(out[~ok]).all() and not ok[:, bad].any()
        note("cell_gradient", within(out, g, B, 8, ok))
        gn, Bn, okn, cnt = ref.node_gradient(f, NAN)
        walks = [raw.node(dev(f), long_list=k) for k in (0, 1, 71, 72, 1 << 40)]          # the wave's walk for all, some, none
        outn = walks[0].cpu().numpy()
        assert all(torch.equal(bits(w), bits(walks[0])) for w in walks[1:])               # one ascending order either way
        assert np.isnan(outn[~okn]).all()
        frac = within(outn, gn, Bn, (8 + cnt)[None, :, None, None], okn)
        note("node_gradient", frac)
        assert frac < 1 and WORST["cell_gradient"] < 1


def test_strided_fields_are_read_in_place(eng):
    pos, tris = mesh_of(300, "tri", seed=9)
    N = len(pos)
    mg = eng.MeshGradient(pos, tris, "tri")
    assert mg.T == 300 and mg.N == N and mg.inc_ptr.dtype == torch.int32 and np.array_equal(mg.inc_tri.cpu().numpy(), lists_of(tris, N)[1])
    big = torch.randn(5, 2, N, 7, device="cuda")
    views = [big[1:4, :, :, 2:5], big[:, 1, :, :3], big[::2, 0, :, 4:], big[0, 0, :, :1], big.permute(1, 0, 2, 3)[..., 1:4]]
    for v in views:
        want_c, want_n = mg.cell_gradient(v.contiguous()), mg.node_gradient(v.contiguous())
        assert want_c.shape == (*v.shape[:-2], 300, v.shape[-1], 2) and want_n.shape == (*v.shape[:-2], N, v.shape[-1], 2)
        assert torch.equal(bits(mg.cell_gradient(v)), bits(want_c)) and torch.equal(bits(mg.node_gradient(v)), bits(want_n))
    with pytest.raises(ValueError):
        mg.cell_gradient(big[..., ::2])
    with pytest.raises(eng._abi.BsmsError):
        mg.cell_gradient(big.cpu())


# ------------------------------------------------------------------------------------------------------ 3. sums
def sums_data(T, S, Cn, seed, kind="tri"):
    pos, tris = mesh_of(T, kind, seed=seed)
    rng = np.random.default_rng(seed + 100)
    pred, target = quantised(rng, (S, len(pos), Cn)), quantised(rng, (S, len(pos), Cn))
    return pos, tris, pred, target, rng


@pytest.mark.parametrize("T,S,Cn", CASES)
def test_sums_against_the_restatement(eng, T, S, Cn):
    pos, tris, pred, target, rng = sums_data(T, S, Cn, T + 7, "quad" if T % 2 == 0 else "tri")
    mask = rng.uniform(0.0, 1.0, (S, len(pos))).astype(np.float32)
    ref, raw = Ref(pos, tris), Raw(eng, pos, tris)
    vel = None if Cn == 1 else (Cn - 1, 0)
    for m in (None, mask, mask[:1]):
        want = ref.sums(pred, target, m, vel)
        out = raw.sums(dev(pred), dev(target), None if m is None else dev(m), vel, poison=True).cpu().numpy()
        assert out.shape == (S, 1 + 2 * Cn + 4) and np.isfinite(out).all()
        err = np.abs(out - want)
        assert (err <= (T + 16) * U53 * want).all(), float((err / np.maximum(want, 1e-300)).max())
        note("sums / ((T + 16) 2^-53)", (err / np.where(want > 0, (T + 16) * U53 * want, 1.0)).max())
    if T == 0:
        assert (out == 0).all()


def test_a_sums_row_does_not_depend_on_its_launch(eng):
    T, Cn = 2049, 3
    pos, tris, pred, target, rng = sums_data(T, 37, Cn, 31)
    N = len(pos)
    raw = Raw(eng, pos, tris)
    mask = dev((rng.uniform(0, 1, (37, N)) > 0.2).astype(np.float32))
    p, t = dev(pred), dev(target)
    vel = (0, 2)
    full = raw.sums(p, t, mask, vel)
    assert torch.equal(bits(full), bits(raw.sums(p, t, mask, vel, poison=True)))          # run to run; NaN in work and sums on entry
    for k in (0, 1, 36):                                                # alone == at position k of the launch of 37
        alone = raw.sums(p[k:k + 1], t[k:k + 1], mask[k:k + 1], vel)
        assert torch.equal(bits(alone[0]), bits(full[k])), k
    # strided views: sets two apart in a larger buffer, rows of 7 floats
    big_p, big_t = torch.zeros(74, N, 7, device="cuda"), torch.zeros(37, N, 5, device="cuda")
    big_p[::2, :, 2:5], big_t[:, :, 1:4] = p, t
    assert torch.equal(bits(raw.sums(big_p[::2, :, 2:5], big_t[:, :, 1:4], mask, vel, poison=True)), bits(full))
    mg = eng.MeshGradient(pos, tris, "tri")
    assert torch.equal(bits(mg.sums(big_p[::2, :, 2:5], big_t[:, :, 1:4], mask, vel)), bits(full))
    assert torch.equal(bits(mg.sums(p.reshape(37, 1, N, Cn)[:, 0], t, mask.reshape(37, N, 1), vel)), bits(full))
    # no pair: zeros in the last four columns, the others unchanged bit for bit
    none = raw.sums(p, t, mask, None)
    assert (none[:, -4:] == 0).all() and torch.equal(bits(none[:, :-4]), bits(full[:, :-4])) and bool((full[:, -4:] > 0).all())
    # pred == target: GE = WE = 0 exactly; GT, DP == DT and WT are the target's
    same = raw.sums(t, t, mask, vel)
    assert (same[:, 1:1 + Cn] == 0).all() and (same[:, -2] == 0).all() and torch.equal(bits(same[:, -4]), bits(same[:, -3]))
    assert torch.equal(bits(same[:, 1 + Cn:1 + 2 * Cn]), bits(full[:, 1 + Cn:1 + 2 * Cn]))


def test_a_zero_one_mask_is_the_mesh_without_the_masked_triangles(eng):
    """Masked nodes chosen so that the triangles they remove are the LAST ones of each 1024-piece they touch: the survivors keep their
    places inside the pieces, so the rows are bit-equal to those of the launch on the shorter mesh; a general mask is within the bound."""
    T, Cn = 1500, 3
    pos, tris, pred, target, rng = sums_data(T, 3, Cn, 41)
    N = len(pos)
    cut = 1400                                           # drop triangles [1400, 1500): the tail of the second piece
    gone = np.setdiff1d(np.unique(tris[cut:]), np.unique(tris[:cut]))
    mask = np.ones(N, dtype=np.float32)
    mask[gone] = 0.0
    touched = ~(mask[tris] == 1).all(1)
    first = int(np.argmax(touched))
    assert touched[first:].all() and first < T - 10     # the masked triangles are exactly a tail
    raw_all, raw_cut = Raw(eng, pos, tris), Raw(eng, pos, tris[:first])
    p, t = dev(pred), dev(target)
    masked = raw_all.sums(p, t, dev(mask[None]), (0, 1))
    assert torch.equal(bits(masked), bits(raw_cut.sums(p, t, None, (0, 1))))
    general = (rng.uniform(0, 1, N) > 0.3).astype(np.float32)            # survivors move inside their pieces: the bound
    keep = (general[tris] == 1).all(1)
    a, b = raw_all.sums(p, t, dev(general[None]), (0, 1)).cpu().numpy(), Raw(eng, pos, tris[keep]).sums(p, t, None, (0, 1)).cpu().numpy()
    assert (np.abs(a - b) <= (T + 16) * U53 * b).all()


# ------------------------------------------------------------------------------------------------------ 4. backward
def bwd_case(eng, T, S, Cn, seed, special=False):
    if special:
        pos, tris, _ = special_mesh()
        rng = np.random.default_rng(seed)
        pred, target = quantised(rng, (S, len(pos), Cn)), quantised(rng, (S, len(pos), Cn))
    else:
        pos, tris, pred, target, rng = sums_data(T, S, Cn, seed)
    mask = (rng.uniform(0.0, 1.0, (S, len(pos))) * (rng.uniform(0, 1, (S, len(pos))) > 0.15)).astype(np.float32)
    coef = rng.uniform(-1.0, 2.0, (S, Cn + 2))
    return pos, tris, pred, target, mask, coef


@pytest.mark.parametrize("T,S,Cn,special", [(0, 1, 2, False), (1, 3, 3, False), (257, 3, 8, False), (1025, 1, 2, False), (2049, 3, 3, False),
                                            (300, 37, 2, False), (0, 3, 3, True)])
def test_backward_against_the_closed_form_and_a_central_difference(eng, T, S, Cn, special):
    pos, tris, pred, target, mask, coef = bwd_case(eng, T, S, Cn, 50 + T, special)
    ref, raw = Ref(pos, tris), Raw(eng, pos, tris)
    vel = (1, 0) if Cn == 2 else (0, Cn - 1)
    for m, v in ((mask, vel), (None, vel), (mask[:1], None)):
        k = coef if v is not None else np.concatenate([coef[:, :Cn], np.zeros((S, 2))], 1)
        g, B, cnt = ref.backward(pred, target, m, k, v)
        out = raw.bwd(dev(pred), dev(target), None if m is None else dev(m), dev(k), v)
        assert torch.equal(bits(out), bits(raw.bwd(dev(pred), dev(target), None if m is None else dev(m), dev(k), v)))      # run to run
        out = out.cpu().numpy()
        frac = within(out, g, B, (32 + cnt)[None, :, None])
        note("backward", frac)
        assert frac < 1
        assert (out[:, cnt == 0] == 0).all()                            # a node without a valid triangle: a gradient of zero
        if ref.valid.any() and m is not None:
            # J is quadratic in pred: the central difference along a direction is exact up to rounding.  The direction follows the
            # gradient's signs, so that <grad, v> has no cancellation.
            rng = np.random.default_rng(7)
            direction = g * rng.uniform(0.5, 1.5, g.shape)
            h = 2.0 ** -6
            p64 = pred.astype(np.float64)
            dJ = (ref.objective(p64 + h * direction, target, m, k, v) - ref.objective(p64 - h * direction, target, m, k, v)).sum() / (2 * h)
            got = float((out.astype(np.float64) * direction).sum())
            if dJ == 0:                                                 # every triangle masked: nothing to differentiate
                assert got == 0
                continue
            rel = abs(got - dJ) / abs(dJ)
            print(f"diffop parity: backward against the central difference: relative difference {rel:.3g}")
            WORST["central difference (relative)"] = max(WORST.get("central difference (relative)", 0.0), rel)
            assert rel < 1e-6


def test_backward_accumulates_and_gives_exact_zeros(eng):
    pos, tris, pred, target, mask, coef = bwd_case(eng, 700, 3, 3, 77)
    N = len(pos)
    raw = Raw(eng, pos, tris)
    p, t, m, k = dev(pred), dev(target), dev(mask), dev(coef)
    g = raw.bwd(p, t, m, k, (0, 1))
    base = torch.randn(3, N, 3, device="cuda")
    acc = raw.bwd(p, t, m, k, (0, 1), out=base.clone(), accumulate=True)
    assert torch.equal(bits(acc), bits(base + g))                       # one fp32 addition to what was there
    assert (raw.bwd(p, t, m, torch.zeros_like(k), (0, 1)) == 0).all()   # zero coefficients
    assert (raw.bwd(p, t, torch.zeros_like(m), k, (0, 1)) == 0).all()   # every corner masked
    # masked corners: a node whose triangles all have a masked corner gets an exact zero
    node_mask = np.ones((1, N), dtype=np.float32)
    masked = np.unique(tris[::40])
    node_mask[0, masked] = 0.0
    live = np.zeros(N, dtype=bool)
    live[np.unique(tris[(node_mask[0][tris] == 1).all(1)])] = True
    out = raw.bwd(p, t, dev(node_mask), k, (0, 1)).cpu().numpy()
    assert not live[masked].any() and live.sum() > N // 4               # the masked nodes themselves, and whoever has no other triangle
    assert (out[:, ~live] == 0).all() and (out[:, live] != 0).all(-1).any()
    # through MeshGradient: strided operands, out / accumulate
    mg = eng.MeshGradient(pos, tris, "tri")
    big = torch.zeros(3, N, 8, device="cuda")
    big[:, :, 3:6] = p
    assert torch.equal(bits(mg.backward(big[:, :, 3:6], t, m, k, (0, 1))), bits(g))
    assert torch.equal(bits(mg.backward(p, t, m, k, (0, 1), out=base.clone(), accumulate=True)), bits(acc))
    with pytest.raises(ValueError):
        mg.backward(p, t, m, k[:, :4], (0, 1))
    with pytest.raises(ValueError):
        mg.sums(p, t, m, (1, 1))


# ------------------------------------------------------------------------------------------------------ 5. the loss
def test_cell_gradient_loss_value_gradient_and_graph_replay(eng):
    pos, tris, pred, target, mask, _ = bwd_case(eng, 1100, 3, 3, 91)
    N = len(pos)
    ref, mg = Ref(pos, tris), eng.MeshGradient(pos, tris, "tri")
    w, kd, kw, vel = [0.5, 2.0, 1.25], 0.75, 1.5, (0, 1)
    p = dev(pred).requires_grad_(True)
    t, m = dev(target), dev(mask)
    loss = eng.cell_gradient_loss(mg, p, t, m, channel_weights=w, div_weight=kd, vort_weight=kw, velocity=vel)
    assert loss.dtype == torch.float32 and loss.dim() == 0
    s = ref.sums(pred, target, mask, vel)
    want = ((np.array(w) * s[:, 1:4]).sum() + kd * s[:, 7].sum() + kw * s[:, 9].sum()) / s[:, 0].sum()
    assert abs(float(loss) - want) <= float(np.spacing(np.float32(want)))              # one fp32 ulp of the fp64 definition
    loss.backward()
    coef = np.tile(np.array(w + [kd, kw]) / s[:, 0].sum(), (3, 1))
    g, B, cnt = ref.backward(pred, target, mask, coef, vel)
    frac = within(p.grad.cpu().numpy(), g, B, (32 + cnt)[None, :, None] + 4)            # + the coefficient's own division and cast
    note("cell_gradient_loss gradient", frac)
    assert frac < 1
    plain = eng.cell_gradient_loss(mg, p.detach(), t)                                   # no mask, no pair, unit weights
    s1 = ref.sums(pred, target)
    assert abs(float(plain) - s1[:, 1:4].sum() / s1[:, 0].sum()) <= float(np.spacing(np.float32(plain.item())))

    # graph replay with changing pred == eager, bit for bit
    static = dev(pred).requires_grad_(True)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                                       # warm-up outside the capture
        eng.cell_gradient_loss(mg, static, t, m, w, kd, kw, vel).backward()
    torch.cuda.current_stream().wait_stream(side)
    static.grad = None
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = eng.cell_gradient_loss(mg, static, t, m, w, kd, kw, vel)
        out.backward()
    rng = np.random.default_rng(17)
    for _ in range(3):
        fresh = dev(quantised(rng, pred.shape))
        with torch.no_grad():
            static.copy_(fresh)
        graph.replay()
        eager = fresh.clone().requires_grad_(True)
        value = eng.cell_gradient_loss(mg, eager, t, m, w, kd, kw, vel)
        value.backward()
        assert torch.equal(bits(out.detach().reshape(1)), bits(value.detach().reshape(1))) and torch.equal(bits(static.grad), bits(eager.grad))


# ------------------------------------------------------------------------------------------------------ 6. wiring
def test_bank_ops_trainer_error_and_rasterised_vorticity(eng):
    trajs = same_mesh_trajs(150, 5, 3, seed=21)
    bank = eng.TrajectoryBank(make_cfg(True, depth=1), dataset="airfoil")
    for tr_ in trajs:
        bank.add(tr_)
    ops = bank.gradient_ops(1)
    hand = eng.MeshGradient(trajs[1]["mesh_pos"][0], trajs[1]["cells"][0], "tri")
    assert isinstance(ops, eng.MeshGradient) and ops.N == 150 and ops.T == hand.T and ops.mesh_type == "tri"
    for a, b in ((ops.pos, hand.pos), (ops.tris, hand.tris), (ops.inc_ptr, hand.inc_ptr), (ops.inc_tri, hand.inc_tri)):
        assert torch.equal(a, b)
    torch.manual_seed(0)
    mcfg = model_cfg(True, depth=1)
    tr = eng.Trainer(eng.BSMS_Simulator(mcfg), mcfg, SimpleNamespace(**vars(OPT), ema_decay=0.9))
    tr.iter(bank.batch([(0, 0), (1, 0), (2, 0)], train=False))          # warm-up: normaliser statistics
    assert tr.iter(bank.batch([(0, 1), (1, 2), (2, 3)])) is not None
    data = bank.batch([(0, 1), (2, 0), (1, 3)], train=False)
    for relative, ema, vel in ((True, False, None), (False, True, (0, 1))):
        mean, std = tr.get_cell_error(data, ops, relative=relative, velocity=vel, ema=ema)
        with torch.no_grad():
            pred = tr.get_pred(data, ema)
        want = eng.cell_error_mean_std(ops.sums(pred, data[1], data[2], vel), relative)
        assert mean.dtype == np.float32 and mean.shape == (3,) and std.shape == (3,)
        assert np.allclose(mean, want[0].cpu().numpy(), rtol=2e-6, atol=0) and np.allclose(std, want[1].cpu().numpy(), rtol=2e-6, atol=2e-6 * float(want[0].max()))
    dp, dt = eng.divergence_rms(ops.sums(pred, data[1], data[2], (0, 1)))
    assert dp.shape == (3,) and bool((dp > 0).all()) and bool((dt > 0).all())

    # vorticity and divergence as the sampler takes them: [..., N, 1] -> [..., 1, H, W]
    s = bank.sampler(1)
    x = data[1]                                                          # [3, 150, 3]
    vort, div = ops.vorticity(x), ops.divergence(x, velocity=(1, 0))
    g = ops.node_gradient(x)
    assert vort.shape == (3, 150, 1) and torch.equal(bits(vort), bits((g[..., 1, 0] - g[..., 0, 1]).unsqueeze(-1)))
    assert torch.equal(bits(div), bits((g[..., 1, 0] + g[..., 0, 1]).unsqueeze(-1)))
    img = s.rasterize(vort, 40, 32)
    assert img.shape == (3, 1, 32, 40) and torch.equal(bits(img), bits(s.rasterize((g[..., 1, 0] - g[..., 0, 1]).unsqueeze(-1).contiguous(), 40, 32)))
    frames = eng.rollout_frames(ops.vorticity(x), s, 40, 32, every=2)
    assert frames.shape == (2, 1, 32, 40) and torch.equal(bits(frames[1]), bits(img[2]))


def test_the_parity_record_is_current():
    """What the tests above measured against what profiles/diffop_parity.txt records: every recorded check ran below its bound."""
    import os
    from conftest import ROOT
    body = open(os.path.join(ROOT, "profiles", "diffop_parity.txt")).read()
    for key in ("cell_gradient", "node_gradient", "backward", "central difference"):
        assert key in body, key
    for key, worst in WORST.items():
        if key != "central difference (relative)":
            assert worst < 1, (key, worst)
