"""GPU: the mesh sampler (libbsms_hip_sample.so: bsms_raster_owner, bsms_point_owner, bsms_field_gather) against the
NumPy fp64 restatement of its contract in tests/test_sample_host.py, and the routes above it (MeshSampler, Trainer.eval_panels,
TrajectoryBank.sampler, rollout_frames).

Owners.  On meshes with small-integer coordinates and grids whose pixel centres are dyadic rationals every orient() is exact, so the
owners are bit-equal to the reference with no exclusions.  On the jittered meshes a sample is ambiguous when some live triangle has
min_i |e_i| <= 8 * 2^-53 * M_i; the committed seeds have none (the host test checks it), and every other sample must agree.

Values.  |out - ref| <= 2^-24 F + 64 * 2^-53 (1 + M / |A|) F with F the largest |nodal value| of the owning triangle and M its largest
M_i.  Rounding count behind the 64: an orient() is 4 differences, 2 products and 1 subtraction = 7, three of them 21; the sum of the
e_i 2; the quotients 3; the combination 3 products and 2 sums = 5: 31 fp64 roundings, each amplified by at most M / |A| (the e_i)
or 1 (the rest), plus the one rounding to fp32.  The device performs the same 31 operations in the same order without contraction,
so the measured worst ratio is that of the fp32 rounding alone (printed by the tests, recorded in profiles/sample_parity.txt)."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from test_datapipe import cfg as make_cfg, synthetic_traj
from test_hip_databank import OPT, model_cfg, same_mesh_trajs
from test_sample_host import GENERIC, Located, generic_case, grid_centres, lattice, split_quads

pytestmark = pytest.mark.gpu

U24, U53 = 2.0 ** -24, 2.0 ** -53
NAN = float("nan")


@pytest.fixture(scope="module")
def eng():
    import bsms_gnn_amd as eng
    return eng


# ------------------------------------------------------------------------------------------------------ the raw entries
class Raw:
    """A mesh on the device and the three entries called directly."""

    def __init__(self, eng, pos, tris):
        self.eng, self.X = eng, eng._abi.sample()
        self.pos = torch.as_tensor(np.asarray(pos, dtype=np.float32)).reshape(-1, 2).cuda()
        self.tris = torch.as_tensor(np.asarray(tris, dtype=np.int32)).reshape(-1, 3).contiguous().cuda()
        self.N, self.T = self.pos.shape[0], self.tris.shape[0]
        self.work = torch.empty(self.X.bsms_raster_work_bytes(), dtype=torch.uint8, device="cuda")

    def mesh(self):
        return self.pos.data_ptr() if self.N else None, 2, self.N, self.tris.data_ptr() if self.T else None, self.T

    def raster(self, grid, small_box=0, out=None):
        W, H = grid[:2]
        out = torch.empty(H, W, dtype=torch.int32, device="cuda") if out is None else out
        self.eng._abi.check(self.X.bsms_raster_owner(*self.mesh(), *grid, small_box, out.data_ptr(), self.work.data_ptr(),
                                                     torch.cuda.current_stream().cuda_stream), "bsms_raster_owner")
        return out

    def locate(self, q):
        q = torch.as_tensor(q, dtype=torch.float64).reshape(-1, 2).cuda()
        out = torch.empty(q.shape[0], dtype=torch.int32, device="cuda")
        self.eng._abi.check(self.X.bsms_point_owner(*self.mesh(), q.data_ptr(), q.shape[0], out.data_ptr(),
                                                    torch.cuda.current_stream().cuda_stream), "bsms_point_owner")
        return out

    def gather(self, fields, owner, grid=None, points=None, fill=NAN):
        """fields: a device view [S, N, C] with any set and row stride; the grid form -> [S, C, H, W], the point form -> [S, P, C]."""
        S, _, Cn = fields.shape
        assert Cn == 1 or fields.stride(2) == 1
        if points is None:
            W, H = grid[:2]
            out, q, P = torch.empty(S, Cn, H, W, device="cuda"), None, 0
        else:
            qt = torch.as_tensor(points, dtype=torch.float64).reshape(-1, 2).cuda()
            q, P, grid = qt.data_ptr(), qt.shape[0], (1, 1, 0.0, 0.0, 1.0, 1.0)
            out = torch.empty(S, P, Cn, device="cuda")
        self.eng._abi.check(self.X.bsms_field_gather(*self.mesh(), owner.data_ptr(), q, P, *grid, fields.data_ptr(), S, Cn, fields.stride(0),
                                                     fields.stride(1), fill, out.data_ptr(), torch.cuda.current_stream().cuda_stream),
                            "bsms_field_gather")
        return out


def owners_equal_everywhere(raw, grid, ref=None, small_boxes=(0,)):
    """Rasteriser and point locator at the grid's centres, both bit-equal to the reference; returns the reference."""
    W, H = grid[:2]
    q = grid_centres(*grid)
    ref = Located(raw.pos.cpu().numpy(), raw.tris.cpu().numpy(), q, margins=False) if ref is None else ref
    want = ref.owner.reshape(H, W)
    for small in small_boxes:
        got = raw.raster(grid, small).cpu().numpy()
        assert got.dtype == np.int32 and np.array_equal(got, want), (grid, small, int((got != want).sum()))
    assert np.array_equal(raw.locate(q).cpu().numpy(), ref.owner), grid
    return ref


# ------------------------------------------------------------------------------------------------------ exact cases
# pixel centres on the lattice's vertices, edges and diagonals, on its outer boundary and outside it (the lattice spans [0, 32]^2)
EXACT_GRIDS = [(1, 1, 0.0, 0.0, 32.0, 32.0),                      # the one centre is the vertex (16, 16)
               (7, 5, -2.0, -4.0, 6.0, 8.0),                      # x = 1, 7, .., 37; y = 0, 8, .., 32
               (64, 64, -0.25, -0.25, 0.5, 0.5),                  # 0, 0.5, .., 31.5
               (257, 129, -1.0625, -1.125, 0.125, 0.25)]          # -1, -0.875, .., 31; -1, -0.75, .., 31


@pytest.fixture(scope="module")
def lattice_tri():
    return lattice(33, 33, "tri", flip=True)                      # 2048 triangles, every second cell clockwise


@pytest.mark.parametrize("grid", EXACT_GRIDS, ids=lambda g: f"{g[0]}x{g[1]}")
def test_lattice_owners_are_bit_equal_on_every_grid(eng, lattice_tri, grid):
    pos, tris = lattice_tri
    raw = Raw(eng, pos, tris)
    ref = owners_equal_everywhere(raw, grid, small_boxes=(0, 1, 7, 4096))       # whichever way the boxes are walked
    inside = ((ref.q >= 0) & (ref.q <= 32)).all(-1)
    assert np.array_equal(ref.owner >= 0, inside) and ref.count.max() >= 2      # centres on shared edges and vertices: contested
    # deterministic: run to run, and whatever the image held before
    first = raw.raster(grid)
    garbage = torch.randint(-2 ** 31, 2 ** 31 - 1, first.shape, dtype=torch.int64, device="cuda").to(torch.int32)
    assert torch.equal(raw.raster(grid), first) and torch.equal(raw.raster(grid, out=garbage), first)
    # the triangle list rotated: the same owners, mapped back, wherever one triangle alone contains the centre
    for shift in (1, 777):
        rot = Raw(eng, pos, np.roll(tris, shift, axis=0))
        got = rot.raster(grid).cpu().numpy().reshape(-1)
        back = np.where(got >= 0, (got - shift) % len(tris), -1)
        free = ref.count <= 1
        assert np.array_equal(back[free], ref.owner[free]) and np.array_equal(got >= 0, ref.owner >= 0)


@pytest.mark.parametrize("T", [0, 1, 2, 255, 256, 257, 2049])
def test_owners_at_every_triangle_count(eng, lattice_tri, T):
    pos, tris = lattice_tri
    tris = np.concatenate([tris, tris[:1]])[:T]                   # 2049: the first triangle once more, which never wins
    ref = owners_equal_everywhere(Raw(eng, pos, tris), EXACT_GRIDS[2])
    assert (ref.owner >= 0).any() == (T > 0) and ref.owner.max() < min(max(T, 1), 2048)


def special_mesh():
    """Overlaps (the lower index wins), a duplicate, both orientations, zero area, wholly outside, far outside, partly outside on
    each of the four sides of the 64 x 64 grid over [-0.25, 31.75]^2, and corners that are NaN, +inf and -inf."""
    pts = [(2, 2), (10, 2), (2, 10), (4, 1), (12, 9), (4, 9), (0, 0), (5, 5), (10, 10), (100, 100), (110, 100), (100, 110),
           (-6, 12), (4, 14), (-6, 18), (28, 10), (40, 12), (28, 16), (14, -6), (20, -6), (16, 4), (14, 28), (20, 40), (12, 40),
           (np.nan, 20), (np.inf, 20), (-np.inf, 22), (20, 20), (24, 20), (20, 24), (3e38, 3e38), (3.2e38, 3e38), (3e38, 3.2e38),
           (-3e38, 5), (-3.2e38, 5), (-3e38, 9)]
    tris = [(0, 1, 2), (3, 4, 5), (6, 7, 8), (9, 10, 11), (12, 13, 14), (15, 16, 17), (18, 19, 20), (21, 22, 23),
            (24, 27, 28), (27, 25, 29), (26, 28, 29), (0, 2, 1), (30, 31, 32), (33, 34, 35), (27, 28, 29), (29, 28, 27)]
    return np.array(pts, dtype=np.float32), np.array(tris)


def test_special_triangles(eng):
    pos, tris = special_mesh()
    grid = EXACT_GRIDS[2]
    ref = owners_equal_everywhere(Raw(eng, pos, tris), grid, small_boxes=(0, 1, 4096))
    owners = set(ref.owner.tolist())
    assert owners == {-1, 0, 1, 4, 5, 6, 7, 14}                   # nothing for zero area, outside, NaN / inf corners and the later duplicates
    assert ref.count.max() >= 3                                   # T0, T1 and T0's clockwise twin overlap
    for grid in EXACT_GRIDS[:2] + EXACT_GRIDS[3:]:
        owners_equal_everywhere(Raw(eng, pos, tris), grid)


@pytest.mark.parametrize("shape", [(8, 8), (13, 5), (128, 128), (145, 113), (257, 129)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_a_triangle_over_the_whole_image_at_the_edges_of_the_three_walks(eng, shape):
    """One triangle covers every centre: its box is the whole image -- 64 pixels (the lane's last), 65 (the wave's first), 16384 (the
    wave's last), 16385 and 257 x 129 (the list).  Two small triangles in front of it own their pixels."""
    W, H = shape
    pos = np.array([[-1000, -1000], [3000, -1000], [-1000, 3000], [0, 0], [3, 0], [0, 3], [5, 5], [5, 2], [2, 5]], dtype=np.float32)
    tris = np.array([[3, 4, 5], [6, 7, 8], [0, 1, 2]])
    grid = (W, H, -0.25, -0.5, 0.5, 1.0)
    ref = owners_equal_everywhere(Raw(eng, pos, tris), grid)
    assert (ref.owner >= 0).all() and (ref.owner == 2).sum() > W * H // 2 and {0, 1} <= set(ref.owner.tolist())


def test_more_listed_triangles_than_the_list_holds(eng):
    """1030 triangles over the whole 160 x 112 image (17920 pixels each: above the wave's limit) behind a small one: the list takes
    1023 of them, the others are walked by their waves, and the lowest index wins everywhere."""
    big = np.array([[-1000, -1000], [3000, -1000], [-1000, 3000]], dtype=np.float32)
    pos = np.concatenate([np.array([[0, 0], [6, 0], [0, 6]], dtype=np.float32), big])
    tris = np.array([[0, 1, 2]] + [[3, 4, 5], [4, 5, 3], [5, 4, 3]] * 343 + [[3, 4, 5]])
    assert len(tris) == 1031
    grid = (160, 112, -0.25, -0.25, 0.5, 0.5)
    ref = Located(pos, tris[:4], grid_centres(*grid))             # the later copies never win: the reference needs the first four only
    assert set(ref.owner.tolist()) == {0, 1}
    for tail in (tris, np.concatenate([tris[1:], tris[:1]])):     # ... and with the small triangle last: the first large one owns everything
        raw = Raw(eng, pos, tail)
        got = raw.raster(grid).cpu().numpy().reshape(-1)
        want = ref.owner if tail is tris else np.zeros_like(ref.owner)
        assert np.array_equal(got, want)
        assert np.array_equal(raw.locate(ref.q[::7]).cpu().numpy(), want[::7])


def test_triangles_that_name_nodes_outside_the_mesh_own_nothing(eng):
    """The raw entries (MeshSampler refuses such cells earlier): a triangle with an index of N, above N or below 0 would cover the
    image if its index were read; it owns nothing, in the rasteriser and in the point locator, and a sample whose owner is such a
    triangle -- or no triangle of the list -- gets the fill value.  Reference: the same list with those triangles made zero-area."""
    pos = np.array([[-100, -100], [300, -100], [-100, 300], [2, 2], [20, 3], [4, 25]], dtype=np.float32)
    tris = np.array([[0, 1, 6], [-1, 1, 2], [0, 1 << 30, 2], [3, 4, 5], [0, 1, 2], [6, 6, 6]])
    safe = np.where(((tris < 0) | (tris >= 6)).any(1)[:, None], 0, tris)
    raw, grid = Raw(eng, pos, tris), EXACT_GRIDS[2]
    ref = Located(pos, safe, grid_centres(*grid), margins=False)
    assert set(ref.owner.tolist()) == {3, 4}
    for small in (0, 1, 4096):
        assert np.array_equal(raw.raster(grid, small).cpu().numpy().reshape(-1), ref.owner)
    assert np.array_equal(raw.locate(ref.q).cpu().numpy(), ref.owner)
    f = torch.arange(1.0, 13.0, device="cuda").reshape(1, 6, 2)
    owner = torch.tensor([0, 1, 2, 5, -1, -7, 6, 1 << 30, 3, 4], dtype=torch.int32, device="cuda")
    got = raw.gather(f, owner, points=np.tile([[5.0, 6.0]], (10, 1)), fill=-9.0).cpu().numpy()[0]
    assert (got[:8] == -9.0).all() and np.isfinite(got[8:]).all() and (got[8:] != -9.0).all()
    want = Located(pos, safe, [[5.0, 6.0]]).values(f.cpu().numpy(), -9.0)[0, 0]      # owner 3 contains (5, 6)
    assert np.array_equal(got[8], want.astype(np.float32))


def test_the_owner_cache_is_bounded_and_can_be_cleared(eng):
    pos, tris = lattice(5, 5)
    s = eng.MeshSampler(pos, tris, "tri")
    first = s.owner_image(8, 8)
    for k in range(s.MAX_CACHED + 3):
        s.owner_image(8, 8, bounds=(0.0, 4.0 + k, 0.0, 4.0))
    assert len(s._owners) == s.MAX_CACHED
    again = s.owner_image(8, 8)                                   # dropped as the oldest: computed again, the same image
    assert again is not first and torch.equal(again, first)
    s.clear_cache()
    assert len(s._owners) == 0 and torch.equal(s.owner_image(8, 8), first)
    side = torch.cuda.Stream()                                    # every call brings its own list area: two streams do not share one
    with torch.cuda.stream(side):
        other = s.owner_image(8, 8, bounds=(0.0, 4.0, 0.0, 5.0))
    mine = s.owner_image(8, 8, bounds=(0.0, 5.0, 0.0, 4.0))
    torch.cuda.synchronize()
    for img, bounds in ((other, (0.0, 4.0, 0.0, 5.0)), (mine, (0.0, 5.0, 0.0, 4.0))):
        assert np.array_equal(img.cpu().numpy().reshape(-1), Located(pos, tris, grid_centres(*s.grid(8, 8, bounds)), margins=False).owner)


def test_quad_lattice_through_the_sampler(eng):
    pos, quads = lattice(17, 9, "quad", flip=True)
    s = eng.MeshSampler(pos, quads, "quad")
    assert s.T == 2 * len(quads) and s.bounds == (0.0, 16.0, 0.0, 8.0)
    for W, H, bounds in ((64, 32, None), (33, 17, (-0.25, 16.25, -0.25, 8.25)), (7, 5, (-3.0, 18.0, 1.0, 11.0))):
        W, H, x0, y0, dx, dy = grid = s.grid(W, H, bounds)
        ref = Located(pos, split_quads(quads), grid_centres(*grid))
        cells = s.owner_image(W, H, bounds)
        assert cells.dtype == torch.int32 and cells.shape == (H, W) and s.owner_image(W, H, bounds) is cells          # cached per grid
        assert np.array_equal(cells.cpu().numpy().reshape(-1), ref.owner >> 1)
        assert np.array_equal(s.locate(ref.q).cpu().numpy(), ref.owner >> 1)
        assert np.array_equal(s.pixel_centres(W, H, bounds).reshape(-1, 2), ref.q)
    # the centre of quad k lies on its diagonal: the first of its two triangles
    centres = pos[quads].mean(1)
    assert s.locate(centres).tolist() == list(range(len(quads)))


# ------------------------------------------------------------------------------------------------------ generic cases
@pytest.fixture(scope="module", params=range(len(GENERIC)), ids=[g[0] for g in GENERIC])
def generic(request, eng):
    pos, cells, kind, grid = generic_case(request.param)
    tris = cells if kind == "tri" else split_quads(cells)
    raw = Raw(eng, pos, tris)
    ref = Located(pos, tris, grid_centres(*grid))                 # computed once, shared, never written to
    owner = raw.raster(grid)
    return raw, ref, grid, owner, (pos, cells, kind)


def check_owners(ref, got, what):
    got = np.asarray(got).reshape(-1)
    clear = ~ref.ambiguous
    assert np.array_equal(got[clear], ref.owner[clear]), what
    for k in np.nonzero(ref.ambiguous)[0]:                        # within the margin: any triangle that contains it so, or none if none must
        assert ref.contains_within(k, got[k]) if got[k] >= 0 else not ref.strict_any[k], (what, int(k), int(got[k]))


def test_generic_owners(generic):
    raw, ref, grid, owner, _ = generic
    assert ref.ambiguous.mean() <= 1e-3
    print(f"[generic owners] {raw.T} triangles, grid {grid[0]} x {grid[1]}: {int(ref.ambiguous.sum())} ambiguous samples, {int((ref.owner < 0).sum())} unowned")
    check_owners(ref, owner.cpu().numpy(), "raster")
    located = raw.locate(ref.q)
    check_owners(ref, located.cpu().numpy(), "points")
    assert torch.equal(located, owner.reshape(-1))                # the same device function on the same fp64 inputs
    hole = np.linalg.norm(ref.q - 0.5, axis=1) < 0.1
    assert (owner.cpu().numpy().reshape(-1)[hole] == -1).all()
    for small in (1, 16, 4096):
        assert torch.equal(raw.raster(grid, small), owner)


def value_ratio(ref, fields, got, want=None):
    """max |got - want| / bound over the owned, non-ambiguous samples; got [S, P, C]."""
    f = np.asarray(fields, dtype=np.float64)
    want = ref.values(f, 0.0) if want is None else want
    F = ref.field_scale(f)
    with np.errstate(all="ignore"):
        bound = U24 * F + 64 * U53 * (1 + ref.M / np.abs(ref.A))[None, :, None] * F
    use = (ref.owner >= 0) & ~ref.ambiguous
    err = np.abs(np.asarray(got, dtype=np.float64) - want)[:, use]
    bound = np.broadcast_to(bound, want.shape)[:, use]
    assert (err[bound == 0] == 0).all()
    return float((err[bound > 0] / bound[bound > 0]).max()) if (bound > 0).any() else 0.0


@pytest.mark.parametrize("S,Cn", [(1, 1), (4, 3), (37, 8), (1, 8), (37, 1)])
def test_gather_values_against_the_reference(generic, S, Cn):
    raw, ref, grid, owner, _ = generic
    W, H = grid[:2]
    rng = np.random.default_rng(100 * S + Cn)
    f = (rng.standard_normal((S, raw.N, Cn)) * 10.0 ** rng.integers(-3, 4, (S, 1, Cn))).astype(np.float32)
    ft = torch.from_numpy(f).cuda()
    got = raw.gather(ft, owner, grid=grid)
    assert got.shape == (S, Cn, H, W)
    g = got.cpu().numpy()
    unowned = (ref.owner < 0).reshape(H, W)
    assert np.array_equal(np.isnan(g), np.broadcast_to(unowned, g.shape))                   # NaN fill: the unowned samples and only those
    flat = g.reshape(S, Cn, H * W).transpose(0, 2, 1)
    ratio = value_ratio(ref, f, np.nan_to_num(flat))
    print(f"[gather vs reference] S {S} C {Cn} grid {W} x {H}: worst |out - ref| / bound {ratio:.3f}")
    assert ratio <= 1.0
    # the point form at the same coordinates: bit for bit, in its own layout; another fill value lands on the same samples
    pts = raw.gather(ft, owner.reshape(-1), points=ref.q, fill=-3.5)
    assert pts.shape == (S, H * W, Cn)
    assert torch.equal(pts, raw.gather(ft, owner, grid=grid, fill=-3.5).reshape(S, Cn, H * W).permute(0, 2, 1))
    there = torch.from_numpy(ref.owner < 0).cuda()
    assert bool((pts[:, there] == -3.5).all()) and torch.equal(pts[:, ~there], got.reshape(S, Cn, H * W).permute(0, 2, 1)[:, ~there])


def test_linear_and_constant_fields(generic):
    raw, ref, grid, owner, _ = generic
    W, H = grid[:2]
    pos = raw.pos.cpu().numpy().astype(np.float64)
    # planes with small-integer coefficients on positions that are multiples of 2^-14: the fp32 nodal values are exact
    coef = np.array([[7.0, 3.0, -5.0], [-2.0, 0.0, 9.0], [0.0, 1.0, 1.0], [11.0, -6.0, 0.0]])
    nodal = coef[:, 0, None] + coef[:, 1, None] * pos[None, :, 0] + coef[:, 2, None] * pos[None, :, 1]
    f = nodal.astype(np.float32)
    assert np.array_equal(f.astype(np.float64), nodal)
    got = raw.gather(torch.from_numpy(f[..., None]).cuda(), owner, grid=grid, fill=0.0).cpu().numpy().reshape(4, H * W, 1)
    exact = (coef[:, 0, None] + coef[:, 1, None] * ref.q[None, :, 0] + coef[:, 2, None] * ref.q[None, :, 1])[..., None]
    ratio = value_ratio(ref, f[..., None], got, want=exact)
    print(f"[linear fields] grid {W} x {H}: worst |out - plane| / bound {ratio:.3f}")
    assert ratio <= 1.0
    # constants: within one fp32 ulp (weights that sum to 1 within an fp64 ulp do not give more); 0 and the fill value exactly
    consts = np.array([0.0, 1.0, -3.0, 0.1, 1e-3, 123456.789, -7.3e-12, 3.0e30], dtype=np.float32)
    fc = np.broadcast_to(consts[:, None, None], (len(consts), raw.N, 2)).copy()
    out = raw.gather(torch.from_numpy(fc).cuda(), owner, grid=grid, fill=42.0).cpu().numpy()          # [S, 2, H, W]
    owned = (ref.owner >= 0).reshape(H, W)
    assert (out[:, :, ~owned] == 42.0).all() and (out[0][:, owned] == 0.0).all()
    ulps = np.abs(out[:, :, owned].view(np.int32).astype(np.int64) - consts.view(np.int32).astype(np.int64)[:, None, None])
    print(f"[constant fields] worst distance {int(ulps.max())} ulp, {float((ulps == 0).mean()):.4f} of the samples exact")
    assert ulps.max() <= 1


def test_strided_sets_are_read_in_place(generic):
    raw, ref, grid, owner, _ = generic
    rng = np.random.default_rng(5)
    Tn, B, Cn = 6, 3, 3
    big = torch.from_numpy(rng.standard_normal((Tn, B, raw.N, Cn)).astype(np.float32)).cuda()       # rollout_bank's [T-1, B, N, C]
    for b in range(B):
        view = big[:, b]
        assert not view.is_contiguous()
        assert torch.equal(raw.gather(view, owner, grid=grid, fill=0.0), raw.gather(view.contiguous(), owner, grid=grid, fill=0.0))
    wide = torch.from_numpy(rng.standard_normal((4, raw.N, 8)).astype(np.float32)).cuda()
    for lo, hi in ((0, 3), (2, 5), (7, 8), (1, 8)):
        window = wide[..., lo:hi]
        got = raw.gather(window, owner, grid=grid, fill=0.0)
        assert torch.equal(got, raw.gather(window.contiguous(), owner, grid=grid, fill=0.0))
        assert torch.equal(got, raw.gather(wide, owner, grid=grid, fill=0.0)[:, lo:hi])
    every_other = big[::2, 1, :, 1:]
    pts = ref.q[::5]
    own = raw.locate(pts)
    assert torch.equal(raw.gather(every_other, own, points=pts, fill=1.0), raw.gather(every_other.contiguous(), own, points=pts, fill=1.0))
    assert raw.gather(wide[:0], owner, grid=grid).shape == (0, 8, grid[1], grid[0])             # no sets: nothing is launched


# ------------------------------------------------------------------------------------------------------ through the interface
def test_mesh_sampler_rasterize_and_probe(eng, generic):
    raw, ref, grid, owner, (pos, cells, kind) = generic
    W, H, x0, y0, dx, dy = grid
    bounds = (x0, x0 + W * dx, y0, y0 + H * dy)
    s = eng.MeshSampler(torch.from_numpy(pos), cells, kind, device="cuda")
    g = s.grid(W, H, bounds)
    sref = ref if g == grid else Located(pos, raw.tris.cpu().numpy(), grid_centres(*g))      # (x1 - x0) / W need not give dx back
    per = 1 if kind == "tri" else 2
    cells_img = s.owner_image(W, H, bounds)
    check_owners_cells(sref, cells_img.cpu().numpy(), per)
    rng = np.random.default_rng(8)
    f = rng.standard_normal((2, 3, raw.N, 3)).astype(np.float32)
    ft = torch.from_numpy(f).cuda()
    out = s.rasterize(ft, W, H, bounds)
    assert out.shape == (2, 3, 3, H, W)
    flat = out.reshape(6, 3, H * W).permute(0, 2, 1).cpu().numpy()
    assert np.array_equal(np.isnan(flat[0, :, 0]), sref.owner < 0)
    assert value_ratio(sref, f.reshape(6, raw.N, 3), np.nan_to_num(flat)) <= 1.0
    assert torch.equal(s.rasterize(ft[1], W, H, bounds, fill=0.0), torch.nan_to_num(out[1], nan=0.0))
    assert torch.equal(s.rasterize(ft[1, 2], W, H, bounds, fill=0.0), torch.nan_to_num(out[1, 2], nan=0.0))
    assert torch.equal(s.rasterize(ft.transpose(0, 1), W, H, bounds, fill=0.0), torch.nan_to_num(out.transpose(0, 1), nan=0.0))
    # probes: sensor locations anywhere, the hole and the outside included
    pts = rng.uniform(-0.1, 1.1, (301, 2))
    pref = Located(pos, raw.tris.cpu().numpy(), pts)
    assert not pref.ambiguous.any()
    assert np.array_equal(s.locate(pts).cpu().numpy(), np.where(pref.owner >= 0, pref.owner // per, -1))
    pv = s.probe(ft, pts)
    assert pv.shape == (2, 3, 301, 3) and np.array_equal(np.isnan(pv[0, 0, :, 0].cpu().numpy()), pref.owner < 0)
    assert value_ratio(pref, f.reshape(6, raw.N, 3), np.nan_to_num(pv.reshape(6, 301, 3).cpu().numpy())) <= 1.0
    assert s.probe(ft[0, 0], pts[:0]).shape == (0, 3) and s.probe(ft[0, 0], pts[:1]).shape == (1, 3)
    with pytest.raises(ValueError):
        s.rasterize(ft[..., :-1, :], W, H)
    with pytest.raises(ValueError):
        s.rasterize(ft.transpose(-1, -2).contiguous().transpose(-1, -2), W, H)
    with pytest.raises(eng._abi.BsmsError):
        s.rasterize(ft.cpu(), W, H)


def check_owners_cells(ref, cells, per):
    cells = np.asarray(cells).reshape(-1)
    clear = ~ref.ambiguous
    assert np.array_equal(cells[clear], np.where(ref.owner >= 0, ref.owner // per, -1)[clear])


def test_eval_panels_rollout_frames_and_bank_samplers_consistent(eng, monkeypatch):
    _abi = eng._abi
    trajs = same_mesh_trajs(150, 5, 3, seed=21)
    bank = eng.TrajectoryBank(make_cfg(True, depth=1), dataset="airfoil")
    for t in trajs:
        bank.add(t)
    torch.manual_seed(0)
    mcfg = model_cfg(True, depth=1)
    loaded = _abi._sample
    monkeypatch.setattr(_abi, "_sample", None)                    # as in a process that has not sampled anything
    tr = eng.Trainer(eng.BSMS_Simulator(mcfg), mcfg, SimpleNamespace(**vars(OPT), ema_decay=0.9))
    tr.iter(bank.batch([(0, 0), (1, 0), (2, 0)], train=False))    # warm-up: normaliser statistics
    assert tr.iter(bank.batch([(0, 1), (1, 2), (2, 3)])) is not None
    assert tr.iter(bank.batch([(0, 2), (1, 0), (2, 1)])) is not None
    errors, kept = eng.rollout_bank(tr, bank, batch=3, keep_results=True)
    assert _abi._sample is None                                   # training, evaluation and rollouts never load libbsms_hip_sample.so
    monkeypatch.setattr(_abi, "_sample", loaded)

    for k, t in enumerate(trajs):                                 # an owned int32 copy of frame 0, not a view that keeps [T, n_cells, 3] alive
        kept_cells = bank._trajs[k].cells
        assert kept_cells.base is None and kept_cells.flags.owndata and kept_cells.dtype == np.int32 and np.array_equal(kept_cells, t["cells"][0])
    s = bank.sampler(1)
    assert isinstance(s, eng.MeshSampler) and s.N == 150 and s.T == trajs[1]["cells"].shape[1] and s.mesh_type == "tri"
    assert torch.equal(s.pos.cpu(), torch.from_numpy(trajs[1]["mesh_pos"][0]))
    W, H = 48, 40
    data = bank.batch([(0, 1), (2, 0), (1, 3)], train=False)
    with torch.no_grad():
        assert not torch.equal(tr.get_pred(data, True), tr.get_pred(data, False))        # the averaged weights are other weights
    for sample, ema in ((0, False), (2, True), (1, True)):
        panels = tr.eval_panels(data, s, W, H, sample=sample, ema=ema)
        assert panels.shape == (3, 4, H, W)
        with torch.no_grad():
            pred = tr.get_pred(data, ema)[sample]
        node_in, tar = data[0][sample], data[1][sample]
        for k, field in enumerate((node_in[:, :3], tar, pred, pred - tar)):
            want = s.rasterize(field.contiguous(), W, H)          # [C, H, W]
            assert torch.equal(panels[:, k].contiguous().view(torch.int32), want.view(torch.int32)), (sample, k)
    owned = s.owner_image(W, H) >= 0
    assert bool(owned.any()) and bool((~owned).any()) and bool(torch.isnan(panels[:, :, ~owned]).all()) and bool(torch.isfinite(panels[:, :, owned]).all())

    # a kept rollout: one gather per trajectory over the strided [T-1, N, C] view == frame-by-frame rasterisation
    assert all(r.shape == (4, 150, 3) and not r.is_contiguous() for r in kept)
    for every in (1, 3):
        frames = eng.rollout_frames(kept, s, W, H, every=every)
        assert len(frames) == 3
        for r, fr in zip(kept, frames):
            assert fr.shape == (len(range(0, 4, every)), 3, H, W)
            for k, t in enumerate(range(0, 4, every)):
                assert torch.equal(fr[k].view(torch.int32), s.rasterize(r[t].contiguous(), W, H).view(torch.int32))
    assert torch.equal(eng.rollout_frames(kept[2], s, W, H).view(torch.int32), eng.rollout_frames(kept, [s] * 3, W, H)[2].view(torch.int32))
    with pytest.raises(ValueError):
        eng.rollout_frames(kept, [s, s], W, H)

    def count(name):
        real, calls = getattr(s._lib, name), []
        monkeypatch.setattr(s._lib, name, lambda *a: calls.append(1) or real(*a))
        return calls

    gathers, rasters = count("bsms_field_gather"), count("bsms_raster_owner")
    eng.rollout_frames(kept, s, W, H)
    tr.eval_panels(data, s, W, H)
    assert len(gathers) == 3 + 1 and len(rasters) == 0            # one launch per trajectory / per panel set; the owner image is cached


def test_bank_samplers_on_variable_meshes_and_without_cells(eng):
    mcfg = model_cfg(False, depth=1)
    torch.manual_seed(0)
    model = eng.BSMS_Simulator(mcfg).cuda()
    trajs = [synthetic_traj(100, 4, 1), synthetic_traj(140, 4, 2), synthetic_traj(90, 5, 3)]
    bank = eng.TrajectoryBank(make_cfg(False, depth=1), dataset="cylinder_flow", process=model.process)
    for t in trajs:
        bank.add(t)
    rng = np.random.default_rng(3)
    for i, t in enumerate(trajs):
        s = bank.sampler(i)
        assert s.N == t["mesh_pos"].shape[1] and s.T == t["cells"].shape[1]
        pts = rng.uniform(0.05, 0.95, (64, 2))
        ref = Located(t["mesh_pos"][0], t["cells"][0], pts)
        clear = ~ref.ambiguous
        assert np.array_equal(s.locate(pts).cpu().numpy()[clear], ref.owner[clear]) and (ref.owner[clear] >= 0).sum() > 32
        state = bank.resident(i)[0]                               # [T, N, C] in HBM: probed in place
        vals = s.probe(state, pts, fill=0.0)
        assert vals.shape == (state.shape[0], 64, 3)
        assert value_ratio(ref, state.cpu().numpy(), vals.cpu().numpy()) <= 1.0
    # eval_panels on a variable-mesh batch: ONE sample of sum N rows, so the sampler spans the block-diagonal union
    tr = eng.Trainer(model, mcfg, OPT)
    tr.iter(bank.batch([(0, 0), (1, 0), (2, 0)], train=False))    # warm-up: normaliser statistics
    picks = [(2, 1), (0, 2)]
    data = bank.batch(picks, train=False)
    rows = np.cumsum([0] + [trajs[i]["mesh_pos"].shape[1] for i, _ in picks])
    union = eng.MeshSampler(data[0].x[:, 3:5], np.concatenate([trajs[i]["cells"][0] + r for (i, _), r in zip(picks, rows)]), "tri")
    assert union.N == rows[-1] == data[0].x.shape[0]
    W, H = 40, 36
    panels = tr.eval_panels(data, union, W, H)
    assert panels.shape == (3, 4, H, W)
    with torch.no_grad():
        pred = tr.get_pred(data).reshape(-1, 3)
    for k, field in enumerate((data[0].x[:, :3], data[0].y, pred, pred - data[0].y)):
        assert torch.equal(panels[:, k].contiguous().view(torch.int32), union.rasterize(field.contiguous(), W, H).view(torch.int32)), k
    assert bool(torch.isfinite(panels[:, :, union.owner_image(W, H) >= 0]).all())
    with pytest.raises(IndexError):
        tr.eval_panels(data, union, W, H, sample=1)


def test_a_bank_without_cells_refuses_a_sampler(eng):
    """As node_weights="measure" refuses: a later trajectory of a consistent mesh reads cfg.field_names only."""
    dcfg = make_cfg(True, depth=1)
    trajs = same_mesh_trajs(80, 3, 2, seed=6)
    bank = eng.TrajectoryBank(dcfg, dataset="airfoil")
    bank.add(trajs[0])
    dcfg.field_names = [k for k in dcfg.field_names if k != "cells"]
    assert bank.add(trajs[1]) == 1
    assert bank.sampler(0).T == trajs[0]["cells"].shape[1]
    with pytest.raises(ValueError, match="cells"):
        bank.sampler(1)
