"""Nodal fields of a 2-D mesh sampled on the device (libbsms_hip_sample.so, include/bsms_hip_sample.h): locate points
in the cell complex, interpolate linearly.  `MeshSampler` serves a regular grid of pixel centres (`owner_image`, `rasterize`) and
arbitrary point lists (`locate`, `probe`); `rollout_frames` rasterises a kept rollout, `write_png` puts an image on disk with the
standard library alone.  Nothing here is imported by the training path, and the library is loaded by the first sampler only."""
import struct
import zlib

import numpy as np
import torch

from . import _abi

__all__ = ["MeshSampler", "rollout_frames", "write_png"]

_MAX_C = 8


def _triangles(pos, cells, mesh_type):
    """int32 [T, 3] triangles of `cells` (quads split on the diagonal 0-2: cell k is the triangles 2k and 2k + 1), validated as
    hierarchy.lumped_node_measure64 validates its cells.  Host NumPy; refuses before any device call."""
    if mesh_type not in ("tri", "quad"):
        raise ValueError(f"MeshSampler: mesh type {mesh_type!r} is not a 2-D cell complex (\"tri\" or \"quad\")")
    if pos.ndim != 2 or pos.shape[1] != 2:
        raise ValueError(f"MeshSampler: positions of shape {tuple(pos.shape)} are not [N, 2]")
    cells = np.asarray(cells)
    corners = 3 if mesh_type == "tri" else 4
    if cells.ndim != 2 or cells.shape[1] != corners:
        raise ValueError(f"MeshSampler: {mesh_type!r} cells must have {corners} nodes each, got an array of shape {cells.shape}")
    cells = cells.astype(np.int64)
    if cells.size and (cells.min() < 0 or cells.max() >= pos.shape[0]):
        raise ValueError(f"MeshSampler: a cell names node {int(cells.max())} (or a negative one) of a mesh of {pos.shape[0]}")
    if mesh_type == "quad":
        cells = np.stack([cells[:, [0, 1, 2]], cells[:, [0, 2, 3]]], axis=1).reshape(-1, 3)
    return np.ascontiguousarray(cells, dtype=np.int32)


def _sets(fields, N):
    """The leading dimensions of `fields` [..., N, C] as runs (first set, offset in floats, sets, set stride) that cover them in order
    without a copy: the innermost leading dimensions collapse into one set stride as far as their strides allow, the others are
    walked."""
    lead, strides = list(fields.shape[:-2]), list(fields.stride()[:-2])
    keep = len(lead)                                   # dimensions [keep:] collapse into one run of sets
    while keep > 0:
        inner = lead[keep:]
        if inner and strides[keep - 1] != strides[keep] * lead[keep]:
            break
        keep -= 1
    run = int(np.prod(lead[keep:], dtype=np.int64)) if lead[keep:] else 1
    run_stride = strides[-1] if lead[keep:] else 0
    outer = lead[:keep]
    runs = []
    for flat in range(int(np.prod(outer, dtype=np.int64)) if outer else 1):
        idx, rem = [], flat
        for d in reversed(outer):
            idx.append(rem % d)
            rem //= d
        off = sum(i * s for i, s in zip(reversed(idx), strides[:keep]))
        runs.append((flat * run, off, run, run_stride))
    return runs


class MeshSampler:
    """Point location and linear interpolation on a 2-D mesh, on the device.

    `pos` [N, 2] (any real dtype; kept as float32 on the device, which is what the fields' positions are), `cells` [n_cells, 3]
    ("tri") or [n_cells, 4] ("quad", split on the diagonal 0-2 as `lumped_node_measure` splits them).  Owners are reported as indices
    of the caller's cells.  Other mesh types, positions that are not two-dimensional and cells that name a node outside the mesh raise
    ValueError before any device call."""

    def __init__(self, pos, cells, mesh_type, device=None):
        host = pos.detach().cpu().numpy() if torch.is_tensor(pos) else np.asarray(pos)
        tris = _triangles(host, cells.detach().cpu().numpy() if torch.is_tensor(cells) else cells, mesh_type)
        self.mesh_type, self.per_cell = mesh_type, 1 if mesh_type == "tri" else 2
        if device is None:
            device = pos.device if torch.is_tensor(pos) and pos.is_cuda else torch.device("cuda", torch.cuda.current_device())
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise _abi.BsmsError("MeshSampler needs a GPU device; there is no CPU fallback")
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self.pos = torch.as_tensor(host, dtype=torch.float32).contiguous().to(self.device)
        self.tris = torch.from_numpy(tris).to(self.device)
        self.N, self.T = int(host.shape[0]), int(tris.shape[0])
        p64 = self.pos.cpu().numpy().astype(np.float64)
        self.bounds = (float(p64[:, 0].min()), float(p64[:, 0].max()), float(p64[:, 1].min()), float(p64[:, 1].max())) if self.N else (0.0, 1.0, 0.0, 1.0)
        self._owners = {}                               # grid -> (triangle owners, cell owners), at most MAX_CACHED of them, oldest out first
        self._lib = _abi.sample()

    MAX_CACHED = 8                                      # owner images kept (a 2048 x 2048 image is 16 MB, twice that for quads)

    def clear_cache(self):
        """Drop the cached owner images."""
        self._owners.clear()

    # ------------------------------------------------------------------------------------------------ plumbing
    def _mesh_args(self):
        return self.pos.data_ptr() if self.N else None, 2, self.N, self.tris.data_ptr() if self.T else None, self.T

    def _stream(self):
        return torch.cuda.current_stream(self.device).cuda_stream

    def grid(self, width, height, bounds=None):
        """(W, H, x0, y0, dx, dy) of a grid over `bounds` = (xmin, xmax, ymin, ymax), default the bounding box of the positions:
        pixel (j, i) has its centre at (x0 + (i + 0.5) dx, y0 + (j + 0.5) dy)."""
        W, H = int(width), int(height)
        if W < 1 or H < 1:
            raise ValueError(f"MeshSampler: a grid of {W} x {H} pixels")
        xmin, xmax, ymin, ymax = (float(v) for v in (self.bounds if bounds is None else bounds))
        dx, dy = (xmax - xmin) / W, (ymax - ymin) / H
        if not all(np.isfinite(v) for v in (xmin, ymin, dx, dy)) or dx == 0.0 or dy == 0.0:
            raise ValueError(f"MeshSampler: bounds {(xmin, xmax, ymin, ymax)} do not span a grid")
        return W, H, xmin, ymin, dx, dy

    def pixel_centres(self, width, height, bounds=None):
        """float64 [H, W, 2] on the host: the centres `owner_image` and `rasterize` sample."""
        W, H, x0, y0, dx, dy = self.grid(width, height, bounds)
        x, y = x0 + (np.arange(W) + 0.5) * dx, y0 + (np.arange(H) + 0.5) * dy
        return np.stack(np.broadcast_arrays(x[None, :], y[:, None]), axis=-1)

    def _points(self, points):
        q = torch.as_tensor(points, dtype=torch.float64)
        if q.dim() != 2 or q.shape[1] != 2:
            raise ValueError(f"MeshSampler: points of shape {tuple(q.shape)} are not [P, 2]")
        return q.to(self.device).contiguous()

    def _check_fields(self, fields):
        if not torch.is_tensor(fields) or not fields.is_cuda or fields.device != self.device or fields.dtype != torch.float32:
            raise _abi.BsmsError(f"MeshSampler: fields must be a float32 tensor on {self.device}; there is no CPU fallback")
        if fields.dim() < 2 or fields.shape[-2] != self.N or not 1 <= fields.shape[-1] <= _MAX_C:
            raise ValueError(f"MeshSampler: fields of shape {tuple(fields.shape)} are not [..., {self.N}, C] with C in 1..{_MAX_C}")
        if fields.shape[-1] > 1 and fields.stride(-1) != 1:
            raise ValueError("MeshSampler: the channels of a row must be adjacent (stride 1); rows and sets may be strided")
        if fields.shape[-2] > 1 and fields.stride(-2) < fields.shape[-1]:
            raise ValueError("MeshSampler: the rows of a field set overlap")

    def _tri_owners(self, width, height, bounds=None, small_box=0):
        key = self.grid(width, height, bounds)
        hit = self._owners.get(key)
        if hit is None or small_box:
            W, H, x0, y0, dx, dy = key
            with torch.cuda.device(self.device):
                own = torch.empty(H, W, dtype=torch.int32, device=self.device)
                # the list area of THIS call, from torch's allocator: it belongs to the current stream, so calls on several streams
                # (or in several captures) never share a counter
                work = torch.empty(int(self._lib.bsms_raster_work_bytes()), dtype=torch.uint8, device=self.device)
                _abi.check(self._lib.bsms_raster_owner(*self._mesh_args(), W, H, x0, y0, dx, dy, int(small_box), own.data_ptr(),
                                                       work.data_ptr(), self._stream()), "bsms_raster_owner")
            if small_box:                               # a threshold sweep: not the cached image
                return own
            while len(self._owners) >= self.MAX_CACHED:
                del self._owners[next(iter(self._owners))]
            hit = self._owners[key] = (own, own if self.per_cell == 1 else own >> 1)    # -1 >> 1 == -1
        return hit[0]

    def _gather(self, fields, owners, points, grid, fill):
        self._check_fields(fields)
        lead, C = tuple(fields.shape[:-2]), int(fields.shape[-1])
        S = int(np.prod(lead, dtype=np.int64)) if lead else 1
        if points is None:
            W, H, x0, y0, dx, dy = grid
            out = torch.empty(S, C, H, W, dtype=torch.float32, device=self.device)
            P, qptr, per_set = 0, None, C * H * W
        else:
            W, H, x0, y0, dx, dy = 1, 1, 0.0, 0.0, 1.0, 1.0
            P = int(points.shape[0])
            out = torch.empty(S, P, C, dtype=torch.float32, device=self.device)
            qptr, per_set = points.data_ptr() if P else None, P * C
        row_stride = int(fields.stride(-2)) if self.N > 1 else C
        with torch.cuda.device(self.device):
            for first, off, run, stride in _sets(fields, self.N):
                if run == 0 or per_set == 0:
                    continue
                _abi.check(self._lib.bsms_field_gather(*self._mesh_args(), owners.data_ptr(), qptr, P, W, H, x0, y0, dx, dy,
                                                       fields.data_ptr() + 4 * off, run, C, int(stride), row_stride, float(fill),
                                                       out.data_ptr() + 4 * first * per_set, self._stream()), "bsms_field_gather")
        return out.reshape(*lead, *out.shape[1:])

    # ------------------------------------------------------------------------------------------------ the grid
    def owner_image(self, width, height, bounds=None):
        """int32 [H, W]: the cell that owns every pixel centre (the lowest index among those that contain it), -1 where none does.
        One bsms_raster_owner call per grid; the last MAX_CACHED grids are cached (`clear_cache` drops them).  The image is written on
        the current stream: a caller that reads a cached image on another stream orders the two, as with any tensor."""
        self._tri_owners(width, height, bounds)
        return self._owners[self.grid(width, height, bounds)][1]

    def rasterize(self, fields, width, height, bounds=None, fill=float("nan")):
        """`fields` [..., N, C] (float32 on the sampler's device; sets and rows may be strided views, nothing is copied) -> float32
        [..., C, H, W]: the linear interpolant at every pixel centre, `fill` where no cell owns it."""
        return self._gather(fields, self._tri_owners(width, height, bounds), None, self.grid(width, height, bounds), fill)

    # ------------------------------------------------------------------------------------------------ point lists
    def _locate(self, q):
        own = torch.empty(q.shape[0], dtype=torch.int32, device=self.device)
        with torch.cuda.device(self.device):
            _abi.check(self._lib.bsms_point_owner(*self._mesh_args(), q.data_ptr() if q.shape[0] else None, int(q.shape[0]),
                                                  own.data_ptr() if q.shape[0] else None, self._stream()), "bsms_point_owner")
        return own

    def locate(self, points):
        """int32 [P]: the cell that owns every point of `points` [P, 2] (taken as float64), or -1."""
        own = self._locate(self._points(points))
        return own if self.per_cell == 1 else own >> 1

    def probe(self, fields, points, fill=float("nan")):
        """`fields` [..., N, C] -> float32 [..., P, C]: the linear interpolant at `points` [P, 2], `fill` outside the mesh."""
        q = self._points(points)
        return self._gather(fields, self._locate(q), q, None, fill)


def rollout_frames(results, sampler, width, height, every=1, bounds=None, fill=float("nan")):
    """A kept rollout on a grid: `results` as `rollout_bank(keep_results=True)` returns them -- one [T-1, N, C] device view, or the
    list of them with `sampler` a list of as many samplers (or one for all) -- to float32 [ceil((T-1) / every), C, H, W] each.  One
    bsms_field_gather launch per trajectory, reading the strided view in place."""
    if torch.is_tensor(results):
        return sampler.rasterize(results[::int(every)], width, height, bounds, fill)
    samplers = sampler if isinstance(sampler, (list, tuple)) else [sampler] * len(results)
    if len(samplers) != len(results):
        raise ValueError(f"rollout_frames: {len(results)} results, {len(samplers)} samplers")
    return [s.rasterize(r[::int(every)], width, height, bounds, fill) for r, s in zip(results, samplers)]


# ------------------------------------------------------------------------------------------------------ images
# the one colour map: piecewise linear through these (position, R, G, B) knots -- dark blue, blue-green, green, yellow
_KNOTS = np.array([[0.0, 68, 1, 84], [0.25, 59, 82, 139], [0.5, 33, 145, 140], [0.75, 94, 201, 98], [1.0, 253, 231, 37]], dtype=np.float64)
BACKGROUND = (255, 255, 255)                            # NaN pixels (RGB); greyscale images take its first component


def colour_map(u):
    """uint8 [..., 3] of `u` in [0, 1] (clipped): linear between the knots."""
    u = np.clip(np.asarray(u, dtype=np.float64), 0.0, 1.0)
    return np.stack([np.rint(np.interp(u, _KNOTS[:, 0], _KNOTS[:, k])) for k in (1, 2, 3)], axis=-1).astype(np.uint8)


def _chunk(kind, body):
    return struct.pack(">I", len(body)) + kind + body + struct.pack(">I", zlib.crc32(kind + body) & 0xFFFFFFFF)


def write_png(path, image, vmin=None, vmax=None, grey=False):
    """Write `image` [H, W] (array or tensor) as an 8-bit PNG: through the built-in colour map as RGB, or as greyscale (`grey`).
    Values map linearly from [vmin, vmax] (default: the finite range of the image) to [0, 1]; NaN pixels get BACKGROUND.  Row 0 of
    the image is the BOTTOM line of the picture (y up, as the grids of MeshSampler).  Standard library and NumPy only."""
    a = image.detach().cpu().numpy() if torch.is_tensor(image) else np.asarray(image)
    a = a.astype(np.float64)
    if a.ndim != 2 or a.size == 0:
        raise ValueError(f"write_png: an image of shape {a.shape} is not [H, W]")
    nan = np.isnan(a)
    finite = a[np.isfinite(a)]
    lo = float(vmin) if vmin is not None else (float(finite.min()) if finite.size else 0.0)
    hi = float(vmax) if vmax is not None else (float(finite.max()) if finite.size else 1.0)
    u = np.clip((np.where(nan, lo, a) - lo) / (hi - lo), 0.0, 1.0) if hi > lo else np.zeros_like(a)
    if grey:
        px = np.rint(u * 255.0).astype(np.uint8)[..., None]
        px[nan] = BACKGROUND[0]
    else:
        px = colour_map(u)
        px[nan] = BACKGROUND
    px = px[::-1]                                       # the file's first scan line is the top of the picture
    H, W = a.shape
    lines = np.concatenate([np.zeros((H, 1), dtype=np.uint8), px.reshape(H, -1)], axis=1)      # filter type 0 in front of every line
    data = b"\x89PNG\r\n\x1a\n" + _chunk(b"IHDR", struct.pack(">IIBBBBB", W, H, 8, 0 if grey else 2, 0, 0, 0)) + \
        _chunk(b"IDAT", zlib.compress(lines.tobytes(), 6)) + _chunk(b"IEND", b"")
    with open(path, "wb") as fh:
        fh.write(data)
    return path
