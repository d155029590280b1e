"""Spatial derivatives of nodal fields on a 2-D mesh, on the device (libbsms_hip_diffop.so, include/bsms_hip_diffop.h):
the P1 gradient per cell, its area-weighted recovery at the nodes, divergence and vorticity of a velocity pair, the H1 error sums and
their adjoint.  `MeshGradient` holds a mesh's triangles and its node -> triangle incidence; `cell_gradient_loss` is the differentiable
loss term on top of the sums.  Nothing here is imported by the training path, and the library is loaded by the first `MeshGradient`
only."""
import numpy as np
import torch

from . import _abi
from .sample import MeshSampler, _sets, _triangles

__all__ = ["MeshGradient", "cell_gradient_loss", "incidence"]

TAIL = 4                                                # DP | DT | WE | WT behind A | GE[C] | GT[C]


def incidence(tris, N):
    """(inc_ptr int32 [N + 1], inc_tri int32 [nnz]) of `tris` [T, 3]: the triangles of node n at inc_tri[inc_ptr[n]:inc_ptr[n + 1]],
    ascending, each (node, triangle) pair once -- the sorted distinct keys node * T + triangle.  Host NumPy."""
    tris = np.asarray(tris, dtype=np.int64).reshape(-1, 3)
    T = len(tris)
    if 3 * T > np.iinfo(np.int32).max:
        raise ValueError(f"incidence: {T} triangles exceed an int32 list")
    key = np.unique(tris.ravel() * max(T, 1) + np.repeat(np.arange(T, dtype=np.int64), 3))
    node, tri = key // max(T, 1), key % max(T, 1)
    ptr = np.zeros(int(N) + 1, dtype=np.int64)
    np.cumsum(np.bincount(node, minlength=int(N)), out=ptr[1:])
    return ptr.astype(np.int32), tri.astype(np.int32)


def _cut(runs, bounds):
    """`runs` of `_sets`, cut at the set indices `bounds`."""
    out = []
    for first, off, run, stride in runs:
        cuts = [first] + [b for b in bounds if first < b < first + run] + [first + run]
        out += [(lo, off + (lo - first) * stride, hi - lo, stride) for lo, hi in zip(cuts[:-1], cuts[1:])]
    return out


class MeshGradient:
    """P1 gradients on a 2-D mesh, on the device.

    `pos` [N, 2] and `cells` as `sample.MeshSampler` takes them ("tri", or "quad" split on the diagonal 0-2 by the sampler's own
    `_triangles`); values per cell are reported per TRIANGLE (a quad k is the triangles 2k and 2k + 1).  Other mesh types, positions
    that are not [N, 2] and cells that name a node outside the mesh raise ValueError before any device call; without a GPU the
    constructor raises BsmsError.  The incidence (`incidence`) is built once on the host and kept on the device as int32.

    `fields` is [..., N, C] float32 on the device, C in 1..8; sets and rows may be strided views and are read in place."""

    def __init__(self, pos, cells, mesh_type, device=None):
        host = pos.detach().cpu().numpy() if torch.is_tensor(pos) else np.asarray(pos)
        tris = _triangles(host, cells.detach().cpu().numpy() if torch.is_tensor(cells) else cells, mesh_type)
        self.mesh_type, self.per_cell = mesh_type, 1 if mesh_type == "tri" else 2
        if device is None:
            if torch.is_tensor(pos) and pos.is_cuda:
                device = pos.device
            elif torch.cuda.is_available():
                device = torch.device("cuda", torch.cuda.current_device())
            else:
                device = "cpu"
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise _abi.BsmsError("MeshGradient needs a GPU device; there is no CPU fallback")
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self.N, self.T = int(host.shape[0]), int(tris.shape[0])
        ptr, tri = incidence(tris, self.N)
        self.pos = torch.as_tensor(host, dtype=torch.float32).contiguous().to(self.device)
        self.tris = torch.from_numpy(tris).to(self.device)
        self.inc_ptr, self.inc_tri = torch.from_numpy(ptr).to(self.device), torch.from_numpy(tri).to(self.device)
        self.nnz = int(tri.shape[0])
        self._lib = _abi.diffop()

    # ------------------------------------------------------------------------------------------------ plumbing
    _check_fields = MeshSampler._check_fields            # the sampler's own check: it reads self.N and self.device only

    def _mesh_args(self):
        return self.pos.data_ptr() if self.N else None, 2, self.N, self.tris.data_ptr() if self.T else None, self.T

    def _inc_args(self):
        return self.inc_ptr.data_ptr(), self.inc_tri.data_ptr() if self.nnz else None, self.nnz

    def _stream(self):
        return torch.cuda.current_stream(self.device).cuda_stream

    def _row_stride(self, fields):
        return int(fields.stride(-2)) if self.N > 1 else int(fields.shape[-1])

    def _pair(self, velocity, C):
        if velocity is None:
            return -1, -1
        cu, cv = (int(v) for v in velocity)
        if not (0 <= cu < C and 0 <= cv < C and cu != cv):
            raise ValueError(f"MeshGradient: velocity channels {(cu, cv)} of {C} channels")
        return cu, cv

    def _gradient(self, fields, fill, rows, launch):
        self._check_fields(fields)
        lead, C = tuple(fields.shape[:-2]), int(fields.shape[-1])
        S = int(np.prod(lead, dtype=np.int64)) if lead else 1
        out = torch.empty(S, rows, C, 2, dtype=torch.float32, device=self.device)
        per_set = rows * C * 2
        with torch.cuda.device(self.device):
            for first, off, run, stride in _sets(fields, self.N):
                if run and per_set:
                    launch(fields.data_ptr() + 4 * off, run, C, int(stride), self._row_stride(fields), float(fill),
                           out.data_ptr() + 4 * first * per_set)
        return out.reshape(*lead, rows, C, 2)

    # ------------------------------------------------------------------------------------------------ gradients
    def cell_gradient(self, fields, fill=float("nan")):
        """float32 [..., T, C, 2]: the P1 gradient (d/dx, d/dy) of every channel on every triangle, `fill` on a degenerate one."""
        def launch(f, S, C, set_stride, row_stride, fill, out):
            _abi.check(self._lib.bsms_cell_gradient(*self._mesh_args(), f, S, C, set_stride, row_stride, fill, out, self._stream()),
                       "bsms_cell_gradient")
        return self._gradient(fields, fill, self.T, launch)

    def node_gradient(self, fields, fill=float("nan"), long_list=0):
        """float32 [..., N, C, 2]: the area-weighted mean of the gradients of the triangles around every node, `fill` at a node that
        no valid triangle touches.  Bit-identical run to run (no atomics).  `long_list`: the list length above which a node is walked
        by its wave (0: the measured default); the values do not depend on it."""
        def launch(f, S, C, set_stride, row_stride, fill, out):
            _abi.check(self._lib.bsms_node_gradient(*self._mesh_args(), *self._inc_args(), f, S, C, set_stride, row_stride, fill,
                                                    int(long_list), out, self._stream()), "bsms_node_gradient")
        return self._gradient(fields, fill, self.N, launch)

    def _velocity_gradient(self, fields, velocity):
        C = int(fields.shape[-1]) if torch.is_tensor(fields) and fields.dim() else 0
        cu, cv = self._pair(velocity, C)
        lo = min(cu, cv)
        g = self.node_gradient(fields[..., lo:max(cu, cv) + 1])           # a view: the channels between the pair come along
        return g[..., cu - lo, :], g[..., cv - lo, :]

    def divergence(self, fields, velocity=(0, 1)):
        """float32 [..., N, 1]: du/dx + dv/dy of the channel pair `velocity` = (u, v) at the nodes: ONE fp32 torch addition of two
        components of `node_gradient` (NaN at a node without a valid triangle).  `MeshSampler.rasterize` and `rollout_frames` take
        it as it is."""
        gu, gv = self._velocity_gradient(fields, velocity)
        return (gu[..., 0] + gv[..., 1]).unsqueeze(-1)

    def vorticity(self, fields, velocity=(0, 1)):
        """float32 [..., N, 1]: dv/dx - du/dy at the nodes: ONE fp32 torch subtraction of two components of `node_gradient`."""
        gu, gv = self._velocity_gradient(fields, velocity)
        return (gv[..., 0] - gu[..., 1]).unsqueeze(-1)

    # ------------------------------------------------------------------------------------------------ sums and adjoint
    def _operands(self, pred, target, mask):
        self._check_fields(pred)
        self._check_fields(target)
        if pred.shape != target.shape:
            raise ValueError(f"MeshGradient: pred {tuple(pred.shape)} and target {tuple(target.shape)} differ")
        lead = tuple(pred.shape[:-2])
        S = int(np.prod(lead, dtype=np.int64)) if lead else 1
        mask_stride = 0
        if mask is not None:
            if not torch.is_tensor(mask) or mask.device != self.device:
                raise _abi.BsmsError(f"MeshGradient: mask must be a tensor on {self.device}")
            if mask.numel() not in (self.N, S * self.N):
                raise ValueError(f"MeshGradient: a mask of shape {tuple(mask.shape)} covers neither {self.N} nodes nor {S} x {self.N}")
            mask_stride = self.N if mask.numel() == S * self.N and S > 1 else 0
            mask = mask.to(torch.float32).reshape(-1, self.N).contiguous() if self.N else None
        runs_p, runs_t = _sets(pred, self.N), _sets(target, self.N)
        bounds = sorted({r[0] for r in runs_p} | {r[0] for r in runs_t})
        return S, mask, mask_stride, list(zip(_cut(runs_p, bounds), _cut(runs_t, bounds)))

    def sums(self, pred, target, mask=None, velocity=None):
        """float64 [S, 1 + 2C + 4] on the device, S the product of the leading dimensions: per set the row
        [A | GE[C] | GT[C] | DP | DT | WE | WT] of bsms_cell_gradient_sums -- area, the squared H1 seminorm of pred - target and of
        target per channel, the squared L2 norms of div(pred), div(target), curl(pred - target), curl(target) of the channel pair
        `velocity` (None: the last four are zeros).  `mask` [N], [N, 1] or one per set: a triangle weighs the product of its corners'
        values.  Deterministic: a row is bit-identical whatever S, the strides or its neighbours are."""
        S, mask, mask_stride, runs = self._operands(pred, target, mask)
        C = int(pred.shape[-1])
        cu, cv = self._pair(velocity, C)
        ncol = 1 + 2 * C + TAIL
        out = torch.empty(S, ncol, dtype=torch.float64, device=self.device)
        with torch.cuda.device(self.device):
            for (first, off_p, run, stride_p), (_, off_t, _, stride_t) in runs:
                if run == 0:
                    continue
                work = torch.empty(int(self._lib.bsms_cell_gradient_work_bytes(run, self.T)), dtype=torch.uint8, device=self.device)
                _abi.check(self._lib.bsms_cell_gradient_sums(
                    *self._mesh_args(), pred.data_ptr() + 4 * off_p, int(stride_p), self._row_stride(pred), target.data_ptr() + 4 * off_t,
                    int(stride_t), self._row_stride(target), None if mask is None else mask.data_ptr() + 4 * first * mask_stride, mask_stride,
                    run, C, cu, cv, out.data_ptr() + 8 * first * ncol, work.data_ptr(), self._stream()), "bsms_cell_gradient_sums")
        return out

    def backward(self, pred, target, mask, coef, velocity=None, out=None, accumulate=False):
        """float32 [..., N, C]: the gradient with respect to `pred` of sum_s (sum_c k_c GE[s, c] + k_D DP[s] + k_W WE[s]) with `coef`
        float64 [S, C + 2] = [k_0 .. k_{C-1} | k_D | k_W] on the device (bsms_cell_gradient_bwd: node-owned, deterministic).  Written
        to `out` (contiguous, pred's shape), or ADDED to it in fp32 when `accumulate`."""
        S, mask, mask_stride, runs = self._operands(pred, target, mask)
        C = int(pred.shape[-1])
        cu, cv = self._pair(velocity, C)
        if not torch.is_tensor(coef) or coef.device != self.device or coef.dtype != torch.float64 or tuple(coef.shape) != (S, C + 2):
            raise ValueError(f"MeshGradient.backward: coef must be float64 [{S}, {C + 2}] on {self.device}")
        coef = coef.contiguous()
        if out is None:
            if accumulate:
                raise ValueError("MeshGradient.backward: accumulate needs `out`")
            out = torch.empty(pred.shape, dtype=torch.float32, device=self.device)
        elif out.shape != pred.shape or out.dtype != torch.float32 or out.device != self.device or not out.is_contiguous():
            raise ValueError(f"MeshGradient.backward: out must be a contiguous float32 tensor of shape {tuple(pred.shape)} on {self.device}")
        with torch.cuda.device(self.device):
            for (first, off_p, run, stride_p), (_, off_t, _, stride_t) in runs:
                if run == 0 or self.N == 0:
                    continue
                _abi.check(self._lib.bsms_cell_gradient_bwd(
                    *self._mesh_args(), *self._inc_args(), pred.data_ptr() + 4 * off_p, int(stride_p), self._row_stride(pred),
                    target.data_ptr() + 4 * off_t, int(stride_t), self._row_stride(target),
                    None if mask is None else mask.data_ptr() + 4 * first * mask_stride, mask_stride, run, C, cu, cv,
                    coef.data_ptr() + 8 * first * (C + 2), int(bool(accumulate)), out.data_ptr() + 4 * first * self.N * C, self.N,
                    self._stream()), "bsms_cell_gradient_bwd")
        return out


class _CellSums(torch.autograd.Function):
    """bsms_cell_gradient_sums forward, bsms_cell_gradient_bwd backward: the gradient of sum_s G[s] . sums[s] with respect to pred (G the
    incoming gradient of the sums, already on the device: nothing is read back).  A, GT, DT and WT do not depend on pred."""

    @staticmethod
    def forward(ctx, pred, target, mask, ops, velocity):
        ctx.save_for_backward(pred, target, *(() if mask is None else (mask,)))
        ctx.ops, ctx.velocity = ops, velocity
        return ops.sums(pred, target, mask, velocity)

    @staticmethod
    def backward(ctx, grad_sums):
        pred, target, *rest = ctx.saved_tensors
        C = pred.shape[-1]
        g = grad_sums.to(torch.float64)
        coef = torch.cat([g[:, 1:1 + C], g[:, 1 + 2 * C:2 + 2 * C], g[:, 3 + 2 * C:4 + 2 * C]], dim=1).contiguous()
        return ctx.ops.backward(pred, target, rest[0] if rest else None, coef, ctx.velocity), None, None, None, None


def cell_gradient_loss(ops, pred, target, mask=None, channel_weights=None, div_weight=0.0, vort_weight=0.0, velocity=None):
    """The cell-gradient (H1 seminorm) loss term on `ops`' mesh, a differentiable fp32 scalar:

        J_s = sum_c w_c GE[s, c] + div_weight DP[s] + vort_weight WE[s]          loss = sum_s J_s / sum_s A_s

    with the sums of `MeshGradient.sums` per set s of `pred` / `target` [..., N, C]: the area-weighted mean of |grad(pred - target)|^2
    per channel (`channel_weights`, default ones), of div(pred)^2 (the mass-conservation residual of the predicted velocity) and of
    curl(pred - target)^2 for the channel pair `velocity`.  The sums are bsms_cell_gradient_sums, the gradient with respect to `pred` is
    bsms_cell_gradient_bwd with the coefficients formed from the sums row by fp64 torch ops on the device -- nothing is read back, and
    the term can be captured into a graph as `edge_difference_loss` can; `target` and `mask` get no gradient."""
    C = int(pred.shape[-1])
    if (div_weight or vort_weight) and velocity is None:
        raise ValueError("cell_gradient_loss: div_weight and vort_weight need the velocity channel pair")
    w = [1.0] * C if channel_weights is None else [float(v) for v in np.asarray(channel_weights, dtype=np.float64).reshape(-1)]
    if len(w) != C:
        raise ValueError(f"cell_gradient_loss: {len(w)} channel weights for {C} channels")
    sums = _CellSums.apply(pred, target, mask, ops, None if velocity is None else tuple(int(v) for v in velocity))
    total = sums.sum(0)                                 # fp64 [1 + 2C + 4]; the weights enter as host scalars: no upload, capturable
    J = w[0] * total[1]
    for c in range(1, C):
        J = J + w[c] * total[1 + c]
    if velocity is not None:
        J = (J + float(div_weight) * total[1 + 2 * C]) + float(vort_weight) * total[3 + 2 * C]
    return (J / total[0]).float()
