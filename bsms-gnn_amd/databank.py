"""Device-resident trajectory bank: trajectories live in HBM, and a training batch is picked, noised, packed and masked
there by one kernel (csrc/batch.hip: bsms_batch_assemble).  The host contributes a handful of integers per step: which
(trajectory, frame) pairs make the batch, and the (seed, draw) pair of the noise.

What is replaced: the reference's loader loop -- `proc_data` per sample on the host (datasets/base.py:238-289), the
collate, and the upload of node_in / node_tar / node_mask per step (datapipe.TrajectoryDataset -> make_loader ->
trainer.move_to_device here).  Without noise the batches are bit-equal to that route; with noise they follow the same
arithmetic (`state + noise`, `target + (1 - gamma) * noise`, noise zero on masked nodes) with the generator documented
in include/bsms_hip.h instead of torch's CPU generator.

Meshes: with `cfg.consist_mesh` all trajectories share ONE interned hierarchy and `batch` returns the consistent-mesh
tuple with stride-0 [B,...] index views, so the plan cache hits on every step.  Otherwise every trajectory keeps its
graph.MeshBank entry (plans and edge weights resident) and `batch` returns the per-level LevelData list of
`MeshBank.collate`.

Frame augmentation (`Augment`, `TrajectoryBank(augment=)`): one rigid transform per sample -- a rotation,
optionally after a reflection -- applied to the positions and to the vector fields of the state by the same single launch
(bsms_batch_assemble_xf), before the noise.  `transform_rows` (bsms_rows_transform) applies the same matrices to any other
row tensor: later targets, predictions, node_in."""
import ctypes as C
import dataclasses
import math

import numpy as np
import torch

from . import _abi
from .datapipe import SingleTrajReader, load_fields, pack_levels
from .graph import MeshBank, _upload

VALID_TYPES = {"airfoil": (0.0,), "cylinder_flow": (0.0, 5.0)}     # the codes datapipe.MASKS accepts (airfoil.py:23, cylinder_flow.py:24)
_MASK64 = (1 << 64) - 1


class _Sample(C.Structure):      # bsms_batch_sample (include/bsms_hip.h)
    _fields_ = [("state_in", C.c_void_p), ("state_tar", C.c_void_p), ("pos", C.c_void_p), ("type", C.c_void_p), ("n", C.c_int64)]


def epoch_picks(rng, lengths, order="trajectory"):
    """One epoch of (trajectory, frame) picks.  "trajectory" replays datapipe.TrajectoryDataset.__iter__ draw for draw on the
    same `numpy.random.Generator`: the trajectories are shuffled, then the frames within each as it comes up.  "global"
    shuffles all pairs."""
    if order == "trajectory":
        trajs = list(range(len(lengths)))
        rng.shuffle(trajs)
        out = []
        for si in trajs:
            t_ids = np.arange(lengths[si])
            rng.shuffle(t_ids)
            out.extend((si, int(ti)) for ti in t_ids)
        return out
    if order != "global":
        raise ValueError(f"order must be 'trajectory' or 'global', got {order!r}")
    pairs = [(si, ti) for si, n in enumerate(lengths) for ti in range(n)]
    return [pairs[k] for k in rng.permutation(len(pairs))]


def pick_lengths(frames, horizon=1):
    """Frames of each trajectory that may start a pick: frame t needs its targets t+1 .. t+horizon, so T - horizon of T."""
    return [int(T) - int(horizon) for T in frames]


AUGMENT_TAG = 0x58464D54      # third word of the transform generator's seed: keeps its stream apart from every other use of (seed, draw)
MAX_GROUPS = 4                # vector groups per row (csrc/batch.hip: kMaxVec)


@dataclasses.dataclass(frozen=True)
class Augment:
    """Which frames a training batch is seen in.  `rotate`: a rotation by an angle uniform in (-max_angle, max_angle) -- in 3-D about
    a uniformly distributed axis; `reflect`: with probability 1/2 the first coordinate is negated before the rotation (det = -1).
    `vector_fields`: the output fields whose components turn with the frame; every other channel is a scalar."""
    rotate: bool = True
    max_angle: float = math.pi
    reflect: bool = False
    vector_fields: tuple = ("velocity",)

    def __post_init__(self):
        angle = float(self.max_angle)
        if not 0.0 < angle <= math.pi:
            raise ValueError(f"Augment: max_angle must be in (0, pi], got {self.max_angle!r}")
        if isinstance(self.vector_fields, str) or not all(isinstance(n, str) for n in self.vector_fields):
            raise ValueError(f"Augment: vector_fields must be a sequence of field names, got {self.vector_fields!r}")
        object.__setattr__(self, "rotate", bool(self.rotate))
        object.__setattr__(self, "reflect", bool(self.reflect))
        object.__setattr__(self, "max_angle", angle)
        object.__setattr__(self, "vector_fields", tuple(self.vector_fields))

    @classmethod
    def from_cfg(cls, cfg):
        """The datasets config's optional augment_rotate / augment_max_angle / augment_reflect / vector_fields; None when neither
        a rotation nor a reflection is asked for."""
        rotate, reflect = bool(getattr(cfg, "augment_rotate", False)), bool(getattr(cfg, "augment_reflect", False))
        if not (rotate or reflect):
            return None
        return cls(rotate=rotate, max_angle=getattr(cfg, "augment_max_angle", math.pi), reflect=reflect,
                   vector_fields=tuple(getattr(cfg, "vector_fields", ("velocity",))))

    def sample(self, p, n, seed, draw):
        """[n, p, p] fp32: the transforms of the `n` samples of batch `draw`, evaluated in fp64 and rounded once.  Sample k takes
        the k-th four consecutive uniforms of `np.random.default_rng([seed, draw, AUGMENT_TAG])` -- axis height, axis azimuth, angle,
        reflection -- whatever is switched on, so a sample's frame depends on (seed, draw, k) alone."""
        p, n = int(p), int(n)
        if p not in (2, 3):
            raise ValueError(f"Augment.sample: p must be 2 or 3, got {p}")
        u = np.random.default_rng([int(seed) & _MASK64, int(draw) & _MASK64, AUGMENT_TAG]).random((n, 4))
        theta = (2.0 * u[:, 2] - 1.0) * self.max_angle if self.rotate else np.zeros(n)
        c, s = np.cos(theta), np.sin(theta)
        q = np.zeros((n, p, p))
        if p == 2:
            q[:, 0, 0], q[:, 0, 1], q[:, 1, 0], q[:, 1, 1] = c, -s, s, c
        else:
            z, phi = 2.0 * u[:, 0] - 1.0, 2.0 * np.pi * u[:, 1]
            rad = np.sqrt(np.maximum(1.0 - z * z, 0.0))
            k = np.stack([rad * np.cos(phi), rad * np.sin(phi), z], -1)                # unit axis, uniform on the sphere
            cross = np.zeros((n, 3, 3))
            cross[:, 0, 1], cross[:, 0, 2], cross[:, 1, 0] = -k[:, 2], k[:, 1], k[:, 2]
            cross[:, 1, 2], cross[:, 2, 0], cross[:, 2, 1] = -k[:, 0], -k[:, 1], k[:, 0]
            q = c[:, None, None] * np.eye(3) + s[:, None, None] * cross + (1.0 - c)[:, None, None] * (k[:, :, None] * k[:, None, :])
        if self.reflect:
            q[:, :, 0] = np.where((u[:, 3] < 0.5)[:, None], -q[:, :, 0], q[:, :, 0])   # Q = R diag(-1, 1, ..): x -> -x, then R
        return np.ascontiguousarray(q, dtype=np.float32)


def _host_transforms(transforms, n, p=None):
    """`transforms` (tensor or array) as a contiguous host fp32 [n, p, p]."""
    if torch.is_tensor(transforms):
        transforms = transforms.detach().cpu().numpy()
    xf = np.ascontiguousarray(transforms, dtype=np.float32)
    if xf.ndim != 3 or xf.shape[0] != n or xf.shape[1] != xf.shape[2] or (p is not None and xf.shape[1] != p) or xf.shape[1] not in (2, 3):
        raise ValueError(f"transforms must be [{n}, p, p] with p = {p if p is not None else '2 or 3'}, got {tuple(xf.shape)}")
    return xf


def transform_rows(x, rows_per_sample, transforms, groups, inverse=False, out=None):
    """Q v (Q^T v with `inverse`) on every vector group of the rows of `x`, one matrix per sample (bsms_rows_transform; arithmetic and
    rounding order in include/bsms_hip.h).  `x`: device fp32, contiguous, [R,C], [B,N,C] or [F,R,C]; `rows_per_sample`: an int (every
    sample has that many rows) or one row count per sample; `transforms` [n,p,p] (host or device); `groups`: the first channel of
    every group.  A 3-D `x` is B samples of N rows when B * N is the table's row count and N alone is not; otherwise it is F frames
    of R rows cut by the same table.  Rows past the table stay as they are.  `out=x` works in place; None allocates."""
    n = int(transforms.shape[0])
    xf = _host_transforms(transforms, n)
    rows = [int(rows_per_sample)] * n if isinstance(rows_per_sample, (int, np.integer)) else [int(r) for r in rows_per_sample]
    if len(rows) != n:
        raise ValueError(f"transform_rows: {len(rows)} row counts for {n} transforms")
    if not (x.is_cuda and x.dtype == torch.float32 and x.is_contiguous() and x.dim() in (2, 3)):
        raise ValueError("transform_rows: x must be a contiguous fp32 device tensor [R,C], [B,N,C] or [F,R,C]")
    total, width = sum(rows), int(x.shape[-1])
    if x.dim() == 2 or (x.shape[0] * x.shape[1] == total and x.shape[1] != total):
        frames, per_frame = 1, x.numel() // width
    else:
        frames, per_frame = int(x.shape[0]), int(x.shape[1])
    if total > per_frame:
        raise ValueError(f"transform_rows: the samples hold {total} rows, x of shape {tuple(x.shape)} has {per_frame}")
    if out is None:
        out = torch.empty_like(x) if total == per_frame else x.clone()
    elif not (out.is_cuda and out.dtype == torch.float32 and out.is_contiguous() and out.shape == x.shape):
        raise ValueError("transform_rows: out must be a contiguous fp32 device tensor of x's shape")
    first = (C.c_int32 * max(len(groups), 1))(*[int(g) for g in groups])
    table = (C.c_int64 * n)(*rows)
    with torch.cuda.device(x.device):
        _abi.check(_abi.lib().bsms_rows_transform(x.data_ptr(), out.data_ptr(), frames, per_frame, width, C.addressof(table), n, xf.shape[1],
                                                  xf.ctypes.data, 1 if inverse else 0, C.addressof(first), len(groups),
                                                  torch.cuda.current_stream(x.device).cuda_stream), "bsms_rows_transform")
    return out


class Moments:
    """First and second moments of what the normalisers see (the row layout of bsms_moment_sums, include/bsms_hip_stats.h):
    `per_trajectory` fp64 [S, 4C+4] and `total` fp64 [4C+4] = [R | M | SX[C] | ST | QX[C] | QT | SD[C] | QD[C]] -- the rows, the rows
    whose node type counts for the loss, and the sums and sums of squares of the state channels, of the node type and of the deltas
    fl32(state[t+1] - state[t]) over every row.  The accessors below cut `total`; none of them copies or synchronises.  The tensors may
    live on any device (the arithmetic of `normalizer_stats` is plain torch in fp64)."""

    def __init__(self, per_trajectory, total, C, rows_known=None):
        C = int(C)
        if total.dtype != torch.float64 or tuple(total.shape) != (4 * C + 4,):
            raise ValueError(f"Moments: total must be float64 [{4 * C + 4}], got {total.dtype} {tuple(total.shape)}")
        if per_trajectory is not None and (per_trajectory.dtype != torch.float64 or per_trajectory.dim() != 2 or per_trajectory.shape[1] != 4 * C + 4):
            raise ValueError(f"Moments: per_trajectory must be float64 [S, {4 * C + 4}]")
        self.per_trajectory, self.total, self.C = per_trajectory, total, C
        self._rows_known = rows_known        # the host's knowledge of `rows` (an int from the shapes), or None

    rows = property(lambda self: self.total[0])
    masked = property(lambda self: self.total[1])
    sum_state = property(lambda self: self.total[2:2 + self.C])
    sum_type = property(lambda self: self.total[2 + self.C])
    sumsq_state = property(lambda self: self.total[3 + self.C:3 + 2 * self.C])
    sumsq_type = property(lambda self: self.total[3 + 2 * self.C])
    sum_delta = property(lambda self: self.total[4 + 2 * self.C:4 + 3 * self.C])
    sumsq_delta = property(lambda self: self.total[4 + 3 * self.C:4 + 4 * self.C])

    def all_reduce(self, group=None):
        """Sum `total` over the ranks of `group`: ONE fp64 message of 4C+4 numbers, all-reduced in place as step.FusedStep reduces its
        fp64 loss sums (gloo or RCCL).  `per_trajectory` stays this rank's.  A no-op at world size 1.  Returns self."""
        import torch.distributed as dist
        if dist.is_available() and dist.is_initialized() and dist.get_world_size(group) > 1:
            dist.all_reduce(self.total, op=dist.ReduceOp.SUM, group=group)
            if not self._rows_known:         # this rank holds no row: whether any rank does is on the device only
                self._rows_known = None
        return self

    def _no_rows(self):
        if self._rows_known is not None:
            return self._rows_known == 0
        return float(self.total[0]) == 0.0   # host tensors, or a reduced total of a rank without rows: the one read of R

    def normalizer_stats(self, noise_std=None, noise_gamma=0.0):
        """(in_mean [C+1], in_meansq [C+1], out_mean [C], out_meansq [C]), fp64 on the device of `total`: the statistics of the
        network's inputs [state + n | type] and of its normalised targets delta - gamma n under the training noise of
        bsms_batch_assemble -- n ~ N(0, sigma_c^2) on the M rows whose mask is 1, zero elsewhere -- in closed form:
          in_meansq[c] = QX[c] / R + sigma_c^2 (M / R),   out_meansq[c] = QD[c] / R + gamma^2 sigma_c^2 (M / R),   the means SX / R, ST / R, SD / R
        with sigma_c = double(fl32(noise_std[c])), every operand fp64.  `noise_std` None: the data's own moments, no noise term.
        Nothing is read back when the row count is known from the shapes (a `TrajectoryBank.moments()` result).  ValueError without rows."""
        if self._no_rows():
            raise ValueError("Moments.normalizer_stats: no rows")
        t, C = self.total, self.C
        R = t[0]
        in_mean = torch.cat([self.sum_state, self.sum_type.reshape(1)]) / R
        in_meansq = torch.cat([self.sumsq_state, self.sumsq_type.reshape(1)]) / R
        out_mean, out_meansq = self.sum_delta / R, self.sumsq_delta / R
        if noise_std is not None:
            sigma = np.asarray([float(v) for v in noise_std], dtype=np.float32).astype(np.float64)
            if sigma.shape != (C,):
                raise ValueError(f"Moments.normalizer_stats: noise_std has {sigma.size} entries for {C} channels")
            var = torch.from_numpy(sigma * sigma).to(t.device)
            share = self.masked / R
            in_meansq = torch.cat([in_meansq[:C] + var * share, in_meansq[C:]])
            gamma = float(noise_gamma)
            out_meansq = out_meansq + (gamma * gamma) * var * share
        return in_mean, in_meansq, out_mean, out_meansq


def fit_normalizers(model, bank, noise="expected", indices=None, group=None, ignore_augment=False):
    """Set both normalisers of `model` (a BSMS_Simulator on the bank's device) from the exact moments of `bank`:
    `bank.moments(indices)`, summed over the ranks of `group`, through `Moments.normalizer_stats`.  noise="expected": with the bank's
    training noise (cfg.noise_level, cfg.noise_gamma) in closed form -- what the reference's warm-up samples; "none": the data's own
    moments.  The statistics are written IN PLACE (pointers held by sessions, the fused step and captured graphs stay valid):
    _E_data / _E_data_squared by copy_, _acc_weight = rows / unit, _num_accumulations = _max_accumulations (a later accumulate=True
    call changes nothing), synced = True.  Nothing is read back.  A bank with an `augment` is refused unless `ignore_augment`: the
    statistics are those of the data's frame, and rotations change the per-channel moments of vector fields.  Returns the Moments."""
    if noise not in ("expected", "none"):
        raise ValueError(f'fit_normalizers: noise must be "expected" or "none", got {noise!r}')
    if getattr(bank, "augment", None) is not None and not ignore_augment:
        raise ValueError("fit_normalizers: the bank augments its training batches; the statistics would be those of the data's frame "
                         "(pass ignore_augment=True to take them anyway)")
    mom = bank.moments(indices).all_reduce(group)
    if noise == "expected":
        stats = mom.normalizer_stats([float(v) for v in bank.cfg.noise_level], float(bank.cfg.noise_gamma))
    else:
        stats = mom.normalizer_stats()
    with torch.no_grad():
        for norm, mean, meansq in ((model._inputNormalizer, stats[0], stats[1]), (model._targetNormalizer, stats[2], stats[3])):
            if norm._E_data.device != mean.device or tuple(norm._E_data.shape) != tuple(mean.shape):
                raise ValueError(f"fit_normalizers: {norm.name} holds {tuple(norm._E_data.shape)} on {norm._E_data.device}, the statistics are "
                                 f"{tuple(mean.shape)} on {mean.device}")
            norm._E_data.copy_(mean)
            norm._E_data_squared.copy_(meansq)
            norm._acc_weight.copy_((mom.rows / norm.unit).reshape(1))
            norm._num_accumulations.copy_(norm._max_accumulations.reshape(1))
            norm.synced = True
    return mom


class _Traj:
    __slots__ = ("state", "pos", "type", "pos_static", "type_static", "T", "N", "entry", "weights", "cells")


class TrajectoryBank:
    """`cfg`: what datapipe.TrajectoryDataset takes (field_names, output_field_names, consist_mesh, unet_depth, mesh_type,
    noise_level, noise_gamma, and optionally augment_rotate / augment_max_angle / augment_reflect / vector_fields).  `process`: the model's BSGMP, needed for variable meshes only (it builds the per-mesh plans).
    `horizon` = K > 1 serves an unrolled loss over K steps: a pick (trajectory, t) then needs the frames t+1 .. t+K, so the epoch
    order stops K frames before the end, and `batch` also returns the later targets (frames t+2 .. t+K, without noise).
    `augment` (None: `Augment.from_cfg(cfg)`, which is None for a config without the keys): training batches are seen in a
    freshly drawn frame per sample; evaluation batches, `trajectory` and the rollouts stay in the data's frame.
    `node_weights="measure"`: `add` also keeps every trajectory's `hierarchy.lumped_node_measure` resident (float32 [N],
    from its `cells` and its first frame's positions, which must be static) for a node-weighted objective; `node_weights(picks)` and
    `batch(..., return_weights=True)` hand them out.  None: nothing is computed, kept or returned."""

    def __init__(self, cfg, dataset="airfoil", device=None, seed=0, process=None, max_bytes=None, order="trajectory", cache_dir=None,
                 horizon=1, augment=None, node_weights=None):
        if node_weights not in (None, "measure"):
            raise ValueError(f'TrajectoryBank: node_weights must be None or "measure", got {node_weights!r}')
        self._weights_kind = node_weights
        if dataset not in VALID_TYPES:
            raise ValueError(f"dataset must be one of {sorted(VALID_TYPES)}, got {dataset!r}")
        if order not in ("trajectory", "global"):
            raise ValueError(f"order must be 'trajectory' or 'global', got {order!r}")
        if int(horizon) < 1:
            raise ValueError(f"horizon must be >= 1, got {horizon}")
        self.cfg, self.dataset, self.order, self.cache_dir, self.horizon = cfg, dataset, order, cache_dir, int(horizon)
        self.augment = Augment.from_cfg(cfg) if augment is None else augment
        if not (self.augment is None or isinstance(self.augment, Augment)):
            raise ValueError(f"TrajectoryBank: augment must be an Augment or None, got {type(augment).__name__}")
        # vector groups: the bank's own Augment names them; without one an explicit `transforms=` goes by the config (or "velocity")
        self._vector_fields = self.augment.vector_fields if self.augment is not None else tuple(getattr(cfg, "vector_fields", ("velocity",)))
        self.fields, self._groups, self._group_error = None, None, None      # set by the first `add`
        if self.augment is not None:
            self._check_vector_names()
        self.device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        if self.device.type != "cuda":
            raise _abi.BsmsError("TrajectoryBank needs a GPU device: trajectories are resident in HBM")
        self.max_bytes, self.bytes_resident = max_bytes, 0
        self._valid = (C.c_float * len(VALID_TYPES[dataset]))(*VALID_TYPES[dataset])
        self._std = (C.c_float * len(cfg.noise_level))(*[float(v) for v in cfg.noise_level])
        self._trajs = []
        self._hier = None            # consistent mesh: (m_gs, m_ids) device tensors, shared by every trajectory
        self._views = {}             # ... and their stride-0 [B,...] views per batch size
        self._meshes = None if cfg.consist_mesh else MeshBank(process, self.device)
        if self._meshes is not None and process is None:
            raise ValueError("TrajectoryBank: variable meshes (cfg.consist_mesh = False) need process=model.process")
        self._reseed(seed)

    def _reseed(self, seed):
        self.seed = int(seed) & _MASK64
        self._rng = np.random.default_rng(self.seed)
        self._epoch, self._cursor, self._draw = [], 0, 0

    def __len__(self):
        return len(self._trajs)

    @property
    def lengths(self):
        """Frames with all their targets per trajectory (T - horizon; T - 1 for the single-step loss)."""
        return pick_lengths([tr.T for tr in self._trajs], self.horizon)

    # ------------------------------------------------------------------------------------------------ filling
    def _claim(self, nbytes):
        if self.max_bytes is not None and self.bytes_resident + nbytes > self.max_bytes:
            raise _abi.BsmsError(f"TrajectoryBank: {self.bytes_resident + nbytes} bytes would be resident, max_bytes is {self.max_bytes}")
        self.bytes_resident += nbytes

    def _put(self, t):
        t = t.contiguous()
        self._claim(t.numel() * t.element_size())
        return _upload(t, self.device)

    def _check_vector_names(self):
        names = list(self._vector_fields)
        for name in names:
            if name not in self.cfg.output_field_names:
                raise ValueError(f"vector field {name!r} is not one of cfg.output_field_names {list(self.cfg.output_field_names)}")
        if len(set(names)) != len(names) or len(names) > MAX_GROUPS:
            raise ValueError(f"vector_fields must be at most {MAX_GROUPS} different names, got {names}")

    def _record_fields(self, fields, p):
        """Channel offset and width of every output field; the named vector fields become the groups of the transform."""
        layout, off = {}, 0
        for k in self.cfg.output_field_names:
            layout[k] = (off, int(fields[k].shape[-1]))
            off += layout[k][1]
        if self.fields is None:
            self.fields = layout
            try:
                self._check_vector_names()
                for name in self._vector_fields:
                    if layout[name][1] != p:
                        raise ValueError(f"vector field {name!r} has {layout[name][1]} components, the positions have {p}")
                first = [layout[name][0] for name in self._vector_fields]
                self._groups = (tuple(first), (C.c_int32 * max(len(first), 1))(*first))
            except ValueError as e:
                if self.augment is not None:
                    self.fields = None
                    raise
                self._group_error = str(e)          # no augmentation asked for: only an explicit `transforms=` would need the groups
        elif layout != self.fields and self.augment is not None:
            raise ValueError(f"TrajectoryBank.add: output fields laid out as {layout}, the bank holds {self.fields}")

    @property
    def vector_groups(self):
        """First channel of every vector group of the state (what `transform_rows` takes as `groups`)."""
        if self._group_error is not None:
            raise ValueError(self._group_error)
        return () if self._groups is None else self._groups[0]

    def add(self, source):
        """Upload ONE trajectory (a path or a dict, read through datapipe.load_fields).  Returns its index."""
        cfg = self.cfg
        reader = None
        if self._hier is None:       # variable meshes, or the first trajectory of a consistent mesh: build / load the hierarchy
            reader = SingleTrajReader(cfg, source, "train", self.cache_dir)
            fields = reader.fields
        else:
            fields = load_fields(source, cfg.field_names)
        state = torch.cat([fields[k] for k in cfg.output_field_names], dim=-1)
        pos, typ = fields["mesh_pos"], fields["node_type"]
        tr = _Traj()
        tr.T, tr.N = int(state.shape[0]), int(state.shape[1])
        if tr.T < 2:
            raise ValueError("TrajectoryBank.add: a trajectory needs at least two frames")
        if tr.T < self.horizon + 1:
            raise ValueError(f"TrajectoryBank.add: horizon = {self.horizon} needs at least {self.horizon + 1} frames, this trajectory has {tr.T}")
        if state.shape[-1] != len(cfg.noise_level):
            raise ValueError(f"TrajectoryBank.add: {state.shape[-1]} state channels, cfg.noise_level has {len(cfg.noise_level)}")
        if typ.shape[-1] != 1:
            raise ValueError(f"TrajectoryBank.add: node_type must be [T,N,1], got {tuple(typ.shape)}")
        self._record_fields(fields, int(pos.shape[-1]))
        tr.pos_static, tr.type_static = bool((pos == pos[:1]).all()), bool((typ == typ[:1]).all())
        measure = None
        if self._weights_kind == "measure":           # refused before anything of this trajectory is uploaded or claimed
            if fields.get("cells") is None:
                raise ValueError('TrajectoryBank.add: node_weights="measure" needs the trajectory\'s "cells" (cfg.field_names)')
            if not tr.pos_static:
                raise ValueError('TrajectoryBank.add: node_weights="measure" needs static positions: one measure per trajectory')
            from .hierarchy import lumped_node_measure
            cells = np.asarray(fields["cells"])
            measure = torch.from_numpy(lumped_node_measure(pos[0].numpy(), cells[0] if cells.ndim == 3 else cells, cfg.mesh_type))
        tr.entry = None
        if cfg.consist_mesh:
            if self._hier is None:
                self._hier = ([self._put(g) for g in reader.m_gs], [self._put(i) for i in reader.m_ids], tr.N)
            elif tr.N != self._hier[2]:
                raise ValueError(f"TrajectoryBank.add: consistent mesh of {self._hier[2]} nodes, this trajectory has {tr.N}")
        else:
            before = len(self._meshes._by_content)
            tr.entry = self._meshes.entry(pack_levels(state[0], None, None, reader.m_gs, reader.m_ids))
            if len(self._meshes._by_content) > before:
                self._claim(sum(t.numel() * t.element_size() for pair in tr.entry["keep"] for t in pair if t is not None))
        tr.state = self._put(state)
        tr.pos = self._put(pos[0] if tr.pos_static else pos)
        tr.type = self._put(typ[0] if tr.type_static else typ)
        tr.weights = None if measure is None else self._put(measure)
        cells = fields.get("cells")                   # host: what `sampler` triangulates (nothing is uploaded for it).  An OWNED int32 copy
        if cells is not None:                         # of frame 0 -- a view would keep the [T, n_cells, k] array of `fields` alive
            cells = np.asarray(cells)
            cells = np.array(cells[0] if cells.ndim == 3 else cells, dtype=np.int32, copy=True)
        tr.cells = cells
        self._trajs.append(tr)
        return len(self._trajs) - 1

    def add_sharded(self, sources, group=None):
        """Data parallelism: rank r uploads its `rollout.rank_slice` of `sources` and mixes its rank into the seed, so the
        ranks draw different orders and different noise.  Returns the indices added on this rank."""
        import torch.distributed as dist
        from .rollout import rank_slice
        sources = list(sources)
        lo, hi = rank_slice(len(sources), group)
        rank = dist.get_rank(group) if dist.is_available() and dist.is_initialized() else 0
        if rank:
            self._reseed((self.seed + 0x9E3779B97F4A7C15 * rank) & _MASK64)
        return [self.add(s) for s in sources[lo:hi]]

    # ------------------------------------------------------------------------------------------------ batches
    def _assemble(self, picks, noisy, draw, return_noise, horizon=1, xf=None):
        """`xf`: host fp32 [len(picks), p, p] or None.  None makes exactly the calls of a bank without augmentation."""
        cfg = self.cfg
        n_c, table = len(self._std), (_Sample * len(picks))()
        p, rows = None, 0
        for k, (si, ti) in enumerate(picks):
            tr = self._trajs[si]
            if not 0 <= ti < tr.T - horizon:
                raise IndexError(f"frame {ti} of trajectory {si}: it has {tr.T - horizon} frames with " +
                                 ("a target" if horizon == 1 else f"{horizon} targets"))
            frame = tr.N * 4
            s = table[k]
            s.state_in = tr.state.data_ptr() + ti * frame * n_c
            s.state_tar = tr.state.data_ptr() + (ti + 1) * frame * n_c
            s.pos = tr.pos.data_ptr() + (0 if tr.pos_static else ti * frame * tr.pos.shape[-1])
            s.type = tr.type.data_ptr() + (0 if tr.type_static else ti * frame)
            s.n = tr.N
            rows += tr.N
            if p is None:
                p = int(tr.pos.shape[-1])
            elif p != tr.pos.shape[-1]:
                raise ValueError("TrajectoryBank: trajectories with different position widths in one batch")
        new = lambda w: torch.empty(rows, w, device=self.device, dtype=torch.float32)
        node_in, node_tar, node_mask = new(n_c + p + 1), new(n_c), new(1)
        noise = new(n_c) if return_noise else None
        later = torch.empty(horizon - 1, rows, n_c, device=self.device, dtype=torch.float32) if horizon > 1 else None
        if xf is not None:
            groups, first = self.vector_groups, self._groups[1]
            if xf.shape != (len(picks), p, p):
                raise ValueError(f"TrajectoryBank: transforms must be [{len(picks)}, {p}, {p}], got {tuple(xf.shape)}")
        with torch.cuda.device(self.device):
            stream = torch.cuda.current_stream(self.device).cuda_stream
            if later is not None:
                _abi.check(_abi.lib().bsms_batch_targets(C.addressof(table), len(picks), n_c, horizon - 1, later.data_ptr(),
                                                         torch.cuda.current_stream(self.device).cuda_stream), "bsms_batch_targets")
                if xf is not None:                  # the later targets in the frame of their sample: in place, same matrices
                    seg = (C.c_int64 * len(picks))(*[table[k].n for k in range(len(picks))])
                    _abi.check(_abi.lib().bsms_rows_transform(later.data_ptr(), later.data_ptr(), horizon - 1, rows, n_c, C.addressof(seg),
                                                              len(picks), p, xf.ctypes.data, 0, C.addressof(first), len(groups), stream),
                               "bsms_rows_transform")
            if xf is not None:
                _abi.check(_abi.lib().bsms_batch_assemble_xf(
                    C.addressof(table), len(picks), n_c, p, xf.ctypes.data, C.addressof(first), len(groups),
                    C.addressof(self._std) if noisy else None, float(cfg.noise_gamma), C.addressof(self._valid), len(self._valid), self.seed,
                    int(draw) & _MASK64, node_in.data_ptr(), node_tar.data_ptr(), node_mask.data_ptr(),
                    None if noise is None else noise.data_ptr(), stream), "bsms_batch_assemble_xf")
                return node_in, node_tar, node_mask, noise, later
            _abi.check(_abi.lib().bsms_batch_assemble(
                C.addressof(table), len(picks), n_c, p, C.addressof(self._std) if noisy else None, float(cfg.noise_gamma),
                C.addressof(self._valid), len(self._valid), self.seed, int(draw) & _MASK64, node_in.data_ptr(), node_tar.data_ptr(),
                node_mask.data_ptr(), None if noise is None else noise.data_ptr(), torch.cuda.current_stream(self.device).cuda_stream),
                "bsms_batch_assemble")
        return node_in, node_tar, node_mask, noise, later

    def _hier_views(self, B):
        v = self._views.get(B)
        if v is None:
            m_gs, m_ids, _ = self._hier
            v = self._views[B] = ([g.unsqueeze(0).expand(B, *g.shape) for g in m_gs], [i.unsqueeze(0).expand(B, *i.shape) for i in m_ids])
        return v

    def node_weights(self, picks):
        """The node weights of the samples of `picks` as the step takes them: [B, N] on a consistent mesh, the flat concatenation
        [rows] for variable meshes (a copy; the resident vectors are per trajectory)."""
        if self._weights_kind is None:
            raise ValueError('TrajectoryBank.node_weights: the bank was built without node_weights="measure"')
        picks = list(picks)
        if not picks:
            raise ValueError("TrajectoryBank.node_weights: no picks")
        w = [self._trajs[int(si)].weights for si, _ in picks]
        return torch.stack(w) if self.cfg.consist_mesh else torch.cat(w)

    def sampler(self, i):
        """A `sample.MeshSampler` on the mesh of trajectory `i`: its stored `cells` and its frame-0 positions.  Built
        on every call (the sampler caches its owner images: keep it)."""
        tr = self._trajs[int(i)]
        if tr.cells is None:
            raise ValueError('TrajectoryBank.sampler: needs the trajectory\'s "cells" (cfg.field_names)')
        from .sample import MeshSampler
        return MeshSampler(tr.pos if tr.pos_static else tr.pos[0], tr.cells, self.cfg.mesh_type, device=self.device)

    def gradient_ops(self, i):
        """A `diffop.MeshGradient` on the mesh of trajectory `i`, the twin of `sampler`: its stored `cells` and its
        frame-0 positions.  Built on every call (the incidence is built on the host: keep it)."""
        tr = self._trajs[int(i)]
        if tr.cells is None:
            raise ValueError('TrajectoryBank.gradient_ops: needs the trajectory\'s "cells" (cfg.field_names)')
        from .diffop import MeshGradient
        return MeshGradient(tr.pos if tr.pos_static else tr.pos[0], tr.cells, self.cfg.mesh_type, device=self.device)

    def batch(self, picks, train=True, draw=None, return_noise=False, horizon=None, transforms=None, return_transforms=False,
              return_weights=False):
        """The device batch of `picks`, a list of (trajectory, frame).  `train`: inject the training noise; `draw` selects the
        noise of this batch (None: the bank's running batch counter, which then advances).  Consistent mesh:
        [node_in [B,N,C+p+1], node_tar [B,N,C], node_mask [B,N,1], m_gs, m_ids]; variable meshes: the per-level LevelData list.
        `return_noise` appends the noise tensor that was added ([B,N,C] / [rows,C]; zeros when `train` is false).
        `horizon` (None: the bank's) = K > 1 returns (batch, later) -- or (batch, later, noise) -- with the targets of the steps after
        the first, later [K-1,B,N,C] / [K-1,rows,C] = frames t+2 .. t+K as they are resident: the noise (and its `gamma` correction
        of node_tar) belongs to the first step alone, whose tensors are bit-equal to those of horizon = 1 for the same draw.
        Frames: a bank with an `augment` sees a `train` batch through `augment.sample(p, B, seed, draw)`, one matrix per pick,
        applied before the noise to positions and vector fields, and to the later targets; `train=False` stays in the data's frame.
        `transforms` [B,p,p] (tensor or array) is applied instead, whatever `train` says and with or without an `augment`.
        `return_transforms` appends the host fp32 array that was applied (None when the batch is in the data's frame).
        `return_weights` appends `node_weights(picks)` last (a bank with node_weights="measure" only)."""
        if return_weights and self._weights_kind is None:
            raise ValueError('TrajectoryBank.batch: return_weights needs a bank built with node_weights="measure"')
        horizon = self.horizon if horizon is None else int(horizon)
        if horizon < 1:
            raise ValueError(f"horizon must be >= 1, got {horizon}")
        picks = [(int(si), int(ti)) for si, ti in picks]
        if not picks:
            raise ValueError("TrajectoryBank.batch: no picks")
        if draw is None:
            draw, self._draw = self._draw, self._draw + 1
        xf = None
        if transforms is not None:
            xf = _host_transforms(transforms, len(picks))
        elif self.augment is not None and train:
            xf = self.augment.sample(self._trajs[picks[0][0]].pos.shape[-1], len(picks), self.seed, draw)
        node_in, node_tar, node_mask, noise, later = self._assemble(picks, bool(train), draw, return_noise, horizon, xf)
        if self.cfg.consist_mesh:
            B, N = len(picks), self._hier[2]
            m_gs, m_ids = self._hier_views(B)
            out = [node_in.view(B, N, -1), node_tar.view(B, N, -1), node_mask.view(B, N, 1), m_gs, m_ids]
            noise = None if noise is None else noise.view(B, N, -1)
            later = None if later is None else later.view(horizon - 1, B, N, -1)
        else:
            out = self._meshes.assemble([self._trajs[si].entry for si, _ in picks], node_in, node_tar, node_mask)
        extra = ([later] if later is not None else []) + ([noise] if return_noise else []) + ([xf] if return_transforms else [])
        if return_weights:
            extra.append(self.node_weights(picks))
        return (out, *extra) if extra else out

    def next_picks(self, B):
        """The next `B` picks of the epoch order (fewer at the end of an epoch, like a loader without drop_last)."""
        if self._cursor >= len(self._epoch):
            if not self._trajs:
                raise ValueError("TrajectoryBank: no trajectory has been added")
            self._epoch, self._cursor = epoch_picks(self._rng, self.lengths, self.order), 0
        picks = self._epoch[self._cursor:self._cursor + int(B)]
        self._cursor += len(picks)
        return picks

    def sample(self, B, train=True, return_noise=False):
        """`batch` of the next `B` picks of the epoch order; the noise draw counts the batches."""
        return self.batch(self.next_picks(B), train=train, return_noise=return_noise)

    # ------------------------------------------------------------------------------------------------ statistics
    def moments(self, indices=None):
        """The `Moments` of the chosen trajectories (None: all, in order) over EVERY pair of frames (t, t+1) they hold, whatever
        `horizon` is: one bsms_moment_sums pass over the resident state and node type plus its fold, on the current stream.  Row k
        of `per_trajectory` belongs to indices[k] and depends on that trajectory alone.  In the data's frame, without noise."""
        from .ops import moment_fold, moment_sums
        chosen = list(range(len(self._trajs))) if indices is None else [int(i) for i in indices]
        table = []
        for i in chosen:
            tr = self._trajs[i]               # IndexError for a trajectory the bank does not hold
            table.append((tr.state, tr.type, 0, tr.T - 1))
        C_ = len(self._std)
        with torch.cuda.device(self.device):
            per = moment_sums(table, C_, list(self._valid), out=torch.empty(len(table), 4 * C_ + 4, device=self.device, dtype=torch.float64))
            total = moment_fold(per)
        return Moments(per, total, C_, rows_known=sum((self._trajs[i].T - 1) * self._trajs[i].N for i in chosen))

    # ------------------------------------------------------------------------------------------------ rollout
    def hierarchy(self, i):
        """(m_gs, m_ids) of trajectory `i` as device tensors ([2,E_l] / [N_{l+1}])."""
        if self.cfg.consist_mesh:
            return list(self._hier[0]), list(self._hier[1])
        keep = self._trajs[i].entry["keep"]
        return [g for g, _ in keep], [f for _, f in keep[:len(keep) - 1]]

    def resident(self, i):
        """The resident tensors of trajectory `i` themselves, not copies: (state [T,N,C], node_type [N,1] if it is static else
        [T,N,1]).  rollout.rollout_bank reads its targets from `state[1:]` in place."""
        tr = self._trajs[i]
        return tr.state, tr.type

    def trajectory(self, i):
        """What datapipe.TrajectoryDataset(mode="rollout") yields for trajectory `i`, on the device and without noise:
        (node_in [T-1,N,C+p+1], node_tar [T-1,N,C], node_mask [T-1,N,1], m_gs, m_ids)."""
        tr = self._trajs[i]
        node_in, node_tar, node_mask, _, _ = self._assemble([(i, t) for t in range(tr.T - 1)], False, 0, False)
        m_gs, m_ids = self.hierarchy(i)
        return node_in.view(tr.T - 1, tr.N, -1), node_tar.view(tr.T - 1, tr.N, -1), node_mask.view(tr.T - 1, tr.N, 1), m_gs, m_ids

    def rollouts(self, indices=None):
        """Iterable of rollout batches for rollout.rollout_dataset: `trajectory(i)` with the loader's batch axis of 1."""
        for i in (range(len(self._trajs)) if indices is None else indices):
            inp, tar, mask, m_gs, m_ids = self.trajectory(i)
            yield inp.unsqueeze(0), tar.unsqueeze(0), mask.unsqueeze(0), [g.unsqueeze(0) for g in m_gs], [f.unsqueeze(0) for f in m_ids]
