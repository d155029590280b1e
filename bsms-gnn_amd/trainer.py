"""Training harness around the hot path, mirroring the reference's `Trainer` (src/trainer/trainer.py) and
LR schedule (src/utils/basic.py:168-184): masked-RMSE loss, backward, global-norm clip, AdamW, warm-up +
cosine decay, save / restore.  The optimizer step is ONE fused HIP launch pair over the flat parameter and
gradient buffers (bsms_adamw_step) instead of ~180 small tensor updates; under data parallelism the gradients
are all-reduced (dp.py) before it, so every rank applies the identical update."""
import math
import os

import torch

from . import _abi
from .dp import DataParallel
from .ops import bump_param_epoch


class WarmupCosineDecay:
    """utils/basic.py:168-184: factor = epoch/warmup up to `warmup`, then 0.5 (1 + cos(pi * progress)).
    Like torch's _LRScheduler the first optimizer step sees epoch 0 (factor 0)."""

    def __init__(self, base_lr, warmup, max_iters):
        self.base_lr, self.warmup, self.max_iters, self.last_epoch = base_lr, warmup, max_iters, 0

    def factor(self, epoch=None):
        epoch = self.last_epoch if epoch is None else epoch
        if epoch <= self.warmup:
            return epoch * 1.0 / self.warmup
        return 0.5 * (1 + math.cos(math.pi * (epoch - self.warmup) / (self.max_iters - self.warmup)))

    def lr(self):
        return self.base_lr * self.factor()

    def step(self):
        self.last_epoch += 1


def param_groups(model, no_decay_bias=False, lr_scales=None):
    """Parameter groups for FusedAdamW / Trainer in torch's shape, `[{"params": [...], "lr_scale": s, "weight_decay": wd}, ...]`
    (a key that is left out takes the optimizer's default).  `no_decay_bias`: every trainable 1-D tensor (biases, LayerNorm
    weights) gets weight_decay 0.  `lr_scales`: {prefix of named_parameters(): factor on the learning rate}, e.g.
    {"process": 0.1, "process.bottom_gmp": 0.5}; a prefix ends at a dot or at the end of the name, the longest matching prefix
    wins, a prefix that matches no trainable parameter raises ValueError.  Parameters no rule touches are not listed: they form
    the optimizer's default group."""
    lr_scales = dict(lr_scales or {})
    for k, f in lr_scales.items():
        if not (math.isfinite(float(f)) and float(f) >= 0.0):
            raise ValueError(f"param_groups: lr_scales[{k!r}] = {f!r} is not a finite non-negative factor")
    hit, by_key = set(), {}
    for name, p in model.named_parameters():
        if not p.requires_grad:
            continue
        best = None
        for prefix in lr_scales:
            if (name == prefix or name.startswith(prefix + ".")) and (best is None or len(prefix) > len(best)):
                best = prefix
        if best is not None:
            hit.add(best)
        scale = float(lr_scales[best]) if best is not None else None
        no_decay = bool(no_decay_bias) and p.dim() == 1
        if scale is None and not no_decay:
            continue
        by_key.setdefault((scale, no_decay), []).append(p)
    missing = sorted(set(lr_scales) - hit)
    if missing:
        raise ValueError(f"param_groups: lr_scales prefix {missing[0]!r} matches no trainable parameter")
    out = []
    for (scale, no_decay), plist in by_key.items():
        g = {"params": plist}
        if scale is not None:
            g["lr_scale"] = scale
        if no_decay:
            g["weight_decay"] = 0.0
        out.append(g)
    return out


def segment_table(grads, groups, weight_decay):
    """The groups of a FusedAdamW as segments of the flat buffer of `grads` (a GradBuckets): a list of (offset, count, lr_scale,
    weight_decay), sorted, tiling [0, n) exactly, neighbours with equal hyper-parameters merged.  Parameters no group lists take
    (1.0, `weight_decay`).  ValueError for a parameter listed twice or one without a slot in `grads` (frozen, or foreign)."""
    hyper = {}
    for gi, g in enumerate(groups):
        unknown = set(g) - {"params", "lr_scale", "weight_decay"}
        if unknown:
            raise ValueError(f"FusedAdamW: group {gi}: unknown key {sorted(unknown)[0]!r} (per-group betas / eps are not supported)")
        scale, wd = float(g.get("lr_scale", 1.0)), float(g.get("weight_decay", weight_decay))
        if not (math.isfinite(scale) and scale >= 0.0 and math.isfinite(wd) and wd >= 0.0):
            raise ValueError(f"FusedAdamW: group {gi}: lr_scale = {scale}, weight_decay = {wd} must be finite and >= 0")
        for p in g["params"]:
            if p not in grads._slot:
                raise ValueError(f"FusedAdamW: group {gi} lists a parameter without a gradient slot (frozen, or not of this model)")
            if p in hyper:
                raise ValueError(f"FusedAdamW: group {gi} lists a parameter that an earlier group (or this one) lists already")
            hyper[p] = (scale, wd)
    segs = []
    for p in sorted(grads.params, key=lambda q: grads._slot[q][0]):
        off, n = grads._slot[p]
        if n == 0:
            continue
        scale, wd = hyper.get(p, (1.0, float(weight_decay)))
        if segs and segs[-1][0] + segs[-1][1] == off and segs[-1][2:] == (scale, wd):
            segs[-1] = (segs[-1][0], segs[-1][1] + n, scale, wd)
        else:
            segs.append((off, n, scale, wd))
    return segs


class _OptimGroups:
    """Owner of a bsms_optim_groups_t handle (the device copy of a segment table)."""

    def __init__(self, segments, n):
        import ctypes as C
        table = (_abi.OptimGroup * len(segments))(*[_abi.OptimGroup(o, c, s, w) for o, c, s, w in segments])
        h = C.c_void_p()
        _abi.check(_abi.lib().bsms_optim_groups_create(C.cast(table, C.c_void_p), len(segments), int(n), C.cast(C.byref(h), _abi.PP)),
                   "bsms_optim_groups_create")
        self.handle = h

    def __del__(self):
        h, self.handle = getattr(self, "handle", None), None
        if h:
            try:
                _abi.lib().bsms_optim_groups_destroy(h)
            except Exception:  # noqa: BLE001  (interpreter shutdown)
                pass


class FusedAdamW:
    """AdamW over the flat buffers of a GradBuckets (dp.py).  Parameters are re-pointed into one flat fp32
    array with the gradient buffer's layout, so clip + update are two kernel launches for the whole model.

    Optional (with none of them set the object holds no extra state and `step` calls bsms_adamw_step as ever):
    `groups` -- torch-style parameter groups with `lr_scale` / `weight_decay` (see `param_groups`); `ema_decay` > 0 -- a flat
    `ema` buffer with the layout of `flat_p`, updated in the same pass (`ema_warmup`: the decay of call t is
    min(ema_decay, (1 + t) / (10 + t))); `skip_nonfinite` -- a step whose gradient norm is inf / NaN writes nothing and is
    counted in a device counter instead (`applied_steps()` / `skipped_steps()`; the bias corrections then follow the applied steps)."""

    def __init__(self, grads, lr=1e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, max_grad_norm=0.0, groups=None,
                 ema_decay=0.0, ema_warmup=True, skip_nonfinite=False):
        self.grads, self.lr, self.betas, self.eps, self.wd, self.max_norm = grads, lr, betas, eps, weight_decay, max_grad_norm
        ema_decay = float(ema_decay or 0.0)
        if not 0.0 <= ema_decay <= 1.0:
            raise ValueError(f"FusedAdamW: ema_decay = {ema_decay} outside [0, 1]")
        segments = segment_table(grads, groups, weight_decay) if groups is not None else None     # raises before anything is re-pointed
        flat = torch.empty_like(grads.flat)
        for p in grads.params:
            off, n = grads._slot[p]
            flat[off:off + n].copy_(p.data.reshape(-1))
            p.data = flat[off:off + n].view_as(p)
        self.flat_p = flat
        self.exp_avg = torch.zeros_like(flat)
        self.exp_avg_sq = torch.zeros_like(flat)
        self.step_count = 0
        self.grad_norm = torch.zeros(1, device=flat.device, dtype=torch.float32)
        self._work = torch.empty(max(int(_abi.lib().bsms_adamw_work_bytes()), 4), dtype=torch.uint8, device=flat.device)
        self.ema_decay, self.ema_warmup = ema_decay, bool(ema_warmup)
        self.segments, self._groups, self.ema, self.counters = segments, None, None, None
        if segments:
            self._groups = _OptimGroups(segments, flat.numel())
        if ema_decay > 0.0:
            self.ema = flat.clone()
        if skip_nonfinite:
            self.counters = torch.zeros(2, dtype=torch.int64, device=flat.device)
        if self.extended:
            self._work = torch.empty(max(int(_abi.lib().bsms_optim_work_bytes()), 4), dtype=torch.uint8, device=flat.device)

    @property
    def extended(self):
        """Whether `step` goes through bsms_optim_step (any of groups / EMA / guard is in use)."""
        return self._groups is not None or self.ema is not None or self.counters is not None

    def ema_decay_at(self, t):
        """The EMA decay of the step() call after `t` earlier ones (evaluated on the host, handed over as a scalar)."""
        return min(self.ema_decay, (1.0 + t) / (10.0 + t)) if self.ema_warmup else self.ema_decay

    def step(self, lr=None):
        self.step_count += 1
        b1, b2 = self.betas
        if not self.extended:
            _abi.check(_abi.lib().bsms_adamw_step(
                self.flat_p.data_ptr(), self.grads.flat.data_ptr(), self.exp_avg.data_ptr(), self.exp_avg_sq.data_ptr(),
                self.flat_p.numel(), float(self.lr if lr is None else lr), b1, b2, self.eps, self.wd, self.step_count,
                float(self.max_norm), self.grad_norm.data_ptr(), self._work.data_ptr(), torch.cuda.current_stream().cuda_stream),
                "bsms_adamw_step")
        else:
            guard = self.counters is not None
            _abi.check(_abi.lib().bsms_optim_step(
                self.flat_p.data_ptr(), self.grads.flat.data_ptr(), self.exp_avg.data_ptr(), self.exp_avg_sq.data_ptr(),
                self.flat_p.numel(), None if self._groups is None else self._groups.handle,
                float(self.lr if lr is None else lr), b1, b2, self.eps, self.wd, 0 if guard else self.step_count, float(self.max_norm),
                None if self.ema is None else self.ema.data_ptr(), self.ema_decay_at(self.step_count - 1) if self.ema is not None else 0.0,
                self.counters.data_ptr() if guard else None, self.grad_norm.data_ptr(), self._work.data_ptr(),
                torch.cuda.current_stream().cuda_stream), "bsms_optim_step")
        bump_param_epoch()           # raw-pointer update: invalidates weight packs cached by ops.InferenceSession

    def applied_steps(self):
        """Steps that changed the parameters (synchronises: reads the device counter back)."""
        return int(self.counters[0]) if self.counters is not None else self.step_count

    def skipped_steps(self):
        """Steps skipped by the non-finite guard (synchronises)."""
        return int(self.counters[1]) if self.counters is not None else 0

    def ema_model(self, model):
        """A structural copy of `model` whose trainable parameters are views into `ema`; everything else -- frozen parameters and
        the normalisers' statistics (Parameter objects that do not require grad) and buffers -- is SHARED with `model`, object for
        object, so it follows the live model (the normalisers re-assign `.data` while they accumulate).  No copy is made and
        none is needed later: the views see every `step`."""
        import copy
        if self.ema is None:
            raise ValueError("FusedAdamW.ema_model: no EMA is kept (ema_decay = 0)")
        memo = {}
        for p in model.parameters():
            if p in self.grads._slot:
                off, n = self.grads._slot[p]
                memo[id(p)] = torch.nn.Parameter(self.ema[off:off + n].view_as(p), requires_grad=False)
            else:
                memo[id(p)] = p
        for b in model.buffers():
            memo[id(b)] = b
        return copy.deepcopy(model, memo)

    def state_dict(self):
        sd = {"exp_avg": self.exp_avg, "exp_avg_sq": self.exp_avg_sq, "step": self.step_count}
        if self.ema is not None:
            sd["ema"] = self.ema
        if self.counters is not None:
            sd["counters"] = self.counters
        return sd

    def load_state_dict(self, sd):
        """The parameters themselves travel with the model: load them first -- a state without `ema` starts the average from them."""
        self.exp_avg.copy_(sd["exp_avg"])
        self.exp_avg_sq.copy_(sd["exp_avg_sq"])
        self.step_count = int(sd["step"])
        if self.ema is not None:
            self.ema.copy_(sd["ema"] if "ema" in sd else self.flat_p)
        if self.counters is not None:
            if "counters" in sd:
                self.counters.copy_(sd["counters"])
            else:
                self.counters.copy_(torch.tensor([self.step_count, 0], dtype=torch.int64))


def usable_cpus():
    """CPUs this process may really use: affinity mask capped by the cgroup CPU quota."""
    n = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    try:
        quota, period = open("/sys/fs/cgroup/cpu.max").read().split()
        if quota != "max":
            n = min(n, max(1, int(int(quota) / int(period))))
    except (OSError, ValueError):
        pass
    return n


def _check_host_threads():
    """PyTorch defaults to one intra-op thread per LOGICAL cpu; under a cgroup CPU quota (containers) the bursts of a few
    CPU tensor copies per step then exhaust the quota and the scheduler parks the whole process for the rest of the
    period -- 80 ms stalls on arbitrary lines of the training loop (profiles/fresh_mesh.py).  Warn once."""
    import warnings
    n = usable_cpus()
    if torch.get_num_threads() > 2 * n:
        warnings.warn(f"torch uses {torch.get_num_threads()} intra-op threads but this process may use ~{n} CPUs (cgroup quota / "
                      f"affinity): call torch.set_num_threads({max(1, min(n, 8))}) to avoid CFS throttling stalls in the training loop",
                      RuntimeWarning, stacklevel=3)


class DevicePrefetcher:
    """`for batch in DevicePrefetcher(loader, trainer): trainer.iter(batch)` -- a background thread takes the host batches of
    `loader` one ahead of the training thread: uploads (pinned, on the copy stream), interning of the index tensors, and
    -- what matters for variable meshes, where every batch is a new block-diagonal graph -- the plans (host CSR builds)
    and the edge-weight chain of the batch.  The training thread then only enqueues the step.  The reference has no
    counterpart (its DataLoader hands CPU batches to `move_to_device`, trainer/trainer.py:143); results are identical to
    feeding `trainer.iter` directly."""

    _END = object()

    def __init__(self, loader, trainer, depth=2):
        self.loader, self.trainer, self.depth = loader, trainer, max(int(depth), 1)

    def __iter__(self):
        import queue
        import threading
        q = queue.Queue(maxsize=self.depth)
        stop = threading.Event()

        def put(item):                 # bounded put that gives up when the consumer has gone away
            while not stop.is_set():
                try:
                    q.put(item, timeout=0.05)
                    return True
                except queue.Full:
                    continue
            return False

        def work():
            try:
                torch.cuda.set_device(self.trainer.device)
                for data in self.loader:
                    if not put(self.trainer.prefetch(data)):
                        return
                put(self._END)
            except BaseException as e:     # surfaces in the training thread
                put(e)

        th = threading.Thread(target=work, name="bsms-prefetch", daemon=True)
        th.start()
        try:
            while True:
                item = q.get()
                if item is self._END:
                    return
                if isinstance(item, BaseException):
                    raise item
                yield item
        finally:
            stop.set()
            th.join(timeout=5.0)


def recompute_from_cfg(model_cfg):
    """`model_cfg.recompute_activations` (optional): absent or None is False, the route without the key."""
    v = getattr(model_cfg, "recompute_activations", None)
    if v is None:
        return False
    if not isinstance(v, bool):
        raise TypeError(f"model_cfg.recompute_activations is a bool, got {v!r}")
    return v


class Trainer:
    """src/trainer/trainer.py:9-229.  `model_cfg` needs consistent_mesh, accumulation_steps; `opt_cfg` needs
    peak_lr, weight_decay, warmup_steps, decay_steps, gnorm_clip (configs/opt/default.yaml).  Optional in `opt_cfg` (DESIGN.md 4.15;
    with none set the optimizer is the plain fused AdamW): no_decay_bias, lr_scales (`param_groups`), ema_decay, ema_warmup
    (`ema_model()`, `get_pred / get_loss / get_error(..., ema=True)`, `{step}_ema_params.pth` in `save`), skip_nonfinite.  Optional in `model_cfg`:
    unroll_steps (default 1: the reference's single-step loss), unroll_weights, unroll_detach -- the loss over that many
    autoregressive steps (step.FusedStep); `iter` then takes `(batch, later_targets)`, what TrajectoryBank(horizon=K) hands out;
    loss_space ("physical" / "normalized"), loss_kind ("rmse" / "mse", or the robust "mae" / "huber" of DESIGN.md 4.20),
    loss_delta (the Huber threshold in the units of loss_space, a float or one per channel: required by "huber", refused by every other
    kind), loss_channel_weights, loss_edge_weight / loss_edge_weighting (the edge term) -- the training objective
    (objective.Objective; absent: the reference's masked RMSE in physical units), which `iter` trains on and `get_loss` reports;
    loss_node_weights (absent or false: off) -- the objective weights every node by what `iter(data, node_weights=)` and
    `get_loss(data, node_weights=)` are given, e.g. the lumped measure; `get_error` and the rollout statistics stay unweighted;
    recompute_activations (absent or false: off) -- the fused step holds the U-Net blocks' inputs instead of their
    activations and recomputes in the backward: the same parameters after every step, bit for bit, less memory per unrolled step.
    Optional in `opt_cfg`: gradient_accumulation_steps = M (absent or 1: every `iter` is an optimizer step) and
    accumulation_reduction ("batch", the default: the exact loss over the M micro-batches; "mean": the mean of their gradients).  After
    warm-up the optimizer step, the LR-schedule step and the parameter epoch then happen on every M-th `iter` only; `train_step`
    counts calls; `last_accumulated_loss` is the device scalar of the last completed cycle.  `save` inside a cycle does not keep
    the partial sum: `restore` starts the cycle again."""

    def __init__(self, model, model_cfg, opt_cfg):
        self.model_cfg, self.opt_cfg = model_cfg, opt_cfg
        self.device = torch.device("cuda", torch.cuda.current_device())
        self.model = model.to(self.device)
        self.unroll = int(getattr(model_cfg, "unroll_steps", 1) or 1)
        from .objective import Objective
        self.objective = Objective.from_cfg(model_cfg)
        opt = lambda key, default: getattr(opt_cfg, key, default)
        self.accumulate = int(opt("gradient_accumulation_steps", 1) or 1)       # the reference's key (configs/opt/default.yaml), unread there
        self.last_accumulated_loss = None          # device scalar: the loss over every sample of the last completed cycle
        self.dp = DataParallel(self.model, unroll=self.unroll, step_weights=getattr(model_cfg, "unroll_weights", None),
                               detach=bool(getattr(model_cfg, "unroll_detach", False)), objective=self.objective,      # world size 1: no collective is issued
                               accumulate=self.accumulate, reduction=opt("accumulation_reduction", None) or "batch",
                               recompute=recompute_from_cfg(model_cfg))
        no_decay_bias, lr_scales = bool(opt("no_decay_bias", False)), opt("lr_scales", None)
        groups = param_groups(self.model, no_decay_bias, lr_scales) if (no_decay_bias or lr_scales) else None
        self.optimizer = FusedAdamW(self.dp.grads, lr=opt_cfg.peak_lr, weight_decay=opt_cfg.weight_decay,
                                    max_grad_norm=opt_cfg.gnorm_clip, groups=groups, ema_decay=opt("ema_decay", 0.0) or 0.0,
                                    ema_warmup=bool(opt("ema_warmup", True)), skip_nonfinite=bool(opt("skip_nonfinite", False)))
        self._ema_model = None
        self.lr_scheduler = WarmupCosineDecay(opt_cfg.peak_lr, opt_cfg.warmup_steps, opt_cfg.decay_steps)
        self.train_step = 0
        _check_host_threads()
        self._synced = False
        self._norm_base = None     # statistics every rank already shares (restore followed by warm-up)
        self._fitted = False       # fit_normalizers has set the statistics: no warm-up iterations, no merge

    def move_to_device(self, data):
        """trainer/trainer.py:143 semantics (nested lists -> device), except that INDEX tensors (edge lists, kept ids)
        are interned by content (graph.intern_index): a batch of the same mesh maps to the same device tensors every
        step, so the per-mesh plans (CSR layouts, edge weights) are built once, not once per step."""
        from .graph import LevelData, intern_index, _upload
        if isinstance(data, (list, tuple)):
            return [self.move_to_device(d) for d in data]
        if isinstance(data, LevelData):
            return data.to(self.device, intern=True)
        if data.dtype == torch.int64 and not data.is_cuda:
            return intern_index(data, self.device, shared_batch_axis=bool(self.model_cfg.consistent_mesh))
        return _upload(data, self.device)

    def collate(self, samples):
        """Variable meshes (`consistent_mesh: false`): the device batch of a list of SAMPLES (each a per-level list of host LevelData,
        what a dataset item is before PyG's `Batch` collation, datasets/base.py:325-349), assembled on the GPU from per-mesh state
        that stays in HBM (graph.MeshBank: the meshes' plans and edge weights are built once, a batch costs one bsms_plan_concat per
        level).  `iter` / `get_loss` / `get_pred` accept the result like any device batch.  Use it as the loader's `collate_fn`
        consumer: `trainer.iter(trainer.collate(samples))` -- a fresh combination of meshes then costs what a cached one does
        (profiles/fresh_mesh.py: 2.4 against 3.9 ms per cylinder batch of 8)."""
        from .graph import MeshBank
        if self.model_cfg.consistent_mesh:
            raise ValueError("Trainer.collate is the variable-mesh path (model_cfg.consistent_mesh = False)")
        if getattr(self, "_bank", None) is None:
            self._bank = MeshBank(self.model.process, self.device)
        return self._bank.collate(samples)

    def prefetch(self, data):
        """move_to_device + everything mesh-dependent a step of this batch will look up (plans, edge weights): what
        DevicePrefetcher runs one batch ahead.  Returns the device batch; `iter` accepts it as it accepts a host batch."""
        data = self.move_to_device(data)
        if self.model_cfg.consistent_mesh:
            node_in, m_gs, m_ids = data[0], [g[0] for g in data[3]], [i[0] for i in data[4]]
            n0 = node_in.shape[1]
        else:
            m_gs = [d.edge_index for d in data]
            m_ids = [data[i].face for i in range(len(m_gs) - 1)]
            n0 = data[0].x.shape[0]
        self.model.process.prepare(m_ids, m_gs, n0, self.device)
        return data

    def _warming_up(self):
        return not self._fitted and self.train_step < self.model_cfg.accumulation_steps

    def fit_normalizers(self, bank, noise="expected", indices=None, ignore_augment=False):
        """Set the normalisers from the exact moments of `bank` (databank.fit_normalizers) instead of sampling them
        over model_cfg.accumulation_steps warm-up iterations: every resident pair of frames of the chosen trajectories, the training
        noise in closed form (noise="expected") or left out ("none"), summed over the ranks of the trainer's process group, so every
        rank holds identical statistics and no merge follows.  The trainer is then fitted: `iter` trains from its next call on,
        whatever `train_step` is.  The statistics travel in the model's state_dict as ever, so `save` / `restore` carry them; a
        trainer that restores such a checkpoint with train_step < accumulation_steps calls this again, or is configured with
        accumulation_steps = 0, to skip the warm-up.  Returns the Moments."""
        from .databank import fit_normalizers
        mom = fit_normalizers(self.model, bank, noise=noise, indices=indices, group=self.dp.group, ignore_augment=ignore_augment)
        self._fitted, self._synced, self._norm_base = True, True, None
        return mom

    def ema_model(self):
        """The model with the averaged weights (opt_cfg.ema_decay > 0): FusedAdamW.ema_model of the live one, built once.  Its
        trainable parameters are views into the optimizer's `ema` buffer, everything else is the live model's: always current."""
        if self._ema_model is None:
            self._ema_model = self.optimizer.ema_model(self.model)
        return self._ema_model

    def _model_forward(self, data, ema=False):
        return (self.ema_model() if ema else self.model)(data, self.model_cfg.consistent_mesh, self._warming_up())

    def get_label_mask(self, data):
        if self.model_cfg.consistent_mesh:
            return data[1], data[2]
        return data[0].y, data[0].mask

    def get_pred(self, data, ema=False):
        """`ema=True` (here, in get_loss and in get_error): the averaged weights (`ema_model()`) instead of the live ones."""
        return self._model_forward(self.move_to_device(data), ema)

    def eval_panels(self, data, sampler, width, height, sample=0, ema=False, bounds=None, fill=float("nan")):
        """The panels of the reference's eval_plot (src/utils/train_utils.py:60-101) on the device: float32 [C, 4, H, W] -- per
        channel the input state, the label, the prediction and prediction - label of batch entry `sample`, each rasterised on
        `sampler`'s mesh (sample.MeshSampler) in ONE gather launch.  A variable-mesh batch is one sample of sum N
        rows, so `sampler` then spans the union and `sample` is 0.  `ema` as in `get_pred`."""
        data = self.move_to_device(data)
        with torch.no_grad():
            pred = self.get_pred(data, ema)
            tar, _ = self.get_label_mask(data)
            node_in = data[0] if self.model_cfg.consistent_mesh else data[0].x
            C = pred.shape[-1]
            if self.model_cfg.consistent_mesh:
                pred, tar, node_in = pred[sample], tar[sample], node_in[sample]
            elif sample != 0:
                raise IndexError(f"eval_panels: a variable-mesh batch is one sample, got sample={sample}")
            else:
                pred = pred.reshape(-1, C)
            sets = torch.stack([node_in[..., :C], tar, pred, pred - tar])         # [4, N, C]: the one (small) copy on the way
            return sampler.rasterize(sets, width, height, bounds, fill).permute(1, 0, 2, 3)

    def get_loss(self, data, ema=False, node_weights=None):
        """The training objective on `data` (autograd).  `node_weights`: as `iter` takes them, with model_cfg.loss_node_weights."""
        node_weights = self.objective.check_node_weights(node_weights)
        if node_weights is not None:
            node_weights = node_weights.to(self.device)
        data = self.move_to_device(data)
        pred = self._model_forward(data, ema)
        tar, mask = self.get_label_mask(data)
        from .objective import masked_loss                    # the default objective: model.masked_rmse, the reference's formula
        std = None if self.objective.space == "physical" else self.model._targetNormalizer.std_with_epsilon()
        g = pos = None
        if self.objective.has_edge_term:              # J = L + lambda T: the level-0 edge list, the mesh positions
            node_in, g = (data[0], data[3][0][0]) if self.model_cfg.consistent_mesh else (data[0].x, data[0].edge_index)
            pos = node_in[..., pred.shape[-1]:-1]
        return masked_loss(pred, tar, mask, self.objective, std, node_weights=node_weights, g=g, pos=pos)

    def get_error(self, data, relative=True, ema=False):
        """trainer/trainer.py:231-271: (error_mean, error_std) per channel as float32 NumPy arrays [C] -- the masked absolute
        error, divided by each sample's target scale when `relative`.  The reference copies prediction, target and mask to the
        host and reduces there; here one bsms_error_sums launch reduces over the nodes, eval.error_mean_std finishes on the
        device, and 2C numbers are copied back.  Consistent mesh: B samples of N rows; variable meshes: the reference sees the
        block-diagonal batch as [1, sum N, C], i.e. ONE sample of sum N rows (its target and mask stay [sum N, C] / [sum N, 1]
        there, which NumPy broadcasts for the error but reduces over the CHANNEL axis for the scale; the scale here is the
        per-channel one over the sum N rows, what the function computes whenever target and prediction have the same rank).
        During warm-up the prediction is zeros (and the normalisers accumulate), as in the reference."""
        from .eval import error_mean_std
        from .ops import error_sums
        data = self.move_to_device(data)
        with torch.no_grad():
            pred = self.get_pred(data, ema)
            tar, mask = self.get_label_mask(data)
            rows = pred.shape[-2]
            mean, std = error_mean_std(error_sums(pred.reshape(-1, rows, pred.shape[-1]), tar, mask, rows), rows, relative)
            out = torch.stack([mean, std]).float().cpu().numpy()
        return out[0], out[1]

    def get_edge_error(self, data, relative=True, weighting="difference", ema=False):
        """(mean, std) per channel as float32 NumPy arrays [C] of the EDGE-DIFFERENCE error: per sample the RMS
        difference of the error field along the mesh edges, E = sqrt(DE / ME), divided by that of the target field, sqrt(TE / ME),
        when `relative`; `weighting="quotient"` divides every squared difference by the squared edge length (the position columns
        of node_in, copied contiguous once).  Mean and population standard deviation run over the batch's samples; a variable-mesh
        batch is ONE sample of sum N rows, as in `get_error`.  One bsms_edge_diff_sums launch pair on the level-0 plan; 2C numbers
        are copied back."""
        from .eval import edge_error_mean_std
        from .graph import plan_for
        from .ops import edge_diff_sums
        data = self.move_to_device(data)
        with torch.no_grad():
            pred = self.get_pred(data, ema)
            tar, mask = self.get_label_mask(data)
            if self.model_cfg.consistent_mesh:
                node_in, g = data[0], data[3][0][0]
            else:
                node_in, g = data[0].x, data[0].edge_index
            rows, C = pred.shape[-2], pred.shape[-1]
            pos = node_in[..., C:-1].reshape(-1, rows, node_in.shape[-1] - C - 1).contiguous() if weighting == "quotient" else None
            sums = edge_diff_sums(pred.reshape(-1, rows, C), tar.reshape(-1, rows, C), mask.reshape(-1, rows), plan_for(g, rows), pos=pos,
                                  weighting=weighting)
            out = torch.stack(edge_error_mean_std(sums, relative)).float().cpu().numpy()
        return out[0], out[1]

    def get_cell_error(self, data, ops, relative=True, velocity=None, ema=False):
        """(mean, std) per channel as float32 NumPy arrays [C] of the CELL-GRADIENT error: per sample the RMS P1
        gradient of the error field over `ops`' mesh (diffop.MeshGradient), E = sqrt(GE / A), divided by that of the target field,
        sqrt(GT / A), when `relative`.  Mean and population standard deviation run over the batch's samples; a variable-mesh batch is
        ONE sample of sum N rows, as in `get_error`, so `ops` then spans the union.  `velocity` is handed to `ops.sums` (it does not
        change these figures).  One bsms_cell_gradient_sums launch pair; 2C numbers are copied back."""
        from .eval import cell_error_mean_std
        data = self.move_to_device(data)
        with torch.no_grad():
            pred = self.get_pred(data, ema)
            tar, mask = self.get_label_mask(data)
            rows, C = pred.shape[-2], pred.shape[-1]
            sums = ops.sums(pred.reshape(-1, rows, C), tar.reshape(-1, rows, C), mask.reshape(-1, rows), velocity)
            out = torch.stack(cell_error_mean_std(sums, relative)).float().cpu().numpy()
        return out[0], out[1]

    def iter(self, data, node_weights=None):
        """One training iteration (trainer.py:134-156): statistics only during warm-up, otherwise
        fwd + loss + bwd (+ gradient all-reduce) + clip + AdamW + LR schedule.  With model_cfg.unroll_steps = K > 1 `data` is
        `(batch, later_targets)`; the warm-up iterations look at the batch only.  With opt_cfg.skip_nonfinite a step whose
        gradient norm is inf / NaN changes nothing on the device (FusedAdamW.skipped_steps() counts it); the non-finite loss is
        returned as ever and the LR schedule still advances -- what torch does around a skipped GradScaler step -- because
        the host does not read the decision back.
        `node_weights` (model_cfg.loss_node_weights): the batch's node weights -- [N], [B, N] or flat [rows], what
        `TrajectoryBank(node_weights="measure").node_weights(picks)` hands out; required with the key, refused without it.  The warm-up
        iterations check and then ignore them: they form no loss."""
        node_weights = self.objective.check_node_weights(node_weights)
        later = None
        if self.unroll > 1:
            if not (isinstance(data, (tuple, list)) and len(data) == 2 and torch.is_tensor(data[1]) and not torch.is_tensor(data[0])):
                raise ValueError(f"Trainer.iter: unroll_steps = {self.unroll} takes (batch, later_targets)")
            data, later = data[0], self.move_to_device(data[1])
        data = self.move_to_device(data)
        if self._warming_up():
            self._model_forward(data)
            loss = None
        else:
            if not self._synced:                                  # merge normaliser statistics once (dp.py)
                self.dp.sync_normalizers(self._norm_base)
                self._synced, self._norm_base = True, None
            loss = self.dp.step_loss_backward(data, self.model_cfg.consistent_mesh, later, node_weights=node_weights)
            if self.accumulate == 1 or self.dp.fused.ready:       # a micro-batch inside a cycle changes no parameter
                if self.accumulate > 1:
                    self.last_accumulated_loss = self.dp.fused.accumulated_loss()
                self.optimizer.step(self.lr_scheduler.lr())
                self.lr_scheduler.step()
        self.train_step += 1
        return loss

    def save(self, save_dir):
        os.makedirs(save_dir, exist_ok=True)
        torch.save(self.model.state_dict(), f"{save_dir}/{self.train_step}_params.pth")     # reference layout
        if self.optimizer.ema is not None:                                                  # the averaged weights, same layout
            torch.save(self.ema_model().state_dict(), f"{save_dir}/{self.train_step}_ema_params.pth")
        torch.save({"opt": self.optimizer.state_dict(), "epoch": self.lr_scheduler.last_epoch, "train_step": self.train_step},
                   f"{save_dir}/{self.train_step}_opt_state.pth")                           # the reference's TODO

    def restore(self, save_dir, step, restore_opt_state=True):
        self.model.load_state_dict(torch.load(f"{save_dir}/{step}_params.pth", map_location=self.device))
        if self.optimizer.ema is not None:          # no optimizer state (or one without `ema`): the average restarts from the parameters
            self.optimizer.ema.copy_(self.optimizer.flat_p)
        if self.dp.fused is not None:               # a checkpoint taken inside a cycle loses the partial sum: the cycle starts again
            self.dp.fused.reset_accumulation()
        opt_path = f"{save_dir}/{step}_opt_state.pth"
        if restore_opt_state and os.path.exists(opt_path):
            st = torch.load(opt_path, map_location=self.device)
            self.optimizer.load_state_dict(st["opt"])
            self.lr_scheduler.last_epoch = st["epoch"]
            self.train_step = st["train_step"]
        # Restored normaliser statistics are already the merged ones.  If no warm-up follows they must not be merged
        # again (it would multiply _acc_weight / _num_accumulations by the world size).  If warm-up does follow
        # (restore_opt_state=False, no optimizer-state file, or a checkpoint taken during warm-up) every rank goes on
        # accumulating its own shard on top of them: the merge then runs once after warm-up, over the per-rank
        # additions only, with the restored part counted once (Normalizer.synchronize(base=...)).
        if self._warming_up():
            self._synced, self._norm_base = False, {m: m.snapshot() for m in self.dp.normalizers()}
        else:
            self._synced, self._norm_base = True, None
