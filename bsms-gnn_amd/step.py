"""One training step of `BSMS_Simulator` -- forward, masked-RMSE loss, backward -- as a fixed sequence of C-ABI calls on
static buffers, without autograd (reference: models/model.py:127-164, trainer/trainer.py:79-98,144-147).

Why: the autograd mirror of the reference (model.py / ops.py) spends ~40 tiny element-wise launches per step on the
normaliser and the loss, re-creates ~190 gradient views and pointer tables in Python every backward, and cannot be
captured in a HIP graph.  Here the step is

    bsms_pack_group_launch -> bsms_sim_prologue -> bsms_mlp_fwd (encode) -> bsms_bsgmp_fwd (process) -> bsms_mlp_fwd (decode) -> bsms_sim_epilogue
    [data parallel: all-reduce of the two loss sums]
    bsms_sim_loss_bwd -> bsms_mlp_bwd (decode) -> bsms_bsgmp_bwd (process) -> bsms_mlp_bwd (encode)
    [data parallel: all-reduce of the flat gradient buffer]

with every weight gradient written straight into its slot of the flat gradient buffer (`GradBuckets.flat`), which the
parameters' `.grad` alias.  Same kernels as the autograd path for everything but the glue: U-Net / MLP gradients are
bit-identical to it, the loss and its gradient agree to fp32 round-off (tests/test_hip_training.py).  With
`use_graph=True` the two halves are captured into HIP graphs and replayed (inputs are copied into static buffers).

The weights change once per step, so the step packs them once: ONE bsms_pack_group_launch at its head writes the weight packs of the
encoder, every U-Net block and the decoder (and clears their bound slots) straight into the saved buffers, and the three forwards run
with their `reuse` flags -- instead of 13 prepack launches inside them.  A group belongs to one set of pointer tables and
buffers, and building one costs an allocation and blocking copies: it is built only when a step meets the tables and buffers of the step
before it.  While they keep changing (a new mesh combination every step) the forwards pack per call, as they always did, and the host
never waits for the device.

`unroll=K > 1` trains on K autoregressive steps: K forwards, each with its own saved activations, chained by
the rollout rule (bsms_sim_epilogue's `next_in`), then K backwards in reverse order; bsms_sim_unroll_bwd carries the gradient
from step k+1 into step k (or cuts it, `detach=True`), and every step but the last-run-first writes its weight gradients into a
scratch flat buffer that bsms_grad_accumulate folds into `GradBuckets.flat`.

`input_grad=True` also forms the gradient w.r.t. `node_in`: the U-Net backward goes through bsms_bsgmp_bwd_pos_ev
(the same schedule plus the position kernels), the encoder's backward returns its input gradient at every step, and one
bsms_sim_input_grad launch per step folds them, with the step's g_pred, into a static [B, N, C+p+1] buffer (`input_grad()`).

`accumulate=M > 1`: a call is one micro-batch of a cycle of M.  The first is the plain step; every later one writes
its gradient into the scratch flat buffer, bsms_accum_coef forms two coefficients on the device from the running loss sums, and
bsms_grad_fold leaves a * grads.flat + b * scratch: the gradient of the loss over every sample seen so far in the cycle.

Frozen parameters: an MLP -- encoder, decoder, a block's node or edge MLP -- all of whose parameters have
`requires_grad == False` gets NULL entries in the gradient tables; the backward then launches nothing for its weight gradients.
With nothing trainable (or `param_grad=False`) and `input_grad=True` the backward is data-only.

An objective with an EDGE TERM (`Objective(edge_weight=)`): behind bsms_error_sums every forward runs bsms_edge_diff_sums on
the level-0 plan and bsms_edge_diff_fold into the tail of the step's fp64 sums row, which widens to [M | SE | AE | TT | ME | DE]; the backward
starts with bsms_sim_edge_objective_bwd in bsms_sim_objective_bwd's place.  Everything behind the loss gradient is the same step.

`recompute=True`: the U-Net's forward keeps only the inputs of its blocks (the lean `s_proc`, BSMS_FWD_LEAN) and its
backward rebuilds every block's activations just before it needs them (BSMS_BWD_RECOMPUTE), into two blobs in `work`, which all K steps
share.  Every loss, prediction and gradient keeps its bits; a backward costs one more U-Net forward; what a step holds per unrolled
step drops by the blocks' saved activations -- nearly all of it."""
import os
import sys

import torch
import torch.distributed as dist

from . import _abi
from .objective import EDGE_WEIGHTINGS, KINDS, ROBUST_KINDS, SPACES, Objective
from .ops import BWD_FROZEN_BF16, BWD_RECOMPUTE, FWD_LEAN, PRECISIONS, _param_ptrs, _stream


REDUCTIONS = {"batch": 0, "mean": 1}             # BSMS_ACCUM_BATCH / BSMS_ACCUM_MEAN


def _ptr(t):
    return None if t is None else t.data_ptr()


def _mlps(model):
    """The units of freezing, in the order (encoder, U-Net blocks in storage order: node MLP then edge MLP, decoder)."""
    proc = model.process
    blocks = [*proc.down_gmps, proc.bottom_gmp, *proc.up_gmps]
    return [model.encode, *(q for b in blocks for q in (b.mlp_node, b.mlp_edge)), model.decode]


def _freeze_state(mlp):
    """True: every parameter trainable; False: every parameter frozen; None: some of each."""
    req = [p.requires_grad for p in mlp.flat_params()]
    return True if all(req) else (False if not any(req) else None)


class _Arena:
    """Grow-only device buffers by name.  With variable meshes (the reference's cylinder_flow path) every batch has its
    own node / edge counts: buffers sized exactly would be released and re-allocated every step -- hundreds of MB through
    hipMalloc, 30-70 ms per step against a 2.5 ms step (profiles/fresh_mesh.py).  A buffer is re-allocated only when
    a batch needs more than its capacity, then with 25 % headroom."""

    def __init__(self):
        self._t = {}

    def bytes(self, name, nbytes, dev):
        nbytes = max(int(nbytes), 1)
        t = self._t.get(name)
        if t is None or t.numel() < nbytes or t.device != dev:
            cap = nbytes if t is None else nbytes + nbytes // 4
            self._t[name] = None                     # release the old block before asking for the larger one
            t = self._t[name] = torch.empty((cap + 255) // 256 * 256, device=dev, dtype=torch.uint8)
        return t[:nbytes]

    def f32(self, name, dev, *shape):
        n = 1
        for d in shape:
            n *= int(d)
        return self.bytes(name, 4 * max(n, 1), dev)[:4 * n].view(torch.float32).view(*shape)


class FusedStep:
    def __init__(self, model, grads, group=None, use_graph=False, unroll=1, step_weights=None, detach=False, objective=None,
                 input_grad=False, param_grad=True, accumulate=1, reduction="batch", recompute=False):
        """`recompute`: activation recomputation in the U-Net's backward: the same bits from a fraction of the memory
        per (unrolled) step, for one more U-Net forward per backward.  Off: nothing changes.
        `accumulate=M > 1`: every call is one MICRO-batch; after the t-th call of a cycle `grads.flat` holds the
        gradient of the loss over all samples of the cycle so far (`reduction="batch"`), or the mean of the micro-batch gradients
        (`reduction="mean"`, what `(loss / M).backward()` gives); `ready` after the M-th, and the next call starts a new cycle.
        `objective` (objective.Objective): None or the default objective keeps the reference's masked RMSE on the kernels it
        always ran on; any other runs bsms_error_sums after every forward and bsms_sim_objective_bwd in front of every backward --
        their `_w` entries with `objective.node_weighted`, which takes `node_weights=` with every call.  A robust
        objective (kind "mae" / "huber") runs bsms_robust_sums and bsms_sim_robust_bwd in their places, with or
        without node weights; everything behind the sums and the loss gradient is the same step.
        `input_grad`: every backward also forms the gradient of the (K-step) loss w.r.t. `node_in` -- state, mesh
        positions and node type -- into a static [B, N, C+p+1] buffer, handed out by `input_grad()`.  Off: nothing changes.
        `param_grad=False` (with `input_grad=True`): the backward is data-only whatever `requires_grad` says -- no weight gradient is
        formed, `grads` may be None and no `p.grad` is touched."""
        from .model import BSMS_Simulator
        if not isinstance(model, BSMS_Simulator):
            raise TypeError("FusedStep drives a bsms_gnn_amd.BSMS_Simulator")
        if model.process.per_block:
            raise ValueError("FusedStep uses the one-call U-Net (BSGMP.per_block must be False)")
        unroll = int(unroll)
        if unroll < 1:
            raise ValueError(f"FusedStep: unroll must be >= 1, got {unroll}")
        if unroll > 1 and use_graph:
            raise ValueError("FusedStep: the unrolled step (unroll > 1) is not captured into HIP graphs; use use_graph=False")
        if step_weights is None:
            step_weights = [1.0 / unroll] * unroll
        step_weights = [float(w) for w in step_weights]
        if len(step_weights) != unroll:
            raise ValueError(f"FusedStep: {len(step_weights)} step_weights for unroll = {unroll}")
        self.model, self.grads, self.group, self.use_graph = model, grads, group, use_graph
        self.unroll, self.step_weights, self.detach = unroll, step_weights, bool(detach)
        if not isinstance(input_grad, bool):
            raise TypeError(f"FusedStep: input_grad is a bool, got {type(input_grad).__name__}")
        self._input_grad, self._ig_ran = input_grad, False
        if not isinstance(recompute, bool):
            raise TypeError(f"FusedStep: recompute is a bool, got {type(recompute).__name__}")
        self.recompute = recompute
        self._proc_flags = BWD_RECOMPUTE if recompute else 0       # `flags` of the U-Net's size queries
        self._param_grad = bool(param_grad)
        if not self._param_grad and not input_grad:
            raise ValueError("FusedStep: param_grad=False without input_grad=True would compute nothing")
        if grads is None and self._param_grad:
            raise ValueError("FusedStep: weight gradients need a GradBuckets (grads=None goes with param_grad=False)")
        self._any_live = False                      # some MLP gets weight gradients (set by _pointer_tables)
        self._frozen_bit = 0                        # BSMS_BWD_FROZEN_BF16 iff a bf16 precision and an MLP is frozen (set by _pointer_tables)
        if not input_grad and not any(p.requires_grad for q in _mlps(model) for p in q.flat_params()):
            raise ValueError("FusedStep: nothing is trainable and input_grad is off: the step would compute nothing")
        self._guard_params = [q.flat_params()[0] for q in _mlps(model)]
        self.objective = (Objective() if objective is None else objective).bind(model.cfg.out_dim)
        self._obj = None if self.objective.is_default else self.objective      # None: the default route, untouched
        if isinstance(accumulate, bool) or int(accumulate) != accumulate or int(accumulate) < 1:
            raise ValueError(f"FusedStep: accumulate must be an integer >= 1, got {accumulate!r}")
        if reduction not in REDUCTIONS:
            raise ValueError(f"FusedStep: unknown reduction {reduction!r} (one of {sorted(REDUCTIONS)})")
        self.accumulate, self.reduction = int(accumulate), reduction
        if self.accumulate > 1:
            if use_graph:
                raise ValueError("FusedStep: accumulate > 1 is not captured into HIP graphs; use use_graph=False")
            if input_grad:
                raise ValueError("FusedStep: input_grad=True with accumulate > 1: the static input-gradient buffer carries one call's "
                                 "loss coefficient; use accumulate=1")
            if self.objective.has_edge_term:
                raise ValueError("FusedStep: accumulate > 1 with an edge term: the objective has two ratios with different denominators "
                                 "and bsms_accum_coef folds one; use accumulate=1")
            if unroll > 1 and reduction == "batch" and self.objective.kind == "rmse":
                raise ValueError("FusedStep: accumulate > 1 with unroll > 1 and an rmse loss has no exact batch gradient (the steps' "
                                 'coefficients scale differently): use reduction="mean" or loss_kind="mse"')
        self._edge = self.objective.has_edge_term   # J = L + lambda T: the widened sums row and the edge entries
        self._micro = 0                             # micro-batches of the current cycle that have run
        self._acc = None                            # accumulate > 1: dict(running fp64 [K,3], coef fp32 [2], loss fp32 [K]) on the device
        self._gsum = None                           # accumulate > 1 and unroll > 1: where a micro-batch t >= 1 sums its K steps
        self._obj_w = None                          # the channel weights on the device (fp64 [C]), or None for unit weights
        self._obj_delta = None                      # a Huber objective: delta on the device (fp64 [C])
        self._gscratch, self._wts = None, None     # unroll > 1: scratch flat gradient buffer (GradBuckets layout), weights on the device
        self._shape_key, self._graphs, self._ptr_guard = None, None, None
        self._pg, self._pg_builds = None, 0   # pack group of the current pointer tables and buffers (_pack_group), built lazily; how often
        self._pg_key, self._use_group = None, False   # tables + buffers of the previous step; this step packs through the group
        self._arena = _Arena()
        self._overlap = None          # bucket schedule of the overlapped gradient all-reduce (_bucket_schedule), built lazily
        self._comm = None             # communication stream the bucket all-reduces are issued from
        for p in (grads.params if self._param_grad else ()):      # .grad aliases the flat buffer once and for all
            off, n = grads._slot[p]
            p.grad = grads.flat[off:off + n].view_as(p)

    # ------------------------------------------------------------------------------------------------ helpers
    @staticmethod
    def supports(model):
        """A standard one-call BSMS_Simulator whose MLPs (encoder, decoder, each block's node and edge MLP) are each all-trainable
        or all-frozen; anything frozen needs the fp32 precision or, in a bf16 precision, a latent width of 128 or 256
        (DESIGN.md 4.23)."""
        from .model import BSMS_Simulator
        if not isinstance(model, BSMS_Simulator) or model.process.per_block:
            return False
        states = [_freeze_state(q) for q in _mlps(model)]
        return None not in states and (all(states) or model.process.precision == "f32" or model.cfg.latent_dim in (128, 256))

    collectives_at_world_one = False     # tests: issue the step's collectives in a process group of ONE rank as well (a sum over one
                                         # rank is the identity) -- the only way to run the RCCL path on a single-GPU box

    pack_group = True                    # tests and A/B runs: False keeps the per-call prepacks inside the three forwards at every step (13
                                         # launches per step instead of one); every pack, and so every result, is the same bit for bit

    def _world(self):
        return dist.get_world_size(self.group) if dist.is_available() and dist.is_initialized() else 1

    def _collectives(self):
        """The step issues its all-reduces: in a world larger than one, or (`collectives_at_world_one`) in a process group of one rank."""
        return self._world() > 1 or (self.collectives_at_world_one and dist.is_available() and dist.is_initialized())

    def _unpack(self, data, consistent):
        if consistent:
            node_in, tar, mask, m_gs, m_ids = data
            m_gs, m_ids = [g[0] for g in m_gs], [i[0] for i in m_ids]
        else:
            node_in, tar, mask = data[0].x.unsqueeze(0), data[0].y.unsqueeze(0), data[0].mask.unsqueeze(0)
            m_gs = [d.edge_index for d in data]
            m_ids = [data[i].face for i in range(len(m_gs) - 1)]
        self._validate(node_in, tar, mask, m_gs, m_ids)
        f = lambda t: t if (t.is_contiguous() and t.dtype == torch.float32) else t.contiguous().float()
        return f(node_in), f(tar), f(mask), m_gs, m_ids

    def _validate(self, node_in, tar, mask, m_gs, m_ids):
        """The C entries take raw pointers with sizes from cfg: a mis-shaped batch must fail HERE, like the shape
        error PyTorch would raise in the reference (models/model.py:127-164), not read device memory out of bounds."""
        cfg = self.model.cfg
        C, p, depth = cfg.out_dim, self.model.pos_dim, cfg.unet_depth
        if node_in.dim() != 3 or node_in.shape[-1] != C + p + 1:
            raise RuntimeError(f"node_in must be [B, N, out_dim + pos_dim + 1 = {C + p + 1}], got {tuple(node_in.shape)}")
        B, N = node_in.shape[0], node_in.shape[1]
        if tuple(tar.shape) != (B, N, C):
            raise RuntimeError(f"target must be [B, N, out_dim] = {(B, N, C)}, got {tuple(tar.shape)}")
        if mask.numel() != B * N or (mask.dim() == 3 and tuple(mask.shape) != (B, N, 1)) or mask.dim() not in (2, 3):
            raise RuntimeError(f"mask must be [B, N, 1] = {(B, N, 1)}, got {tuple(mask.shape)}")
        if len(m_gs) != depth + 1 or len(m_ids) != depth:
            raise RuntimeError(f"unet_depth = {depth} needs {depth + 1} edge lists and {depth} kept-id lists, "
                               f"got {len(m_gs)} and {len(m_ids)}")
        dev = node_in.device
        for name, t in (("target", tar), ("mask", mask), *((f"m_gs[{i}]", g) for i, g in enumerate(m_gs)),
                        *((f"m_ids[{i}]", g) for i, g in enumerate(m_ids))):
            if t.device != dev:
                raise RuntimeError(f"{name} is on {t.device}, node_in on {dev}: all tensors of a step must share one device")
        if next(self.model.parameters()).device != dev:
            raise RuntimeError(f"the model is on {next(self.model.parameters()).device}, the batch on {dev}")

    def _pointer_tables(self):
        m = self.model
        enc, proc, dec = m.encode.flat_params(), m.process.block_params(), m.decode.flat_params()
        # which MLPs get weight gradients: part of the guard, so a requires_grad_() between two calls rebuilds the tables
        states = tuple(_freeze_state(q) if self._param_grad else False for q in _mlps(m))
        # (one pointer per MLP: an optimizer re-points the trainable MLPs only, which may be any subset)
        guard = (enc[0].data_ptr(), proc[-1].data_ptr(), dec[-1].data_ptr(), *(t.data_ptr() for t in self._guard_params), states)
        if guard != self._ptr_guard:                # parameters were re-pointed (optimizer flat buffer, .to(), load) or (un)frozen
            if None in states:
                raise ValueError("FusedStep: an MLP with some frozen and some trainable parameters (an MLP is frozen as a whole)")
            # a bf16 precision with a frozen MLP: the U-Net's backward takes null entries under BSMS_BWD_FROZEN_BF16
            self._frozen_bit = BWD_FROZEN_BF16 if (not all(states) and m.process.precision != "f32") else 0
            if not any(states) and not self._input_grad:
                raise ValueError("FusedStep: nothing is trainable and input_grad is off: the step would compute nothing")
            live = {}
            for q, st in zip(_mlps(m), states):
                for t in q.flat_params():
                    live[t] = st
                    if st and t not in self.grads._slot:
                        raise ValueError("FusedStep: a trainable parameter has no slot in `grads` (it was frozen when the GradBuckets "
                                         "was built: build the GradBuckets after requires_grad_())")
            # NULL entries for frozen MLPs: the backward launches nothing for their weight gradients
            table = lambda flat, ps: _abi.ptr_array([flat[self.grads._slot[t][0]:].data_ptr() if live[t] else None for t in ps])
            groups = (("enc", enc), ("proc", proc), ("dec", dec))
            self._any_live = any(states)
            self._tabs = {k: (_param_ptrs(ps), table(self.grads.flat if self._any_live else None, ps)) for k, ps in groups}
            self._tabs_scratch = self._tabs_sum = None
            fits = lambda t: t is not None and t.device == self.grads.flat.device and t.numel() == self.grads.flat.numel()
            scratch = self.unroll > 1 or self.accumulate > 1
            if scratch and self._any_live:          # the same slots in the scratch flat buffer: where all steps but the first-run write
                if not fits(self._gscratch):
                    self._gscratch = torch.zeros_like(self.grads.flat)       # zeros: a slot no kernel writes adds nothing
                self._tabs_scratch = {k: (self._tabs[k][0], table(self._gscratch, ps)) for k, ps in groups}
                if self.unroll > 1 and self.accumulate > 1:      # a micro-batch t >= 1 sums its K steps here, never in grads.flat
                    if not fits(self._gsum):
                        self._gsum = torch.zeros_like(self.grads.flat)
                    self._tabs_sum = {k: (self._tabs[k][0], table(self._gsum, ps)) for k, ps in groups}
            elif scratch:                           # nothing trainable: every table is NULLs, no scratch buffer
                self._tabs_scratch = self._tabs_sum = self._tabs
            self._ptr_guard = guard
            self._graphs = None
            self._drop_pack_group()
            self._overlap = None                    # the bucket schedule depends on which blocks run side lanes
        return self._tabs

    def _buffers(self, B, N, plans, dev):
        m, L = self.model, _abi.lib()
        C, p, D, H = m.cfg.out_dim, m.pos_dim, m.cfg.latent_dim, m.cfg.hidden_layer
        key = (B, N, tuple(q.uid for q in plans), str(dev), m.process.precision)
        if key == self._shape_key:
            return self._buf
        R, depth = B * N, len(plans) - 1
        pl, keep = _abi.ptr_array([q.handle.value if hasattr(q.handle, "value") else q.handle for q in plans])
        ar = self._arena                              # views of grow-only buffers: a batch of another size re-uses the memory
        f = lambda name, *s: ar.f32(name, dev, *s)
        u8 = lambda name, n: ar.bytes(name, n, dev)
        b = dict(R=R, pl=pl, pl_keep=keep, plans=plans, depth=depth,
                 norm_in=f("norm_in", R, C + 1), pos=f("pos", R, p), h0=f("h0", R, D), h1=f("h1", R, D),
                 norm_pred=f("norm_pred", R, C), pred=f("pred", B, N, C),
                 sums=f("sums", 2), loss=f("loss", 1), g_np=f("g_np", R, C), gh1=f("gh1", R, D), gh0=f("gh0", R, D),
                 s_enc=u8("s_enc", L.bsms_mlp_saved_bytes(R, C + 1, D, D, H)), s_dec=u8("s_dec", L.bsms_mlp_saved_bytes(R, D, D, C, H)),
                 s_proc=u8("s_proc", L.bsms_bsgmp_saved_bytes_ex(pl, depth, B, D, p, H, PRECISIONS[m.process.precision], self._proc_flags)),
                 prec=m.process.precision,
                 work=u8("work", max(L.bsms_mlp_work_bytes(R, C + 1, D, D, H), L.bsms_mlp_work_bytes(R, D, D, C, H),
                                     L.bsms_bsgmp_work_bytes_ex(pl, depth, B, D, p, H, PRECISIONS[m.process.precision], self._proc_flags),
                                     L.bsms_sim_work_bytes(R))),
                 work_enc=u8("work_enc", L.bsms_mlp_work_bytes(R, C + 1, D, D, H)),   # the encoder's backward overlaps the U-Net's last weight gradients
                 work_dec=u8("work_dec", L.bsms_mlp_work_bytes(R, D, D, C, H)),       # the decoder's weight gradients run under the U-Net's first block
                 in_static=None)
        if self._obj is not None:                     # fp64 [M | SE | AE | TT] of bsms_error_sums, the per-channel terms, its scratch
            b.update(osums=self._f64("osums", dev, 1, self._row(C))[0], chan=f("chan", 1, C)[0],
                     work_obj=u8("work_obj", L.bsms_error_sums_work_bytes(1, R)))
            if self._edge:                            # the per-sample rows [ME | DE | TE], their scratch, (L, T) of the step
                h0 = plans[0].handle
                b.update(esums=self._f64("esums", dev, B, 1 + 2 * C), work_edge=u8("work_edge", L.bsms_edge_diff_work_bytes(B, N)),
                         parts=f("parts", 2), plan0=h0.value if hasattr(h0, "value") else h0)
            if self._obj_w is None or self._obj_w.device != dev:
                self._obj_w = self._obj.weights_tensor(dev)
            if self._obj.delta is not None and (self._obj_delta is None or self._obj_delta.device != dev):
                self._obj_delta = self._obj.delta_tensor(C, dev)
            if self._obj.node_weighted:               # the step's own copy of the node weights, one per row
                b["nw"] = f("nw", R)
        if self._input_grad:                          # shared by the K steps: every launch that touches them is on the caller's stream
            b["ig"] = dict(g_pos=f("g_pos", R, p), grad_in=f("grad_in", B, N, C + p + 1), g_pred=f("g_pred@0", R, C), g_nin=f("g_nin", R, C + 1),
                           pos_work=u8("pos_work", L.bsms_bsgmp_pos_work_bytes(pl, depth, B, p)))
        self._shape_key, self._buf, self._graphs, self._ig_ran = key, b, None, False
        self._drop_pack_group()
        return b

    # ------------------------------------------------------------------------------------------------ the step's weight packs
    def _drop_pack_group(self):
        if getattr(self, "_pg", None) is not None:     # (a graph that captured its launch was dropped with it: _graphs is None here)
            _abi.lib().bsms_pack_group_destroy(self._pg)
        self._pg = None

    def __del__(self):
        if sys is None or sys.is_finalizing():        # interpreter shutdown: the process frees the device
            return
        try:
            self._graphs = None
            self._drop_pack_group()
        except Exception:
            pass

    def _pack_group(self, b, B):
        """The packs of every buffer set of the step (one set, or the K sets of the unrolled step: the weights are the same for all
        K forwards) as ONE group: encoder, the 2L+1 blocks, decoder -- where the forwards with `reuse` read them.
        `recompute`: the encoder and the decoder only -- the lean forward keeps the blocks' packs in `work`, which the encoder's forward
        scribbles on behind the group's launch, so the U-Net packs per call (2L + 1 launches on its pack lane, as without a group); the
        backward's re-run forwards pack for themselves anyway."""
        if self._pg is not None:
            return self._pg
        import ctypes
        m, L = self.model, _abi.lib()
        C, p, D, H = m.cfg.out_dim, m.pos_dim, m.cfg.latent_dim, m.cfg.hidden_layer
        R, t = b["R"], self._tabs
        h = ctypes.c_void_p()
        _abi.check(L.bsms_pack_group_create(ctypes.cast(ctypes.byref(h), _abi.PP)), "bsms_pack_group_create")
        try:
            for bk in (b.get("steps") or [b]):
                _abi.check(L.bsms_pack_group_add_mlp(h, R, C + 1, D, D, H, 1, t["enc"][0][0], bk["s_enc"].data_ptr(), None), "bsms_pack_group_add_mlp(encode)")
                if not self.recompute:
                    _abi.check(L.bsms_pack_group_add_bsgmp(h, b["pl"], b["depth"], B, D, p, H, t["proc"][0][0], bk["s_proc"].data_ptr(), None,
                                                           PRECISIONS[b["prec"]]), "bsms_pack_group_add_bsgmp")
                _abi.check(L.bsms_pack_group_add_mlp(h, R, D, D, C, H, 0, t["dec"][0][0], bk["s_dec"].data_ptr(), None), "bsms_pack_group_add_mlp(decode)")
        except Exception:
            L.bsms_pack_group_destroy(h)
            raise
        self._pg, self._pg_builds = h, self._pg_builds + 1
        return h

    def _decide_packs(self):
        """Once per step, behind _pointer_tables and _buffers: the group serves this step if it exists (those two drop it when anything
        it points at changes), or if the step before had the same tables and buffers -- then it is worth building.  Captured steps
        always use it: their graphs are rebuilt with the tables and buffers anyway."""
        key = (self._ptr_guard, self._shape_key)
        stable, self._pg_key = key == self._pg_key, key
        self._use_group = bool(self.pack_group) and (self._pg is not None or stable or self.use_graph)

    def _launch_packs(self, b, B):
        _abi.check(_abi.lib().bsms_pack_group_launch(self._pack_group(b, B), _stream()), "bsms_pack_group_launch")

    def _f64(self, name, dev, *shape):
        n = 1
        for d in shape:
            n *= int(d)
        return self._arena.bytes(name, 8 * n, dev).view(torch.float64).view(*shape)

    def _row(self, C):
        """Doubles in a step's sums row: [M | SE | AE | TT] of bsms_error_sums, and [ME | DE] behind it with an edge term."""
        return 2 + 4 * C if self._edge else 1 + 3 * C

    def _set_node_weights(self, b, w, B, N):
        """Copy this call's node weights into the step's own buffer of R floats: [N] is tiled over the B samples, [B, N]
        and the flat [R] of a block-diagonal batch give a weight per row.  Both kernels then read a weight per row, whatever shape came
        in.  The buffer is a view of the arena like every other, so a captured graph that reads it replays with whatever the copy in
        front of the replay put there."""
        if w is None:
            return
        R, shape = B * N, tuple(w.shape)
        if shape not in ((N,), (B, N), (R,)):
            raise ValueError(f"FusedStep: node_weights must be [N] = {(N,)}, [B, N] = {(B, N)} or flat [R] = {(R,)}, got {shape}")
        if w.is_cuda and w.device != b["nw"].device:
            raise RuntimeError(f"node_weights is on {w.device}, the batch on {b['nw'].device}")
        n = w.numel()
        b["nw"].view(-1, n).copy_(w.reshape(1, n).expand(R // n, n), non_blocking=True)

    def _loss_sums(self, b):
        """What data parallelism all-reduces (SUM) between the forwards and the backwards: the fp32 pairs of the default route, or
        the fp64 rows of bsms_error_sums (one contiguous message; the backward reads the 1 + C leading doubles of each row -- and, with an
        edge term, the 1 + C trailing ones [ME | DE] of the widened row)."""
        if self._obj is None:
            return b["sums_all"] if self.unroll > 1 else b["sums"]
        return b["osums_all"] if self.unroll > 1 else b["osums"]

    # ------------------------------------------------------------------------------------------------ the two halves
    def _forward(self, b, node_in, tar, mask, ews, B, N, next_in=None, ic=None, pack=True):
        """`next_in` / `ic` (unrolled step only): the epilogue also writes the next step's input by the rollout rule.
        `pack=False` (the unrolled step): one group launch in front of the K forwards covers every buffer set."""
        m, L, s = self.model, _abi.lib(), _stream()
        C, p, D, H = m.cfg.out_dim, m.pos_dim, m.cfg.latent_dim, m.cfg.hidden_layer
        R, t = b["R"], self._tabs
        work = b["work"]                      # owned scratch: the launches are ordered on one stream, also under capture
        ni, no = m._inputNormalizer, m._targetNormalizer
        ck = _abi.check
        reuse = 1 if self._use_group else 0   # BSMS_MLP_REUSE_PACKS / bit 0 of bsms_bsgmp_fwd_p's `reuse`
        if pack and reuse:                    # head of the caller's stream: every pack of the step, every bound slot cleared
            self._launch_packs(b, B)
        ck(L.bsms_sim_prologue(node_in.data_ptr(), R, C, p, ni._E_data.data_ptr(), ni._E_data_squared.data_ptr(),
                               ni.std_eps.data_ptr(), b["norm_in"].data_ptr(), b["pos"].data_ptr(), s), "bsms_sim_prologue")
        ck(L.bsms_mlp_fwd_ex(b["norm_in"].data_ptr(), R, C + 1, D, D, H, 1, t["enc"][0][0], b["h0"].data_ptr(), b["s_enc"].data_ptr(),
                             work.data_ptr(), reuse, s), "bsms_mlp_fwd(encode)")
        ewp, keep = _abi.ptr_array([e.data_ptr() for e in ews])
        ck(L.bsms_bsgmp_fwd_p(b["pl"], ewp, b["depth"], b["h0"].data_ptr(), b["pos"].data_ptr(), B, D, p, N * p, H, t["proc"][0][0],
                              b["h1"].data_ptr(), b["s_proc"].data_ptr(), work.data_ptr(), FWD_LEAN if self.recompute else reuse,
                              PRECISIONS[b["prec"]], s), "bsms_bsgmp_fwd")     # (the lean forward packs per call: _pack_group)
        ck(L.bsms_mlp_fwd_ex(b["h1"].data_ptr(), R, D, D, C, H, 0, t["dec"][0][0], b["norm_pred"].data_ptr(), b["s_dec"].data_ptr(),
                             work.data_ptr(), reuse, s), "bsms_mlp_fwd(decode)")
        own = self._obj is None               # the default route: the epilogue forms the fp32 pair itself
        ck(L.bsms_sim_epilogue(b["norm_pred"].data_ptr(), node_in.data_ptr(), mask.data_ptr(), tar.data_ptr() if own else None, R, C, p,
                               no._E_data.data_ptr(), no._E_data_squared.data_ptr(), no.std_eps.data_ptr(), b["pred"].data_ptr(),
                               _ptr(next_in), _ptr(ic), b["sums"].data_ptr() if own else None, work.data_ptr(), s), "bsms_sim_epilogue")
        self._objective_sums(b, tar, mask, B, N)

    def _objective_sums(self, b, tar, mask, B, N):
        """The sums of another objective than the default, behind the epilogue: one segment of R rows into the step's fp64 row
        (deterministic).  Robust: [M | S] into the first 1 + C fields, the rest of the row is not written.  Node weights: mu = mask * weight
        in the mask's place; the row [M | SE] downstream is none the wiser.  An edge term: B segments of N rows through the level-0 plan
        (a variable-mesh batch: one, the union's), folded into the tail of the row."""
        o = self._obj
        if o is None:
            return
        m, L, s, ck = self.model, _abi.lib(), _stream(), _abi.check
        C, p, R, no = m.cfg.out_dim, m.pos_dim, b["R"], m._targetNormalizer
        rows = (b["pred"].data_ptr(), tar.data_ptr(), mask.data_ptr())
        nw = b["nw"].data_ptr() if o.node_weighted else None
        if o.is_robust:
            ck(L.bsms_robust_sums(*rows, nw, 1, R, C, R, R, R, R, no._E_data.data_ptr(), no._E_data_squared.data_ptr(),
                                  no.std_eps.data_ptr(), _ptr(self._obj_delta), SPACES[o.space], ROBUST_KINDS[o.kind], b["osums"].data_ptr(),
                                  1 + 3 * C, b["work_obj"].data_ptr(), s), "bsms_robust_sums")
        elif o.node_weighted:
            ck(L.bsms_error_sums_w(*rows, nw, 1, R, C, R, R, R, R, b["osums"].data_ptr(), b["work_obj"].data_ptr(), s), "bsms_error_sums_w")
        else:
            ck(L.bsms_error_sums(*rows, 1, R, C, R, R, R, b["osums"].data_ptr(), b["work_obj"].data_ptr(), s), "bsms_error_sums")
            if self._edge:
                ck(L.bsms_edge_diff_sums(b["plan0"], 0, N, *rows, b["pos"].data_ptr(), B, C, p, EDGE_WEIGHTINGS.index(o.edge_weighting),
                                         N, N, N, N, b["esums"].data_ptr(), b["work_edge"].data_ptr(), s), "bsms_edge_diff_sums")
                ck(_abi.ext().bsms_edge_diff_fold(b["esums"].data_ptr(), B, C, b["osums"][1 + 3 * C:].data_ptr(), s), "bsms_edge_diff_fold")

    def _loss_gradient(self, b, tar, mask, chain, B, N):
        """The head of a backward: the loss of the step and its gradient w.r.t. the decoder's output, `g_np`, from the entry of the
        step's objective -- the default: bsms_sim_loss_bwd, or bsms_sim_unroll_bwd with a `chain`; robust;
        with an edge term; squared, with or without node weights.  Without a `chain`: w = 1, nothing carried, no g_pred."""
        m, L, s, ck = self.model, _abi.lib(), _stream(), _abi.check
        C, p, R, o = m.cfg.out_dim, m.pos_dim, b["R"], self._obj
        c = chain or dict(w=1.0, g_pred_next=None, g_nin_next=None, g_pred=None)
        stats = lambda n: (n._E_data.data_ptr(), n._E_data_squared.data_ptr(), n.std_eps.data_ptr())
        rows = (b["pred"].data_ptr(), tar.data_ptr(), mask.data_ptr())
        out_stats, both_stats = stats(m._targetNormalizer), (*stats(m._targetNormalizer), *stats(m._inputNormalizer))
        carried = (c["w"], _ptr(c["g_pred_next"]), _ptr(c["g_nin_next"]), b["loss"].data_ptr())
        outs = (_ptr(c["g_pred"]), b["g_np"].data_ptr(), s)
        if o is None and chain is None:
            ck(L.bsms_sim_loss_bwd(*rows, R, C, *out_stats, b["sums"].data_ptr(), b["loss"].data_ptr(), b["g_np"].data_ptr(), s), "bsms_sim_loss_bwd")
        elif o is None:
            ck(L.bsms_sim_unroll_bwd(*rows, R, C, *both_stats, b["sums"].data_ptr(), *carried, *outs), "bsms_sim_unroll_bwd")
        elif o.is_robust:
            ck(L.bsms_sim_robust_bwd(*rows, b["nw"].data_ptr() if o.node_weighted else None, R, R, C, *both_stats, b["osums"].data_ptr(),
                                     _ptr(self._obj_w), _ptr(self._obj_delta), SPACES[o.space], ROBUST_KINDS[o.kind], *carried,
                                     b["chan"].data_ptr(), *outs), "bsms_sim_robust_bwd")
        elif self._edge:
            ck(_abi.ext().bsms_sim_edge_objective_bwd(b["plan0"], N, B, *rows, b["pos"].data_ptr(), C, p, EDGE_WEIGHTINGS.index(o.edge_weighting),
                                                      *both_stats, b["osums"].data_ptr(), b["osums"][1 + 3 * C:].data_ptr(), _ptr(self._obj_w),
                                                      SPACES[o.space], KINDS[o.kind], o.edge_weight, *carried, b["parts"].data_ptr(),
                                                      b["chan"].data_ptr(), *outs), "bsms_sim_edge_objective_bwd")
        else:                                         # node weights: the same call with the step's weights behind the mask: one per row, period R
            name, nw = ("bsms_sim_objective_bwd_w", (b["nw"].data_ptr(), R)) if o.node_weighted else ("bsms_sim_objective_bwd", ())
            ck(getattr(L, name)(*rows, *nw, R, C, *both_stats, b["osums"].data_ptr(), _ptr(self._obj_w), SPACES[o.space], KINDS[o.kind],
                                *carried, b["chan"].data_ptr(), *outs), name)

    def _backward(self, b, tar, mask, ews, B, N, events=None, chain=None, tabs=None):
        """`events`: (pointer array, keep-alive) of 2L+1 hipEvent_t for bsms_bsgmp_bwd_ev, or None.
        `tabs` (without `chain`; gradient accumulation): the weight gradients of the plain step go to the slots of these tables.
        `chain` (unrolled step only): dict(w, g_pred_next, g_nin_next, g_pred, grad_x, tabs) -- the loss gradient comes from
        bsms_sim_unroll_bwd with the carried pair, the encoder's backward returns its input gradient into `grad_x`, and the
        weight gradients go to the slots of `tabs`."""
        m, L, s = self.model, _abi.lib(), _stream()
        C, p, D, H = m.cfg.out_dim, m.pos_dim, m.cfg.latent_dim, m.cfg.hidden_layer
        R, t = b["R"], ((tabs or self._tabs) if chain is None else chain["tabs"])
        work = b["work"]
        ck = _abi.check
        ig = b["ig"] if self._input_grad else None
        if ig is not None and chain is None:          # the single step as a chain of one: w = 1, nothing carried, g_pred kept
            chain = dict(w=1.0, tabs=t, g_pred_next=None, g_nin_next=None, g_pred=ig["g_pred"], grad_x=ig["g_nin"], first_step=1, overwrite=1)
        self._loss_gradient(b, tar, mask, chain, B, N)
        ck(L.bsms_mlp_bwd_ex(b["h1"].data_ptr(), b["g_np"].data_ptr(), R, D, D, C, H, 0, t["dec"][0][0], b["s_dec"].data_ptr(),
                             b["work_dec"].data_ptr(), b["gh1"].data_ptr(), t["dec"][1][0], 1, s), "bsms_mlp_bwd(decode)")   # 1 = BSMS_BWD_DEFER_JOIN
        ewp, keep = _abi.ptr_array([e.data_ptr() for e in ews])
        flags = 1 | self._proc_flags | self._frozen_bit      # BSMS_BWD_DEFER_JOIN (| BSMS_BWD_RECOMPUTE) (| BSMS_BWD_FROZEN_BF16)
        # BSMS_BWD_DEFER_JOIN: the weight gradients of the last (level-0) block are still running on the engine's side
        # streams (~0.2 ms on half the chip) while the encoder's backward -- own scratch, own gradient slots -- runs here
        if ig is None:
            ck(L.bsms_bsgmp_bwd_ev(b["pl"], ewp, b["depth"], b["h0"].data_ptr(), b["pos"].data_ptr(), b["gh1"].data_ptr(), B, D, p, N * p, H,
                                   t["proc"][0][0], b["s_proc"].data_ptr(), work.data_ptr(), b["gh0"].data_ptr(), t["proc"][1][0],
                                   PRECISIONS[b["prec"]], flags, None if events is None else events[0], s), "bsms_bsgmp_bwd")
        else:                                         # the same schedule, plus the position kernels on this stream (g_pos is complete on return)
            ck(L.bsms_bsgmp_bwd_pos_ev(b["pl"], ewp, b["depth"], b["h0"].data_ptr(), b["pos"].data_ptr(), b["gh1"].data_ptr(), B, D, p, N * p, H,
                                       t["proc"][0][0], b["s_proc"].data_ptr(), work.data_ptr(), b["gh0"].data_ptr(), t["proc"][1][0],
                                       PRECISIONS[b["prec"]], flags, None if events is None else events[0], ig["g_pos"].data_ptr(),
                                       ig["pos_work"].data_ptr(), s), "bsms_bsgmp_bwd_pos")
        ck(L.bsms_mlp_bwd(b["norm_in"].data_ptr(), b["gh0"].data_ptr(), R, C + 1, D, D, H, 1, t["enc"][0][0], b["s_enc"].data_ptr(),
                          b["work_enc"].data_ptr(), None if chain is None else _ptr(chain["grad_x"]), t["enc"][1][0], s),
           "bsms_mlp_bwd(encode)")
        if ig is not None:                            # fold this step into dJ / d node_in: own buffers, no `work`, no `grads` -- before the join
            ni = m._inputNormalizer
            ck(L.bsms_sim_input_grad(chain["g_pred"].data_ptr(), chain["grad_x"].data_ptr(), ig["g_pos"].data_ptr(), mask.data_ptr(), R, C, p,
                                     ni._E_data.data_ptr(), ni._E_data_squared.data_ptr(), ni.std_eps.data_ptr(), chain["first_step"],
                                     chain["overwrite"], ig["grad_in"].data_ptr(), s), "bsms_sim_input_grad")
            self._ig_ran = True
        ck(L.bsms_side_lanes_join(s), "bsms_side_lanes_join")

    # ------------------------------------------------------------------------------------------------ the step
    def __call__(self, data, consistent=True, later_targets=None, node_weights=None):
        """`later_targets` (unroll = K > 1 only): the targets of steps 1 .. K-1, [K-1, B, N, C] for consistent meshes and
        [K-1, rows, C] for variable meshes (frames t+2 .. t+K; TrajectoryBank(horizon=K) hands them out).
        `node_weights`: float32 [N] (shared by the batch), [B, N], or flat [rows] for variable meshes; required by an
        objective with `node_weighted`, refused by any other.  They are copied into a buffer the step owns; all K steps read it."""
        node_weights = self.objective.check_node_weights(node_weights)
        node_in, tar, mask, m_gs, m_ids = self._unpack(data, consistent)
        if (self.unroll > 1) != (later_targets is not None):
            raise ValueError(f"FusedStep: unroll = {self.unroll} " + ("needs later_targets" if self.unroll > 1 else "takes no later_targets"))
        if not node_in.is_cuda:
            raise _abi.BsmsError("FusedStep: the BSMS engine runs on the GPU only; there is no CPU fallback")
        B, N = node_in.shape[0], node_in.shape[1]
        plans, ews, bottom = self.model.process.prepare(m_ids, m_gs, N, node_in.device)
        plans = [*plans, bottom]
        self._pointer_tables()
        b = self._buffers(B, N, plans, node_in.device)
        self._set_node_weights(b, node_weights, B, N)
        self._decide_packs()
        coll = self._collectives()
        if self.accumulate > 1:
            return self._micro_batch(b, node_in, tar, mask, later_targets, ews, B, N, coll, consistent)
        if self.unroll > 1:
            return self._unrolled(b, node_in, tar, mask, later_targets, ews, B, N, coll, consistent)
        if self.use_graph:
            return self._replay(b, node_in, tar, mask, ews, B, N, coll)
        self._forward(b, node_in, tar, mask, ews, B, N)
        if coll:
            dist.all_reduce(self._loss_sums(b), op=dist.ReduceOp.SUM, group=self.group)
        if coll and self._any_live and self._overlap_now():
            self._backward_overlapped(b, tar, mask, ews, B, N)
        else:
            self._backward(b, tar, mask, ews, B, N)
            if coll and self._any_live:
                dist.all_reduce(self.grads.flat, op=dist.ReduceOp.SUM, group=self.group)
        self._probe_end()
        return b["loss"][0].clone()       # the static buffer is overwritten by the next step: hand out a copy (4 bytes)

    # ------------------------------------------------------------------------------------------------ the unrolled step
    _PER_STEP = ("s_enc", "s_proc", "s_dec", "norm_in", "h0", "h1", "pred", "sums")     # saved per step; everything else is shared

    def held_bytes(self):
        """dict(per_step=, shared=): the bytes of the step's device buffers (capacities of its arena; no allocator statistics).
        `per_step`: what one unrolled step owns -- the `_PER_STEP` names, and with unroll > 1 the step's input (`in@k`; the first
        step's is the caller's), i.e. what unroll + 1 would add.  `shared`: everything else, whatever the unroll.  All buffers
        together: shared + (step 0: the `_PER_STEP` names) + (unroll - 1) x per_step."""
        if self._shape_key is None:
            raise RuntimeError("FusedStep.held_bytes: the step has not run yet")
        cap = {n: t.numel() * t.element_size() for n, t in self._arena._t.items() if t is not None}
        owned = lambda k: sum(cap.get(n if k == 0 else f"{n}@{k}", 0) for n in (*self._PER_STEP, *(("in",) if k else ())))
        steps = [owned(k) for k in range(self.unroll)]
        return dict(per_step=steps[1] if self.unroll > 1 else steps[0], shared=sum(cap.values()) - sum(steps))

    def _unroll_buffers(self, b, B, N, dev):
        """Step k's own buffers (`name@k` in the arena) on top of the shared ones of `_buffers`, which serve as step 0's."""
        if b.get("steps") is not None:
            return b["steps"]
        m, K = self.model, self.unroll
        C, p = m.cfg.out_dim, m.pos_dim
        R, ar = b["R"], self._arena
        sums = ar.f32("sums_all", dev, K, 2)              # ONE buffer: the data-parallel all-reduce of the sums is one message
        losses = ar.f32("loss_all", dev, K)
        if self._obj is not None:
            osums, chans = self._f64("osums_all", dev, K, self._row(C)), ar.f32("chan_all", dev, K, C)
            parts = ar.f32("parts_all", dev, K, 2) if self._edge else None
        steps = []
        for k in range(K):
            bk = dict(b)
            if self._obj is not None:
                bk["osums"], bk["chan"] = osums[k], chans[k]
                if self._edge:
                    bk["parts"] = parts[k]
            for name in self._PER_STEP:
                if name == "sums":
                    bk[name] = sums[k]
                elif k > 0:
                    src = b[name]
                    nbytes = src.numel() * src.element_size()
                    bk[name] = ar.bytes(f"{name}@{k}", nbytes, dev) if src.dtype == torch.uint8 else ar.f32(f"{name}@{k}", dev, *src.shape)
            bk["loss"] = losses[k:k + 1]
            bk["in"] = None if k == 0 else ar.f32(f"in@{k}", dev, B, N, C + p + 1)
            steps.append(bk)
        b.update(steps=steps, pred=steps[K - 1]["pred"], sums_all=sums, loss_all=losses, g_pred=(ar.f32("g_pred@0", dev, R, C), ar.f32("g_pred@1", dev, R, C)),
                 g_nin=ar.f32("g_nin", dev, R, C + 1))
        if self._obj is not None:
            b.update(osums_all=osums, chan_all=chans)
            if self._edge:
                b["parts_all"] = parts
        if self._wts is None or self._wts.device != dev:
            self._wts = torch.tensor(self.step_weights, device=dev, dtype=torch.float32)
        return steps

    def _later(self, later, node_in, consistent):
        K, C = self.unroll, self.model.cfg.out_dim
        B, N = node_in.shape[0], node_in.shape[1]
        if not torch.is_tensor(later):
            raise RuntimeError("later_targets must be a tensor")
        if later.dim() == 3 and not consistent:          # variable meshes: [K-1, rows, C]
            later = later.unsqueeze(1)
        if tuple(later.shape) != (K - 1, B, N, C):
            raise RuntimeError(f"later_targets must be [K-1, B, N, out_dim] = {(K - 1, B, N, C)} (or [K-1, rows, out_dim] for variable "
                               f"meshes), got {tuple(later.shape)}")
        if later.device != node_in.device:
            raise RuntimeError(f"later_targets is on {later.device}, node_in on {node_in.device}")
        return later if (later.is_contiguous() and later.dtype == torch.float32) else later.contiguous().float()

    def _unrolled(self, b, node_in, tar, mask, later, ews, B, N, coll, consistent, into=None):
        """`into` (gradient accumulation): (tables, flat buffer) that receive the K-step sum instead of grads.flat, and no gradient
        all-reduce here; the steps that are folded in then go through `_tabs_scratch` / `_gscratch` as ever."""
        K, L, s = self.unroll, _abi.lib(), _stream()
        tabs_sum, flat_sum = (self._tabs, None if self.grads is None else self.grads.flat) if into is None else into   # (param_grad=False: no grads)
        later = self._later(later, node_in, consistent)
        steps = self._unroll_buffers(b, B, N, node_in.device)
        tars = [tar, *(later[k] for k in range(K - 1))]
        if self._use_group:
            self._launch_packs(b, B)                      # the weights are fixed across the K forwards: every set's packs in ONE launch
        # K forwards: step k's epilogue writes in_{k+1} = where(mask == 0, in_0, cat[pred_k, mesh_pos | type])
        for k, bk in enumerate(steps):
            nxt = steps[k + 1]["in"] if k + 1 < K else None
            self._forward(bk, node_in if k == 0 else bk["in"], tars[k], mask, ews, B, N, next_in=nxt, ic=None if nxt is None else node_in,
                          pack=False)
        if coll:
            dist.all_reduce(self._loss_sums(b), op=dist.ReduceOp.SUM, group=self.group)
        # K backwards, k = K-1 .. 0.  The first one run writes grads.flat itself, the others the scratch buffer, folded in after
        # the join: the deferred weight-gradient lanes of step k still write it (and read work / work_enc / work_dec) until then
        n = self.grads.flat.numel() if self._any_live else 0
        for k in range(K - 1, -1, -1):
            bk, last = steps[k], k == K - 1
            carry = not last and not self.detach
            keep = self._input_grad or (k > 0 and not self.detach)      # input_grad: g_pred and the encoder's grad_x of EVERY step
            chain = dict(w=self.step_weights[k], tabs=tabs_sum if last else self._tabs_scratch,
                         g_pred_next=b["g_pred"][(k + 1) & 1] if carry else None, g_nin_next=b["g_nin"] if carry else None,
                         g_pred=b["g_pred"][k & 1] if keep else None, grad_x=b["g_nin"] if keep else None,
                         first_step=int(k == 0), overwrite=int(last))
            self._backward(bk, tars[k], mask, ews, B, N, chain=chain)          # ends with bsms_side_lanes_join
            if not last and self._any_live:
                _abi.check(L.bsms_grad_accumulate(flat_sum.data_ptr(), self._gscratch.data_ptr(), n, 0, s), "bsms_grad_accumulate")
        if coll and self._any_live and into is None:
            dist.all_reduce(self.grads.flat, op=dist.ReduceOp.SUM, group=self.group)
        return torch.dot(b["loss_all"], self._wts)

    # ------------------------------------------------------------------------------------------------ gradient accumulation
    def _micro_batch(self, b, node_in, tar, mask, later, ews, B, N, coll, consistent):
        """One micro-batch of a cycle of `accumulate`.  Micro-batch 0 is the plain (or unrolled) step into grads.flat;
        micro-batch t >= 1 writes its whole gradient into the scratch flat buffer, and behind the join bsms_accum_coef forms (a, b)
        on the device from the (all-reduced) loss sums and bsms_grad_fold leaves a * grads.flat + b * scratch in grads.flat.  The host
        reads nothing back.  Data parallel: every rank folds with the same global coefficients; ONE all-reduce of the flat buffer
        after the last fold of the cycle."""
        L, s, K = _abi.lib(), _stream(), self.unroll
        dev = node_in.device
        if self._micro >= self.accumulate:            # the (M+1)-th call starts a new cycle by itself
            self._micro = 0
        t = self._micro
        if self._acc is None or self._acc["coef"].device != dev:
            self._acc = dict(running=torch.zeros(K, 3, device=dev, dtype=torch.float64), coef=torch.zeros(2, device=dev),
                             loss=torch.zeros(K, device=dev))
        if K > 1:                                     # t >= 1: the K-step sum in _gsum, the folded-in steps through _gscratch
            into = (self._tabs, self.grads.flat) if t == 0 else (self._tabs_sum, self._gsum)
            loss = self._unrolled(b, node_in, tar, mask, later, ews, B, N, coll, consistent, into=into)
            g = self._gsum
        else:
            self._forward(b, node_in, tar, mask, ews, B, N)
            if coll:
                dist.all_reduce(self._loss_sums(b), op=dist.ReduceOp.SUM, group=self.group)
            self._backward(b, tar, mask, ews, B, N, tabs=None if t == 0 else self._tabs_scratch)       # ends with bsms_side_lanes_join
            loss, g = b["loss"][0].clone(), self._gscratch
        sums, no, o = self._loss_sums(b), self.model._targetNormalizer, self.objective
        row = self._obj is not None
        C = self.model.cfg.out_dim
        # A robust loss is sum_c w_c S_c / (M C): the mse algebra of the PHYSICAL space on the row [M | S] (the scaling by s_c is
        # already inside S_c) -- bsms_accum_coef forms that loss and its fold coefficients exactly, with no entry of their own.
        space, kind = (SPACES["physical"], KINDS["mse"]) if o.is_robust else (SPACES[o.space], KINDS[o.kind])
        _abi.check(L.bsms_accum_coef(sums.data_ptr(), int(row), (1 + 3 * C) if row else 2, C, no._E_data.data_ptr(),
                                     no._E_data_squared.data_ptr(), no.std_eps.data_ptr(), _ptr(self._obj_w) if row else None,
                                     space, kind, REDUCTIONS[self.reduction], t, K, self._acc["running"].data_ptr(),
                                     self._acc["coef"].data_ptr(), self._acc["loss"].data_ptr(), s), "bsms_accum_coef")
        if t > 0 and self._any_live:
            _abi.check(L.bsms_grad_fold(self.grads.flat.data_ptr(), g.data_ptr(), self.grads.flat.numel(), self._acc["coef"].data_ptr(), s),
                       "bsms_grad_fold")
        self._micro = t + 1
        if self.ready and coll and self._any_live:
            dist.all_reduce(self.grads.flat, op=dist.ReduceOp.SUM, group=self.group)
        return loss

    @property
    def micro_index(self):
        """Micro-batches of the current cycle that have run: 0 after construction or `reset_accumulation()`, `accumulate` when `ready`."""
        return self._micro

    @property
    def ready(self):
        """True after the last micro-batch of a cycle (always, with accumulate = 1): `grads.flat` holds the cycle's gradient."""
        return self.accumulate == 1 or self._micro == self.accumulate

    def reset_accumulation(self):
        """Drop the partial cycle: the next call is micro-batch 0 (which overwrites `grads.flat` and the running sums)."""
        self._micro = 0

    def _accumulating(self, what):
        if self.accumulate == 1:
            raise ValueError(f"FusedStep.{what}: the step was built with accumulate = 1")
        if self._acc is None:
            raise RuntimeError(f"FusedStep.{what}: the step has not run yet")

    def accumulated_loss(self):
        """Device scalar sum_k w_k Lc_k: the loss over every sample of the cycle so far (`reduction="batch"`) or the running mean of the
        micro-batch losses (`"mean"`), weighted over the unroll steps like the value a call returns (a copy)."""
        self._accumulating("accumulated_loss")
        return torch.dot(self._acc["loss"], self._wts) if self.unroll > 1 else self._acc["loss"][0].clone()

    def accumulation_coefficients(self):
        """Device [2]: a copy of (a, b) of the last bsms_accum_coef -- (0, 1) after micro-batch 0.  For tests."""
        self._accumulating("accumulation_coefficients")
        return self._acc["coef"].clone()

    def predictions(self):
        """The K predictions of the last step, [B,N,C] each (static buffers: clone to keep)."""
        return [bk["pred"] for bk in self._buf["steps"]] if self.unroll > 1 else [self._buf["pred"]]

    def input_grad(self):
        """dJ / d node_in of the last call, [B, N, C+p+1] in the column layout of `node_in` ([1, rows, .] for variable meshes): the
        gradient of the weighted K-step loss w.r.t. the initial state, the mesh positions and the node type.  A
        static buffer, overwritten by the next call: clone to keep.  Under data parallelism it covers this rank's samples, with the
        global loss coefficient."""
        if not self._input_grad:
            raise ValueError("FusedStep.input_grad: the step was built without input_grad=True")
        if not self._ig_ran:
            raise RuntimeError("FusedStep.input_grad: the step has not run yet")
        return self._buf["ig"]["grad_in"]

    def step_losses(self):
        """Device [K]: the loss (the masked RMSE by default, else the objective) of every step of the last call, unweighted (a copy)."""
        return (self._buf["loss_all"] if self.unroll > 1 else self._buf["loss"]).clone()

    def channel_losses(self):
        """Device [K, C]: the per-channel terms a_c SE_c / (M C) of every step of the last call -- they add up to Q, the loss under
        kind = "mse" and its square under "rmse"; w_c S_c / (M C) of a robust objective (a copy).  Only the objective route (bsms_sim_objective_bwd's `chan_out`) forms them."""
        if self._obj is None:
            raise ValueError("FusedStep.channel_losses: the default objective runs the reference's kernels, which form no per-channel "
                             "terms; pass objective=Objective(channel_weights=[1.0] * out_dim) to get them for the same loss")
        return (self._buf["chan_all"] if self.unroll > 1 else self._buf["chan"].reshape(1, -1)).clone()

    def loss_parts(self):
        """Device fp32 [2]: (L, T) of the last call -- the pointwise loss and the edge term of J = L + edge_weight * T, each weighted
        over the unroll steps like the value a call returns (a copy).  Only an objective with an edge term forms them."""
        if not self._edge:
            raise ValueError("FusedStep.loss_parts: the objective has no edge term (Objective(edge_weight=))")
        if self._shape_key is None:
            raise RuntimeError("FusedStep.loss_parts: the step has not run yet")
        return self._wts @ self._buf["parts_all"] if self.unroll > 1 else self._buf["parts"].clone()

    # ------------------------------------------------------------------------------------------------ overlapped all-reduce
    # False (BSMS_OVERLAP_ALLREDUCE=0): ONE all-reduce of the whole flat buffer after the backward (rounds 1-3)
    overlap_allreduce = os.environ.get("BSMS_OVERLAP_ALLREDUCE", "1") == "1"

    overlap_min_gain = 0.97       # the overlapped form is kept only if its step time <= this x the plain form's (>= 3 % gain)
    force_overlap = False         # tests: take the overlapped path on any backend, without the self-check below
    probe_any_backend = False     # tests: run the self-check on a backend other than nccl

    def _overlap_now(self):
        """Overlapped (per-bucket) or plain (one message) gradient all-reduce for THIS step.
        * Only on the nccl backend (= RCCL): there an asynchronous collective issued from a side stream is stream-ordered
          and costs the host nothing.  gloo stages CUDA tensors through the host from a worker thread; four asynchronous
          works per step behind stream-side event waits measured 0.1-2 s per step against 8 ms for one blocking message
          (profiles/dbg_overlap.py) -- the CPU tests and the one-GPU functional runs use the plain form.
        * SELF-CHECK: no multi-GPU machine was available to the builder, so the first four data-parallel steps of a process
          measure both forms (two plain, two overlapped, each timed with HIP events and synchronised), the ranks agree on
          the maxima with one tiny all-reduce, and the overlapped form is kept only if it PROVES a gain of at least 3 %
          (round 5; round 4 kept it unless it was 1.25x slower -- the plain single message is the de-risked default, the
          overlap has to earn its machinery).  The decision is identical on every rank (a mixed choice would mismatch
          the collectives)."""
        if self.force_overlap:
            return True
        if not self.overlap_allreduce or (dist.get_backend(self.group) != "nccl" and not self.probe_any_backend):
            return False
        st = self.__dict__.setdefault("_ov_probe", {"n": 0, "t": {False: [], True: []}, "use": None, "ev": None})
        if st["use"] is not None:
            return st["use"]
        mode = st["n"] >= 2
        st["mode"] = mode
        st["ev"] = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
        st["ev"][0].record()
        return mode

    def _probe_end(self):
        st = self.__dict__.get("_ov_probe")
        if not st or st["use"] is not None or st["ev"] is None:
            return
        st["ev"][1].record()
        st["ev"][1].synchronize()
        st["t"][st["mode"]].append(st["ev"][0].elapsed_time(st["ev"][1]))
        st["ev"] = None
        st["n"] += 1
        if st["n"] == 4:
            t = torch.tensor([min(st["t"][False]), min(st["t"][True])], device=self.grads.flat.device, dtype=torch.float64)
            dist.all_reduce(t, op=dist.ReduceOp.MAX, group=self.group)
            plain, over = float(t[0]), float(t[1])
            st["use"] = over <= self.overlap_min_gain * plain
            st["measured_ms"] = {"plain": plain, "overlapped": over}
            if not st["use"] and over > 1.25 * plain:      # not merely "no gain" but clearly worse: worth a warning
                import warnings
                warnings.warn(f"FusedStep: the overlapped gradient all-reduce measured {over:.2f} ms per step against {plain:.2f} ms "
                              "for one message after the backward -- using the plain form (BSMS_OVERLAP_ALLREDUCE=0 skips this check)",
                              RuntimeWarning)

    def _bucket_schedule(self, depth):
        """Which `block_done_events` entry of bsms_bsgmp_bwd_ev releases each bucket of `self.grads`.
        The backward produces the weight gradients in this order: decoder (deferred onto side lane 0 in front of the U-Net),
        the U-Net blocks in EXECUTION order e = 0..2L -- up_gmps[L-1] .. up_gmps[0], bottom_gmp, down_gmps[L-1] .. down_gmps[0]
        -- and the encoder (on the caller's stream, after which the lanes are joined).  The flat gradient buffer is laid out
        in reversed parameter order (dp.GradBuckets), i.e. roughly in this order too, so consecutive buckets complete
        one after the other.  A bucket is released by the LAST stage any of its parameters belongs to; `None` = only the
        final join (encoder, and whatever shares a bucket with it)."""
        m, L = self.model, depth
        stage = {}
        blocks = [*m.process.down_gmps, m.process.bottom_gmp, *m.process.up_gmps]
        with_lanes = []                                           # execution indices of the blocks that run side lanes
        for k, blk in enumerate(blocks):
            e = (2 * L - k) if k < L else (L if k == L else L - 1 - (k - (L + 1)))     # storage index -> execution index
            for q in (*blk.mlp_node.flat_params(), *blk.mlp_edge.flat_params()):
                stage[q] = e
            if _freeze_state(blk.mlp_node) or _freeze_state(blk.mlp_edge):
                with_lanes.append(e)
        # the decoder: covered by the event of the first block that runs side lanes (in-order lanes); a block with both MLPs frozen
        # records its event on the caller's stream, which says nothing about the lanes -- with every block frozen, the final join
        for q in m.decode.flat_params():
            stage[q] = min(with_lanes) if with_lanes else None
        out = []
        for bk in self.grads.buckets:
            st = [stage.get(q) for q in bk["params"]]
            out.append(None if any(v is None for v in st) else max(st))
        return out

    def _backward_overlapped(self, b, tar, mask, ews, B, N):
        """The backward with the gradient all-reduce issued PER BUCKET from a communication stream that waits for the
        side-lane event after which the bucket's gradients are final -- the ring transfer of the decoder / up-path buckets
        runs under the down-path blocks; only the last bucket (first down block + encoder) is exposed after the join.
        The host enqueues the whole backward first (it runs ~4 ms ahead of the GPU), then the waits + all-reduces: they
        execute on the GPU as soon as their event fires, not when the host gets there.  Every rank issues the same
        collectives in the same order (the schedule depends on the model only); sums are bitwise rank-independent."""
        depth = b["depth"]
        if self._overlap is None or self._overlap["depth"] != depth:
            evs = [torch.cuda.Event() for _ in range(2 * depth + 1)]
            for e in evs:
                e.record()                     # materialises the hipEvent_t (torch creates it on first use)
            sched = self._bucket_schedule(depth)
            used = {e for e in sched if e is not None}
            ptrs = [evs[i].cuda_event if i in used else None for i in range(2 * depth + 1)]
            self._overlap = dict(depth=depth, events=evs, sched=sched, ptrs=_abi.ptr_array(ptrs))
            self._comm = torch.cuda.Stream(device=b["h0"].device)
        ov = self._overlap
        self._backward(b, tar, mask, ews, B, N, events=ov["ptrs"])        # ends with bsms_side_lanes_join on the caller's stream
        main = torch.cuda.current_stream()
        works = []
        for k, e in self._issue_order(ov["sched"]):                       # identical on every rank: a function of the model only
            bk = self.grads.buckets[k]
            if e is None:                                                    # what only the final join releases: caller's stream
                works.append(dist.all_reduce(bk["view"], op=dist.ReduceOp.SUM, group=self.group, async_op=True))
                continue
            with torch.cuda.stream(self._comm):
                self._comm.wait_event(ov["events"][e])
                works.append(dist.all_reduce(bk["view"], op=dist.ReduceOp.SUM, group=self.group, async_op=True))
        for w in works:
            w.wait()                           # the caller's stream waits for the collectives (no host block with nccl)
        main.wait_stream(self._comm)

    @staticmethod
    def _issue_order(sched):
        """Order in which the bucket all-reduces are issued: [(bucket index, releasing event or None)].  First the buckets an
        event releases, in bucket order (= the order their events fire: the flat buffer is laid out in backward order, and
        `_bucket_schedule` makes the event index non-decreasing along it), then the buckets only the final join releases.
        A pure function of the schedule, which is a pure function of the model: every rank issues the same collectives in
        the same order (tests/test_dp_gloo.py::test_overlapped_allreduce_issue_order_is_rank_independent)."""
        first = [(k, e) for k, e in enumerate(sched) if e is not None]
        return first + [(k, None) for k, e in enumerate(sched) if e is None]

    def prediction(self):
        """[B,N,C] prediction of the last step (a static buffer: clone it to keep it)."""
        return self._buf["pred"]

    def _replay(self, b, node_in, tar, mask, ews, B, N, coll):
        if b["in_static"] is None:
            b["in_static"] = (torch.empty_like(node_in), torch.empty_like(tar), torch.empty_like(mask))
            self._graphs = None
        sn, st, sm = b["in_static"]
        sn.copy_(node_in); st.copy_(tar); sm.copy_(mask)
        if self._graphs is None:
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):             # warm-up outside capture: workspaces, lazy kernel attributes, lanes
                self._forward(b, sn, st, sm, ews, B, N)
                self._backward(b, st, sm, ews, B, N)
            torch.cuda.current_stream().wait_stream(side)
            gf, gb = torch.cuda.CUDAGraph(), torch.cuda.CUDAGraph()
            # thread_local: a trainer.DevicePrefetcher thread may be allocating / uploading the NEXT batch's plans right
            # now (hipMalloc, hipMemcpyAsync on its own streams); in the default global mode such a call from another
            # thread invalidates this capture
            with torch.cuda.graph(gf, capture_error_mode="thread_local"):
                self._forward(b, sn, st, sm, ews, B, N)
            with torch.cuda.graph(gb, capture_error_mode="thread_local"):
                self._backward(b, st, sm, ews, B, N)
            self._graphs = (gf, gb, ews)              # the graphs hold raw pointers: keep what they point at alive
        gf, gb, _ = self._graphs
        gf.replay()
        if coll:
            dist.all_reduce(self._loss_sums(b), op=dist.ReduceOp.SUM, group=self.group)
        gb.replay()
        if coll and self._any_live:
            dist.all_reduce(self.grads.flat, op=dist.ReduceOp.SUM, group=self.group)
        return b["loss"][0].clone()


def _input_gradient_key(K, step_weights, detach, objective, param_grad, recompute=False):
    """Cache key of `input_gradient`'s steps: one FusedStep per (K, step_weights, detach, objective, param_grad, recompute)."""
    return (int(K), None if step_weights is None else tuple(float(w) for w in step_weights), bool(detach), objective, bool(recompute),
            bool(param_grad))


def input_gradient(model, data, consistent=True, later_targets=None, step_weights=None, detach=False, objective=None, param_grad=True,
                   recompute=False, node_weights=None):
    """Sensitivity of a (rollout) objective of a trained `BSMS_Simulator`: returns `(loss, grad_node_in)`, the weighted K-step loss
    and its gradient w.r.t. `node_in` -- initial state, mesh positions, node type; [B, N, C+p+1], or [1, rows, C+p+1] for variable
    meshes.  K = 1 without `later_targets`, else `later_targets.shape[0] + 1`; `step_weights`, `detach` and
    `objective` are FusedStep's.  The gradient is a clone: it stays valid after the next call.

    A convenience over a `FusedStep(input_grad=True)` that is built once per (K, step_weights, detach, objective) and cached on the
    model, together with ONE `GradBuckets` for all of them.  The parameters themselves are left untouched.  Their `.grad`s are
    written as `GradBuckets` writes them: after the first call every `p.grad` is a view into the flat gradient buffer and holds
    the weight gradients of the last call (the backward forms them anyway).  A model that a `Trainer` or `DataParallel` drives
    owns its `GradBuckets` already: take `engine.fused.input_grad()` there (`DataParallel(input_grad=True)`) instead.

    `param_grad=False`: the backward is data-only whatever `requires_grad` says -- no weight gradient is formed,
    no `GradBuckets` is created and no `p.grad` is touched or created; loss and gradient are bit-identical to `param_grad=True`'s.
    Every precision; a bf16 precision at latent width 128 or 256.

    `recompute=True`: FusedStep's -- the adjoint through a long rollout holds the blocks' inputs per step instead of
    their activations; loss and gradient keep their bits.

    `node_weights`: FusedStep's, for an `objective` with `node_weighted`."""
    from .dp import GradBuckets
    K = 1 if later_targets is None else int(later_targets.shape[0]) + 1
    objective = Objective() if objective is None else objective
    if not isinstance(recompute, bool):
        raise TypeError(f"input_gradient: recompute is a bool, got {type(recompute).__name__}")
    key = _input_gradient_key(K, step_weights, detach, objective, param_grad, recompute)
    cache = model.__dict__.setdefault("_bsms_input_grad_steps", {})
    step = cache.get(key)
    if step is None:
        if param_grad and "grads" not in cache:
            cache["grads"] = GradBuckets(list(model.parameters()))
        step = cache[key] = FusedStep(model, cache["grads"] if param_grad else None, unroll=K, step_weights=step_weights, detach=detach,
                                      objective=objective, input_grad=True, param_grad=bool(param_grad), recompute=recompute)
    loss = step(data, consistent, later_targets, node_weights=node_weights)
    return loss, step.input_grad().clone()
