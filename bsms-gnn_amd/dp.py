"""Data parallelism for the BSMS path: one process per GPU, full model replica, the batch of
independent meshes sharded across ranks.  Collectives go through
torch.distributed (backend "nccl" = RCCL over xGMI on ROCm; "gloo" for the CPU tests):

  * gradients: ONE flat fp32 buffer (7.7 MB for the airfoil model) whose slices are the parameters'
    `.grad`; it is cut into a few large buckets that are all-reduced (SUM) asynchronously as soon
    as backward has produced every gradient in the bucket, so the ring transfer hides behind the rest of
    backward.  xGMI is point-to-point and a ring all-reduce is bound by one link, hence few, large
    messages rather than per-parameter ones.
  * loss: the masked RMSE (trainer/trainer.py:96-97) is non-linear in the batch, so the two global
    sums (sum se*mask, sum mask) are all-reduced BEFORE backward; local gradients are then exact
    partial derivatives of the global loss and are summed, not averaged.
  * the reference replaced nothing here: it wraps nn.DataParallel (trainer/trainer.py:15-18) and then
    disables it (train.py:16); Normalizer.synchronize is dead code (normalizer.py:92-114).
"""
import torch
import torch.distributed as dist


class GradBuckets:
    """Flat fp32 gradient buffer cut into a few large buckets.  Every parameter owns a slot; the engine's
    backward kernels write weight gradients directly into the slots (ops._grad_targets), gradients that
    arrive from plain autograd are copied in by the hook.  A bucket is all-reduced as soon as all of its
    parameters have their gradient."""

    def __init__(self, params, bucket_bytes=2 << 20, group=None, overlap=True):
        self.group = group
        self.overlap = overlap   # False: every bucket is reduced in finish() (after backward)
        params = list(params)
        self.params = [p for p in params if p.requires_grad]
        order = list(reversed(self.params))  # roughly the order backward produces them
        total = sum(p.numel() for p in order)
        ref = order[0] if order else (params[0] if params else torch.zeros(0))      # nothing trainable: an empty buffer (a data-only step)
        dev, dt = ref.device, ref.dtype
        self.flat = torch.zeros(total, device=dev, dtype=dt)
        self.buckets, self._bucket_of, self._slot = [], {}, {}
        off, start, cur = 0, 0, []
        for p in order:
            n = p.numel()
            self._slot[p] = (off, n)
            p._bsms_grad_slot = (self.flat, off, n)
            p._bsms_slot_used = False
            p.grad = None
            cur.append(p)
            off += n
            if (off - start) * self.flat.element_size() >= bucket_bytes:
                self._close(start, off, cur)
                start, cur = off, []
        if cur:
            self._close(start, off, cur)
        self._pending, self._handles = [len(b["params"]) for b in self.buckets], []
        self._seen, self._launched = set(), set()
        for p in self.params:
            p.register_post_accumulate_grad_hook(self._on_grad)

    def _close(self, start, end, plist):
        idx = len(self.buckets)
        self.buckets.append({"view": self.flat[start:end], "params": list(plist)})
        for p in plist:
            self._bucket_of[p] = idx

    def _on_grad(self, p):
        off, n = self._slot[p]
        if p.grad.data_ptr() != self.flat.data_ptr() + off * self.flat.element_size():
            view = self.flat[off:off + n].view_as(p)   # gradient produced outside the engine: move it in
            view.copy_(p.grad)
            p.grad = view
        b = self._bucket_of[p]
        if p in self._seen:
            # second gradient of the same parameter in one backward (a module used twice, accumulation without zero()):
            # the early reduction of its bucket would miss it -- such a bucket is reduced in finish() instead
            if b in self._launched:
                raise RuntimeError("GradBuckets: a parameter received a second gradient after its bucket was all-reduced; "
                                   "call zero() between backward passes or disable bucket overlap")
            self._pending[b] = -1
            return
        self._seen.add(p)
        if self._pending[b] < 0:
            return
        self._pending[b] -= 1
        if self._pending[b] == 0 and self._world() > 1 and self.overlap:
            self._launched.add(b)
            self._handles.append(dist.all_reduce(self.buckets[b]["view"], op=dist.ReduceOp.SUM, group=self.group, async_op=True))

    def _world(self):
        return dist.get_world_size(self.group) if dist.is_available() and dist.is_initialized() else 1

    def zero(self):
        self.flat.zero_()
        for p in self.params:
            p.grad = None
            p._bsms_slot_used = False
        self._pending = [len(b["params"]) for b in self.buckets]
        self._seen.clear()
        self._launched.clear()

    def finish(self):
        """Wait for the in-flight bucket reductions (call after backward)."""
        if self._world() > 1:
            for b, left in enumerate(self._pending):  # buckets not reduced during backward (missing / repeated gradients)
                if b not in self._launched:
                    self._launched.add(b)
                    self._handles.append(dist.all_reduce(self.buckets[b]["view"], op=dist.ReduceOp.SUM, group=self.group, async_op=True))
        for h in self._handles:
            h.wait()
        self._handles = []

    def clip_(self, max_norm):
        """Global-norm clip on the reduced buffer (identical on every rank; trainer/trainer.py:151)."""
        total = torch.linalg.vector_norm(self.flat)
        self.flat.mul_(torch.clamp(max_norm / (total + 1e-6), max=1.0))
        return total


def global_masked_rmse(pred, tar, mask, group=None):
    """sqrt(sum_global(se*mask) / sum_global(mask) / C): value identical on all ranks, gradient flows
    through the local part only (sum over ranks of these local gradients = gradient of the global loss)."""
    se = (pred - tar) ** 2
    s_loc, m_loc = (se * mask).sum(), mask.sum()
    if dist.is_available() and dist.is_initialized() and dist.get_world_size(group) > 1:
        tot = torch.stack([s_loc.detach(), m_loc.detach()])
        dist.all_reduce(tot, op=dist.ReduceOp.SUM, group=group)
        s = s_loc + (tot[0] - s_loc.detach())
        m = tot[1]
    else:
        s, m = s_loc, m_loc
    return torch.sqrt(s / m / se.shape[-1])


def global_masked_loss(pred, tar, mask, objective, std, group=None, node_weights=None, g=None, pos=None):
    """objective.masked_loss under data parallelism: the 1 + C fp64 sums (M, SE_c) -- (M, S_c) of a robust objective -- are all-reduced, the value is identical on all
    ranks and the gradient flows through the local part only, as in global_masked_rmse (which the default objective is).  With an
    edge term (`g`, `pos` as `masked_loss` takes them) the 1 + C sums (ME, DE_c) travel in the same message."""
    from .objective import _edge_sums_any, channel_sums, edge_term, finish_loss, robust_sums
    if objective is None or objective.is_default:
        return global_masked_rmse(pred, tar, mask, group)
    objective.bind(pred.shape[-1])
    if objective.is_robust:                   # (M, S_c) in (M, SE_c)'s place: the loss is linear in them
        M, SE = robust_sums(pred, tar, mask, objective, std, objective.check_node_weights(node_weights))
    else:
        M, SE = channel_sums(pred, tar, mask, objective.check_node_weights(node_weights))
    C, ME, DE = SE.shape[0], None, None
    if objective.has_edge_term:
        if g is None or (pos is None and objective.edge_weighting == "quotient"):
            raise ValueError("global_masked_loss: an objective with an edge term needs g (and pos for the quotient weighting)")
        es = _edge_sums_any(pred, tar, mask, g, pos, objective.edge_weighting)
        ME, DE = es[:, 0].sum(), es[:, 1:1 + C].sum(0)
    if dist.is_available() and dist.is_initialized() and dist.get_world_size(group) > 1:
        tot = torch.cat([M.detach().reshape(1), SE.detach(), *(() if ME is None else (ME.detach().reshape(1), DE.detach()))])
        dist.all_reduce(tot, op=dist.ReduceOp.SUM, group=group)
        M, SE = tot[0], SE + (tot[1:1 + C] - SE.detach())
        if ME is not None:
            ME, DE = tot[1 + C], DE + (tot[2 + C:] - DE.detach())
    if ME is None:
        return finish_loss(M, SE, objective, std)[0]
    Q = (objective.coefficients(std, C, SE.device) * SE / (M * C)).sum()              # J as masked_loss forms it: fp64, rounded once
    L = torch.sqrt(Q) if objective.kind == "rmse" else Q
    T = edge_term(torch.cat([ME.reshape(1), DE]).reshape(1, 1 + C), objective, std, C)
    return (L + objective.edge_weight * T).float()


class DataParallel:
    """Wraps a replica: broadcast of parameters at construction, bucketed gradient all-reduce."""

    def __init__(self, model, bucket_bytes=2 << 20, group=None, unroll=1, step_weights=None, detach=False, objective=None,
                 input_grad=False, accumulate=1, reduction="batch", recompute=False):
        """`recompute` (step.FusedStep): activation recomputation in the U-Net's backward -- the same gradients, bit for
        bit, from a fraction of the memory per (unrolled) step.  Only the fused step implements it.
        `accumulate` > 1, `reduction` (step.FusedStep; refused there with an edge term): every `step_loss_backward` is one micro-batch; the loss sums
        are all-reduced per micro-batch, the flat gradient buffer once, after the last fold of the cycle (`fused.ready`).  Only the
        fused step implements it.
        `unroll` > 1: the loss runs over that many autoregressive steps (step.FusedStep; `step_weights` default 1/unroll,
        `detach` cuts the gradient between the steps).  Only the fused step implements it.
        `objective` (objective.Objective): None reads the optional loss_space / loss_kind / loss_delta / loss_channel_weights of `model.cfg`;
        without them it is the reference's masked RMSE.
        `input_grad`: the fused step also forms the gradient of the loss w.r.t. `node_in` (`engine.fused.input_grad()`, DESIGN.md
        4.12) -- local to this rank's samples, no collective; only the fused step implements it.
        Frozen parameters: freeze whole MLPs with requires_grad_(False) BEFORE constructing this.  A model with
        nothing trainable is a data-only step and needs `input_grad=True`: without it the constructor raises ValueError."""
        from .objective import Objective
        self.model, self.group, self.unroll = model, group, int(unroll)
        if objective is None:
            objective = Objective.from_cfg(getattr(model, "cfg", None))
        out_dim = getattr(getattr(model, "cfg", None), "out_dim", None)
        self.objective = objective if out_dim is None else objective.bind(out_dim)
        if dist.is_available() and dist.is_initialized() and dist.get_world_size(group) > 1:
            for t in list(model.parameters()) + list(model.buffers()):
                dist.broadcast(t.data, src=0, group=group)
        # The U-Net stays ONE bsms_bsgmp_fwd / _bwd call per step under data parallelism too: eight ranks share one
        # host, and the per-block module tree costs every rank ~3x the enqueue time to buy an overlap worth < 3 % (the
        # whole gradient is 7.7 MB: ~0.1-0.2 ms of ring all-reduce over xGMI against a 6-7 ms step).  Buckets complete
        # as autograd hands the gradients over (decoder first, then the whole U-Net, then the encoder) and are
        # all-reduced asynchronously from there.  A model built with BSGMP.per_block = True (BSMS_PY_BSGMP=1) still
        # gets block-by-block overlap.
        self.grads = GradBuckets(list(model.parameters()), bucket_bytes, group)
        # The step itself: direct C-ABI calls on static buffers (step.FusedStep) when the model is the standard
        # BSMS_Simulator; otherwise (or with BSMS_FUSED_STEP=0) autograd over the drop-in modules.
        import os
        from .step import FusedStep
        self.fused = None
        if os.environ.get("BSMS_FUSED_STEP", "1") == "1" and FusedStep.supports(model) and next(model.parameters()).is_cuda:
            self.fused = FusedStep(model, self.grads, group, use_graph=os.environ.get("BSMS_STEP_GRAPH", "0") == "1",   # with unroll > 1: ValueError
                                   unroll=self.unroll, step_weights=step_weights, detach=detach, objective=self.objective,
                                   input_grad=input_grad, accumulate=accumulate, reduction=reduction, recompute=recompute)
        elif not isinstance(input_grad, bool):
            raise TypeError(f"DataParallel: input_grad is a bool, got {type(input_grad).__name__}")
        elif not isinstance(recompute, bool):
            raise TypeError(f"DataParallel: recompute is a bool, got {type(recompute).__name__}")
        if recompute and self.fused is None:
            raise ValueError("DataParallel: recompute needs the fused step (a standard BSMS_Simulator on the GPU, BSMS_FUSED_STEP != 0)")
        if self.fused is None and (isinstance(accumulate, bool) or int(accumulate) != accumulate or int(accumulate) < 1):
            raise ValueError(f"DataParallel: accumulate must be an integer >= 1, got {accumulate!r}")
        if self.fused is None and int(accumulate) > 1:
            raise ValueError("DataParallel: accumulate > 1 needs the fused step (a standard BSMS_Simulator on the GPU, BSMS_FUSED_STEP != 0)")
        if input_grad and self.fused is None:
            raise ValueError("DataParallel: input_grad needs the fused step (a standard BSMS_Simulator on the GPU, BSMS_FUSED_STEP != 0)")
        if self.unroll > 1 and self.fused is None:
            raise ValueError("DataParallel: unroll > 1 needs the fused step (a standard BSMS_Simulator on the GPU, BSMS_FUSED_STEP != 0)")

    def __call__(self, *a, **k):
        return self.model(*a, **k)

    def step_loss_backward(self, data, consistent_mesh=True, later_targets=None, node_weights=None):
        """One fwd + exact global loss + bwd + gradient reduction.  Returns the (global) loss.  `later_targets`: the targets
        of steps 1 .. unroll-1 of an unrolled loss (step.FusedStep.__call__).  `node_weights`: this rank's node weights for an
        objective with `node_weighted`: required with it, refused without."""
        node_weights = self.objective.check_node_weights(node_weights)
        if self.fused is not None:
            kw = {} if node_weights is None else dict(node_weights=node_weights)
            return self.fused(data, consistent_mesh, **kw) if later_targets is None else self.fused(data, consistent_mesh, later_targets, **kw)
        if later_targets is not None:
            raise ValueError("DataParallel: later_targets need the fused step")
        self.grads.zero()
        pred = self.model(data, consistent_mesh, False)
        tar = data[1] if consistent_mesh else data[0].y.unsqueeze(0)
        mask = data[2] if consistent_mesh else data[0].mask.unsqueeze(0)
        if self.objective.is_default:
            loss = global_masked_rmse(pred, tar, mask, self.group)
        else:
            if node_weights is not None:
                node_weights = node_weights.to(pred.device)
            g = pos = None
            if self.objective.has_edge_term:          # the level-0 edge list and the position columns of node_in
                node_in, g = (data[0], data[3][0][0]) if consistent_mesh else (data[0].x, data[0].edge_index)
                pos = node_in[..., pred.shape[-1]:-1]
            loss = global_masked_loss(pred, tar, mask, self.objective, self.model._targetNormalizer.std_with_epsilon(), self.group,
                                      node_weights=node_weights, g=g, pos=pos)
        loss.backward()
        self.grads.finish()
        return loss

    def normalizers(self):
        return [m for m in self.model.modules() if hasattr(m, "synchronize") and hasattr(m, "_E_data")]

    def sync_normalizers(self, base=None):
        """`base`: {normaliser: snapshot} of statistics all ranks already share (Trainer.restore before more warm-up)."""
        for m in self.normalizers():
            m.synchronize(self.group, None if base is None else base.get(m))
