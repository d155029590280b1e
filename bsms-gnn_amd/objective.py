"""The training objective: a family of masked losses around the reference's masked RMSE.

With d = fl32(pred - tar), M = sum m, SE_c = sum m d_c^2 (fp64), std_c the target normaliser's `std_with_epsilon()` and w the
channel weights (default 1):

    a_c  = w_c                  space = "physical"
    a_c  = w_c / std_c^2        space = "normalized"   (the squared error of the NORMALISED targets, as MeshGraphNets trains)
    Q    = sum_c a_c SE_c / (M C)
    loss = Q  (kind = "mse")   or   sqrt(Q)  (kind = "rmse")

`Objective()` -- physical, rmse, no weights -- is the reference's loss (trainer/trainer.py:96-97) and stays on the kernels it
always ran on; everything else goes through bsms_error_sums + bsms_sim_objective_bwd (step.FusedStep) or `masked_loss` (autograd).

`node_weighted=True`: every node carries a weight omega >= 0 -- the measure it represents (`lumped_node_measure`), or
any other importance -- and mu = m * omega takes the mask's place in M and SE_c: the discrete L2 norm of the error field instead of a
mean over the mesher's points.  The weights come with every batch (`node_weights=`); the step runs the `_w` entries of the two kernels.

The ROBUST kinds replace the square by a function that grows linearly: with s_c = 1 ("physical") or std_c
("normalized"), u_c = double(d_c) / s_c, mu = m or m * omega and S_c = sum mu rho(u_c) (fp64),

    rho(u) = |u|                                                     kind = "mae"
    rho(u) = u^2 / 2 if |u| <= delta_c, else delta_c (|u| - delta_c / 2)   kind = "huber"   (`delta` in the units of the space)
    loss   = sum_c w_c S_c / (M C)                                   no square root, and no 1 / std^2 on top of s_c

on bsms_robust_sums + bsms_sim_robust_bwd in the step.

The EDGE TERM: `edge_weight=lam` adds the edge-difference (discrete H1) term of 4.21 to a "mse" / "rmse" objective.  With
ME, DE_c the sums of `edge_difference_sums` over ALL samples of the batch (`edge_weighting`: "difference" or "quotient") and a_c the
coefficients above,

    H = sum_c a_c DE_c / (ME C)        T = H ("mse")  or  sqrt(H) ("rmse")        J = loss + lam T

on bsms_edge_diff_sums + bsms_edge_diff_fold + bsms_sim_edge_objective_bwd in the step."""
import math

import torch

SPACES = {"physical": 0, "normalized": 1}      # BSMS_LOSS_PHYSICAL / BSMS_LOSS_NORMALIZED
KINDS = {"rmse": 0, "mse": 1}                  # BSMS_LOSS_RMSE / BSMS_LOSS_MSE
ROBUST_KINDS = {"mae": 0, "huber": 1}          # BSMS_ROBUST_MAE / BSMS_ROBUST_HUBER


class Objective:
    """A value: `space`, `kind`, `channel_weights` (a tuple of floats or None), `node_weighted` (bool), `delta` (the Huber threshold:
    a float, a tuple of one float per channel, or None), `edge_weight` (lambda of the edge term: None or a finite float > 0) and
    `edge_weighting` ("difference" / "quotient").  Validated here; the number of weights and of thresholds is checked against
    a model's `out_dim` by `bind`."""

    __slots__ = ("space", "kind", "channel_weights", "node_weighted", "delta", "edge_weight", "edge_weighting")

    def __init__(self, space="physical", kind="rmse", channel_weights=None, node_weighted=False, *, delta=None, edge_weight=None,
                 edge_weighting="difference"):
        if space not in SPACES:
            raise ValueError(f"Objective: space must be one of {sorted(SPACES)}, got {space!r}")
        if not isinstance(kind, str) or (kind not in KINDS and kind not in ROBUST_KINDS):
            raise ValueError(f"Objective: kind must be one of {sorted(KINDS) + sorted(ROBUST_KINDS)}, got {kind!r}")
        if kind == "huber":
            if delta is None:
                raise ValueError('Objective: kind="huber" needs delta (a positive float, or one per channel)')
            if torch.is_tensor(delta):
                delta = delta.detach().reshape(-1).tolist() if delta.dim() else float(delta)
            try:
                if isinstance(delta, (bool, str)):
                    raise TypeError
                delta = tuple(float(x) for x in delta) if hasattr(delta, "__iter__") else float(delta)
            except (TypeError, ValueError):
                raise ValueError(f"Objective: delta must be a number or a sequence of numbers, got {delta!r}") from None
            each = (delta,) if isinstance(delta, float) else delta
            if not each or not all(math.isfinite(x) and x > 0.0 for x in each):
                raise ValueError(f"Objective: delta must be finite and > 0, got {delta}")
        elif delta is not None:
            raise ValueError(f'Objective: delta belongs to kind="huber", not to kind={kind!r}')
        if channel_weights is not None:
            if torch.is_tensor(channel_weights):
                channel_weights = channel_weights.detach().reshape(-1).tolist()
            try:
                channel_weights = tuple(float(w) for w in channel_weights)
            except TypeError:
                raise ValueError(f"Objective: channel_weights must be a sequence of numbers, got {channel_weights!r}") from None
            if not channel_weights:
                raise ValueError("Objective: channel_weights is empty")
            if not all(math.isfinite(w) and w >= 0.0 for w in channel_weights) or not any(w > 0.0 for w in channel_weights):
                raise ValueError(f"Objective: channel_weights must be finite, non-negative and not all zero, got {channel_weights}")
        object.__setattr__(self, "space", space)
        object.__setattr__(self, "kind", kind)
        object.__setattr__(self, "channel_weights", channel_weights)
        if not isinstance(node_weighted, bool):
            raise ValueError(f"Objective: node_weighted is a bool, got {node_weighted!r}")
        object.__setattr__(self, "node_weighted", node_weighted)
        object.__setattr__(self, "delta", delta)
        if edge_weighting not in EDGE_WEIGHTINGS:
            raise ValueError(f"Objective: edge_weighting must be one of {list(EDGE_WEIGHTINGS)}, got {edge_weighting!r}")
        if edge_weight is not None:
            if isinstance(edge_weight, (bool, str)) or not isinstance(edge_weight, (int, float)):
                raise ValueError(f"Objective: edge_weight must be None or a finite float > 0, got {edge_weight!r}")
            edge_weight = float(edge_weight)
            if not (math.isfinite(edge_weight) and edge_weight > 0.0):
                raise ValueError(f"Objective: edge_weight must be None or a finite float > 0, got {edge_weight}")
            if kind in ROBUST_KINDS:
                raise ValueError(f'Objective: the edge term goes with kind "mse" / "rmse", not with the robust kind {kind!r}')
            if node_weighted:
                raise ValueError("Objective: the edge term with node_weighted=True is not built (no node-weighted edge sums)")
        object.__setattr__(self, "edge_weight", edge_weight)
        object.__setattr__(self, "edge_weighting", edge_weighting)

    def __setattr__(self, name, value):
        raise AttributeError("Objective is immutable")

    @property
    def is_default(self):
        """True exactly for physical / rmse / no weights of either kind: the reference's loss, on the default route."""
        return (self.space == "physical" and self.kind == "rmse" and self.channel_weights is None and not self.node_weighted
                and self.edge_weight is None)

    @property
    def has_edge_term(self):
        """True with `edge_weight`: J = loss + edge_weight * T."""
        return self.edge_weight is not None

    @property
    def is_robust(self):
        """True for the kinds that are linear in their per-channel sums ("mae", "huber"): the route of bsms_robust_sums."""
        return self.kind in ROBUST_KINDS

    def bind(self, out_dim):
        """Check the objective against a model with `out_dim` output channels; returns self."""
        if self.channel_weights is not None and len(self.channel_weights) != int(out_dim):
            raise ValueError(f"Objective: {len(self.channel_weights)} channel_weights for a model with out_dim = {out_dim}")
        if isinstance(self.delta, tuple) and len(self.delta) != int(out_dim):
            raise ValueError(f"Objective: {len(self.delta)} values of delta for a model with out_dim = {out_dim}")
        return self

    @classmethod
    def from_cfg(cls, cfg):
        """From the optional `loss_space`, `loss_kind`, `loss_channel_weights`, `loss_node_weights`, `loss_delta`, `loss_edge_weight`,
        `loss_edge_weighting` of a model config; absent keys give the default."""
        w = getattr(cfg, "loss_channel_weights", None)
        nw = getattr(cfg, "loss_node_weights", None)
        dl = getattr(cfg, "loss_delta", None)
        return cls(getattr(cfg, "loss_space", None) or "physical", getattr(cfg, "loss_kind", None) or "rmse",
                   None if w is None else list(w), False if nw is None else nw,
                   delta=dl if dl is None or isinstance(dl, (int, float)) else list(dl),
                   edge_weight=getattr(cfg, "loss_edge_weight", None),
                   edge_weighting=getattr(cfg, "loss_edge_weighting", None) or "difference")

    def weights_tensor(self, device):
        """fp64 [C] on `device`, or None for unit weights."""
        return None if self.channel_weights is None else torch.tensor(self.channel_weights, dtype=torch.float64, device=device)

    def delta_tensor(self, C, device):
        """fp64 [C] on `device` (a scalar delta repeated), or None for every kind but "huber"."""
        if self.delta is None:
            return None
        each = (self.delta,) * int(C) if isinstance(self.delta, float) else self.delta
        return torch.tensor(each, dtype=torch.float64, device=device)

    def scales(self, std, C, device):
        """s_c of the robust kinds, fp64 [C]: ones in the physical space, the target normaliser's std in the normalized one."""
        if self.space == "physical":
            return torch.ones(C, dtype=torch.float64, device=device)
        if std is None:
            raise ValueError("Objective: the normalized space needs the target normaliser's std_with_epsilon()")
        return std.to(device=device, dtype=torch.float64).reshape(-1)

    def coefficients(self, std, C, device):
        """a_c, fp64 [C] (the robust kinds: w_c alone -- their scaling is inside S_c)."""
        a = torch.ones(C, dtype=torch.float64, device=device) if self.channel_weights is None else self.weights_tensor(device)
        if self.space == "normalized" and not self.is_robust:
            if std is None:
                raise ValueError("Objective: the normalized space needs the target normaliser's std_with_epsilon()")
            a = a / std.to(device=device, dtype=torch.float64).reshape(-1) ** 2
        return a

    def _key(self):
        return (self.space, self.kind, self.channel_weights, self.node_weighted, self.delta, self.edge_weight, self.edge_weighting)

    def __eq__(self, other):
        return isinstance(other, Objective) and self._key() == other._key()

    def __hash__(self):
        return hash(self._key())

    def __repr__(self):
        tail = ", node_weighted=True" if self.node_weighted else ""
        if self.delta is not None:
            tail += f", delta={self.delta}"
        if self.edge_weight is not None:
            tail += f", edge_weight={self.edge_weight}, edge_weighting={self.edge_weighting!r}"
        return f"Objective(space={self.space!r}, kind={self.kind!r}, channel_weights={self.channel_weights}{tail})"

    def check_node_weights(self, node_weights):
        """The pairing rule of every interface that takes `node_weights=`: a node-weighted objective needs them, any other refuses
        them (ValueError); then `validate_node_weights`.  Returns the weights (or None)."""
        if self.node_weighted and node_weights is None:
            raise ValueError("Objective: node_weighted is set but no node_weights were given")
        if node_weights is not None and not self.node_weighted:
            raise ValueError("Objective: node_weights were given to an objective without node_weighted=True")
        return None if node_weights is None else validate_node_weights(node_weights)


def validate_node_weights(w):
    """Node weights are a float32 tensor, finite and >= 0.  The values are looked at where the tensor lives on the host; a device
    tensor is never read back (what it holds shows in the sums)."""
    if not torch.is_tensor(w) or w.dtype != torch.float32:
        raise ValueError(f"node_weights must be a float32 tensor, got {w.dtype if torch.is_tensor(w) else type(w).__name__}")
    if not w.is_cuda and w.numel() and not bool((torch.isfinite(w) & (w >= 0)).all()):
        raise ValueError("node_weights must be finite and >= 0")
    return w


def channel_sums(pred, tar, mask, node_weights=None):
    """(M, SE[C]) in fp64 from fp32 tensors [..., C] and a mask broadcastable to [..., 1]: d is rounded to fp32 once, products and
    sums are fp64 -- the M and SE fields of bsms_error_sums, differentiable in `pred`.  `node_weights` (broadcastable to [..., 1]):
    mu = double(mask) * double(weight) takes the mask's place -- the fields of bsms_error_sums_w."""
    C = pred.shape[-1]
    d = (pred - tar).double()
    m = mask.double().reshape(*pred.shape[:-1], 1)
    if node_weights is not None:
        w = node_weights.double()
        m = m * (w.reshape(*w.shape, 1) if w.dim() < pred.dim() else w)     # [N] / [B, N] / [..., 1] against [..., 1]
    return m.sum(), (m * d * d).reshape(-1, C).sum(0)


def robust_sums(pred, tar, mask, objective, std=None, node_weights=None):
    """(M, S[C]) of a robust objective in fp64 -- the row of bsms_robust_sums, differentiable in `pred`: d is rounded to fp32 once
    (as `channel_sums`), u = double(d) / s_c, S_c = sum mu rho(u_c)."""
    C = pred.shape[-1]
    u = (pred - tar).double() / objective.scales(std, C, pred.device)
    m = mask.double().reshape(*pred.shape[:-1], 1)
    if node_weights is not None:
        w = node_weights.double()
        m = m * (w.reshape(*w.shape, 1) if w.dim() < pred.dim() else w)
    au = u.abs()
    if objective.kind == "huber":
        dl = objective.delta_tensor(C, pred.device)
        rho = torch.where(au <= dl, 0.5 * (u * u), dl * (au - 0.5 * dl))
    else:
        rho = au                                            # autograd's sign(0) is 0
    return m.sum(), (m * rho).reshape(-1, C).sum(0)


def finish_loss(M, SE, objective, std):
    """loss (fp32 scalar) and the per-channel terms a_c SE_c / (M C) (fp64 [C]) from the sums.  The robust kinds take their S_c in
    SE's place: the coefficients are w_c alone and there is no square root."""
    C = SE.shape[0]
    terms = objective.coefficients(std, C, SE.device) * SE / (M * C)
    Q = terms.sum()
    return (torch.sqrt(Q) if objective.kind == "rmse" else Q).float(), terms


def edge_term(sums, objective, std, C=None):
    """T (fp64 scalar) from the rows [ME | DE | ..] of `edge_difference_sums` over all samples: H = sum_c a_c DE_c / (ME C), T = H
    ("mse") or sqrt(H) ("rmse").  `C`: the channels, for rows that are not [ME | DE | TE] (dp.global_masked_loss: one row [ME | DE])."""
    C = (sums.shape[-1] - 1) // 2 if C is None else int(C)
    a = objective.coefficients(std, C, sums.device)
    H = (a * sums[:, 1:1 + C].sum(0) / (sums[:, 0].sum() * C)).sum()
    return torch.sqrt(H) if objective.kind == "rmse" else H


def masked_loss(pred, tar, mask, objective=None, std=None, node_weights=None, g=None, pos=None):
    """The objective in torch.  `std`: the target normaliser's `std_with_epsilon()` (needed for space = "normalized").  The default
    objective is `model.masked_rmse`, bit for bit.  `node_weights`: required by a node-weighted objective, refused by any other.
    `g` [2, E] (required by an objective with an edge term: the edge list the samples share, or that of a variable-mesh union) and
    `pos` ([N, p] or [B, N, p]; required by edge_weighting = "quotient"): J = loss + edge_weight * T, formed in fp64 and rounded once;
    the sums are `edge_difference_sums` on CPU tensors and bsms_edge_diff_sums / bsms_edge_diff_bwd on GPU tensors."""
    if objective is None:
        if node_weights is not None:
            raise ValueError("masked_loss: node_weights need an Objective(node_weighted=True)")
    else:
        node_weights = objective.check_node_weights(node_weights)
    if objective is None or objective.is_default:
        from .model import masked_rmse
        return masked_rmse(pred, tar, mask)
    objective.bind(pred.shape[-1])
    if objective.is_robust:
        M, SE = robust_sums(pred, tar, mask, objective, std, node_weights)
    else:
        M, SE = channel_sums(pred, tar, mask, node_weights)
    if not objective.has_edge_term:
        return finish_loss(M, SE, objective, std)[0]
    if g is None:
        raise ValueError("masked_loss: an objective with an edge term needs g (the [2, E] edge list)")
    if objective.edge_weighting == "quotient" and pos is None:
        raise ValueError('masked_loss: edge_weighting="quotient" needs pos')
    C = SE.shape[0]
    Q = (objective.coefficients(std, C, SE.device) * SE / (M * C)).sum()
    L = torch.sqrt(Q) if objective.kind == "rmse" else Q
    T = edge_term(_edge_sums_any(pred, tar, mask, g, pos, objective.edge_weighting), objective, std)
    return (L + objective.edge_weight * T).float()


# ------------------------------------------------------------------------------------ edge differences
EDGE_WEIGHTINGS = ("difference", "quotient")   # BSMS_EDGE_DIFFERENCE / BSMS_EDGE_QUOTIENT


def _edge_operands(pred, tar, mask, pos, weighting):
    """pred / tar as [S, N, C], mask as [S or 1, N], pos as [S or 1, N, p] or None -- views, nothing is copied."""
    if weighting not in EDGE_WEIGHTINGS:
        raise ValueError(f"edge differences: weighting must be one of {list(EDGE_WEIGHTINGS)}, got {weighting!r}")
    if pred.dim() not in (2, 3) or tar.shape != pred.shape:
        raise ValueError(f"edge differences: pred and tar [B, N, C] or [R, C] expected, got {tuple(pred.shape)} and {tuple(tar.shape)}")
    N, C = int(pred.shape[-2]), int(pred.shape[-1])
    if mask.numel() % max(N, 1) or (N and mask.numel() // N not in (1, pred.numel() // max(N * C, 1))):
        raise ValueError(f"edge differences: a mask of shape {tuple(mask.shape)} does not cover {tuple(pred.shape[:-1])} nodes")
    if weighting == "quotient":
        if pos is None:
            raise ValueError('edge differences: weighting="quotient" needs pos')
        if pos.dim() not in (2, 3) or int(pos.shape[-2]) != N or (pos.dim() == 3 and (pred.dim() != 3 or pos.shape[0] != pred.shape[0])):
            raise ValueError(f"edge differences: pos [N, p] or [B, N, p] expected for pred {tuple(pred.shape)}, got {tuple(pos.shape)}")
        pos = pos.reshape(-1, N, pos.shape[-1])
    else:
        pos = None
    return pred.reshape(-1, N, C), tar.reshape(-1, N, C), mask.reshape(-1, N), pos


def edge_difference_sums(pred, tar, mask, g, pos=None, weighting="difference"):
    """The edge-difference sums in torch, on any device: fp64 [S, 1+2C] = [ME | DE | TE] per sample -- the row of bsms_edge_diff_sums,
    differentiable in `pred` (and in `tar` and `pos`).  `pred` / `tar` are [B, N, C] with ONE edge list `g` [2, E] shared by the
    samples, or [R, C] (one segment: the rows of a variable-mesh union with its edge list); `mask` covers the nodes of every sample or
    of one, shared; `pos` is [N, p] or [B, N, p].  Over the directed edges e = (g[0, e] -> g[1, e]) -- a mesh edge listed in both
    directions counts twice --

        mu_e = m_i m_j        w_e = 1 ("difference")   or   1 / |x_i - x_j|^2 ("quotient"; an edge of length 0 has mu_e = w_e = 0)
        ME = sum mu_e         DE_c = sum mu_e w_e (d_ic - d_jc)^2         TE_c = sum mu_e w_e (t_ic - t_jc)^2

    with d = pred - tar rounded once in the tensors' own precision (fp32 tensors: the one fp32 rounding of the kernel) and every
    product and sum after it in fp64."""
    pred, tar, mask, pos = _edge_operands(pred, tar, mask, pos, weighting)
    i, j = g[0].long(), g[1].long()
    d, t, m = (pred - tar).double(), tar.double(), mask.double()
    mu = m[:, i] * m[:, j]                                              # [S or 1, E]
    w = torch.ones_like(mu)
    if pos is not None:
        x = pos.double()
        l2 = ((x[:, i] - x[:, j]) ** 2).sum(-1)
        flat = l2 == 0
        w = torch.where(flat, torch.zeros_like(l2), 1.0 / torch.where(flat, torch.ones_like(l2), l2))
        mu = torch.where(flat, torch.zeros_like(l2), mu)                # broadcasts a shared mask / shared positions
    mw = (mu * w).unsqueeze(-1)
    DE = (mw * (d[:, i] - d[:, j]) ** 2).sum(1)
    TE = (mw * (t[:, i] - t[:, j]) ** 2).sum(1)
    ME = mu.sum(1, keepdim=True).expand(DE.shape[0], 1)
    return torch.cat([ME, DE, TE], dim=1)


class _EdgeDiffSums(torch.autograd.Function):
    """bsms_edge_diff_sums forward, bsms_edge_diff_bwd backward: the gradient of sum_{s,c} G[s, 1 + c] DE[s, c] with respect to pred
    (G the incoming gradient of the sums, already on the device: nothing is read back).  ME and TE do not depend on pred."""

    @staticmethod
    def forward(ctx, pred, tar, mask, pos, plan, weighting):
        from . import ops
        ctx.save_for_backward(pred, tar, mask, *(() if pos is None else (pos,)))
        ctx.plan, ctx.weighting = plan, weighting
        return ops.edge_diff_sums(pred, tar, mask, plan, pos=pos, weighting=weighting, row0=0, seg_rows=pred.shape[1])

    @staticmethod
    def backward(ctx, grad_sums):
        from . import ops
        pred, tar, mask, *rest = ctx.saved_tensors
        C = pred.shape[-1]
        coef = grad_sums[:, 1:1 + C].to(torch.float64).contiguous()
        grad = ops.edge_diff_bwd(pred, tar, mask, ctx.plan, coef, pos=rest[0] if rest else None, weighting=ctx.weighting, row0=0,
                                 seg_rows=pred.shape[1])
        return grad, None, None, None, None, None


def _edge_sums_any(pred, tar, mask, g, pos, weighting):
    """[S, 1+2C] fp64, differentiable in `pred`: the torch definition on CPU tensors, the two kernels on GPU tensors."""
    if not pred.is_cuda:
        return edge_difference_sums(pred, tar, mask, g, pos, weighting)
    from .graph import plan_for
    p3, t3, m2, x3 = _edge_operands(pred, tar, mask, pos, weighting)
    m2 = m2.contiguous()
    return _EdgeDiffSums.apply(p3.contiguous(), t3.contiguous(), m2 if m2.shape[0] == p3.shape[0] else m2[0],
                               None if x3 is None else (x3.contiguous() if x3.shape[0] == p3.shape[0] else x3[0].contiguous()),
                               plan_for(g, p3.shape[1]), weighting)


def edge_difference_loss(pred, tar, mask, g, pos=None, *, weighting="difference", space="physical", kind="mse", channel_weights=None,
                         std=None):
    """The edge-difference (discrete H1) loss term, an fp32 scalar:

        H = sum_c a_c DE_c / (ME C)          term = H (kind = "mse")   or   sqrt(H) (kind = "rmse")

    with DE and ME the sums of `edge_difference_sums` over all samples and a_c exactly the coefficients of `Objective`: w_c in the
    physical space, w_c / std_c^2 in the normalized one (`std`: the target normaliser's `std_with_epsilon()`).  Shapes as
    `edge_difference_sums` takes them.  On GPU tensors the sums are bsms_edge_diff_sums and the gradient with respect to `pred` is
    bsms_edge_diff_bwd, with the coefficients k_c = g_out a_c / (ME C) ("mse") or g_out a_c / (2 term ME C) ("rmse") formed by fp64
    torch ops on the device; `tar`, `mask` and `pos` get no gradient there.  On CPU tensors it is the torch definition.  Use it next
    to the training objective: `loss = trainer.get_loss(data) + lam * edge_difference_loss(pred, tar, mask, g)`."""
    if kind not in KINDS:
        raise ValueError(f"edge_difference_loss: kind must be one of {sorted(KINDS)}, got {kind!r}")
    objective = Objective(space, kind, channel_weights).bind(pred.shape[-1])
    for what, t in (("tar", tar), ("mask", mask), ("g", g)) + ((("pos", pos),) if pos is not None and weighting == "quotient" else ()):
        if t.device != pred.device:
            raise RuntimeError(f"edge_difference_loss: {what} lives on {t.device}, pred on {pred.device}")
    C = int(pred.shape[-1])
    sums = _edge_sums_any(pred, tar, mask, g, pos, weighting)
    a = objective.coefficients(std, C, pred.device)
    H = (a * sums[:, 1:1 + C].sum(0)).sum() / (sums[:, 0].sum() * C)
    return (torch.sqrt(H) if kind == "rmse" else H).float()
