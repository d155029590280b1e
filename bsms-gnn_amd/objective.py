"""The training objective: a family of masked losses around the reference's masked RMSE.

With d = fl32(pred - tar), M = sum m, SE_c = sum m d_c^2 (fp64), std_c the target normaliser's `std_with_epsilon()` and w the
channel weights (default 1):

    a_c  = w_c                  space = "physical"
    a_c  = w_c / std_c^2        space = "normalized"   (the squared error of the NORMALISED targets, as MeshGraphNets trains)
    Q    = sum_c a_c SE_c / (M C)
    loss = Q  (kind = "mse")   or   sqrt(Q)  (kind = "rmse")

`Objective()` -- physical, rmse, no weights -- is the reference's loss (trainer/trainer.py:96-97) and stays on the kernels it
always ran on; everything else goes through bsms_error_sums + bsms_sim_objective_bwd (step.FusedStep) or `masked_loss` (autograd)."""
import math

import torch

SPACES = {"physical": 0, "normalized": 1}      # BSMS_LOSS_PHYSICAL / BSMS_LOSS_NORMALIZED
KINDS = {"rmse": 0, "mse": 1}                  # BSMS_LOSS_RMSE / BSMS_LOSS_MSE


class Objective:
    """A value: `space`, `kind`, `channel_weights` (a tuple of floats or None).  Validated here; the number of weights is checked
    against a model's `out_dim` by `bind`."""

    __slots__ = ("space", "kind", "channel_weights")

    def __init__(self, space="physical", kind="rmse", channel_weights=None):
        if space not in SPACES:
            raise ValueError(f"Objective: space must be one of {sorted(SPACES)}, got {space!r}")
        if kind not in KINDS:
            raise ValueError(f"Objective: kind must be one of {sorted(KINDS)}, got {kind!r}")
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

    def __setattr__(self, name, value):
        raise AttributeError("Objective is immutable")

    @property
    def is_default(self):
        """True exactly for physical / rmse / no weights: the reference's loss, on the default route."""
        return self.space == "physical" and self.kind == "rmse" and self.channel_weights is None

    def bind(self, out_dim):
        """Check the objective against a model with `out_dim` output channels; returns self."""
        if self.channel_weights is not None and len(self.channel_weights) != int(out_dim):
            raise ValueError(f"Objective: {len(self.channel_weights)} channel_weights for a model with out_dim = {out_dim}")
        return self

    @classmethod
    def from_cfg(cls, cfg):
        """From the optional `loss_space`, `loss_kind`, `loss_channel_weights` of a model config; absent keys give the default."""
        w = getattr(cfg, "loss_channel_weights", None)
        return cls(getattr(cfg, "loss_space", None) or "physical", getattr(cfg, "loss_kind", None) or "rmse",
                   None if w is None else list(w))

    def weights_tensor(self, device):
        """fp64 [C] on `device`, or None for unit weights."""
        return None if self.channel_weights is None else torch.tensor(self.channel_weights, dtype=torch.float64, device=device)

    def coefficients(self, std, C, device):
        """a_c, fp64 [C]."""
        a = torch.ones(C, dtype=torch.float64, device=device) if self.channel_weights is None else self.weights_tensor(device)
        if self.space == "normalized":
            if std is None:
                raise ValueError("Objective: the normalized space needs the target normaliser's std_with_epsilon()")
            a = a / std.to(device=device, dtype=torch.float64).reshape(-1) ** 2
        return a

    def __eq__(self, other):
        return isinstance(other, Objective) and (self.space, self.kind, self.channel_weights) == (other.space, other.kind, other.channel_weights)

    def __hash__(self):
        return hash((self.space, self.kind, self.channel_weights))

    def __repr__(self):
        return f"Objective(space={self.space!r}, kind={self.kind!r}, channel_weights={self.channel_weights})"


def channel_sums(pred, tar, mask):
    """(M, SE[C]) in fp64 from fp32 tensors [..., C] and a mask broadcastable to [..., 1]: d is rounded to fp32 once, products and
    sums are fp64 -- the M and SE fields of bsms_error_sums, differentiable in `pred`."""
    C = pred.shape[-1]
    d = (pred - tar).double()
    m = mask.double().reshape(*pred.shape[:-1], 1)
    return m.sum(), (m * d * d).reshape(-1, C).sum(0)


def finish_loss(M, SE, objective, std):
    """loss (fp32 scalar) and the per-channel terms a_c SE_c / (M C) (fp64 [C]) from the sums."""
    C = SE.shape[0]
    terms = objective.coefficients(std, C, SE.device) * SE / (M * C)
    Q = terms.sum()
    return (Q if objective.kind == "mse" else torch.sqrt(Q)).float(), terms


def masked_loss(pred, tar, mask, objective=None, std=None):
    """The objective in torch.  `std`: the target normaliser's `std_with_epsilon()` (needed for space = "normalized").  The default
    objective is `model.masked_rmse`, bit for bit."""
    if objective is None or objective.is_default:
        from .model import masked_rmse
        return masked_rmse(pred, tar, mask)
    objective.bind(pred.shape[-1])
    M, SE = channel_sums(pred, tar, mask)
    return finish_loss(M, SE, objective, std)[0]
