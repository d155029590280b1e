"""Evaluation figures from the masked error sums of `ops.error_sums` (csrc/errsum.hip).  The reference's `Trainer.get_error`
(src/trainer/trainer.py:231-271) copies prediction, target and mask to the host and reduces them there with NumPy; here the
reduction over the nodes is one kernel and what is left is arithmetic on [B, 1+3C] numbers, in fp64 on whatever device the
sums live on (the GPU in the product path; the CPU in the host tests)."""
import torch


def error_mean_std(sums, rows_per_segment, relative=True):
    """(error_mean [C], error_std [C]) in fp64 from `sums` [B, 1+3C] = [M | SE | AE | TT] per sample (`ops.error_sums`), each
    sample having `rows_per_segment` = n rows:

        scale[b,c] = sqrt(TT / (M + 1e-6)) + 1e-6          (1 if not `relative`)
        mean_c     = sum_b AE / scale / (B n)
        E2_c       = sum_b SE / scale^2 / (B n)
        std_c      = sqrt(max(E2 - mean^2, 0))

    which is the arithmetic of the reference's `get_error` for 0/1 masks: the error of a node is |pred - target| where the
    mask is set and ZERO elsewhere, and mean and standard deviation run over all B n nodes, masked-out ones included.  The
    clamp at zero is this formula's own: in fp64 the difference of the two moments can fall fractionally below zero where
    every error is equal, which `np.std` (a sum of squared deviations) cannot.  For masks other than 0/1 all four sums are
    m-weighted (the reference tests `mask != 0` for the errors but sums the mask values for the scale)."""
    sums = sums.to(torch.float64)
    if sums.dim() != 2 or (sums.shape[1] - 1) % 3 or sums.shape[1] < 4:
        raise ValueError(f"error_mean_std: sums [B, 1+3C] expected, got {tuple(sums.shape)}")
    B, C = sums.shape[0], (sums.shape[1] - 1) // 3
    M, SE, AE, TT = sums[:, :1], sums[:, 1:1 + C], sums[:, 1 + C:1 + 2 * C], sums[:, 1 + 2 * C:]
    scale = torch.sqrt(TT / (M + 1e-6)) + 1e-6 if relative else torch.ones_like(TT)
    count = B * int(rows_per_segment)
    mean = (AE / scale).sum(0) / count
    e2 = (SE / scale ** 2).sum(0) / count
    return mean, torch.sqrt(torch.clamp(e2 - mean ** 2, min=0.0))


def edge_error_mean_std(sums, relative=True):
    """(mean [C], std [C]) in fp64 over the samples of `sums` [B, 1+2C] = [ME | DE | TE] (`ops.edge_diff_sums`):

        E[b,c] = sqrt(DE / ME)          divided by sqrt(TE / ME) when `relative`

    the RMS difference of the error field along the mesh edges, against that of the target field.  The standard deviation is the
    population one, as `error_mean_std` takes it."""
    sums = sums.to(torch.float64)
    if sums.dim() != 2 or (sums.shape[1] - 1) % 2 or sums.shape[1] < 3:
        raise ValueError(f"edge_error_mean_std: sums [B, 1+2C] expected, got {tuple(sums.shape)}")
    C = (sums.shape[1] - 1) // 2
    ME, DE, TE = sums[:, :1], sums[:, 1:1 + C], sums[:, 1 + C:]
    E = torch.sqrt(DE / ME)
    if relative:
        E = E / torch.sqrt(TE / ME)
    return E.mean(0), E.std(0, unbiased=False)


def _cell_columns(sums, who):
    sums = sums.to(torch.float64)
    if sums.dim() != 2 or (sums.shape[1] - 5) % 2 or sums.shape[1] < 7:
        raise ValueError(f"{who}: sums [B, 1+2C+4] expected, got {tuple(sums.shape)}")
    return sums, (sums.shape[1] - 5) // 2


def cell_error_mean_std(sums, relative=True):
    """(mean [C], std [C]) in fp64 over the samples of `sums` [B, 1+2C+4] = [A | GE | GT | DP DT WE WT] (`MeshGradient.sums`,
    DESIGN.md 4.30):

        E[b,c] = sqrt(GE / A)          divided by sqrt(GT / A) when `relative`

    the RMS P1 gradient of the error field over the mesh (its H1 seminorm over the square root of the area), against that of the
    target field.  The standard deviation is the population one, as `edge_error_mean_std` takes it."""
    sums, C = _cell_columns(sums, "cell_error_mean_std")
    A, GE, GT = sums[:, :1], sums[:, 1:1 + C], sums[:, 1 + C:1 + 2 * C]
    E = torch.sqrt(GE / A)
    if relative:
        E = E / torch.sqrt(GT / A)
    return E.mean(0), E.std(0, unbiased=False)


def divergence_rms(sums):
    """(pred [B], target [B]) in fp64 from `sums` [B, 1+2C+4] (`MeshGradient.sums` with a velocity pair): the RMS divergence of the
    predicted and of the target velocity field over the mesh, sqrt(DP / A) and sqrt(DT / A)."""
    sums, C = _cell_columns(sums, "divergence_rms")
    return torch.sqrt(sums[:, 1 + 2 * C] / sums[:, 0]), torch.sqrt(sums[:, 2 + 2 * C] / sums[:, 0])


def equivariance_error(model, batch, transforms, groups, rows_per_sample=None):
    """How far `model` is from commuting with a change of frame, per channel, as a relative RMS difference (fp64 [C]):

        pred   = model(batch)
        pred_q = model(batch seen through `transforms`)          state groups and the position columns of node_in, Q v
        back   = Q^T pred_q on the same groups
        err_c  = sqrt( sum m (back_c - pred_c)^2 / sum m pred_c^2 )      over all unmasked rows of the batch

    Exactly 0 for identity matrices; 0 up to rounding for an equivariant model.  `model` is a Trainer (anything with
    `get_pred(batch)`); `batch` a consistent-mesh device batch [node_in [B,N,C+p+1], node_tar, node_mask, ..] or the per-level
    list of variable meshes, for which `rows_per_sample` lists the nodes of every sample; `transforms` [B,p,p]; `groups` the first
    channel of every vector group of the state (`TrajectoryBank.vector_groups`).  The reduction is `ops.error_sums`; nothing but
    the C results leaves the device."""
    from .databank import transform_rows
    from .graph import LevelData
    from .ops import error_sums
    levels = isinstance(batch[0], LevelData)
    node_in, node_tar, mask = (batch[0].x, batch[0].y, batch[0].mask) if levels else batch[:3]
    n_c, p = int(node_tar.shape[-1]), int(transforms.shape[-1])
    if rows_per_sample is None:
        if levels:
            raise ValueError("equivariance_error: a variable-mesh batch needs rows_per_sample")
        rows_per_sample = int(node_in.shape[-2])
    groups = [int(g) for g in groups]
    with torch.no_grad():
        turned = transform_rows(node_in.contiguous(), rows_per_sample, transforms, groups + [n_c])     # the positions follow the state
        if levels:
            seen = [LevelData(batch[0].edge_index, batch[0].num_nodes, batch[0].face, turned, node_tar, mask), *batch[1:]]
        else:
            seen = [turned, *batch[1:]]
        pred = model.get_pred(batch).contiguous()
        back = model.get_pred(seen).contiguous()
        pred, back = pred.reshape(-1, n_c), back.reshape(-1, n_c)
        transform_rows(back, rows_per_sample, transforms, groups, inverse=True, out=back)
        sums = error_sums(back, pred, mask.reshape(-1, 1).contiguous(), pred.shape[0]).sum(0)
        se, tt = sums[1:1 + n_c], sums[1 + 2 * n_c:]
        return torch.where(se == 0, torch.zeros_like(se), torch.sqrt(se / tt))      # identical predictions: 0 even where pred itself is 0
