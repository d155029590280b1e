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
