"""Masked-region feature regression (``visual_target=1``) restated in numpy float64, in the compacted form the
kernel sees (the role tests/dynattn_ref.py plays for dynamic attention).

The reference (vilbert_k3m.py:2745-2752), with C = v_target_size and pred the image head's output of regions
1..R-1:

    img_loss = (pred - image_target) ** 2                                   # [B, R-1, C]
    masked_img_loss = sum(img_loss * (image_label == 1)[..., None]) / max(sum(image_label == 1) * C, 1)

Compacted: the n masked regions in row-major order of [B, R-1] are the rows of ``pred_rows`` [n, C]; row r regresses
target row ``trow[r]`` of the [B*(R-1), C] target matrix.  Each row carries loss_rows[r] = mean_c (pred - target)^2 and
the upstream weight row_scale[r] = 1/n, so the loss is sum_r row_scale[r] * loss_rows[r] and
d loss / d pred[r, c] = row_scale[r] * (2/C) * (pred[r, c] - target[trow[r], c]).  No masked region: 0.0 and no
gradient (the clamped denominator), where the KL of visual_target 0 gives 0/0.
"""
import numpy as np


def compact(image_label):
    """(trow, row_scale) of a [B, R-1] label array: the flat indices of the masked regions (label == 1) in row-major
    order and 1/n for each (empty arrays when none is masked)."""
    lab = np.asarray(image_label).reshape(-1)
    trow = np.flatnonzero(lab == 1).astype(np.int32)
    n = len(trow)
    return trow, np.full((n,), 1.0 / n if n else 0.0, np.float64)


def mse_rows(pred_rows, target, trow, row_scale):
    """What the kernel computes.  pred_rows [n, C], target [N, C], trow [n], row_scale [n] ->
    (loss_rows [n], grad [n, C]) in float64."""
    p = np.asarray(pred_rows, np.float64)
    t = np.asarray(target, np.float64)[np.asarray(trow, np.int64)]
    sc = np.asarray(row_scale, np.float64)
    C = p.shape[1]
    d = p - t
    return (d * d).sum(1) / C, sc[:, None] * (2.0 / C) * d


def masked_img_loss(pred_rows, image_target, image_label):
    """(loss, gradient with respect to pred_rows) from the masked regions' predictions [n, C] (row-major order of the
    masked regions), image_target [B, R-1, C] and image_label [B, R-1]."""
    tgt = np.asarray(image_target, np.float64)
    tgt = tgt.reshape(-1, tgt.shape[-1])
    trow, sc = compact(image_label)
    p = np.asarray(pred_rows, np.float64).reshape(len(trow), tgt.shape[-1])
    lr, grad = mse_rows(p, tgt, trow, sc)
    return float((lr * sc).sum()), grad


def dense_loss(pred, image_target, image_label):
    """The same from the full [B, R-1, C] predictions: (loss, gradient [B, R-1, C], zero at unmasked regions)."""
    pred = np.asarray(pred, np.float64)
    C = pred.shape[-1]
    trow, _ = compact(image_label)
    loss, g = masked_img_loss(pred.reshape(-1, C)[trow], image_target, image_label)
    grad = np.zeros((pred.size // C, C), np.float64)
    grad[trow] = g
    return loss, grad.reshape(pred.shape)
