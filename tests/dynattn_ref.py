"""numpy restatement of the four dynamic-attention kernels (k3m_amd/csrc/dynattn.hip), written from the formulas of
BertImageSelfAttention.forward with config.dynamic_attention:

    pool = (txt * m).sum(1) / m.sum(1);  g = 1 + sigmoid(z), z = dyLinear_{q|k}(pool);  Q' = Q * g, K' = K * g

Shapes: x [nseq, L, H], mask [nseq, L] (0/1), qkv [nseq, R, C] with C >= 2 Hv (Q | K | V...), z [nseq, 2 Hv].
Everything is computed in the dtype of the inputs (pass float64 for a reference)."""
import numpy as np


def sigmoid(z):
    return 1.0 / (1.0 + np.exp(-z))


def pool_fwd(x, mask):
    """-> pool [nseq, H], inv_count [nseq]; a sequence with no kept token has pool 0 and inv_count 0"""
    cnt = mask.sum(1)
    ic = np.where(cnt > 0, 1.0 / np.where(cnt > 0, cnt, 1.0), 0.0).astype(x.dtype)
    return (x * mask[:, :, None]).sum(1) * ic[:, None], ic


def pool_bwd(dpool, mask, inv_count, dx):
    """-> dx + mask * inv_count * dpool"""
    return dx + (mask * inv_count[:, None])[:, :, None] * dpool[:, None, :]


def scale_fwd(qkv, z):
    out = qkv.copy()
    c = z.shape[1]
    out[:, :, :c] = qkv[:, :, :c] * (1.0 + sigmoid(z))[:, None, :]
    return out


def scale_bwd(dqkv, qkv_gated, z):
    """dqkv w.r.t. the gated Q'|K' -> (dz, dqkv w.r.t. the ungated projections)"""
    c = z.shape[1]
    s = sigmoid(z)
    g = 1.0 + s
    S = (dqkv[:, :, :c] * qkv_gated[:, :, :c]).sum(1)
    dz = S / g * s * (1.0 - s)
    out = dqkv.copy()
    out[:, :, :c] = dqkv[:, :, :c] * g[:, None, :]
    return dz, out
