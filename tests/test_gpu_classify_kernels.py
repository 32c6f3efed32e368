"""The item-classification head's kernels (k3m_amd/csrc/classify.hip) one by one.

* drop / tanh-drop, forward and backward, against numpy in float64 with the masks restated by dropmask.keep_scale
  (counter off + b * H + c); (B, H) = (1, 4), (3, 768) and (5, 1002): the last is no multiple of 4 and takes the
  one-element-per-thread path.  Bar: the project's fp32 kernel tolerance, 1e-5 of the tensor's
  max |value|.
* the cross entropy, forward and backward, against F.cross_entropy in float64 on the CPU and its autograd gradient:
  C below, at and above one wave's (64) and one workgroup's (256) width, C == 1, label smoothing, class weights with
  a zero entry, unlabelled rows, a row stride ld > C, a planted tie for pred, the forward-only form, S == 0 both
  ways, rows == 0 and run-to-run bits.  Bars: loss 1e-5 relative plus one fp32 rounding of the magnitude of its terms
  (_term_scale), lse 1e-5 relative, dz 1e-5 of max |dz|.  With C == 1 the
  weight vector keeps its one entry positive (a zero there is the S == 0 case, tested on its own).
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import dropmask as DM

pytestmark = pytest.mark.gpu
BAR = 1e-5
SEED = 0x1234ABCD5
OFF = (1 << 44) + 12345


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda")


def _close(got, ref, what):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    err = np.abs(got - ref).max()
    print(what, "max err", err, "max |ref|", np.abs(ref).max())
    assert err <= BAR * np.abs(ref).max() + 1e-30, (what, err, np.abs(ref).max())


def _ew(name, dev, *lead, B, H, p, out=None):
    from k3m_amd import _lib as L
    out = out if out is not None else torch.empty((B, H), dtype=torch.float32, device=dev)
    L.call(name, *[t.data_ptr() for t in lead], B, H, p, SEED, OFF, out.data_ptr(), L.stream())
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("B,H", [(1, 4), (3, 768), (5, 1002)])
def test_drop_and_tanh_drop_match_numpy(dev, B, H, p):
    rng = np.random.default_rng(B * 1000 + H)
    a = (rng.standard_normal((B, H)) * 1.5).astype(np.float32)
    g = rng.standard_normal((B, H)).astype(np.float32)
    keep = DM.keep_scale(SEED, OFF, B * H, p).reshape(B, H).astype(np.float64)
    if p > 0 and B * H > 100:
        assert 0 < (keep == 0).sum() < B * H
    at, gt = torch.from_numpy(a).to(dev), torch.from_numpy(g).to(dev)
    a64, g64 = a.astype(np.float64), g.astype(np.float64)
    _close(_ew("k3m_cls_drop_fwd", dev, at, B=B, H=H, p=p).cpu().numpy(), a64 * keep, "drop_fwd")
    _close(_ew("k3m_cls_drop_bwd", dev, gt, B=B, H=H, p=p).cpu().numpy(), g64 * keep, "drop_bwd")
    _close(_ew("k3m_cls_tanh_drop_fwd", dev, at, B=B, H=H, p=p).cpu().numpy(), np.tanh(a64) * keep, "tanh_drop_fwd")
    ref = g64 * keep * (1.0 - np.tanh(a64) ** 2)
    _close(_ew("k3m_cls_tanh_drop_bwd", dev, gt, at, B=B, H=H, p=p).cpu().numpy(), ref, "tanh_drop_bwd")
    # in place over dh, as the model's backward calls it
    g2 = gt.clone()
    _close(_ew("k3m_cls_tanh_drop_bwd", dev, g2, at, B=B, H=H, p=p, out=g2).cpu().numpy(), ref, "tanh_drop_bwd in place")


def test_elementwise_rejects_bad_arguments(dev):
    from k3m_amd import _lib as L
    x = torch.zeros((2, 8), dtype=torch.float32, device=dev)
    for args in ((x.data_ptr(), 2, 8, 1.0, 0, 0, x.data_ptr()), (x.data_ptr(), 2, 0, 0.1, 0, 0, x.data_ptr()),
                 (None, 2, 8, 0.1, 0, 0, x.data_ptr())):
        with pytest.raises(RuntimeError, match="bad argument"):
            L.call("k3m_cls_drop_fwd", *args, L.stream())
    L.call("k3m_cls_drop_fwd", x.data_ptr(), 0, 8, 0.1, 0, 0, x.data_ptr(), L.stream())   # B == 0: a no-op


# ---------------------------------------------------------------- cross entropy
def _ce(dev, z, labels, weight, eps, grad=True, ld=None):
    """Run k3m_cls_ce_fwd_bwd (or _fwd) on a copy of z [B, C] laid out with row stride ld; returns a dict."""
    from k3m_amd import _lib as L
    B, C = z.shape
    ld = ld or C
    buf = torch.full((B, ld), 7.5, dtype=torch.float32, device=dev)
    buf[:, :C] = torch.from_numpy(z).to(dev)
    before = buf.clone()
    lab = torch.from_numpy(np.asarray(labels, np.int64)).to(dev)
    w = torch.from_numpy(weight).to(dev) if weight is not None else None
    rows = torch.empty((B,), dtype=torch.float32, device=dev)
    lse = torch.empty((B,), dtype=torch.float32, device=dev)
    loss = torch.full((1,), -123.0, dtype=torch.float32, device=dev)
    pred = torch.empty((B,), dtype=torch.int32, device=dev)
    den = torch.empty((2,), dtype=torch.float32, device=dev)
    L.call("k3m_cls_ce_fwd_bwd" if grad else "k3m_cls_ce_fwd", buf.data_ptr(), ld, lab.data_ptr(), L.ptr(w), eps, B, C,
           rows.data_ptr(), lse.data_ptr(), loss.data_ptr(), pred.data_ptr(), den.data_ptr(), L.stream())
    torch.cuda.synchronize()
    return {"buf": buf, "before": before, "loss": loss.cpu(), "lse": lse.cpu(), "pred": pred.cpu(), "rows": rows.cpu(),
            "den": den.cpu()}


def _ce_ref(z, labels, weight, eps):
    zt = torch.tensor(z.astype(np.float64), requires_grad=True)
    w = torch.tensor(weight.astype(np.float64)) if weight is not None else None
    loss = F.cross_entropy(zt, torch.tensor(np.asarray(labels, np.int64)), weight=w, ignore_index=-1,
                           label_smoothing=eps)
    loss.backward()
    return float(loss.detach()), zt.grad.numpy(), torch.logsumexp(zt.detach(), 1).numpy()


def _term_scale(z, labels, weight, eps, lse):
    """The sum of the magnitudes of the terms the loss adds and subtracts, over S.  Where they cancel (C == 1: lse is
    the one logit and the loss is exactly 0) a bar relative to the loss is no bar at all; the absolute part of the
    loss bar is one fp32 rounding (2^-23) of this magnitude."""
    z = z.astype(np.float64)
    C = z.shape[1]
    w = np.ones(C) if weight is None else weight.astype(np.float64)
    s = sum(w[y] for y in labels if y >= 0)
    t = sum((1.0 - eps) * w[y] * (abs(lse[i]) + abs(z[i, y])) + eps / C * (abs(lse[i]) * w.sum() + (w * np.abs(z[i])).sum())
            for i, y in enumerate(labels) if y >= 0)
    return t / s


def _case(B, C, weighted):
    rng = np.random.default_rng(B * 100003 + C)
    z = (rng.standard_normal((B, C)) * 2.0).astype(np.float32)
    weight, zc = None, -1
    if weighted:
        weight = rng.uniform(0.25, 2.0, C).astype(np.float32)
        if C >= 2:
            zc = C // 2
            weight[zc] = 0.0
    labels = rng.integers(0, C, B)
    labels[0] = (zc + 1) % C          # row 0 is labelled and carries weight
    if B >= 2:
        labels[1] = -1                # an unlabelled row
    if B >= 3 and zc >= 0:
        labels[2] = zc                # a labelled row of weight 0
    if C >= 2:                        # a tie of the two largest logits of row 0: pred takes the lower index
        j1, j2 = sorted(rng.choice(C, 2, replace=False).tolist())
        z[0, j1] = z[0, j2] = np.float32(z[0].max() + 1.0)
    return z, labels, weight


SHAPES = [(1, 1), (1, 2), (3, 3), (4, 63), (4, 64), (4, 65), (2, 257), (3, 1601), (2, 5003)]


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("eps", [0.0, 0.1])
@pytest.mark.parametrize("B,C", SHAPES)
def test_ce_matches_torch_float64(dev, B, C, eps, weighted):
    z, labels, weight = _case(B, C, weighted)
    ref_loss, ref_dz, ref_lse = _ce_ref(z, labels, weight, eps)
    ld = C + 3 if (B, C) == (4, 65) else C     # the one case with a row stride above C
    r = _ce(dev, z, labels, weight, eps, ld=ld)
    got = float(r["loss"])
    print("ce", (B, C), eps, weighted, "loss", got, ref_loss)
    assert abs(got - ref_loss) <= BAR * abs(ref_loss) + 2.0 ** -23 * _term_scale(z, labels, weight, eps, ref_lse)
    assert np.all(np.abs(r["lse"].numpy() - ref_lse) <= BAR * np.maximum(1.0, np.abs(ref_lse)))
    _close(r["buf"][:, :C].cpu().numpy(), ref_dz, "dz")
    assert torch.equal(r["buf"][:, C:], r["before"][:, C:])              # the padding past C is not touched
    assert np.array_equal(r["pred"].numpy(), z.argmax(1).astype(np.int32))   # numpy: the first of equal maxima
    s = sum(float(weight[y]) if weight is not None else 1.0 for y in labels if y >= 0)
    assert abs(float(r["den"][0]) - s) <= 1e-6 * max(1.0, s)
    # the forward-only form: the same bits, z left intact
    f = _ce(dev, z, labels, weight, eps, grad=False, ld=ld)
    assert torch.equal(f["buf"], f["before"])
    for k in ("loss", "lse", "pred", "rows"):
        assert torch.equal(f[k], r[k]), k
    # a second run: the same bits
    r2 = _ce(dev, z, labels, weight, eps, ld=ld)
    for k in ("loss", "lse", "pred", "rows", "buf"):
        assert torch.equal(r2[k], r[k]), k


@pytest.mark.parametrize("eps", [0.0, 0.1])
def test_ce_without_a_weighted_label_is_zero(dev, eps):
    """S == 0 both ways: every row unlabelled, and every labelled row of weight 0 (torch: NaN; here 0, stated)."""
    rng = np.random.default_rng(7)
    z = rng.standard_normal((3, 65)).astype(np.float32)
    w = rng.uniform(0.5, 1.5, 65).astype(np.float32)
    w[[4, 9]] = 0.0
    for labels, weight in (([-1, -1, -1], None), ([-1, -1, -1], w), ([4, -1, 9], w)):
        r = _ce(dev, z, labels, weight, eps)
        assert float(r["loss"]) == 0.0 and float(r["den"][0]) == 0.0
        assert float(r["buf"].abs().max()) == 0.0
        assert float(r["rows"].abs().max()) == 0.0
        assert np.array_equal(r["pred"].numpy(), z.argmax(1).astype(np.int32))


def test_ce_label_out_of_range_is_nan(dev):
    z = np.random.default_rng(3).standard_normal((3, 7)).astype(np.float32)
    for bad in (7, -2):
        r = _ce(dev, z, [1, bad, -1], None, 0.0)
        assert np.isnan(float(r["loss"])) and np.isnan(float(r["rows"][1]))
        assert bool(torch.isnan(r["buf"][1]).all()) and bool(torch.isfinite(r["buf"][[0, 2]]).all())


def test_ce_no_rows_and_bad_arguments(dev):
    from k3m_amd import _lib as L
    for name in ("k3m_cls_ce_fwd_bwd", "k3m_cls_ce_fwd"):
        L.call(name, None, 5, None, None, 0.0, 0, 5, None, None, None, None, None, L.stream())   # rows == 0
    torch.cuda.synchronize()
    z = torch.zeros((2, 5), dtype=torch.float32, device=dev)
    lab = torch.zeros((2,), dtype=torch.int64, device=dev)
    f = torch.zeros((2,), dtype=torch.float32, device=dev)
    i = torch.zeros((2,), dtype=torch.int32, device=dev)
    ok = [z.data_ptr(), 5, lab.data_ptr(), None, 0.0, 2, 5, f.data_ptr(), f.data_ptr(), f.data_ptr(), i.data_ptr(),
          f.data_ptr()]
    for pos, val in ((1, 4), (4, 1.0), (4, -0.1), (6, 0), (0, None), (2, None), (10, None)):
        args = list(ok)
        args[pos] = val
        with pytest.raises(RuntimeError, match="bad argument"):
            L.call("k3m_cls_ce_fwd_bwd", *args, L.stream())
