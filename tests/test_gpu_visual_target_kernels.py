"""k3m_mse_fwd_bwd (k3m_amd/csrc/loss.hip), the masked-region feature-regression kernel of visual_target=1, called
directly against the float64 restatement of tests/visual_target_ref.py.

Shapes: 1 and 3 rows; 1, 7, 260 and 2048 columns (the scalar path, a ragged tail past one 256-thread sweep, one
vector sweep with idle lanes, and the workload's two vector sweeps); row strides equal to the column count and padded
(ncols + 4 for the predictions, ncols + 1 for the targets, so that a vectorisable column count must fall back to the
scalar path).  The target rows are gathered out of order with one row used twice from a matrix with more rows than
are used; with 3 rows the middle one has row_scale 0.

Bars, from the arithmetic and not from the kernel:
* loss_rows, rtol 1e-5: the terms are non-negative; about 18 roundings of 2^-24 accumulate through the per-thread
  partial sums and the block_sum tree (1.1e-6), with about 10x room for another reduction order or contraction;
* gradient, rtol 1e-6 elementwise: at most four roundings (p - t, 2/ncols, times row_scale, the product), 2.4e-7;
* exact zeros in the row_scale == 0 row; the padding columns and the target matrix are left as they were."""
import numpy as np
import pytest
import torch

import visual_target_ref as VR

pytestmark = pytest.mark.gpu
LOSS_RTOL = 1e-5
GRAD_RTOL = 1e-6
GUARD = 777.0
EINVAL = 1


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from k3m_amd import _lib
    _lib.load()
    return torch.device("cuda")


def _case(rows, ncols, padded, seed):
    rng = np.random.default_rng(seed)
    ld, ldt = (ncols + 4, ncols + 1) if padded else (ncols, ncols)
    ntgt = 7
    pred = np.full((rows, ld), GUARD, np.float32)
    pred[:, :ncols] = rng.standard_normal((rows, ncols)).astype(np.float32)
    tgt = np.full((ntgt, ldt), GUARD, np.float32)
    tgt[:, :ncols] = np.abs(rng.standard_normal((ntgt, ncols))).astype(np.float32) * 0.5
    trow = np.array([5, 2, 5][:rows] if rows > 1 else [4], np.int32)
    scale = np.full((rows,), 1.0 / rows, np.float32)
    if rows > 1:
        scale[1] = 0.0
    return pred, tgt, trow, scale, ld, ldt


@pytest.mark.parametrize("padded", [False, True])
@pytest.mark.parametrize("ncols", [1, 7, 260, 2048])
@pytest.mark.parametrize("rows", [1, 3])
def test_mse_fwd_bwd_matches_restatement(dev, rows, ncols, padded):
    from k3m_amd import _lib as L
    pred, tgt, trow, scale, ld, ldt = _case(rows, ncols, padded, 100 * ncols + 10 * rows + int(padded))
    want_loss, want_grad = VR.mse_rows(pred[:, :ncols], tgt[:, :ncols], trow, scale)
    d_pred, d_tgt = torch.from_numpy(pred).to(dev), torch.from_numpy(tgt).to(dev)
    d_trow, d_scale = torch.from_numpy(trow).to(dev), torch.from_numpy(scale).to(dev)
    loss_rows = torch.full((rows + 1,), GUARD, dtype=torch.float32, device=dev)
    L.call("k3m_mse_fwd_bwd", d_pred.data_ptr(), ld, d_tgt.data_ptr(), ldt, d_trow.data_ptr(), d_scale.data_ptr(), rows,
           ncols, loss_rows.data_ptr(), L.stream())
    torch.cuda.synchronize()
    got_loss = loss_rows.cpu().numpy().astype(np.float64)
    got = d_pred.cpu().numpy()
    got_grad = got[:, :ncols].astype(np.float64)
    print("loss rel err", np.abs(got_loss[:rows] - want_loss).max() / np.abs(want_loss).max(),
          "grad rel err", (np.abs(got_grad - want_grad) / np.maximum(np.abs(want_grad), 1e-30)).max())
    assert np.isfinite(got_loss[:rows]).all() and got_loss[rows] == GUARD
    np.testing.assert_allclose(got_loss[:rows], want_loss, rtol=LOSS_RTOL, atol=0)
    np.testing.assert_allclose(got_grad, want_grad, rtol=GRAD_RTOL, atol=0)
    if rows > 1:
        assert np.all(got[1, :ncols] == 0.0)   # exact zeros, not small numbers
        assert np.abs(got[0, :ncols]).max() > 0 and np.abs(got[2, :ncols]).max() > 0
    assert np.all(got[:, ncols:] == GUARD)   # the padding columns
    assert np.array_equal(d_tgt.cpu().numpy(), tgt)


def test_no_rows_returns_zero_and_touches_nothing(dev):
    from k3m_amd import _lib as L
    pred = torch.full((2, 8), GUARD, dtype=torch.float32, device=dev)
    tgt = torch.zeros((2, 8), dtype=torch.float32, device=dev)
    trow = torch.zeros((2,), dtype=torch.int32, device=dev)
    scale = torch.ones((2,), dtype=torch.float32, device=dev)
    loss_rows = torch.full((2,), GUARD, dtype=torch.float32, device=dev)
    rc = L.load().k3m_mse_fwd_bwd(pred.data_ptr(), 8, tgt.data_ptr(), 8, trow.data_ptr(), scale.data_ptr(), 0, 8,
                                  loss_rows.data_ptr(), L.stream())
    torch.cuda.synchronize()
    assert rc == 0
    assert bool((pred == GUARD).all()) and bool((loss_rows == GUARD).all())


def test_bad_arguments_are_refused_before_any_launch(dev):
    """K3M_ARG returns before the launch: only the return code is read, nothing runs."""
    from k3m_amd import _lib as L
    fn = L.load().k3m_mse_fwd_bwd
    pred = torch.full((2, 8), GUARD, dtype=torch.float32, device=dev)
    tgt = torch.zeros((2, 8), dtype=torch.float32, device=dev)
    trow = torch.zeros((2,), dtype=torch.int32, device=dev)
    scale = torch.ones((2,), dtype=torch.float32, device=dev)
    loss_rows = torch.full((2,), GUARD, dtype=torch.float32, device=dev)
    p, t, r, s, lr, st = (pred.data_ptr(), tgt.data_ptr(), trow.data_ptr(), scale.data_ptr(), loss_rows.data_ptr(),
                          L.stream())
    assert fn(None, 8, t, 8, r, s, 2, 8, lr, st) == EINVAL
    assert fn(p, 8, None, 8, r, s, 2, 8, lr, st) == EINVAL
    assert fn(p, 8, t, 8, None, s, 2, 8, lr, st) == EINVAL
    assert fn(p, 8, t, 8, r, None, 2, 8, lr, st) == EINVAL
    assert fn(p, 8, t, 8, r, s, 2, 8, None, st) == EINVAL
    assert fn(p, 8, t, 8, r, s, 2, 0, lr, st) == EINVAL    # ncols <= 0
    assert fn(p, 8, t, 8, r, s, 2, -4, lr, st) == EINVAL
    assert fn(p, 4, t, 8, r, s, 2, 8, lr, st) == EINVAL    # ld < ncols
    assert fn(p, 8, t, 4, r, s, 2, 8, lr, st) == EINVAL    # ldt < ncols
    torch.cuda.synchronize()
    assert bool((pred == GUARD).all()) and bool((loss_rows == GUARD).all())
