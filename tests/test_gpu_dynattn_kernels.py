"""The four dynamic-attention kernels (k3m_amd/csrc/dynattn.hip: k3m_dyn_pool_fwd, k3m_dyn_pool_bwd,
k3m_dyn_scale_fwd, k3m_dyn_scale_bwd) against the numpy restatement of tests/dynattn_ref.py in float64, fp32 and bf16,
at the smallest shapes where they can go wrong: one and several sequences, one row, a row count that is no multiple
of the block's four waves (37), one and several column blocks (H 8 / 768), masks with a single kept token, interior
zeros and all ones, z up to +-8, operands that are strided views of wider buffers.

Tolerances.  fp32 data: 1e-5 of the tensor's max |value|.  bf16 data: the inputs are bf16-exact (the float64
reference reads the rounded values), the accumulation is fp32, so an fp32 output (pool, inv_count, dz) keeps the
fp32 bar, and a bf16 output differs from the reference by its own rounding: 2^-8 relative per element (twice the
half-ulp of an 8-bit significand) plus the fp32 bar as an absolute floor.  Neither comes from the kernels."""
import numpy as np
import pytest
import torch

import dynattn_ref as R

pytestmark = pytest.mark.gpu
DTYPES = [torch.float32, torch.bfloat16]
F32_BAR = 1e-5
BF16_REL = 2.0 ** -8


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from k3m_amd import _lib
    _lib.load()
    return torch.device("cuda")


def vec(dtype):
    return 8 if dtype == torch.bfloat16 else 4


def rnd(rng, shape, dtype, scale=1.0):
    """host tensor of `dtype` and its exact float64 value"""
    t = torch.from_numpy((scale * rng.standard_normal(shape)).astype(np.float32)).to(dtype)
    return t, t.to(torch.float64).numpy()


def close(got, ref, dtype, what):
    got = got.detach().to(torch.float64).cpu().numpy()
    floor = F32_BAR * max(np.abs(ref).max(), 1e-30)
    bar = floor + (BF16_REL * np.abs(ref) if dtype == torch.bfloat16 else 0.0)
    err = np.abs(got - ref)
    assert (err <= bar).all(), (what, float(err.max()), float(np.abs(ref).max()))


def masks(nseq, L, first):
    """rows cycle through: a single kept token, interior zeros, all ones"""
    m = np.ones((nseq, L), np.float32)
    for s in range(nseq):
        kind = (s + first) % 3
        if kind == 0:
            m[s] = 0
            m[s, (L - 1) // 2] = 1
        elif kind == 1 and L > 2:
            m[s, 1:L - 1:2] = 0
    return m


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("H", [8, 768])
@pytest.mark.parametrize("nseq,L,first", [(1, 1, 0), (3, 1, 0), (1, 37, 1), (3, 37, 0), (3, 128, 1), (1, 128, 2)])
def test_pool_fwd_and_bwd(dev, dtype, H, nseq, L, first):
    from k3m_amd import ops
    rng = np.random.default_rng(1000 * H + 10 * L + nseq)
    pad = vec(dtype)
    # the text rows are a view into a wider buffer with guard sequences before and after
    buf, bufr = rnd(rng, ((nseq + 2) * L, H + pad), dtype)
    buf = buf.to(dev)
    x = buf[L:(nseq + 1) * L, :H]
    xr = bufr[L:(nseq + 1) * L, :H].reshape(nseq, L, H)
    m = masks(nseq, L, first)
    md = torch.from_numpy(m).to(dev)
    pool = torch.full((nseq, H), float("nan"), device=dev)
    ic = torch.full((nseq,), float("nan"), device=dev)
    ops.dyn_pool_fwd(x, md, pool, ic)
    pr, icr = R.pool_fwd(xr, m.astype(np.float64))
    close(pool, pr, torch.float32, "pool")
    close(ic, icr, torch.float32, "inv_count")
    pool2, ic2 = torch.empty_like(pool), torch.empty_like(ic)
    ops.dyn_pool_fwd(x, md, pool2, ic2)
    assert torch.equal(pool, pool2) and torch.equal(ic, ic2)                       # bit-identical runs

    dpool, dpr = rnd(rng, (nseq, H), torch.float32)
    dpool = dpool.to(dev)
    before = buf.clone()
    ops.dyn_pool_bwd(dpool, md, ic, x)
    torch.cuda.synchronize()
    ref = R.pool_bwd(dpr, m.astype(np.float64), ic.double().cpu().numpy(), xr)
    close(buf[L:(nseq + 1) * L, :H], ref.reshape(nseq * L, H), dtype, "dx")
    assert torch.equal(buf[:L], before[:L]) and torch.equal(buf[(nseq + 1) * L:], before[(nseq + 1) * L:])
    assert torch.equal(buf[:, H:], before[:, H:])                                   # guard rows and columns
    keep = torch.from_numpy(m.reshape(-1) != 0).to(dev)
    assert torch.equal(x[~keep], before[L:(nseq + 1) * L, :H][~keep])               # masked tokens bit-unchanged
    again = before.clone()
    ops.dyn_pool_bwd(dpool, md, ic, again[L:(nseq + 1) * L, :H])
    assert torch.equal(again, buf)


@pytest.mark.parametrize("dtype", DTYPES)
def test_pool_of_an_empty_sequence_is_zero(dev, dtype):
    """count 0 cannot come from the collator ([CLS] is kept); the kernel defines pool = 0, inv_count = 0"""
    from k3m_amd import ops
    x = torch.ones((2 * 5, 16), dtype=dtype, device=dev)
    m = torch.tensor([[0, 0, 0, 0, 0], [1, 1, 0, 0, 0]], dtype=torch.float32, device=dev)
    pool, ic = torch.full((2, 16), float("nan"), device=dev), torch.full((2,), float("nan"), device=dev)
    ops.dyn_pool_fwd(x, m, pool, ic)
    assert ic.tolist() == [0.0, 0.5] and torch.equal(pool[0], torch.zeros(16, device=dev))
    assert torch.equal(pool[1], torch.ones(16, device=dev))
    before = x.clone()
    ops.dyn_pool_bwd(torch.ones((2, 16), device=dev), m, ic, x)
    assert torch.equal(x[:5], before[:5]) and torch.equal(x[7:], before[7:])
    assert torch.equal(x[5:7], torch.full((2, 16), 1.5, dtype=dtype, device=dev))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("H", [8, 768])
@pytest.mark.parametrize("nseq,Rr", [(1, 1), (1, 37), (3, 1), (3, 37)])
def test_scale_fwd_and_bwd(dev, dtype, H, nseq, Rr):
    from k3m_amd import ops
    rng = np.random.default_rng(77 * H + 5 * Rr + nseq)
    pad = vec(dtype)
    W = 3 * H + pad
    rows = slice(Rr, (nseq + 1) * Rr)
    buf, bufr = rnd(rng, ((nseq + 2) * Rr, W), dtype)
    buf = buf.to(dev)
    z = np.clip(3.0 * rng.standard_normal((nseq, 2 * H)), -8, 8).astype(np.float32)
    z[0, :4] = [-8, 8, 0, -0.5]
    zd = torch.from_numpy(z).to(dev)
    before = buf.clone()
    qkv = buf[rows, :3 * H]                                                         # row stride 3 H + pad
    ops.dyn_scale_fwd(qkv, zd, Rr)
    torch.cuda.synchronize()
    ref = R.scale_fwd(bufr[rows, :3 * H].reshape(nseq, Rr, 3 * H), z.astype(np.float64))
    close(buf[rows, :2 * H], ref[:, :, :2 * H].reshape(nseq * Rr, 2 * H), dtype, "gated q|k")
    assert torch.equal(buf[rows, 2 * H:], before[rows, 2 * H:])                     # V and the pad columns
    assert torch.equal(buf[:Rr], before[:Rr]) and torch.equal(buf[(nseq + 1) * Rr:], before[(nseq + 1) * Rr:])
    again = before.clone()
    ops.dyn_scale_fwd(again[rows, :3 * H], zd, Rr)
    assert torch.equal(again, buf)

    # backward: the saved gated qkv (as the kernel left it) and a gradient in its own wider buffer
    gated = buf[rows, :3 * H]
    gr = gated.to(torch.float64).cpu().numpy().reshape(nseq, Rr, 3 * H)
    dbuf, dbufr = rnd(rng, ((nseq + 2) * Rr, W + pad), dtype)
    dbuf = dbuf.to(dev)
    dbefore = dbuf.clone()
    dz = torch.full((nseq, 2 * H), float("nan"), device=dev)
    ops.dyn_scale_bwd(dbuf[rows, :3 * H], gated, zd, dz, Rr)
    torch.cuda.synchronize()
    dzr, dqr = R.scale_bwd(dbufr[rows, :3 * H].reshape(nseq, Rr, 3 * H), gr, z.astype(np.float64))
    close(dz, dzr, torch.float32, "dz")
    close(dbuf[rows, :2 * H], dqr[:, :, :2 * H].reshape(nseq * Rr, 2 * H), dtype, "dq|dk")
    assert torch.equal(dbuf[rows, 2 * H:], dbefore[rows, 2 * H:])
    assert torch.equal(dbuf[:Rr], dbefore[:Rr]) and torch.equal(dbuf[(nseq + 1) * Rr:], dbefore[(nseq + 1) * Rr:])
    assert torch.equal(buf, again)                                                  # the saved qkv is read only
    dagain, dz2 = dbefore.clone(), torch.empty_like(dz)
    ops.dyn_scale_bwd(dagain[rows, :3 * H], gated, zd, dz2, Rr)
    assert torch.equal(dagain, dbuf) and torch.equal(dz, dz2)


@pytest.mark.parametrize("dtype", DTYPES)
def test_bad_shapes_and_alignment_are_refused_without_a_launch(dev, dtype):
    """K3M_EINVAL (1), as k3m_gate2_* return it; the outputs keep their NaN fill"""
    from k3m_amd import _lib as L
    lib = L.load()
    st = L.stream()
    dt = L.BF16 if dtype == torch.bfloat16 else L.F32
    v = vec(dtype)
    H, n, ln = 4 * v, 2, 3
    x = torch.ones((n * ln + 1, H + v), dtype=dtype, device=dev)
    m = torch.ones((n, ln), dtype=torch.float32, device=dev)
    pool = torch.full((n + 1, H), float("nan"), device=dev)
    ic = torch.full((n,), float("nan"), device=dev)
    z = torch.zeros((n + 1, 2 * H), device=dev)
    dz = torch.full((n + 1, 2 * H), float("nan"), device=dev)
    q = torch.ones((n * ln + 1, 3 * H + v), dtype=dtype, device=dev)
    p = lambda t: t.data_ptr()  # noqa: E731
    one = x.element_size()
    ld, ldq = H + v, 3 * H + v
    bad = [
        lib.k3m_dyn_pool_fwd(p(x), ld, p(m), p(pool), p(ic), n, ln, H - 1, dt, st),          # H no multiple
        lib.k3m_dyn_pool_fwd(p(x), ld, p(m), p(pool), p(ic), n, ln, H + v // 2, dt, st),
        lib.k3m_dyn_pool_fwd(p(x) + one, ld, p(m), p(pool), p(ic), n, ln, H, dt, st),        # misaligned x
        lib.k3m_dyn_pool_fwd(p(x), ld + 1, p(m), p(pool), p(ic), n, ln, H, dt, st),          # row stride
        lib.k3m_dyn_pool_fwd(p(x), H - v, p(m), p(pool), p(ic), n, ln, H, dt, st),           # stride < H
        lib.k3m_dyn_pool_fwd(p(x), ld, p(m), p(pool) + 4, p(ic), n, ln, H, dt, st),          # misaligned pool
        lib.k3m_dyn_pool_fwd(p(x), ld, p(m), p(pool), p(ic), n, ln, H, 7, st),               # unknown dtype
        lib.k3m_dyn_pool_bwd(p(pool), p(m), p(ic), p(x), ld, n, ln, H - 1, dt, st),
        lib.k3m_dyn_pool_bwd(p(pool), p(m), p(ic), p(x) + one, ld, n, ln, H, dt, st),
        lib.k3m_dyn_pool_bwd(p(pool) + 4, p(m), p(ic), p(x), ld, n, ln, H, dt, st),
        lib.k3m_dyn_scale_fwd(p(q), ldq, p(z), n, ln, H - 1, dt, st),
        lib.k3m_dyn_scale_fwd(p(q) + one, ldq, p(z), n, ln, H, dt, st),
        lib.k3m_dyn_scale_fwd(p(q), 2 * H - v, p(z), n, ln, H, dt, st),                      # stride < 2 H
        lib.k3m_dyn_scale_fwd(p(q), ldq, p(z) + 4, n, ln, H, dt, st),
        lib.k3m_dyn_scale_bwd(p(q), ldq, p(q), ldq, p(z), p(dz), n, ln, H - 1, dt, st),
        lib.k3m_dyn_scale_bwd(p(q) + one, ldq, p(q), ldq, p(z), p(dz), n, ln, H, dt, st),
        lib.k3m_dyn_scale_bwd(p(q), ldq, p(q) + one, ldq, p(z), p(dz), n, ln, H, dt, st),
        lib.k3m_dyn_scale_bwd(p(q), ldq, p(q), ldq + 1, p(z), p(dz), n, ln, H, dt, st),
        lib.k3m_dyn_scale_bwd(p(q), ldq, p(q), ldq, p(z), p(dz) + 4, n, ln, H, dt, st),
        lib.k3m_dyn_scale_bwd(p(q), ldq, p(q), ldq, None, p(dz), n, ln, H, dt, st),
    ]
    torch.cuda.synchronize()
    assert bad == [1] * len(bad), bad
    assert bool(torch.isnan(pool).all()) and bool(torch.isnan(ic).all()) and bool(torch.isnan(dz).all())
    assert bool((x == 1).all()) and bool((q == 1).all())
    # empty problems are not errors
    assert lib.k3m_dyn_pool_fwd(p(x), ld, p(m), p(pool), p(ic), 0, ln, H, dt, st) == 0
    assert lib.k3m_dyn_scale_fwd(p(q), ldq, p(z), n, 0, H, dt, st) == 0
