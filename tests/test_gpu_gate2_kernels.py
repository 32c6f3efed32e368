"""The two-candidate gate kernels of the model without the image modality (k3m_amd/csrc/fusion.hip:
k3m_relu_cat2, k3m_gate2_fwd, k3m_gate2_bwd, k3m_relu_split2_bwd) against a numpy restatement of
pre_sampling_sequence with two candidates (vilbert_k3m.py:2331-2374, sequence_c1 = None) written here.

Shapes: (3, 8); (5, 772) — neither a power of two nor a multiple of the 256 lanes; (10923, 768) — 8,388,864
elements, just past the 8192 x 256 x 4 elements one grid trip covers, so the grid-stride loop runs twice.

Bars.  The restatement adds score and noise in fp32 (as the kernel does) and evaluates everything else in
float64.  idx must equal the restated argmax except where |z0 - z1| < 1e-5 (an fp32 softmax may order such a
pair either way); those elements are skipped everywhere and may be at most 0.1 % (the logistic density of
z0 - z1 is <= 0.25, so ~5e-6 of them are expected).  fp32 outputs: 1e-6 absolute — ys <= 1 carries a few
2^-24 from expf and the division; |dpre| <= y0 y1 |dy0 - dy1| / 4 stays below ~1 for the N(0,1) inputs with a
handful of fp32 roundings.  bf16 outputs (out, dc, dpre with bf16 operands): one bf16 ulp of the value.
Exactly equal logits (which the seeded inputs do not contain, and the restatement would skip) have a test of
their own: the first maximum wins."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
SHAPES = [(3, 8), (5, 772), (10923, 768)]
DTYPES = ["f32", "bf16"]
TIE, TIE_SHARE, ATOL = 1e-5, 1e-3, 1e-6
REF_NOISE = 64 * 2.0 ** -52


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from k3m_amd import _lib as L
    L.load()
    return torch.device("cuda")


def _T(dtype):
    return torch.float32 if dtype == "f32" else torch.bfloat16


def _inputs(rows, d, dtype, dev, seed=0):
    """x0, x1 (the two streams, operand dtype), a (sigmoid scores), noise (gumbel), dout — seeded."""
    g = torch.Generator(device=dev).manual_seed(1000 * seed + rows + d)
    r = lambda *s: torch.randn(s, generator=g, device=dev)  # noqa: E731
    x0, x1, dout = r(rows, d).to(_T(dtype)), r(rows, d).to(_T(dtype)), r(rows, d).to(_T(dtype))
    a = torch.rand((rows, 2 * d), generator=g, device=dev) * (1 - 2e-3) + 1e-3
    u = torch.rand((rows, 2 * d), generator=g, device=dev).clamp_(1e-7, 1 - 1e-7)
    noise = -torch.log(-torch.log(u))
    return x0, x1, a, noise, dout


def relu_cat2(x0, x1):
    from k3m_amd import _lib as L, ops
    rows, d = x0.shape
    c = torch.full((rows, 2 * d), 7.0, dtype=x0.dtype, device=x0.device)
    L.call("k3m_relu_cat2", x0.data_ptr(), x1.data_ptr(), c.data_ptr(), rows, d, ops.dt(x0), L.stream())
    return c


def gate2_fwd(a, c, noise, seed=0, off=0):
    from k3m_amd import _lib as L, ops
    rows, d = c.shape[0], c.shape[1] // 2
    ys = torch.full_like(a, 7.0)
    idx = torch.full((rows * d,), 9, dtype=torch.uint8, device=a.device)
    out = torch.full((rows, d), 7.0, dtype=c.dtype, device=a.device)
    L.call("k3m_gate2_fwd", a.data_ptr(), c.data_ptr(), L.ptr(noise), ys.data_ptr(), idx.data_ptr(), out.data_ptr(),
           rows, d, seed, off, ops.dt(c), L.stream())
    return ys, idx, out


def gate2_bwd(dout, a, c, ys, idx):
    from k3m_amd import _lib as L, ops
    rows, d = dout.shape
    dc, dpre = torch.full_like(c, 7.0), torch.full_like(c, 7.0)
    L.call("k3m_gate2_bwd", dout.data_ptr(), a.data_ptr(), c.data_ptr(), ys.data_ptr(), idx.data_ptr(), dc.data_ptr(),
           dpre.data_ptr(), rows, d, ops.dt(c), L.stream())
    return dc, dpre


def relu_split2_bwd(dc, c, dx0, dx1, acc):
    from k3m_amd import _lib as L, ops
    rows, d = c.shape[0], c.shape[1] // 2
    L.call("k3m_relu_split2_bwd", dc.data_ptr(), c.data_ptr(), L.ptr(dx0), L.ptr(dx1), rows, d, acc, ops.dt(c),
           L.stream())


def _np(t):
    return t.float().cpu().numpy()


def _restate(a, c, noise, dout):
    """numpy: [rows, 2, d] views; z in fp32, the rest in float64."""
    rows, d = dout.shape
    z = (a + noise).astype(np.float32).reshape(rows, 2, d).astype(np.float64)
    a3, c3 = a.reshape(rows, 2, d).astype(np.float64), c.reshape(rows, 2, d).astype(np.float64)
    e = np.exp(z - z.max(1, keepdims=True))
    y = e / e.sum(1, keepdims=True)
    idx = (z[:, 1] > z[:, 0]).astype(np.uint8)          # the first maximum wins a tie
    tie = np.abs(z[:, 0] - z[:, 1]) < TIE
    out = np.where(idx == 1, c3[:, 1], c3[:, 0])
    g = dout.astype(np.float64)
    hard = np.stack([idx == 0, idx == 1], 1).astype(np.float64)
    dc = hard * g[:, None]
    dy = g[:, None] * c3
    dpre = y * (dy - (y * dy).sum(1, keepdims=True)) * a3 * (1.0 - a3)
    return y, idx, tie, out, dc, dpre


def _bf16_ulp(ref):
    return 2.0 ** (np.floor(np.log2(np.maximum(np.abs(ref), 2.0 ** -120))) - 7)


def _check(got, ref, keep, bf16, what):
    err = np.abs(got.astype(np.float64) - ref)
    # + REF_NOISE: the float64 restatement's own cancellation error in dy - sum(y dy) (<= 2^-52 |dy|, |dy| < 64);
    # equal bf16 candidates c0 == c1 have an exactly zero dpre that the restatement returns as ~1e-18
    bar = _bf16_ulp(ref) + REF_NOISE if bf16 else np.full(ref.shape, ATOL)
    bad = np.argwhere((err > bar) & keep)
    assert len(bad) == 0, (what, len(bad), [(tuple(i), float(got[tuple(i)]), float(ref[tuple(i)])) for i in bad[:4]])


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("rows,d", SHAPES)
def test_explicit_noise_matches_restatement(dev, rows, d, dtype):
    x0, x1, a, noise, dout = _inputs(rows, d, dtype, dev)
    c = relu_cat2(x0, x1)
    assert torch.equal(c, torch.cat([torch.relu(x0), torch.relu(x1)], 1))
    ys, idx, out = gate2_fwd(a, c, noise)
    dc, dpre = gate2_bwd(dout, a, c, ys, idx)
    torch.cuda.synchronize()
    y_r, idx_r, tie, out_r, dc_r, dpre_r = _restate(_np(a), _np(c), _np(noise), _np(dout))
    share = tie.mean()
    print("rows %d d %d %s: skipped (|z0 - z1| < %g) share %.2e" % (rows, d, dtype, TIE, share))
    assert share <= TIE_SHARE
    keep = ~tie
    keep2 = np.broadcast_to(keep[:, None], (rows, 2, d))
    bf = dtype == "bf16"
    assert (idx.cpu().numpy().reshape(rows, d)[keep] == idx_r[keep]).all()
    _check(_np(ys).reshape(rows, 2, d), y_r, keep2, False, "ys")
    assert (_np(out).astype(np.float64)[keep] == out_r[keep]).all()      # a copy of the chosen operand: exact
    assert (_np(dc).reshape(rows, 2, d).astype(np.float64)[keep2] == dc_r[keep2]).all()   # hard * g: exact
    _check(_np(out), out_r, keep, bf, "out")
    _check(_np(dc).reshape(rows, 2, d), dc_r, keep2, bf, "dc")
    _check(_np(dpre).reshape(rows, 2, d), dpre_r, keep2, bf, "dpre")


@pytest.mark.parametrize("dtype", DTYPES)
def test_exactly_equal_logits_pick_the_first_candidate(dev, dtype):
    """z0 == z1 bit for bit (the same score and the same noise for both candidates): torch.max over the candidate
    dimension returns the first maximum, so candidate 0 is picked, with y = (0.5, 0.5) exactly.  Every second
    channel has z1 = z0 + 2^-7 instead (far above the 1e-5 band in which an fp32 softmax may round the two
    probabilities equal) and must pick candidate 1: the rule is 'the first maximum', not 'always candidate 0'.
    The backward routes dout by the same index."""
    rows, d = 5, 772
    x0, x1, a, noise, dout = _inputs(rows, d, dtype, dev, seed=3)
    a = a.view(rows, 2, d)
    noise = noise.view(rows, 2, d)
    a[:, 1] = a[:, 0]
    noise[:, 1] = noise[:, 0]
    z = a[:, 0] + noise[:, 0]
    up = z + 2.0 ** -7
    a[:, 0, 1::2], noise[:, 0, 1::2] = z[:, 1::2], 0.0
    a[:, 1, 1::2], noise[:, 1, 1::2] = up[:, 1::2], 0.0
    a, noise = a.reshape(rows, 2 * d).contiguous(), noise.reshape(rows, 2 * d).contiguous()
    c = relu_cat2(x0, x1) + 1.0      # both candidates non-zero, so out tells them apart
    c[:, d:] += 2.0
    ys, idx, out = gate2_fwd(a, c, noise)
    dc, _ = gate2_bwd(dout, a, c, ys, idx)
    torch.cuda.synchronize()
    want = torch.zeros((rows, d), dtype=torch.uint8, device=dev)
    want[:, 1::2] = 1
    assert torch.equal(idx.view(rows, d), want)
    assert bool((ys.view(rows, 2, d)[:, :, 0::2] == 0.5).all())
    assert torch.equal(out, torch.where(want.bool(), c[:, d:], c[:, :d]))
    zero = torch.zeros_like(dout)
    assert torch.equal(dc, torch.cat([torch.where(want.bool(), zero, dout), torch.where(want.bool(), dout, zero)], 1))


@pytest.mark.parametrize("dtype", DTYPES)
def test_rng_path_reproduces_and_depends_on_offset(dev, dtype):
    rows, d = 5, 772
    x0, x1, a, _, _ = _inputs(rows, d, dtype, dev, seed=1)
    c = relu_cat2(x0, x1)
    r1 = gate2_fwd(a, c, None, seed=1234567, off=4096)
    r2 = gate2_fwd(a, c, None, seed=1234567, off=4096)
    r3 = gate2_fwd(a, c, None, seed=1234567, off=4096 + 2 * rows * d)
    torch.cuda.synchronize()
    for u, v in zip(r1, r2):
        assert torch.equal(u, v)
    assert not torch.equal(r1[0], r3[0]) and not torch.equal(r1[1], r3[1])
    assert bool((r1[0][:, :d] + r1[0][:, d:] - 1.0).abs().max() < 1e-6) and int(r1[1].max()) <= 1


def test_rng_pick_rate_with_equal_scores(dev):
    """Equal scores: the pick is decided by the two gumbel draws alone, so candidate 1 wins half the time."""
    rows, d = 64, 768
    a = torch.full((rows, 2 * d), 0.5, device=dev)
    c = torch.ones((rows, 2 * d), device=dev)
    _, idx, _ = gate2_fwd(a, c, None, seed=99, off=12345)
    n = rows * d
    rate = float(idx.float().mean())
    sigma = 0.5 / np.sqrt(n)
    print("pick rate of candidate 1: %.5f (sigma %.5f)" % (rate, sigma))
    assert abs(rate - 0.5) <= 4 * sigma


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("rows,d", SHAPES)
def test_relu_split2_bwd(dev, rows, d, dtype):
    x0, x1, _, _, _ = _inputs(rows, d, dtype, dev, seed=2)
    c = relu_cat2(x0, x1)
    g = torch.Generator(device=dev).manual_seed(5)
    dc = torch.randn((rows, 2 * d), generator=g, device=dev).to(_T(dtype))
    want = [torch.where(c[:, k * d:(k + 1) * d] > 0, dc[:, k * d:(k + 1) * d], torch.zeros_like(x0)) for k in (0, 1)]
    dx0, dx1 = torch.full_like(x0, 7.0), torch.full_like(x0, 7.0)
    relu_split2_bwd(dc, c, dx0, dx1, 0)
    assert torch.equal(dx0, want[0]) and torch.equal(dx1, want[1])
    base = torch.randn((rows, d), generator=g, device=dev).to(_T(dtype))
    dx0, dx1 = base.clone(), base.clone()
    relu_split2_bwd(dc, c, dx0, dx1, 1)   # accumulate: one rounding of the fp32 sum into the operand dtype
    for got, w in zip((dx0, dx1), want):
        assert torch.equal(got, (base.float() + w.float()).to(_T(dtype)))
    dx1 = torch.full_like(x0, 7.0)
    relu_split2_bwd(dc, c, None, dx1, 0)   # a NULL output is skipped
    assert torch.equal(dx1, want[1])
    dx0 = torch.full_like(x0, 7.0)
    relu_split2_bwd(dc, c, dx0, None, 0)
    assert torch.equal(dx0, want[0])


def test_bad_width_and_misaligned_pointers_are_refused(dev):
    """D = 6 (no multiple of 4) and an operand off its 4-element boundary: K3M_EINVAL (1), nothing launched."""
    from k3m_amd import _lib as L
    lib = L.load()
    st = L.stream()
    outs = []

    def buf(*shape, dtype=torch.float32):
        t = torch.full(shape, 7, dtype=dtype, device=dev)
        outs.append(t)
        return t

    def calls(rows, d, x0, x1, c, a, ys, idx, out, dc, dpre, dx0, dx1):
        p = lambda t: t.data_ptr()  # noqa: E731
        return [lib.k3m_relu_cat2(p(x0), p(x1), p(c), rows, d, L.F32, st),
                lib.k3m_gate2_fwd(p(a), p(c), None, p(ys), p(idx), p(out), rows, d, 1, 0, L.F32, st),
                lib.k3m_gate2_bwd(p(out), p(a), p(c), p(ys), p(idx), p(dc), p(dpre), rows, d, L.F32, st),
                lib.k3m_relu_split2_bwd(p(dc), p(c), p(dx0), p(dx1), rows, d, 0, L.F32, st)]

    rows, d = 2, 6
    t = [buf(rows, d), buf(rows, d), buf(rows, 2 * d), buf(rows, 2 * d), buf(rows, 2 * d),
         buf(rows * d, dtype=torch.uint8), buf(rows, d), buf(rows, 2 * d), buf(rows, 2 * d), buf(rows, d), buf(rows, d)]
    assert calls(rows, d, *t) == [1, 1, 1, 1]
    torch.cuda.synchronize()
    for b in t:
        assert bool((b == 7).all())   # a refused call writes nothing
    rows, d = 2, 8
    big = [buf(rows * d + 4), buf(rows * d + 4), buf(rows * 2 * d + 4), buf(rows * 2 * d + 4), buf(rows * 2 * d + 4),
           buf(rows * d + 4, dtype=torch.uint8), buf(rows * d + 4), buf(rows * 2 * d + 4), buf(rows * 2 * d + 4),
           buf(rows * d + 4), buf(rows * d + 4)]
    ok = [b[4:] for b in big]
    assert calls(rows, d, *[b[0:] for b in big]) == [0, 0, 0, 0]          # aligned: accepted
    for b in big:
        b.fill_(7)
    torch.cuda.synchronize()
    # one operand at a time shifted by one element; every entry point that takes it answers K3M_EINVAL
    uses = {0: [0], 1: [0], 2: [0, 1, 2, 3], 3: [1, 2], 4: [1, 2], 5: [1, 2], 6: [1, 2], 7: [2, 3], 8: [2], 9: [3],
            10: [3]}
    for i, hit in uses.items():
        args = list(ok)
        args[i] = big[i][1:]
        rc = calls(rows, d, *args)
        for k in range(4):
            assert rc[k] == (1 if k in hit else 0), (i, k, rc)
    # the bf16 boundary is 8 bytes: a 2-element shift is still misaligned, a 4-element shift is not
    x = torch.zeros((rows * d + 8,), dtype=torch.bfloat16, device=dev)
    cb = torch.zeros((rows * 2 * d + 8,), dtype=torch.bfloat16, device=dev)
    assert lib.k3m_relu_cat2(x[2:].data_ptr(), x.data_ptr(), cb.data_ptr(), rows, d, L.BF16, st) == 1
    assert lib.k3m_relu_cat2(x[4:].data_ptr(), x.data_ptr(), cb.data_ptr(), rows, d, L.BF16, st) == 0
    # rows = 0: a no-op
    assert calls(0, 8, *ok) == [0, 0, 0, 0]
    torch.cuda.synchronize()
