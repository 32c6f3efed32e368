"""The forward-only kernel forms of the item-embedding path: k3m_embed_fwd without xhat / rstd (and
with the encoder copy written in bf16), k3m_gate_fwd / k3m_gate2_fwd without ys / idx, the pair heads without any
gradient output.  For each: the outputs are torch.equal to the saving form's on the same inputs, seed and offsets;
a mixed NULL pair is an argument error (status 1).  Shapes: the smallest that reach each path (the embedding kernel
takes four rows per workgroup: 21 rows and 1 row exercise the tail; the gates run a grid-stride loop over rows * d,
gate2 over rows * d / 4)."""
import pytest
import torch

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from k3m_amd import _lib
    _lib.load()
    return torch.device("cuda")


def _status(name, *args):
    from k3m_amd import _lib as L
    return getattr(L.load(), name)(*args)


# ---------------------------------------------------------------- embedding
def _embed_inputs(dev, nseq, ln, hidden, seed):
    g = torch.Generator(device="cpu").manual_seed(seed)
    V = 50
    ids = torch.randint(0, V, (nseq, ln), generator=g).to(dev)
    tt = torch.randint(0, 2, (nseq, ln), generator=g).to(dev)
    word = torch.randn(V, hidden, generator=g).to(dev)
    pos = torch.randn(64, hidden, generator=g).to(dev)
    typ = torch.randn(2, hidden, generator=g).to(dev)
    gamma = (1.0 + 0.1 * torch.randn(hidden, generator=g)).to(dev)
    beta = (0.1 * torch.randn(hidden, generator=g)).to(dev)
    return ids, tt, word, pos, typ, gamma, beta


@pytest.mark.parametrize("p_out", [0.0, 0.1])
@pytest.mark.parametrize("shape", [(3, 7, 768), (1, 1, 256), (2, 36, 1024)])
def test_embed_forward_only(dev, shape, p_out):
    from k3m_amd import ops
    nseq, ln, hidden = shape
    inp = _embed_inputs(dev, nseq, ln, hidden, sum(shape))
    rows = nseq * ln
    f32 = dict(dtype=torch.float32, device=dev)
    seed, off = 1234567, 4096

    def bufs(n, dtype=torch.float32):
        return [torch.full((rows, hidden), float("nan"), dtype=dtype, device=dev) for _ in range(n)]
    y0, y1, y2, xh = bufs(4)
    rs = torch.full((rows,), float("nan"), **f32)
    ops.embed_fwd(*inp, y0, y1, y2, xh, rs, p_out, seed, off)
    # forward-only, all three outputs
    z0, z1, z2 = bufs(3)
    ops.embed_fwd(*inp, z0, z1, z2, None, None, p_out, seed, off)
    # forward-only, y1 = y2 = NULL
    w0, = bufs(1)
    ops.embed_fwd(*inp, w0, None, None, None, None, p_out, seed, off)
    # forward-only, the encoder copy in bf16 beside the fp32 individual candidate; y2 NULL, then y1 NULL
    m0, = bufs(1)
    m1, m2 = bufs(2, torch.bfloat16)
    ops.embed_fwd(*inp, m0, m1, None, None, None, p_out, seed, off)
    n0, = bufs(1)
    ops.embed_fwd(*inp, n0, None, m2, None, None, p_out, seed, off)
    torch.cuda.synchronize()
    assert torch.isfinite(y0).all() and torch.isfinite(xh).all() and torch.isfinite(rs).all()
    assert torch.equal(y1, y0) and torch.equal(y2, y0)
    for t in (z0, z1, z2, w0, m0, n0):
        assert torch.equal(t, y0)
    conv = ops.convert(y0, torch.empty((rows, hidden), dtype=torch.bfloat16, device=dev))
    torch.cuda.synchronize()
    assert torch.equal(m1, conv) and torch.equal(m2, conv)


def test_embed_mixed_null_pair_is_an_argument_error(dev):
    from k3m_amd import _lib as L
    inp = _embed_inputs(dev, 1, 4, 256, 1)
    y0 = torch.empty((4, 256), device=dev)
    xh = torch.empty_like(y0)
    rs = torch.empty((4,), device=dev)
    base = [t.data_ptr() for t in inp] + [y0.data_ptr(), None, None]
    tail = [1, 4, 256, 1e-12, 0.0, 0, 0, L.F32, L.stream()]
    assert _status("k3m_embed_fwd", *base, xh.data_ptr(), None, *tail) == 1
    assert _status("k3m_embed_fwd", *base, None, rs.data_ptr(), *tail) == 1
    # the mixed-dtype form is forward-only
    tail_ex = [1, 4, 256, 1e-12, 0.0, 0, 0, L.F32, L.BF16, L.stream()]
    assert _status("k3m_embed_fwd_ex", *base, xh.data_ptr(), rs.data_ptr(), *tail_ex) == 1
    assert _status("k3m_embed_fwd_ex", *base, None, None, *tail_ex) == 0
    torch.cuda.synchronize()


# ---------------------------------------------------------------- gates
def _gate_case(dev, name, k, rows, d, explicit):
    from k3m_amd import _lib as L
    g = torch.Generator(device="cpu").manual_seed(rows * 1000 + d + k)
    a = torch.sigmoid(torch.randn(rows, k * d, generator=g)).to(dev)
    c = torch.relu(torch.randn(rows, k * d, generator=g)).to(dev)
    nz = None
    if explicit:
        nz = (-torch.log(torch.empty(rows, k, d).exponential_(generator=g))).to(dev)
    ys = torch.full((rows, k * d), float("nan"), device=dev)
    idx = torch.full((rows * d,), 255, dtype=torch.uint8, device=dev)
    out = torch.full((rows, d), float("nan"), device=dev)
    out2 = torch.full((rows, d), float("nan"), device=dev)
    seed, off = 987654321, 12345 * 4
    L.call(name, a.data_ptr(), c.data_ptr(), L.ptr(nz), ys.data_ptr(), idx.data_ptr(), out.data_ptr(), rows, d, seed, off,
           L.F32, L.stream())
    L.call(name, a.data_ptr(), c.data_ptr(), L.ptr(nz), None, None, out2.data_ptr(), rows, d, seed, off, L.F32,
           L.stream())
    torch.cuda.synchronize()
    assert torch.isfinite(ys).all() and int(idx.max()) < k and torch.isfinite(out).all()
    assert len(torch.unique(idx)) > 1 or rows * d < 8   # the draw chooses among the candidates
    assert torch.equal(out2, out)
    args = [a.data_ptr(), c.data_ptr(), L.ptr(nz)]
    tail = [out2.data_ptr(), rows, d, seed, off, L.F32, L.stream()]
    assert _status(name, *args, ys.data_ptr(), None, *tail) == 1
    assert _status(name, *args, None, idx.data_ptr(), *tail) == 1


@pytest.mark.parametrize("explicit", [True, False], ids=["noise", "philox"])
@pytest.mark.parametrize("shape", [(5, 768), (3, 1024), (1, 256)])
def test_gate_forward_only(dev, shape, explicit):
    _gate_case(dev, "k3m_gate_fwd", 3, shape[0], shape[1], explicit)


@pytest.mark.parametrize("explicit", [True, False], ids=["noise", "philox"])
@pytest.mark.parametrize("shape", [(5, 768), (1, 4)])
def test_gate2_forward_only(dev, shape, explicit):
    _gate_case(dev, "k3m_gate2_fwd", 2, shape[0], shape[1], explicit)


# ---------------------------------------------------------------- pair heads
@pytest.mark.parametrize("B", [1, 3])
def test_ce_head_forward_only(dev, B):
    from k3m_amd import _lib as L
    H = 768
    g = torch.Generator(device="cpu").manual_seed(B)
    u = torch.randn(B, H, generator=g).to(dev)
    W = (0.05 * torch.randn(2, H, generator=g)).to(dev)
    b = torch.randn(2, generator=g).to(dev)
    labels = torch.tensor([1.0, 0.0, 1.0][:B], device=dev)
    f = lambda *s: torch.full(s, float("nan"), device=dev)   # noqa: E731
    logits, probs, dlog, rows, loss, du = f(B, 2), f(B, 2), f(B, 2), f(B), f(1), f(B, H)
    gW, gb = torch.zeros(2, H, device=dev), torch.zeros(2, device=dev)
    L.call("k3m_align_ce_fwd_bwd", u.data_ptr(), W.data_ptr(), b.data_ptr(), labels.data_ptr(), B, H, 0.0, 0, 0,
           logits.data_ptr(), probs.data_ptr(), dlog.data_ptr(), rows.data_ptr(), loss.data_ptr(), du.data_ptr(),
           gW.data_ptr(), gb.data_ptr(), L.stream())
    logits2, probs2, rows2, loss2 = f(B, 2), f(B, 2), f(B), f(1)
    L.call("k3m_align_ce_fwd", u.data_ptr(), W.data_ptr(), b.data_ptr(), labels.data_ptr(), B, H, 0.0, 0, 0,
           logits2.data_ptr(), probs2.data_ptr(), rows2.data_ptr(), loss2.data_ptr(), L.stream())
    torch.cuda.synchronize()
    assert torch.isfinite(loss).all() and torch.isfinite(probs).all()
    assert torch.equal(logits2, logits) and torch.equal(probs2, probs) and torch.equal(loss2, loss)
    assert torch.equal(rows2, rows)


@pytest.mark.parametrize("B", [1, 3])
def test_cosine_head_forward_only(dev, B):
    from k3m_amd import _lib as L
    H = 768
    g = torch.Generator(device="cpu").manual_seed(10 + B)
    e = torch.randn(2 * B, H, generator=g).to(dev)
    labels = torch.tensor([1.0, 0.0, 1.0][:B], device=dev)
    f = lambda *s: torch.full(s, float("nan"), device=dev)   # noqa: E731
    loss, probs, rows, de = f(1), f(B), f(B), f(2 * B, H)
    L.call("k3m_align_cosine_fwd_bwd", e.data_ptr(), labels.data_ptr(), B, H, 0.0, loss.data_ptr(), probs.data_ptr(),
           rows.data_ptr(), de.data_ptr(), L.stream())
    loss2, probs2, rows2 = f(1), f(B), f(B)
    L.call("k3m_align_cosine_fwd", e.data_ptr(), labels.data_ptr(), B, H, 0.0, loss2.data_ptr(), probs2.data_ptr(),
           rows2.data_ptr(), L.stream())
    torch.cuda.synchronize()
    assert torch.isfinite(loss).all() and torch.isfinite(de).all()
    assert torch.equal(loss2, loss) and torch.equal(probs2, probs) and torch.equal(rows2, rows)
