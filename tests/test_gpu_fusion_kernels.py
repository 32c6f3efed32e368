"""The streaming kernels of the soft (if_pre_sampling 2) and interactive-only (3) fusion modes
(k3m_amd/csrc/fusion.hip: k3m_soft_scale, k3m_soft_scale_bwd, k3m_mean2, k3m_mean2_bwd) against a float64
restatement computed from the same inputs.

fp32 outputs: rtol 1e-6, atol 1e-12 (z is one rounded product, dpre four: a few 2^-24).  bf16 outputs are
bit-identical to ops.convert (round to nearest even) of the kernel's own fp32 output — the fused operand copy
equals what a separate convert pass would have produced.  bf16 activations are compared the same way against
the fp32 kernel run on the exactly upcast inputs."""
import os
import re

import pytest
import torch

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(1, 4, "f32"), (3, 24, "f32"), (5, 768, "f32"), (5, 1024, "f32"), (3, 24, "bf16"), (5, 1024, "bf16")]
RTOL, ATOL = 1e-6, 1e-12


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from k3m_amd import _lib as L
    L.load()
    return torch.device("cuda")


def _rand(shape, seed, dev, lo=None):
    g = torch.Generator(device="cpu").manual_seed(seed)
    x = torch.randn(shape, generator=g) if lo is None else torch.rand(shape, generator=g) * (1 - 2 * lo) + lo
    return x.to(dev)


def _T(dtype):
    return torch.float32 if dtype == "f32" else torch.bfloat16


def _close(got, ref64):
    torch.testing.assert_close(got.double(), ref64, rtol=RTOL, atol=ATOL)


def _bf16(x32):
    from k3m_amd import ops
    return ops.convert(x32.contiguous(), torch.empty(x32.shape, dtype=torch.bfloat16, device=x32.device))


def soft_scale(c, a, z, rows, d):
    from k3m_amd import _lib as L, ops
    L.call("k3m_soft_scale", c.data_ptr(), a.data_ptr(), z.data_ptr(), rows, d, ops.dt(c), ops.dt(z), L.stream())
    return z


def soft_scale_bwd(dz, c, a, dc, dpre, dlo, rows, d):
    from k3m_amd import _lib as L, ops
    L.call("k3m_soft_scale_bwd", dz.data_ptr(), c.data_ptr(), a.data_ptr(), dc.data_ptr(), dpre.data_ptr(), L.ptr(dlo),
           rows, d, ops.dt(c), L.stream())


def mean2(x1, x2, out):
    from k3m_amd import _lib as L, ops
    L.call("k3m_mean2", x1.data_ptr(), x2.data_ptr(), out.data_ptr(), out.numel(), ops.dt(out), L.stream())
    return out


def mean2_bwd(dout, dx1, dx2, acc):
    from k3m_amd import _lib as L, ops
    L.call("k3m_mean2_bwd", dout.data_ptr(), L.ptr(dx1), L.ptr(dx2), dout.numel(), acc, ops.dt(dout), L.stream())


def _soft_inputs(rows, d, dtype, dev, seed=0):
    n = (rows, 3 * d)
    c = torch.relu(_rand(n, seed + 1, dev)).to(_T(dtype))     # the relu-cat of three streams
    a = _rand(n, seed + 2, dev, lo=1e-3)                       # sigmoid scores in (0, 1), fp32
    dz = _rand(n, seed + 3, dev).to(_T(dtype))
    return c, a, dz


@pytest.mark.parametrize("rows,d,dtype", SHAPES)
def test_soft_scale(dev, rows, d, dtype):
    c, a, _ = _soft_inputs(rows, d, dtype, dev)
    z32 = soft_scale(c, a, torch.full_like(a, float("nan")), rows, d)
    z16 = soft_scale(c, a, torch.zeros(a.shape, dtype=torch.bfloat16, device=dev), rows, d)
    _close(z32, c.double() * a.double())
    assert torch.equal(z16, _bf16(z32))


@pytest.mark.parametrize("rows,d,dtype", SHAPES)
def test_soft_scale_bwd(dev, rows, d, dtype):
    c, a, dz = _soft_inputs(rows, d, dtype, dev)
    dc = torch.full_like(dz, float("nan"))
    dpre = torch.full_like(a, float("nan"))
    dlo = torch.zeros(a.shape, dtype=torch.bfloat16, device=dev)
    soft_scale_bwd(dz, c, a, dc, dpre, dlo, rows, d)
    a64 = a.double()
    _close(dpre, dz.double() * c.double() * a64 * (1.0 - a64))
    assert torch.equal(dlo, _bf16(dpre))
    if dtype == "f32":
        _close(dc, dz.double() * a64)
        dc32, dpre32 = dc, dpre
    else:   # bf16 activations: the fp32 kernel on the exactly upcast inputs, rounded once
        dc32, dpre32 = torch.empty_like(a), torch.empty_like(a)
        soft_scale_bwd(dz.float(), c.float(), a, dc32, dpre32, None, rows, d)
        _close(dc32, dz.double() * a64)
        assert torch.equal(dc, _bf16(dc32)) and torch.equal(dpre, dpre32)
    # without the operand copy (fp32 engine): the same fp32 outputs; dc may overwrite dz (the engine does)
    dz2, dpre2 = dz.clone(), torch.empty_like(a)
    soft_scale_bwd(dz2, c, a, dz2, dpre2, None, rows, d)
    assert torch.equal(dz2, dc) and torch.equal(dpre2, dpre)


@pytest.mark.parametrize("rows,d,dtype", SHAPES)
def test_mean2_and_backward(dev, rows, d, dtype):
    T = _T(dtype)
    x1, x2, dout = [_rand((rows, d), s, dev).to(T) for s in (11, 12, 13)]
    out = mean2(x1, x2, torch.full_like(x1, float("nan")))
    if dtype == "f32":
        _close(out, (x1.double() + x2.double()) / 2)
    else:
        o32 = mean2(x1.float(), x2.float(), torch.empty((rows, d), device=dev))
        _close(o32, (x1.double() + x2.double()) / 2)
        assert torch.equal(out, _bf16(o32))
    d1, d2 = torch.full_like(dout, float("nan")), torch.full_like(dout, float("nan"))
    mean2_bwd(dout, d1, d2, 0)
    half = (dout.double() / 2).to(T)   # halving is exact
    assert torch.equal(d1, half) and torch.equal(d2, half)
    # a null gradient output is skipped, the other one still written
    d2n = torch.full_like(dout, float("nan"))
    mean2_bwd(dout, None, d2n, 0)
    assert torch.equal(d2n, half)
    d1n = torch.full_like(dout, float("nan"))
    mean2_bwd(dout, d1n, None, 0)
    assert torch.equal(d1n, half)
    # accumulate = 1: dx += dout / 2, one rounding in the tensor's dtype
    base = _rand((rows, d), 14, dev).to(T)
    acc1, acc2 = base.clone(), base.clone()
    mean2_bwd(dout, acc1, acc2, 1)
    if dtype == "f32":
        _close(acc1, base.double() + dout.double() / 2)
    else:
        a32 = base.float()
        mean2_bwd(dout.float(), a32, None, 1)
        _close(a32, base.double() + dout.double() / 2)
        assert torch.equal(acc1, _bf16(a32))
    assert torch.equal(acc1, acc2)


def _grid_cap():
    """Blocks of the largest launch, read from the kernel file's grid_for()."""
    src = open(os.path.join(REPO, "k3m_amd", "csrc", "fusion.hip")).read()
    m = re.search(r"int grid_for\(long long n\) \{ return \(int\)std::min<long long>\(\(n \+ 255\) / 256, (\d+)\); \}", src)
    assert m, "grid_for() changed shape: derive the cap again"
    return int(m.group(1))


def test_second_trip_of_the_stride_loop(dev):
    """More elements than one pass of the capped grid covers (cap blocks x 256 lanes x 4 elements): the
    grid-stride loop runs again; every element, the tail included, is right."""
    d = 1024
    per_pass = _grid_cap() * 256 * 4
    rows = per_pass // d + 17
    assert rows * d > per_pass
    x1, x2 = _rand((rows, d), 21, dev), _rand((rows, d), 22, dev)
    out = mean2(x1, x2, torch.full_like(x1, float("nan")))
    _close(out, (x1.double() + x2.double()) / 2)
    d1, d2 = torch.full_like(x1, float("nan")), torch.full_like(x1, float("nan"))
    mean2_bwd(x1, d1, d2, 0)
    assert torch.equal(d1, x1 * 0.5) and torch.equal(d2, d1)
    del out, d1, d2, x2
    rows = per_pass // (3 * d) + 5   # the soft kernels see 3 D columns per row
    assert rows * 3 * d > per_pass
    c, a, dz = _soft_inputs(rows, d, "f32", dev, seed=30)
    z32 = soft_scale(c, a, torch.full_like(a, float("nan")), rows, d)
    _close(z32, c.double() * a.double())
    z16 = soft_scale(c, a, torch.zeros(a.shape, dtype=torch.bfloat16, device=dev), rows, d)
    assert torch.equal(z16, _bf16(z32))
    del z32, z16
    dc, dpre = torch.full_like(a, float("nan")), torch.full_like(a, float("nan"))
    dlo = torch.zeros(a.shape, dtype=torch.bfloat16, device=dev)
    soft_scale_bwd(dz, c, a, dc, dpre, dlo, rows, d)
    _close(dc, dz.double() * a.double())
    _close(dpre, dz.double() * c.double() * a.double() * (1.0 - a.double()))
    assert torch.equal(dlo, _bf16(dpre))


def test_operands_that_are_slices_at_nonzero_offsets(dev):
    """The engine passes row slices of wider buffers (seq_tp[BT:], XT[2BT:2BT+BP]): the kernels work from the
    slice's address and touch nothing outside it."""
    rows, d, lead, tail = 5, 24, 3, 2
    full = rows + lead + tail

    def sl(t):
        return t[lead:lead + rows]
    X1, X2 = _rand((full, d), 41, dev), _rand((full, d), 42, dev)
    OUT = torch.full((full, d), 7.0, device=dev)
    mean2(sl(X1), sl(X2), sl(OUT))
    _close(sl(OUT), (sl(X1).double() + sl(X2).double()) / 2)
    assert bool((OUT[:lead] == 7.0).all()) and bool((OUT[lead + rows:] == 7.0).all())
    D1, D2 = torch.full((full, d), 7.0, device=dev), torch.full((full, d), 7.0, device=dev)
    mean2_bwd(sl(X1), sl(D1), sl(D2), 0)
    assert torch.equal(sl(D1), sl(X1) * 0.5) and torch.equal(sl(D2), sl(D1))
    assert bool((D1[:lead] == 7.0).all()) and bool((D2[lead + rows:] == 7.0).all())
    C = torch.relu(_rand((full, 3 * d), 43, dev))
    A = _rand((full, 3 * d), 44, dev, lo=1e-3)
    DZ = _rand((full, 3 * d), 45, dev)
    Z = torch.full((full, 3 * d), 7.0, device=dev)
    Z16 = torch.full((full, 3 * d), 7.0, dtype=torch.bfloat16, device=dev)
    soft_scale(sl(C), sl(A), sl(Z), rows, d)
    soft_scale(sl(C), sl(A), sl(Z16), rows, d)
    _close(sl(Z), sl(C).double() * sl(A).double())
    assert torch.equal(sl(Z16), _bf16(sl(Z)))
    DC, DP = torch.full_like(Z, 7.0), torch.full_like(Z, 7.0)
    DLO = torch.full_like(Z16, 7.0)
    soft_scale_bwd(sl(DZ), sl(C), sl(A), sl(DC), sl(DP), sl(DLO), rows, d)
    _close(sl(DC), sl(DZ).double() * sl(A).double())
    _close(sl(DP), sl(DZ).double() * sl(C).double() * sl(A).double() * (1.0 - sl(A).double()))
    assert torch.equal(sl(DLO), _bf16(sl(DP)))
    for t in (Z, Z16, DC, DP, DLO):
        assert bool((t[:lead] == 7.0).all()) and bool((t[lead + rows:] == 7.0).all())


def test_bad_width_is_refused_and_empty_input_is_a_no_op(dev):
    """D = 6 is no multiple of 4: K3M_EINVAL (1), nothing launched (the outputs keep their fill).  rows = 0: 0."""
    from k3m_amd import _lib as L
    lib = L.load()
    rows, d = 1, 6
    c, a, dz = _soft_inputs(rows, d, "f32", dev)
    z, dc, dpre = [torch.full_like(a, 7.0) for _ in range(3)]
    st = L.stream()
    assert lib.k3m_soft_scale(c.data_ptr(), a.data_ptr(), z.data_ptr(), rows, d, L.F32, L.F32, st) == 1
    assert lib.k3m_soft_scale_bwd(dz.data_ptr(), c.data_ptr(), a.data_ptr(), dc.data_ptr(), dpre.data_ptr(), None, rows,
                                  d, L.F32, st) == 1
    x = _rand((rows, d), 51, dev)
    o, d1, d2 = [torch.full_like(x, 7.0) for _ in range(3)]
    assert lib.k3m_mean2(x.data_ptr(), x.data_ptr(), o.data_ptr(), x.numel(), L.F32, st) == 1
    assert lib.k3m_mean2_bwd(x.data_ptr(), d1.data_ptr(), d2.data_ptr(), x.numel(), 0, L.F32, st) == 1
    torch.cuda.synchronize()
    for t in (z, dc, dpre, o, d1, d2):
        assert bool((t == 7.0).all())
    assert lib.k3m_soft_scale(c.data_ptr(), a.data_ptr(), z.data_ptr(), 0, 8, L.F32, L.BF16, st) == 0
    assert lib.k3m_soft_scale_bwd(dz.data_ptr(), c.data_ptr(), a.data_ptr(), dc.data_ptr(), dpre.data_ptr(), None, 0, 8,
                                  L.F32, st) == 0
    assert lib.k3m_mean2(x.data_ptr(), x.data_ptr(), o.data_ptr(), 0, L.F32, st) == 0
    assert lib.k3m_mean2_bwd(x.data_ptr(), d1.data_ptr(), None, 0, 1, L.F32, st) == 0
    torch.cuda.synchronize()
    for t in (z, dc, dpre, o, d1, d2):
        assert bool((t == 7.0).all())
