"""The forward-only kernel forms (a NULL save pointer: DESIGN §18.2): GEMM bias+GELU without aux, LayerNorm without
xhat / rstd, attention without the probabilities / the LSE.

For each form: (1) the output is torch.equal to the saving form's on the same inputs, seed and dropout offsets;
(2) with dropout off it is within the bar the existing kernel tests use for that kernel against torch
(tests/test_gpu_kernels.py 1e-5 for the fp32 GEMM, LayerNorm and attention; tests/test_gpu_gemm_bf16.py 2^-8 for the
bf16 GELU GEMM, 2^-7 for the bf16 LayerNorm, 2e-2 for the bf16 attention context; those bars are stated for p = 0, a
mask being what torch cannot redraw, so the p = 0.1 cases check (1) alone); (3) a mixed NULL pair is an argument error.

The shapes are the smallest that reach each dispatch branch of gemm.hip / gemm_bf16.hip / norm.hip / attention*.hip;
the test id names the kernel reached.  The forms behind switches that the library reads once when it loads (the
one-workgroup-per-tile x6 grids, the 128 x 128 x6 tile, the compiler-scheduled and LDS-DMA x6 walks, the bf16
persistent walk and per-tile kernels under the GELU epilogue, the f32-MFMA register-softmax forward, the
register-staged flash-long forward) run in a fresh child process per knob setting
(test_forms_behind_load_time_knobs), as tests/test_gpu_gemm_x6.py::test_persistent_walk_bit_identical does."""
import math

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


def _rel(a, b):
    return float((a.float() - b.float()).abs().max() / (b.float().abs().max() + 1e-12))


# ---------------------------------------------------------------- GEMM
# (id, dtype, m, n, k, f32_algo): branch conditions in gemm.hip gemm_f32_tiles / gemm_bf16.hip k3m_gemm_bf16_impl
GEMM_CASES = [
    ("x6-persist-2560x1280x64", "fp32", 2560, 1280, 64, None),        # 100 tiles of 256 x 128: the persistent walk
    ("x6-persist-edge-2500x1300x72", "fp32", 2500, 1300, 72, None),   # edge tiles, a partial last k-tile
    ("x6-64x64-200x136x72", "fp32", 200, 136, 72, None),              # few tiles: 64 x 64, edge path, partial k-tile
    ("x6-64x64-interior-512x256x64", "fp32", 512, 256, 64, None),
    ("smallsplitk-reduce-64x768x1024", "fp32", 64, 768, 1024, None),  # ops.small_splitk: epilogue in the reduction
    ("f32-unaligned-64x64-100x136x70", "fp32", 100, 136, 70, None),   # k % 4 != 0: the exact-f32 scalar-load kernel
    ("f32-64x64-512x256x64", "fp32", 512, 256, 64, "f32"),
    ("f32-64x128-1024x3072x64", "fp32", 1024, 3072, 64, "f32"),
    ("f32-128x128-2048x3072x64", "fp32", 2048, 3072, 64, "f32"),
    ("f32-256x256-4096x3328x64", "fp32", 4096, 3328, 64, "f32"),
    ("b16-small-64x64-512x256x128", "bf16", 512, 256, 128, None),     # 4 large tiles < 80: the small-grid kernel
    ("b16-small-k72-512x256x72", "bf16", 512, 256, 72, None),         # K not a multiple of 64
    ("b16-small-128x128-2048x3072x72", "bf16", 2048, 3072, 72, None),
    ("b16-dual-2560x1024x128", "bf16", 2560, 1024, 128, None),        # 80 large tiles: the dual kernel (GELU)
    ("b16-dual-edge-2500x1032x128", "bf16", 2500, 1032, 128, None),
]


def _gemm_inputs(dev, dtype, m, n, k, seed):
    g = torch.Generator(device="cpu").manual_seed(seed)
    td = torch.float32 if dtype == "fp32" else torch.bfloat16
    x = torch.randn(m, k, generator=g).to(dev).to(td)
    W = (torch.randn(n, k, generator=g) * 0.05).to(dev).to(td)
    b = torch.randn(n, generator=g).to(dev)
    return x, W, b


@pytest.mark.parametrize("case", GEMM_CASES, ids=[c[0] for c in GEMM_CASES])
def test_gemm_gelu_without_aux(dev, case):
    from k3m_amd import ops, _lib as L
    _, dtype, m, n, k, algo = case
    x, W, b = _gemm_inputs(dev, dtype, m, n, k, m + n + k)
    fa = L.F32_MFMA_F32 if algo == "f32" else None
    pre = torch.full((m, n), float("nan"), dtype=x.dtype, device=dev)
    y_save = torch.empty((m, n), dtype=x.dtype, device=dev)
    y_only = torch.empty_like(y_save)
    ops.gemm(x, 0, W, 1, y_save, m, n, k, L.EPI_BIAS_GELU, b, pre, f32_algo=fa)
    ops.gemm(x, 0, W, 1, y_only, m, n, k, L.EPI_BIAS_GELU, b, None, f32_algo=fa)
    torch.cuda.synchronize()
    assert torch.isfinite(pre.float()).all()
    assert torch.equal(y_only, y_save)
    ref = torch.nn.functional.gelu(x.float() @ W.float().t() + b)
    err = _rel(y_only, ref)
    print(case[0], "rel err", err)
    assert err < (1e-5 if dtype == "fp32" else 2.0 ** -8)


@pytest.mark.parametrize("dtype,shapes", [("fp32", [(2560, 1280, 64), (300, 256, 72)]),
                                          ("bf16", [(2560, 1024, 128), (2304, 1024, 64)])],
                         ids=["x6-grouped-persist", "b16-grouped-dual"])
def test_grouped_gemm_gelu_without_aux(dev, dtype, shapes):
    """k3m_gemm_grouped: two problems in one launch, both without aux; and one with, one without (no shared template:
    each then runs through k3m_gemm)."""
    from k3m_amd import ops, _lib as L
    ins = [_gemm_inputs(dev, dtype, m, n, k, 7 * m + k) for m, n, k in shapes]
    want = []
    for x, W, b in ins:
        pre = torch.empty((x.shape[0], W.shape[0]), dtype=x.dtype, device=dev)
        want.append(ops.linear(x, W, b, epi=L.EPI_BIAS_GELU, aux=pre))
    with ops.grouped():
        got = [ops.linear(x, W, b, epi=L.EPI_BIAS_GELU, aux=None) for x, W, b in ins]
    pre0 = torch.empty_like(want[0])
    with ops.grouped():
        mixed = [ops.linear(*ins[0], epi=L.EPI_BIAS_GELU, aux=pre0), ops.linear(*ins[1], epi=L.EPI_BIAS_GELU, aux=None)]
    torch.cuda.synchronize()
    for (x, W, b), w, a, c in zip(ins, want, got, mixed):
        ref = torch.nn.functional.gelu(x.float() @ W.float().t() + b)
        assert _rel(w, ref) < (1e-5 if dtype == "fp32" else 2.0 ** -8)
        # a grouped launch may run a problem on another tile than its own launch would: compare it with torch, and
        # with the saving form of the same grouped launch below
        assert _rel(a, ref) < (1e-5 if dtype == "fp32" else 2.0 ** -8)
        assert _rel(c, ref) < (1e-5 if dtype == "fp32" else 2.0 ** -8)
    with ops.grouped():
        saved = [ops.linear(x, W, b, epi=L.EPI_BIAS_GELU, aux=torch.empty((x.shape[0], W.shape[0]), dtype=x.dtype,
                                                                         device=dev)) for x, W, b in ins]
    torch.cuda.synchronize()
    for a, s in zip(got, saved):
        assert torch.equal(a, s)


def test_gemm_internal_epilogue_value_is_refused(dev):
    """The forward-only epilogue is chosen by the library from aux == NULL; its template value is no public enum."""
    from k3m_amd import ops
    x, W, b = _gemm_inputs(dev, "fp32", 64, 64, 64, 1)
    y = torch.empty(64, 64, device=dev)
    with pytest.raises(RuntimeError, match="bad argument"):
        ops.gemm(x, 0, W, 1, y, 64, 64, 64, 5, b, None)
    with pytest.raises(RuntimeError, match="bad argument"):   # the dGELU epilogue still needs its aux
        ops.gemm(x, 0, W, 1, y, 64, 64, 64, 3, None, None)


# ---------------------------------------------------------------- LayerNorm
LN_CASES = [("f32-5x768", "fp32", 5, 768), ("f32-37x1024", "fp32", 37, 1024), ("b16-wave-37x768", "bf16", 37, 768),
            ("b16-halfwave-4100x768", "bf16", 4100, 768), ("b16-halfwave-4099x1024", "bf16", 4099, 1024)]


@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("case", LN_CASES, ids=[c[0] for c in LN_CASES])
def test_layernorm_without_saves(dev, case, p):
    from k3m_amd import ops
    _, dtype, M, cols = case
    td = torch.float32 if dtype == "fp32" else torch.bfloat16
    g_ = torch.Generator(device="cpu").manual_seed(M + cols)
    x = torch.randn(M, cols, generator=g_).to(dev).to(td)
    r = torch.randn(M, cols, generator=g_).to(dev).to(td)
    g = (1 + 0.1 * torch.randn(cols, generator=g_)).to(dev)
    b = (0.1 * torch.randn(cols, generator=g_)).to(dev)
    y_save, y_only, xh = torch.empty_like(x), torch.empty_like(x), torch.empty_like(x)
    rs = torch.empty(M, device=dev)
    ops.ln_fwd(x, r, g, b, y_save, xh, rs, p_in=p, seed=5, off_in=77)
    ops.ln_fwd(x, r, g, b, y_only, None, None, p_in=p, seed=5, off_in=77)
    torch.cuda.synchronize()
    assert torch.equal(y_only, y_save)
    if p == 0.0:
        s = x.float() + r.float()
        u = s.mean(-1, keepdim=True)
        v = (s - u).pow(2).mean(-1, keepdim=True)
        ref = g * (s - u) / torch.sqrt(v + 1e-12) + b
        assert _rel(y_only, ref) < (1e-5 if dtype == "fp32" else 2.0 ** -7)
    for xhat, rstd in ((None, rs), (xh, None)):   # both NULL or both given
        with pytest.raises(RuntimeError, match="k3m_ln_fwd failed with status 1"):
            ops.ln_fwd(x, r, g, b, y_only, xhat, rstd, p_in=p, seed=5, off_in=77)


# ---------------------------------------------------------------- attention
def _attn_inputs(dev, td, B, lq, lk, nh, hd):
    D = nh * hd
    g = torch.Generator(device="cpu").manual_seed(lq * 131 + lk + hd)
    qq = torch.randn(B * lq, 3 * D, generator=g).to(dev).to(td)
    kk = torch.randn(B * lk, 3 * D, generator=g).to(dev).to(td)
    m = torch.ones(B, lk, device=dev)
    m[:, max(1, lk - 3):] = 0   # a padded key tail
    return qq[:, :D], kk[:, D:2 * D], kk[:, 2 * D:], ((1 - m) * -10000).contiguous()


def _attn_ref(q, k, v, mask, B, lq, lk, nh, hd):
    D = nh * hd
    qh = q.float().view(B, lq, nh, hd).permute(0, 2, 1, 3)
    kh = k.float().view(B, lk, nh, hd).permute(0, 2, 1, 3)
    vh = v.float().view(B, lk, nh, hd).permute(0, 2, 1, 3)
    p = torch.softmax(qh @ kh.transpose(-1, -2) / math.sqrt(hd) + mask[:, None, None, :], -1)
    return (p @ vh).permute(0, 2, 1, 3).reshape(B * lq, D)


# k3m_attn_fwd / k3m_attn_long_fwd (probabilities): LK * hd <= 8192 takes the bf16x6 register-softmax forward, larger
# heads the LDS kernel, L > 128 (or an image past 160 KB) the chunked long kernel; bf16 operands the LDS / long kernels
ATTN_CASES = [("f32-x6-L36-hd64", "fp32", 36, 36, 64), ("f32-x6-L128-hd64", "fp32", 128, 128, 64),
              ("f32-long-L130-hd64", "fp32", 130, 130, 64), ("f32-x6-128x37-hd128", "fp32", 128, 37, 128),
              ("f32-lds-L128-hd96", "fp32", 128, 128, 96), ("f32-long-L128-hd128", "fp32", 128, 128, 128),
              ("b16-lds-L36-hd64", "bf16", 36, 36, 64), ("b16-long-L130-hd64", "bf16", 130, 130, 64)]


@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("case", ATTN_CASES, ids=[c[0] for c in ATTN_CASES])
def test_attention_without_probabilities(dev, case, p):
    from k3m_amd import ops
    _, dtype, lq, lk, hd = case
    td = torch.float32 if dtype == "fp32" else torch.bfloat16
    B, nh = 2, 2
    q, k, v, mask = _attn_inputs(dev, td, B, lq, lk, nh, hd)
    c_save = torch.empty(B * lq, nh * hd, device=dev, dtype=td)
    c_only = torch.empty_like(c_save)
    probs = torch.empty(B * nh * lq * lk, device=dev)
    sc = 1 / math.sqrt(hd)
    ops.attn_fwd(q, k, v, mask, c_save, probs, B, lq, lk, nh, hd, sc, p, 11, 5)
    ops.attn_fwd(q, k, v, mask, c_only, None, B, lq, lk, nh, hd, sc, p, 11, 5)
    torch.cuda.synchronize()
    assert torch.equal(c_only, c_save)
    if p == 0.0:
        assert _rel(c_only, _attn_ref(q, k, v, mask, B, lq, lk, nh, hd)) < (1e-5 if dtype == "fp32" else 2.0 ** -7)


# k3m_flash_attn_fwd (L <= 128; two heads per workgroup at L <= 64, hd 64) / k3m_flash_attn_long_fwd (L > 128)
FLASH_CASES = [("pair-L36-hd64", 36, 64), ("L128-hd64", 128, 64), ("L36-hd96", 36, 96), ("L128-hd96", 128, 96),
               ("L36-hd128", 36, 128), ("L128-hd128", 128, 128), ("long-L160-hd64", 160, 64),
               ("long-L160-hd128", 160, 128)]


@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("case", FLASH_CASES, ids=[c[0] for c in FLASH_CASES])
def test_flash_attention_without_lse(dev, case, p):
    from k3m_amd import ops
    _, L_, hd = case
    B, nh = 2, 2
    q, k, v, mask = _attn_inputs(dev, torch.bfloat16, B, L_, L_, nh, hd)
    assert ops.flash_fits(L_, L_, hd) == (L_ <= 128)
    c_save = torch.empty(B * L_, nh * hd, device=dev, dtype=torch.bfloat16)
    c_only = torch.empty_like(c_save)
    lse = torch.empty(B * nh * L_, device=dev)
    sc = 1 / math.sqrt(hd)
    ops.flash_attn_fwd(q, k, v, mask, c_save, lse, B, L_, L_, nh, hd, sc, p, 11, 5)
    ops.flash_attn_fwd(q, k, v, mask, c_only, None, B, L_, L_, nh, hd, sc, p, 11, 5)
    torch.cuda.synchronize()
    assert torch.equal(c_only, c_save)
    if p == 0.0:
        assert _rel(c_only, _attn_ref(q, k, v, mask, B, L_, L_, nh, hd)) < 2e-2


# ---------------------------------------------------------------- forms behind load-time knobs
_CHILD = r'''
import math, sys, torch
sys.path.insert(0, sys.argv[1])
from k3m_amd import ops, _lib as L
dev = torch.device("cuda")


def rel(a, b):
    return float((a.float() - b.float()).abs().max() / (b.float().abs().max() + 1e-12))


def gemm_inputs(td, m, n, k):
    g = torch.Generator(device="cpu").manual_seed(m + n + k)
    return (torch.randn(m, k, generator=g).to(dev).to(td), (torch.randn(n, k, generator=g) * 0.05).to(dev).to(td),
            torch.randn(n, generator=g).to(dev))


def gemm(td, shapes, grouped=False):
    ins = [gemm_inputs(td, *s) for s in shapes]
    bar = 1e-5 if td == torch.float32 else 2.0 ** -8
    outs = []
    for aux in (True, False):
        pres = [torch.full((x.shape[0], W.shape[0]), float("nan"), dtype=td, device=dev) if aux else None for x, W, b in ins]
        if grouped:
            with ops.grouped():
                ys = [ops.linear(x, W, b, epi=L.EPI_BIAS_GELU, aux=p) for (x, W, b), p in zip(ins, pres)]
        else:
            ys = [ops.linear(x, W, b, epi=L.EPI_BIAS_GELU, aux=p) for (x, W, b), p in zip(ins, pres)]
        torch.cuda.synchronize()
        if aux:
            assert all(torch.isfinite(p.float()).all() for p in pres)
        outs.append(ys)
    for (x, W, b), ys, yo in zip(ins, *outs):
        assert torch.equal(ys, yo), ("equal", tuple(x.shape), tuple(W.shape))
        ref = torch.nn.functional.gelu(x.float() @ W.float().t() + b)
        assert rel(yo, ref) < bar, ("bar", tuple(x.shape), rel(yo, ref))


def attention(td, flash, cases):
    B, nh = 2, 2
    for lq, lk, hd in cases:
        D = nh * hd
        g = torch.Generator(device="cpu").manual_seed(lq * 131 + lk + hd)
        qq = torch.randn(B * lq, 3 * D, generator=g).to(dev).to(td)
        kk = torch.randn(B * lk, 3 * D, generator=g).to(dev).to(td)
        q, k, v = qq[:, :D], kk[:, D:2 * D], kk[:, 2 * D:]
        m = torch.ones(B, lk, device=dev)
        m[:, max(1, lk - 3):] = 0
        mask = ((1 - m) * -10000).contiguous()
        for p in (0.0, 0.1):
            cs, co = torch.empty(B * lq, D, device=dev, dtype=td), torch.empty(B * lq, D, device=dev, dtype=td)
            stat = torch.empty(B * nh * lq * (1 if flash else lk), device=dev)
            fn = ops.flash_attn_fwd if flash else ops.attn_fwd
            fn(q, k, v, mask, cs, stat, B, lq, lk, nh, hd, 1 / math.sqrt(hd), p, 11, 5)
            fn(q, k, v, mask, co, None, B, lq, lk, nh, hd, 1 / math.sqrt(hd), p, 11, 5)
            torch.cuda.synchronize()
            assert torch.equal(cs, co), ("equal", lq, lk, hd, p)
            if p == 0.0:
                qh = q.float().view(B, lq, nh, hd).permute(0, 2, 1, 3)
                kh = k.float().view(B, lk, nh, hd).permute(0, 2, 1, 3)
                vh = v.float().view(B, lk, nh, hd).permute(0, 2, 1, 3)
                pr = torch.softmax(qh @ kh.transpose(-1, -2) / math.sqrt(hd) + mask[:, None, None, :], -1)
                ref = (pr @ vh).permute(0, 2, 1, 3).reshape(B * lq, D)
                assert rel(co, ref) < (2e-2 if flash else 1e-5), ("bar", lq, lk, hd, rel(co, ref))


F32, B16 = torch.float32, torch.bfloat16
# 280 tiles of 256 x 128 / 140 of 256 x 256: the 256 x 256 tile; 100 / 50: the 256 x 128 tile; edge tiles and a partial
# last k-tile on each
X6_BIG = [(5120, 1792, 64), (5000, 1800, 72), (2560, 1280, 64), (2500, 1300, 72)]
B16_BIG = [(4096, 2048, 128), (4000, 2056, 128), (2560, 1024, 128), (2500, 1032, 128)]   # 256 x 256, 256 x 128
CASES = {
    "x6-tile-grids": lambda: (gemm(F32, X6_BIG), gemm(F32, [(2560, 1280, 64), (300, 256, 72)], grouped=True)),
    "x6-128x128": lambda: gemm(F32, [(2560, 1280, 64), (2500, 1300, 72)]),
    "x6-walk": lambda: (gemm(F32, X6_BIG), gemm(F32, [(2560, 1280, 64), (300, 256, 72)], grouped=True)),
    "b16-walk": lambda: (gemm(B16, B16_BIG), gemm(B16, [(2560, 1024, 128), (2304, 1024, 64)], grouped=True)),
    "attn-reg": lambda: attention(F32, False, [(36, 36, 64), (128, 128, 64), (128, 37, 128), (64, 64, 96)]),
    "flash-long-fwd1": lambda: attention(B16, True, [(160, 160, 64), (160, 160, 96), (130, 200, 128)]),
}
CASES[sys.argv[2]]()
print("ok", sys.argv[2])
'''

# (id: knobs and the kernels they select, case of _CHILD)
KNOB_CASES = [
    ("K3M_X6_PERSIST=0:gemm_x6_kernel-256x256+256x128,gemm_x6_grouped_kernel", {"K3M_X6_PERSIST": "0"}, "x6-tile-grids"),
    ("K3M_X6_P_MIN=100000:gemm_x6_kernel-128x128", {"K3M_X6_P_MIN": "100000"}, "x6-128x128"),
    ("K3M_X6_PP=0:gemm_x6_persist_kernel-Loop", {"K3M_X6_PP": "0"}, "x6-walk"),
    ("K3M_X6_PP=127:gemm_x6_persist_kernel-PPDLoop", {"K3M_X6_PP": "127"}, "x6-walk"),
    ("K3M_B16_DUAL=0:b16-gemm_persist_kernel", {"K3M_B16_DUAL": "0"}, "b16-walk"),
    ("K3M_B16_DUAL=0,K3M_B16_PREFETCH=1:b16-gemm_persist_kernel-prefetch", {"K3M_B16_DUAL": "0", "K3M_B16_PREFETCH": "1"},
     "b16-walk"),
    ("K3M_B16_DUAL=0,K3M_B16_PP=7:b16-gemm_persist_kernel-pingpong", {"K3M_B16_DUAL": "0", "K3M_B16_PP": "7"}, "b16-walk"),
    ("K3M_B16_DUAL=0,K3M_B16_PERSIST=0:b16-gemm_kernel,gemm_grouped_kernel", {"K3M_B16_DUAL": "0", "K3M_B16_PERSIST": "0"},
     "b16-walk"),
    ("K3M_ATTN_X6=0:attn_fwd_reg_kernel", {"K3M_ATTN_X6": "0"}, "attn-reg"),
    ("K3M_FLASH_LONG_FWD=1:flash_long_fwd_kernel", {"K3M_FLASH_LONG_FWD": "1"}, "flash-long-fwd1"),
]


@pytest.mark.parametrize("case", KNOB_CASES, ids=[c[0] for c in KNOB_CASES])
def test_forms_behind_load_time_knobs(dev, tmp_path, case):
    """The knobs are read when the library loads, so each setting runs in a fresh child process: the saving and the
    NULL-pointer call on one small shape per kernel (interior and edge), torch.equal plus the torch bar, with and
    without dropout for attention."""
    import os
    import subprocess
    import sys
    _, knobs, name = case
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    script = tmp_path / "child.py"
    script.write_text(_CHILD)
    r = subprocess.run([sys.executable, str(script), repo, name], env=dict(os.environ, **knobs), capture_output=True,
                       text=True, timeout=240)
    assert r.returncode == 0 and ("ok " + name) in r.stdout, (r.stdout[-2000:], r.stderr[-3000:])
