"""ops.topk_logits (k3m_amd/csrc/topk_logits.hip) on the GPU against a float64 numpy reference.

Reference: s = x64 @ w64^T + b64, ranked with np.lexsort((index, -s)): descending logit, then ascending index;
lse = log sum exp(s) in float64.  Tolerance: the project's fp32 kernel tolerance (as §21.4):
tol[i, j] = 1e-5 |x_i| |w_j|."""
import ctypes
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

# (n, v, h, k, seed): general case; odd tile edges; k > v (the padding); h no multiple of the 32-deep k-tile; the
# real vocabulary (a partial 32-query block and a partial last tile); the region head.
# Every seed keeps the reference's own near-tie share (positions whose float64 gap to a neighbour is within tol)
# under the 5 % cap; the share is asserted below.
CASES = [(70, 1000, 768, 10, 0), (33, 257, 768, 32, 1), (1, 5, 768, 10, 2), (70, 1000, 100, 10, 3),
         (37, 21128, 768, 16, 4), (40, 1601, 1024, 10, 0)]


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda")


@functools.lru_cache(maxsize=None)
def _inputs(n, v, h, seed):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((n, h)).astype(np.float32)
    w = rng.standard_normal((v, h)).astype(np.float32)
    b = rng.standard_normal((v,)).astype(np.float32)
    for a in (x, w, b):
        a.setflags(write=False)
    return x, w, b


def _lse64(s):
    m = s.max(1, keepdims=True)
    return (m + np.log(np.exp(s - m).sum(1, keepdims=True)))[:, 0]


def _reference(x, w, b):
    """(s [n, v] float64, order [n, v] the ranking, tol [n, v], lse [n] float64)"""
    x64, w64 = x.astype(np.float64), w.astype(np.float64)
    s = x64 @ w64.T
    if b is not None:
        s = s + b.astype(np.float64)[None, :]
    tol = 1e-5 * np.linalg.norm(x64, axis=1)[:, None] * np.linalg.norm(w64, axis=1)[None, :]
    idx = np.arange(w.shape[0])
    order = np.stack([np.lexsort((idx, -s[i])) for i in range(s.shape[0])])
    return s, order, tol, _lse64(s)


@functools.lru_cache(maxsize=None)
def _case_reference(n, v, h, seed):
    return _reference(*_inputs(n, v, h, seed))


def _run(dev, x, w, b, k, gold=None, **kw):
    from k3m_amd import ops
    t = lambda a, **o: None if a is None else torch.tensor(a, device=dev, **o)
    out = ops.topk_logits(t(x), t(w), t(b), k=k, gold=t(gold), **kw)
    torch.cuda.synchronize()
    return tuple(None if o is None else o.cpu().numpy() for o in out)


def _check(scores, idx, s, order, tol, k):
    """Every row, nothing exempted: exact padding, sorted, unique, each score within tol of the float64 score of its
    own index, nothing better than the reference's k-th left out.  Then the index must be the reference's wherever
    the float64 gap to both ranking neighbours exceeds tol (the largest tol of the three); returns (positions under
    that gap condition, positions)."""
    n, v = s.shape
    n_ok = min(k, v)
    skipped = 0
    for i in range(n):
        sc, ix = scores[i], idx[i]
        assert np.all(sc[n_ok:] == -np.inf) and np.all(ix[n_ok:] == -1), "padding slots"
        sc, ix = sc[:n_ok], ix[:n_ok]
        assert np.all(np.isfinite(sc)) and np.all((ix >= 0) & (ix < v))
        assert np.all(sc[:-1] >= sc[1:]), "sorted descending"
        assert len(set(ix.tolist())) == n_ok, "unique indices"
        assert np.all(np.abs(sc - s[i, ix]) <= tol[i, ix]), "score of its own index"
        kth = s[i, order[i, n_ok - 1]]
        assert np.all(s[i, ix] >= kth - tol[i, ix]), "no better row left out"
        rs = s[i, order[i, :n_ok + 1]]
        rt = tol[i, order[i, :n_ok + 1]]
        for p in range(n_ok):
            t = max(rt[max(p - 1, 0)], rt[p], rt[min(p + 1, len(rt) - 1)])
            clear = (p == 0 or rs[p - 1] - rs[p] > t) and (p + 1 >= v or rs[p] - rs[p + 1] > t)
            if clear:
                assert ix[p] == order[i, p], "index at a position with clear gaps"
            else:
                skipped += 1
    return skipped, n * n_ok


def test_exact_integer_inputs(dev):
    rng = np.random.default_rng(7)
    n, v, h, k = 33, 257, 768, 32
    x = rng.integers(-4, 5, (n, h)).astype(np.float32)
    w = rng.integers(-4, 5, (v, h)).astype(np.float32)
    b = rng.integers(-4, 5, (v,)).astype(np.float32)
    gold = rng.integers(0, v, (n,)).astype(np.int64)
    s, order, _, lse = _reference(x, w, b)
    scores, idx, got_lse, gs = _run(dev, x, w, b, k, gold=gold)
    want_i = order[:, :k]
    want_s = np.take_along_axis(s, want_i, 1)
    ties = int((want_s[:, :-1] == want_s[:, 1:]).sum())
    print("tied neighbours in the reference ranking:", ties)
    assert ties > 0
    assert np.array_equal(idx, want_i)
    assert np.array_equal(scores.astype(np.float64), want_s)
    assert np.array_equal(gs.astype(np.float64), s[np.arange(n), gold])
    err = np.abs(got_lse - lse)
    print("lse error, largest: %.3g" % err.max())
    assert np.all(err <= 1e-5 * np.maximum(1.0, np.abs(lse)))


@pytest.mark.parametrize("case", CASES, ids=lambda c: "x".join(str(v) for v in c))
def test_float_inputs(dev, case):
    n, v, h, k, seed = case
    x, w, b = _inputs(n, v, h, seed)
    s, order, tol, lse = _case_reference(n, v, h, seed)
    scores, idx, got_lse, gs = _run(dev, x, w, b, k)
    assert gs is None
    skipped, total = _check(scores, idx, s, order, tol, k)
    print("index check skipped %d of %d positions" % (skipped, total))
    assert skipped <= 0.05 * total
    err = np.abs(got_lse - lse)
    print("lse error, largest: %.3g" % err.max())
    assert np.all(err <= tol.max(1) + 1e-5)


def test_chunk_and_tiling_invariance(dev):
    n, v, h, k = 70, 1000, 768, 10
    x, w, b = _inputs(n, v, h, 0)
    gold = np.random.default_rng(11).integers(0, v, (n,)).astype(np.int64)
    base = _run(dev, x, w, b, k, gold=gold, chunks=1)
    for chunks in (3, 0):
        got = _run(dev, x, w, b, k, gold=gold, chunks=chunks)
        for a, c in zip((got[0], got[3]), (base[0], base[3])):
            assert np.array_equal(a.view(np.uint32), c.view(np.uint32)), chunks
        assert np.array_equal(got[1], base[1]), chunks
        assert np.all(np.abs(got[2] - base[2]) <= 1e-6 * np.maximum(1.0, np.abs(base[2]))), chunks
    # n = 64 runs the 256-row x 64-query tiling, n = 65 the 128 x 128 one
    few = _run(dev, x[:64], w, b, k, gold=gold[:64])
    more = _run(dev, x[:65], w, b, k, gold=gold[:65])
    for a, c in zip((few[0], few[3]), (more[0], more[3])):
        assert np.array_equal(a.view(np.uint32), c[:64].view(np.uint32))
    assert np.array_equal(few[1], more[1][:64])
    assert np.all(np.abs(few[2] - more[2][:64]) <= 1e-6 * np.maximum(1.0, np.abs(few[2])))
    for chunks in (2, 4):
        got = _run(dev, x[:64], w, b, k, gold=gold[:64], chunks=chunks)
        assert np.array_equal(got[0].view(np.uint32), few[0].view(np.uint32)) and np.array_equal(got[1], few[1])
        assert np.array_equal(got[3].view(np.uint32), few[3].view(np.uint32))


def test_gold_and_metrics(dev):
    """Rows planted at x_i = 4 w[g_i] + a_i noise with a_i rising over the rows: the gold is the first prediction
    for small a_i and falls out of the top-k for large ones."""
    from k3m_amd import predict
    n, v, h, k = 70, 1000, 768, 10
    _, w, b = _inputs(n, v, h, 0)
    rng = np.random.default_rng(5)
    gold = rng.integers(0, v, (n,)).astype(np.int64)
    amp = np.linspace(0.0, 120.0, n).astype(np.float32)[:, None]
    x = (4.0 * w[gold] + amp * rng.standard_normal((n, h)).astype(np.float32)).astype(np.float32)
    gold[3] = gold[40] = -1
    s, order, tol, lse = _reference(x, w, b)
    rank = np.array([int(np.nonzero(order[i] == gold[i])[0][0]) if gold[i] >= 0 else -1 for i in range(n)])
    known = gold >= 0
    inside, outside = int(((rank < k) & known).sum()), int((rank >= k).sum())
    print("gold inside the top-%d: %d rows, outside: %d rows" % (k, inside, outside))
    assert inside >= 5 and outside >= 5
    scores, idx, got_lse, gs = _run(dev, x, w, b, k, gold=gold)
    assert np.all(gs[~known] == -np.inf)
    assert np.all(np.abs(gs[known] - s[np.arange(n), gold][known]) <= tol[np.arange(n), gold][known])
    for i in np.nonzero(known)[0]:
        hit = np.nonzero(idx[i] == gold[i])[0]
        if rank[i] < k - 1:   # (a gold at the k-th place itself may trade places with a near tie)
            assert len(hit) == 1
        if len(hit):
            assert gs[i].view(np.uint32) == scores[i, hit[0]].view(np.uint32)
        else:
            assert gs[i] <= scores[i, k - 1]
    res = {"t": {"idx": torch.tensor(idx), "gold": torch.tensor(gold),
                 "gold_logprob": torch.tensor(gs - got_lse), "lse": torch.tensor(got_lse)}}
    m = predict.masked_metrics(res, ks=(1, 5, 10))["t"]
    assert m["n"] == int(known.sum())
    for kk in (1, 5, 10):
        assert m["acc@%d" % kk] == pytest.approx(float((rank[known] < kk).mean()), abs=1e-12), kk
    want_nll = float((lse - s[np.arange(n), gold])[known].mean())
    assert m["nll"] == pytest.approx(want_nll, rel=1e-5)


def test_no_bias_is_zero_bias_and_no_rows(dev):
    from k3m_amd import ops
    x, w, b = _inputs(33, 257, 768, 1)
    none = _run(dev, x, w, None, 32)
    zero = _run(dev, x, w, np.zeros_like(b), 32)
    for a, c in zip(none[:3], zero[:3]):
        assert np.array_equal(a, c)
    s, i, lse, gs = ops.topk_logits(torch.empty((0, 768), device=dev), torch.tensor(w, device=dev), None, k=4,
                                    gold=torch.empty((0,), dtype=torch.int64, device=dev))
    torch.cuda.synchronize()
    assert s.shape == (0, 4) and i.shape == (0, 4) and lse.shape == (0,) and gs.shape == (0,)


def test_argument_errors(dev):
    from k3m_amd import _lib, ops
    x = torch.zeros((4, 8), device=dev)
    w = torch.zeros((6, 8), device=dev)
    for bad in (dict(k=0), dict(k=33), dict(chunks=-1)):
        with pytest.raises(ValueError):
            ops.topk_logits(x, w, **bad)
    with pytest.raises(ValueError):
        ops.topk_logits(torch.zeros((4, 6), device=dev), torch.zeros((6, 6), device=dev), k=2)
    with pytest.raises(ValueError):
        ops.topk_logits(x, torch.zeros((6, 12), device=dev), k=2)
    with pytest.raises(ValueError):
        ops.topk_logits(x, w, bias=torch.zeros((5,), device=dev), k=2)
    # the C entry itself: the argument error code, the outputs untouched
    lib = _lib.load()
    s = torch.full((4, 2), 7.0, device=dev)
    i = torch.full((4, 2), 7, dtype=torch.int64, device=dev)
    lse = torch.full((4,), 7.0, device=dev)
    ws = torch.empty((1 << 16,), dtype=torch.uint8, device=dev)
    nb = ctypes.c_longlong(0)
    EINVAL = 1
    for h, k in ((8, 0), (8, 33), (6, 2), (4100, 2)):
        assert lib.k3m_topk_logits_ws_bytes(4, 6, h, k, 0, ctypes.addressof(nb)) == EINVAL
        rc = lib.k3m_topk_logits(x.data_ptr(), w.data_ptr(), None, 4, 6, h, k, None, 0, s.data_ptr(), i.data_ptr(),
                                 lse.data_ptr(), None, ws.data_ptr(), ws.numel(), _lib.stream())
        assert rc == EINVAL
    # too small a workspace; a gold without its output
    assert lib.k3m_topk_logits(x.data_ptr(), w.data_ptr(), None, 4, 6, 8, 2, None, 0, s.data_ptr(), i.data_ptr(),
                               lse.data_ptr(), None, ws.data_ptr(), 16, _lib.stream()) == EINVAL
    g = torch.zeros((4,), dtype=torch.int64, device=dev)
    assert lib.k3m_topk_logits(x.data_ptr(), w.data_ptr(), None, 4, 6, 8, 2, g.data_ptr(), 0, s.data_ptr(),
                               i.data_ptr(), lse.data_ptr(), None, ws.data_ptr(), ws.numel(), _lib.stream()) == EINVAL
    torch.cuda.synchronize()
    assert bool((s == 7.0).all()) and bool((i == 7).all()) and bool((lse == 7.0).all())
