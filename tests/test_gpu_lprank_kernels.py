"""ops.lp_rank (k3m_amd/csrc/lprank.hip) on the GPU against a float64 numpy reference.

Reference: s64 = sign (2 q64 c64^T - |c64|^2), ranked with np.lexsort((index, -s64)) over the eligible rows:
descending score, then ascending index.  Tolerance: the project's fp32 kernel tolerance 1e-5 |q| |c|
applied to the two terms of the score: tol[i, r] = 1e-5 (2 |q_i| |c_r| + |c_r|^2)."""
import ctypes
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

# (Nq, Nc, H, k, seed): the 128 x 128 tiling; the 256 x 64 tiling; k > Nc (the padding); H no multiple of the 32-deep
# k-tile; two query tiles.  Every seed keeps the reference's own near-tie shares under the caps asserted below (at
# most 5 % of the list positions, at most 25 % of the ranks), checked on the CPU.
CASES = [(70, 1000, 768, 10, 0), (33, 257, 768, 32, 1), (1, 5, 768, 10, 2), (70, 1000, 100, 10, 0),
         (130, 2000, 768, 16, 1)]
MAX_K = 32


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda")


@functools.lru_cache(maxsize=None)
def _inputs(nq, nc, h, seed, ints=False):
    """(q, c, gold, q_gid, c_gid): every even query planted near its gold, q = c[gold] + 0.9 noise, so that about
    half of the golds land inside the top-k; q_gid = c_gid[gold], -1 on every third query."""
    rng = np.random.default_rng(seed)
    if ints:
        c = rng.integers(-4, 5, (nc, h)).astype(np.float32)
        q = rng.integers(-4, 5, (nq, h)).astype(np.float32)
    else:
        c = rng.standard_normal((nc, h)).astype(np.float32)
        q = rng.standard_normal((nq, h)).astype(np.float32)
    gold = rng.integers(0, nc, nq).astype(np.int64)
    if not ints:
        even = np.arange(nq) % 2 == 0
        q[even] = (c[gold[even]] + 0.9 * q[even]).astype(np.float32)
    c_gid = rng.integers(0, max(2, nc // 4), nc).astype(np.int64)
    q_gid = c_gid[gold].copy()
    q_gid[np.arange(nq) % 3 == 0] = -1
    for a in (q, c, gold, q_gid, c_gid):
        a.setflags(write=False)
    return q, c, gold, q_gid, c_gid


def _reference(q, c, gold, q_gid=None, c_gid=None, sign=1.0):
    """dict: s [Nq, Nc] float64, tol, elig (bool), order (per query: the eligible rows, ranked), rank (int64; 0
    without a gold), qq [Nq] float64"""
    q64, c64 = q.astype(np.float64), c.astype(np.float64)
    nq, nc = q.shape[0], c.shape[0]
    cc = (c64 * c64).sum(1)
    s = sign * (2.0 * (q64 @ c64.T) - cc[None, :])
    qn, cn = np.linalg.norm(q64, axis=1), np.linalg.norm(c64, axis=1)
    tol = 1e-5 * (2.0 * qn[:, None] * cn[None, :] + cn[None, :] ** 2)
    elig = np.ones((nq, nc), dtype=bool)
    if q_gid is not None:
        elig = ~((c_gid[None, :] == q_gid[:, None]) & (q_gid[:, None] >= 0))
    has = gold >= 0
    elig[np.arange(nq)[has], gold[has]] = True
    idx = np.arange(nc)
    order, rank = [], np.zeros((nq,), dtype=np.int64)
    for i in range(nq):
        rows = idx[elig[i]]
        o = rows[np.lexsort((rows, -s[i, rows]))]
        order.append(o)
        if has[i]:
            rank[i] = 1 + int(np.nonzero(o == gold[i])[0][0])
    return dict(s=s, tol=tol, elig=elig, order=order, rank=rank, qq=(q64 * q64).sum(1))


@functools.lru_cache(maxsize=None)
def _case_reference(nq, nc, h, seed):
    return _reference(*_inputs(nq, nc, h, seed))


def _run(dev, q, c, gold, k, q_gid=None, c_gid=None, **kw):
    from k3m_amd import ops
    t = lambda a: None if a is None else torch.tensor(a, device=dev)
    out = ops.lp_rank(t(q), t(c), gold=t(gold), k=k, q_gid=t(q_gid), c_gid=t(c_gid), **kw)
    torch.cuda.synchronize()
    return tuple(o.cpu().numpy() for o in out)


def _bits(a):
    return a.view(np.uint32)


def _same(a, b):
    return all(np.array_equal(_bits(x) if x.dtype == np.float32 else x, _bits(y) if y.dtype == np.float32 else y)
               for x, y in zip(a, b))


def _check_list(d2, idx, ref, k, sign=1.0, c_base=0):
    """Every row, nothing exempted: exact padding, sorted, unique, eligible, each d2 within tol + 1e-5 |q|^2 of the
    float64 value at its index, no eligible row better than the k-th by more than tol left out.  Then the index must
    be the reference's wherever the float64 gap to both ranking neighbours exceeds tol (the largest tol of the
    three); returns (positions under that gap condition, positions)."""
    s, tol, elig, qq = ref["s"], ref["tol"], ref["elig"], ref["qq"]
    skipped = total = 0
    for i in range(s.shape[0]):
        order = ref["order"][i]
        n_ok = min(k, len(order))
        assert np.all(d2[i, n_ok:] == np.inf) and np.all(idx[i, n_ok:] == -1), "padding slots"
        dd, ix = d2[i, :n_ok], idx[i, :n_ok] - c_base
        assert np.all(np.isfinite(dd)) and np.all((ix >= 0) & (ix < s.shape[1]))
        assert np.all(elig[i, ix]), "eligible rows only"
        assert np.all(sign * dd[:-1] <= sign * dd[1:]), "sorted"
        assert len(set(ix.tolist())) == n_ok, "unique indices"
        want = np.maximum(qq[i] - sign * s[i, ix], 0.0)
        assert np.all(np.abs(dd - want) <= tol[i, ix] + 1e-5 * qq[i]), "d2 of its own index"
        kth = s[i, order[n_ok - 1]]
        assert np.all(s[i, ix] >= kth - tol[i, ix]), "no better row left out"
        rs, rt = s[i, order[:n_ok + 1]], tol[i, order[:n_ok + 1]]
        for p in range(n_ok):
            t = max(rt[max(p - 1, 0)], rt[p], rt[min(p + 1, len(rt) - 1)])
            clear = (p == 0 or rs[p - 1] - rs[p] > t) and (p + 1 >= len(rs) or rs[p] - rs[p + 1] > t)
            if clear:
                assert ix[p] == order[p], "index at a position with clear gaps"
            else:
                skipped += 1
        total += n_ok
    return skipped, total


def _check_rank(rank, gold_d2, gold, ref, sign=1.0):
    """lo <= rank <= hi for every query, rank == lo wherever lo == hi; returns the number of queries with lo != hi."""
    s, tol, elig, qq = ref["s"], ref["tol"], ref["elig"], ref["qq"]
    loose = 0
    for i in range(s.shape[0]):
        if gold[i] < 0:
            assert rank[i] == 0 and gold_d2[i] == np.inf
            continue
        g = s[i, gold[i]]
        other = elig[i].copy()
        other[gold[i]] = False
        lo = 1 + int(((s[i] > g + tol[i]) & other).sum())
        hi = 1 + int(((s[i] >= g - tol[i]) & other).sum())
        assert lo <= rank[i] <= hi, (i, lo, int(rank[i]), hi)
        loose += lo != hi
        want = max(qq[i] - sign * g, 0.0)
        assert abs(gold_d2[i] - want) <= tol[i, gold[i]] + 1e-5 * qq[i]
    return loose


def _check_invariant(d2, idx, gold_d2, rank, gold, k, c_base=0):
    """1 <= rank <= k: the listed position holds the gold, with gold_d2's bits; a larger rank: the gold is not listed."""
    for i in range(len(rank)):
        if 1 <= rank[i] <= k:
            assert idx[i, rank[i] - 1] == c_base + gold[i], i
            assert _bits(d2[i, rank[i] - 1:rank[i]])[0] == _bits(gold_d2[i:i + 1])[0], i
        elif gold[i] >= 0:
            assert not np.any(idx[i] == c_base + gold[i]), i


def test_exact_integer_inputs(dev):
    """Values in {-4 .. 4}: |s| <= 36,864 < 2^24, every score exact in fp32, so all four outputs equal the reference,
    ties included: the ascending-index rule of the list and of the count."""
    nq, nc, h, k = 33, 257, 768, 32
    q, c, gold, q_gid, c_gid = _inputs(nq, nc, h, 0, True)
    ref = _reference(q, c, gold, q_gid, c_gid)
    d2, idx, gold_d2, rank = _run(dev, q, c, gold, k, q_gid, c_gid)
    want_i = np.stack([o[:k] for o in ref["order"]])
    want_s = np.take_along_axis(ref["s"], want_i, 1)
    ties = int((want_s[:, :-1] == want_s[:, 1:]).sum())
    g = ref["s"][np.arange(nq), gold]
    gold_ties = int(((ref["s"] == g[:, None]) & ref["elig"]).sum() - nq)
    print("tied neighbours in the reference lists: %d, rows tied with a gold: %d" % (ties, gold_ties))
    assert ties > 0 and gold_ties > 0
    assert np.array_equal(idx, want_i)
    assert np.array_equal(d2.astype(np.float64), ref["qq"][:, None] - want_s)
    assert np.array_equal(gold_d2.astype(np.float64), ref["qq"] - g)
    assert np.array_equal(rank, ref["rank"])
    _check_invariant(d2, idx, gold_d2, rank, gold, k)


@pytest.mark.parametrize("case", CASES, ids=lambda c: "x".join(str(v) for v in c))
def test_float_inputs(dev, case):
    nq, nc, h, k, seed = case
    q, c, gold, q_gid, c_gid = _inputs(nq, nc, h, seed)
    ref = _case_reference(nq, nc, h, seed)
    c_base = 1000
    d2, idx, gold_d2, rank = _run(dev, q, c, gold, k, q_gid, c_gid, c_base=c_base)
    skipped, total = _check_list(d2, idx, ref, k, c_base=c_base)
    print("index check skipped %d of %d positions" % (skipped, total))
    assert skipped <= 0.05 * total
    loose = _check_rank(rank, gold_d2, gold, ref)
    inside = int(((rank >= 1) & (rank <= k)).sum())
    print("ranks with lo != hi: %d of %d; golds inside the top-%d: %d" % (loose, nq, k, inside))
    assert loose <= 0.25 * nq
    # the two invariants of the kernel, on the same outputs
    _check_invariant(d2, idx, gold_d2, rank, gold, k, c_base=c_base)
    for chunks in (1, 2):
        assert _same(_run(dev, q, c, gold, k, q_gid, c_gid, c_base=c_base, chunks=chunks), (d2, idx, gold_d2, rank))


def test_duplicates_of_the_gold_row(dev):
    """Copies of the gold row at one lower and one higher index tie with the gold exactly: the lower one is counted
    and listed before it, the higher one after it; with group ids equal to the gold's neither is counted or listed."""
    nq, nc, h, k = 70, 1000, 768, 10
    q, c, gold, _, _ = _inputs(nq, nc, h, 0)
    c, gold = c.copy(), np.full((nq,), 500, dtype=np.int64)
    gold[1::2] = 300 + np.arange(nq // 2)
    q = (c[gold] + 0.1 * q).astype(np.float32)   # every gold is the nearest row
    lower, upper = 37, 901                       # copies of row 500, in other tiles than the gold's
    c[lower] = c[500]
    c[upper] = c[500]
    d2, idx, gold_d2, rank = _run(dev, q, c, gold, k)
    for i in range(nq):
        if gold[i] == 500:
            assert rank[i] == 2 and idx[i, :3].tolist() == [lower, 500, upper], i
            assert len(set(_bits(d2[i, :3]).tolist())) == 1 and _bits(d2[i, 1:2])[0] == _bits(gold_d2[i:i + 1])[0]
        else:
            assert rank[i] == 1 and idx[i, 0] == gold[i], i
    c_gid = np.arange(nc, dtype=np.int64)
    c_gid[[lower, 500, upper]] = 5000
    q_gid = c_gid[gold].copy()
    f = _run(dev, q, c, gold, k, q_gid, c_gid)
    assert np.all(f[3] == 1) and np.array_equal(f[1][:, 0], gold)
    assert not np.any((f[1] == lower) | (f[1] == upper))
    assert np.array_equal(_bits(f[2]), _bits(gold_d2))
    # a query without a group id sees every row again
    q_gid[0] = -1
    f = _run(dev, q, c, gold, k, q_gid, c_gid)
    assert f[3][0] == 2 and f[1][0, :3].tolist() == [lower, 500, upper]


def test_chunk_and_tiling_invariance(dev):
    nq, nc, h, k = 70, 1000, 768, 10
    q, c, gold, q_gid, c_gid = _inputs(nq, nc, h, 0)
    base = _run(dev, q, c, gold, k, q_gid, c_gid, chunks=1)
    for chunks in (3, 0):
        assert _same(_run(dev, q, c, gold, k, q_gid, c_gid, chunks=chunks), base), chunks
    # Nq = 64 runs the 256-row x 64-query tiling, Nq = 65 the 128 x 128 one
    few = _run(dev, q[:64], c, gold[:64], k, q_gid[:64], c_gid)
    more = _run(dev, q[:65], c, gold[:65], k, q_gid[:65], c_gid)
    assert _same(few, tuple(a[:64] for a in more))
    assert _same(few, tuple(a[:64] for a in base))
    for chunks in (2, 4):
        assert _same(_run(dev, q[:64], c, gold[:64], k, q_gid[:64], c_gid, chunks=chunks), few), chunks


def test_farthest(dev):
    nq, nc, h, k, seed = 33, 257, 768, 32, 1
    q, c, gold, q_gid, c_gid = _inputs(nq, nc, h, seed)
    ref = _reference(q, c, gold, q_gid, c_gid, sign=-1.0)
    d2, idx, gold_d2, rank = _run(dev, q, c, gold, k, q_gid, c_gid, farthest=True)
    skipped, total = _check_list(d2, idx, ref, k, sign=-1.0)
    print("index check skipped %d of %d positions" % (skipped, total))
    assert skipped <= 0.05 * total
    loose = _check_rank(rank, gold_d2, gold, ref, sign=-1.0)
    print("ranks with lo != hi: %d of %d" % (loose, nq))
    assert loose <= 0.25 * nq
    _check_invariant(d2, idx, gold_d2, rank, gold, k)
    # integers: equal to the reference
    q, c, gold, q_gid, c_gid = _inputs(nq, nc, h, 0, True)
    ref = _reference(q, c, gold, q_gid, c_gid, sign=-1.0)
    d2, idx, gold_d2, rank = _run(dev, q, c, gold, k, q_gid, c_gid, farthest=True)
    assert np.array_equal(idx, np.stack([o[:k] for o in ref["order"]]))
    assert np.array_equal(rank, ref["rank"])
    assert np.array_equal(gold_d2.astype(np.float64), ref["qq"] + ref["s"][np.arange(nq), gold])


def test_edge_cases(dev):
    from k3m_amd import ops
    # no gold: rank 0 and gold_d2 = +inf, for single queries and for gold=None; the list is the same
    nq, nc, h, k = 70, 1000, 768, 10
    q, c, gold, _, _ = _inputs(nq, nc, h, 0)
    base = _run(dev, q, c, gold, k)
    g2 = gold.copy()
    g2[[3, 40]] = -1
    some = _run(dev, q, c, g2, k)
    assert some[3][3] == 0 and some[3][40] == 0 and some[2][3] == np.inf and some[2][40] == np.inf
    keep = g2 >= 0
    assert _same(tuple(a[keep] for a in some), tuple(a[keep] for a in base))
    none = _run(dev, q, c, None, k)
    assert np.all(none[3] == 0) and np.all(none[2] == np.inf) and _same(none[:2], base[:2])
    # k at its maximum, both tilings
    for n in (33, 70):
        qq_, cc_, gg_, qg_, cg_ = _inputs(n, 1000, 768, 0)
        ref = _reference(qq_, cc_, gg_, qg_, cg_)
        d2, idx, gold_d2, rank = _run(dev, qq_, cc_, gg_, MAX_K, qg_, cg_)
        _check_list(d2, idx, ref, MAX_K)
        _check_rank(rank, gold_d2, gg_, ref)
        _check_invariant(d2, idx, gold_d2, rank, gg_, MAX_K)
    # all-zero candidates: finite values, ties in index order
    z = np.zeros((300, 768), dtype=np.float32)
    gz = np.array([0, 7, 299, -1] + [5] * 29, dtype=np.int64)
    d2, idx, gold_d2, rank = _run(dev, q[:33], z, gz, 10)
    assert np.all(np.isfinite(d2)) and np.array_equal(idx, np.tile(np.arange(10), (33, 1)))
    assert rank[:4].tolist() == [1, 8, 300, 0] and np.all(rank[4:] == 6)
    assert np.all(_bits(d2) == _bits(d2[:, :1])) and np.array_equal(_bits(gold_d2[:3]), _bits(d2[:3, 0]))
    # no query
    out = ops.lp_rank(torch.empty((0, 768), device=dev), torch.tensor(c, device=dev), k=4,
                      gold=torch.empty((0,), dtype=torch.int64, device=dev))
    torch.cuda.synchronize()
    assert [tuple(o.shape) for o in out] == [(0, 4), (0, 4), (0,), (0,)]


def test_argument_errors(dev):
    from k3m_amd import _lib
    lib = _lib.load()
    q = torch.zeros((4, 8), device=dev)
    c = torch.zeros((6, 8), device=dev)
    d2 = torch.full((4, 2), 7.0, device=dev)
    idx = torch.full((4, 2), 7, dtype=torch.int64, device=dev)
    gd = torch.full((4,), 7.0, device=dev)
    rk = torch.full((4,), 7, dtype=torch.int64, device=dev)
    gid = torch.zeros((6,), dtype=torch.int64, device=dev)
    ws = torch.empty((1 << 16,), dtype=torch.uint8, device=dev)
    nb = ctypes.c_longlong(0)
    EINVAL = 1

    def raw(nc=6, h=8, k=2, farthest=0, q_gid=None, c_gid=None, chunks=0, ws_bytes=ws.numel(), qp=q.data_ptr()):
        return lib.k3m_lp_rank(qp, c.data_ptr(), 4, nc, h, k, farthest, 0, None, q_gid, c_gid, chunks, d2.data_ptr(),
                               idx.data_ptr(), gd.data_ptr(), rk.data_ptr(), ws.data_ptr(), ws_bytes, _lib.stream())

    for h, k in ((8, 0), (8, MAX_K + 1), (8, 64), (6, 2), (4100, 2)):
        assert lib.k3m_lp_rank_ws_bytes(4, 6, h, k, 0, ctypes.addressof(nb)) == EINVAL
        assert raw(h=h, k=k) == EINVAL
    assert lib.k3m_lp_rank_ws_bytes(4, 0, 8, 2, 0, ctypes.addressof(nb)) == EINVAL
    assert raw(nc=0) == EINVAL
    assert raw(chunks=-1) == EINVAL
    assert raw(farthest=2) == EINVAL
    assert raw(ws_bytes=16) == EINVAL                       # too small a workspace
    assert raw(c_gid=gid.data_ptr()) == EINVAL              # one group-id array without the other
    assert raw(qp=q.data_ptr() + 4) == EINVAL               # a misaligned pointer
    torch.cuda.synchronize()
    assert bool((d2 == 7.0).all()) and bool((idx == 7).all()) and bool((gd == 7.0).all()) and bool((rk == 7).all())
    assert lib.k3m_lp_rank_ws_bytes(4, 6, 8, 2, 0, ctypes.addressof(nb)) == 0 and nb.value > 0
    assert raw() == 0
    torch.cuda.synchronize()
    assert bool((rk == 0).all()) and bool((idx[:, 0] == 0).all())
