"""Host side of link-prediction evaluation, no GPU: link_metrics, value_keys / property_keys, the argument
checks of ops.lp_rank (raised before any library call) and the train.py options."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from golden_util import REPO


def test_link_metrics():
    from k3m_amd.linkpred import link_metrics
    m = link_metrics(torch.tensor([1, 2, 4, 0, 10, 0]), ks=(1, 3, 10))
    assert m["n"] == 4 and m["skipped"] == 2
    assert m["mr"] == pytest.approx(17 / 4) and m["mrr"] == pytest.approx((1 + 0.5 + 0.25 + 0.1) / 4)
    assert m["hits@1"] == 0.25 and m["hits@3"] == 0.5 and m["hits@10"] == 1.0
    z = link_metrics(np.array([0, 0]), ks=(1, 5))
    assert z == {"n": 0, "mr": 0.0, "mrr": 0.0, "hits@1": 0.0, "hits@5": 0.0, "skipped": 2}
    assert link_metrics([], ks=())["n"] == 0


def _batch():
    """2 items, P 16, NPV 4: item 0 holds 3 triples, item 1 holds 1; the value spans of (0, 0) and (1, 0) carry the
    same tokens, (0, 2)'s differs from (0, 0)'s in one token; one token of (1, 0) is masked."""
    ids = torch.zeros((2, 16), dtype=torch.int64)
    ids[0, :12] = torch.tensor([101, 7, 8, 9, 20, 21, 7, 8, 9, 20, 22, 102])
    ids[1, :8] = torch.tensor([101, 30, 5, 20, 21, 102, 0, 0])
    lab = torch.full((2, 16), -1, dtype=torch.int64)
    ids[1, 4] = 103   # [MASK] over the original 21
    lab[1, 4] = 21
    index_p = torch.zeros((2, 4, 2), dtype=torch.int64)
    index_v = torch.zeros((2, 4, 2), dtype=torch.int64)
    index_p[0, 0], index_v[0, 0] = torch.tensor([1, 3]), torch.tensor([4, 5])
    index_p[0, 1], index_v[0, 1] = torch.tensor([6, 8]), torch.tensor([9, 9])
    index_p[0, 2], index_v[0, 2] = torch.tensor([1, 2]), torch.tensor([9, 10])
    index_p[1, 0], index_v[1, 0] = torch.tensor([1, 2]), torch.tensor([3, 4])
    index_v[1, 1] = torch.tensor([3, 4])   # past nvalid: index_p[1, 1, 0] == 0
    return {"input_ids_pv": ids, "lm_label_ids_pv": lab, "index_p": index_p, "index_v": index_v}


def test_value_and_property_keys():
    from k3m_amd.linkpred import property_keys, value_keys
    b = _batch()
    vk, pk = value_keys(b), property_keys(b)
    assert vk.dtype == torch.int64 and vk.shape == (2, 4) and pk.shape == (2, 4)
    assert vk[0, 3] == -1 and vk[1, 1:].tolist() == [-1, -1, -1] and pk[1, 1] == -1   # -1 past nvalid
    assert bool((vk[0, :3] >= 0).all()) and vk[1, 0] >= 0
    assert vk[0, 0] == vk[1, 0]                       # equal spans, one of them masked and restored by its label
    assert len({int(vk[0, 0]), int(vk[0, 1]), int(vk[0, 2])}) == 3
    assert pk[0, 0] == pk[0, 1] and pk[0, 0] != pk[0, 2]   # (7, 8, 9) twice; (7, 8)
    unmasked = dict(b)
    del unmasked["lm_label_ids_pv"]                   # without the labels the [MASK] id is hashed
    assert value_keys(unmasked)[1, 0] != vk[1, 0] and value_keys(unmasked)[0, 0] == vk[0, 0]
    # the plain FNV-1a of the span's token ids, four little-endian bytes each, sign bit cleared
    h = 0xCBF29CE484222325
    for tok in (20, 21):
        for byte in int(tok).to_bytes(4, "little"):
            h = ((h ^ byte) * 0x100000001B3) % 2 ** 64
    assert int(vk[0, 0]) == h & (2 ** 63 - 1)


def test_value_keys_are_stable_across_processes():
    from k3m_amd.linkpred import value_keys
    code = ("import sys; sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
            "from test_linkpred_host import _batch\n"
            "from k3m_amd.linkpred import value_keys\n"
            "print(value_keys(_batch()).tolist())\n" % (REPO, os.path.join(REPO, "tests")))
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=120,
                         env=dict(os.environ, PYTHONHASHSEED="123"))
    assert out.returncode == 0, out.stderr[-2000:]
    assert out.stdout.strip() == str(value_keys(_batch()).tolist())


def test_lp_rank_validates_before_any_library_call(monkeypatch):
    from k3m_amd import ops

    def boom(*a, **k):
        raise AssertionError("library call")
    monkeypatch.setattr(ops, "call", boom)
    q, c = torch.zeros((4, 8)), torch.zeros((6, 8))
    gold = torch.zeros((4,), dtype=torch.int64)
    gq, gc = torch.zeros((4,), dtype=torch.int64), torch.zeros((6,), dtype=torch.int64)
    bad = [dict(k=0), dict(k=ops.LP_RANK_MAX_K + 1), dict(k=True), dict(k=2.0), dict(chunks=-1), dict(chunks=1.5),
           dict(c_base=0.5), dict(farthest=1), dict(gold=gold[:3]), dict(gold=gold.to(torch.int32)),
           dict(gold=torch.zeros((8,), dtype=torch.int64)[::2]), dict(q_gid=gq), dict(c_gid=gc),
           dict(q_gid=gq, c_gid=gc[:5]), dict(q_gid=gq.float(), c_gid=gc), dict(gold=[0, 1, 2, 3])]
    for kw in bad:
        with pytest.raises(ValueError):
            ops.lp_rank(q, c, **kw)
    for qq, cc in ((q[0], c), (q, c[0]), (q.double(), c), (q, c.double()), (torch.zeros((4, 16))[:, ::2], c),
                   (q, torch.zeros((6, 12))), (torch.zeros((4, 6)), torch.zeros((6, 6))),
                   (torch.zeros((4, 4100)), torch.zeros((6, 4100))), (q, torch.zeros((0, 8))),
                   (q.numpy(), c)):
        with pytest.raises(ValueError):
            ops.lp_rank(qq, cc, k=2)
    with pytest.raises(AssertionError, match="library call"):   # valid arguments reach the library
        ops.lp_rank(q, c, gold=gold, k=2, q_gid=gq, c_gid=gc)


def test_train_py_options():
    sys.path.insert(0, REPO)
    import train
    base = ["--data_dir", "d", "--output_dir", "o", "--file_name", "f"]
    a = train.get_parser(base)
    assert a.k3m_eval_lpm == 0 and a.k3m_lpm_output == "" and a.k3m_lpm_farthest is False
    a = train.get_parser(base + ["--k3m_eval_lpm", "10", "--k3m_lpm_output", "x.jsonl", "--k3m_lpm_farthest"])
    assert a.k3m_eval_lpm == 10 and a.k3m_lpm_output == "x.jsonl" and a.k3m_lpm_farthest is True
    with pytest.raises(SystemExit):
        train.get_parser(base + ["--k3m_eval_lpm", "ten"])
