"""Host side of item retrieval, no GPU: rank_metrics, ItemIndex.add validation, ops.topk_sim argument
validation (before any library call) and the driver's new flags."""
import os
import sys

import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_rank_metrics_by_hand():
    from k3m_amd.retrieve import rank_metrics
    ids = [["a", "b", "c"],        # truth first
           ["x", None, "b"],       # truth third, an empty slot before it
           ["x", "y", "z"],        # truth absent
           [None, None, None]]     # nothing retrieved
    truth = ["a", "b", "q", "a"]
    m = rank_metrics(ids, truth, ks=(1, 2, 3))
    assert m == {"rank@1": 0.25, "rank@2": 0.25, "rank@3": 0.5}
    assert list(rank_metrics(ids, truth)) == ["rank@1", "rank@5", "rank@10"]
    assert rank_metrics(ids, truth)["rank@10"] == 0.5


def test_rank_metrics_set_truth_none_and_empty():
    from k3m_amd.retrieve import rank_metrics
    ids = [[7, 8, 9], [1, 2, 3], [None, 5, None]]
    truth = [{9, 100}, (4, 5), {None}]   # any one counts; a None truth never matches an empty slot
    m = rank_metrics(ids, truth, ks=(1, 3))
    assert m == {"rank@1": 0.0, "rank@3": 1.0 / 3.0}
    assert rank_metrics([], [], ks=(1, 5)) == {"rank@1": 0.0, "rank@5": 0.0}
    with pytest.raises(ValueError):
        rank_metrics([[1]], [1, 2])


def test_item_index_add_validation():
    from k3m_amd.retrieve import ItemIndex
    with pytest.raises(ValueError):
        ItemIndex(metric="l2")
    index = ItemIndex(device="cpu")
    assert len(index) == 0
    ok = torch.zeros((2, 8))
    for ids, emb in ((["a", "b"], torch.zeros((2, 8), dtype=torch.float64)),   # dtype
                     (["a", "b"], torch.zeros((2, 8), dtype=torch.bfloat16)),
                     (["a", "b"], torch.zeros((8,))),                           # not 2-D
                     (["a"], ok),                                               # ids / rows
                     (["a", "b"], torch.zeros((2, 6))),                         # H no multiple of 4
                     (["a", "b"], [[0.0] * 8] * 2)):                            # not a tensor
        with pytest.raises(ValueError):
            index.add(ids, emb)
    assert len(index) == 0 and index.blocks == []
    index.add(["a", "b"], ok)
    assert len(index) == 2 and index.hidden == 8
    with pytest.raises(ValueError):
        index.add(["c"], torch.zeros((1, 12)))   # another H
    index.add(["c"], torch.ones((1, 8)))
    assert len(index) == 3 and index.ids == ["a", "b", "c"] and index.embeddings().shape == (3, 8)


def test_item_index_blocks_and_save_load(tmp_path):
    from k3m_amd.retrieve import ItemIndex
    index = ItemIndex(metric="inner", device="cpu", block_rows=4)
    e = torch.arange(7 * 8, dtype=torch.float32).reshape(7, 8)
    index.add([10, 11, 12], e[:3])
    index.add([13, 14, 15, 16], e[3:])
    assert [b.shape[0] for b in index.blocks] == [4, 3] and torch.equal(index.embeddings(), e)
    index.save(str(tmp_path / "i"))
    back = ItemIndex.load(str(tmp_path / "i"), device="cpu")
    assert back.ids == [10, 11, 12, 13, 14, 15, 16] and back.metric == "inner" and back.block_rows == 4
    assert torch.equal(back.embeddings(), e)
    mixed = ItemIndex(device="cpu")
    mixed.add([1, ("t",)], torch.zeros((2, 8)))
    with pytest.raises(ValueError):
        mixed.save(str(tmp_path / "m"))


def test_topk_sim_validates_before_any_library_call(monkeypatch):
    from k3m_amd import ops

    def no_call(*a, **kw):
        raise AssertionError("library call before validation")

    monkeypatch.setattr(ops, "call", no_call)
    q, c = torch.zeros((4, 8)), torch.zeros((6, 8))
    bad = [dict(k=0), dict(k=65), dict(k=2.0), dict(k=2, metric="l2"), dict(k=2, chunks=-1),
           dict(k=2, accumulate=True),
           dict(k=2, q_ids=torch.zeros((4,), dtype=torch.int32)), dict(k=2, q_ids=torch.zeros((5,), dtype=torch.int64)),
           dict(k=2, out=(torch.zeros((4, 3)), torch.zeros((4, 3), dtype=torch.int64))),
           dict(k=2, out=(torch.zeros((4, 2)), torch.zeros((4, 2), dtype=torch.int32)))]
    for kw in bad:
        with pytest.raises(ValueError):
            ops.topk_sim(q, c, **kw)
    for qq, cc in ((torch.zeros((4, 6)), torch.zeros((6, 6))),       # H = 6
                   (torch.zeros((4, 4100)), torch.zeros((6, 4100))),  # H > 4096
                   (q, torch.zeros((6, 12))),                         # H differs
                   (q.double(), c), (q, c.to(torch.bfloat16)),        # dtype
                   (torch.zeros((4, 16))[:, :8], c),                  # not contiguous
                   (torch.zeros((8,)), c)):                           # not 2-D
        with pytest.raises(ValueError):
            ops.topk_sim(qq, cc, 2)
    with pytest.raises(AssertionError):   # valid arguments do reach the library
        ops.topk_sim(q, c, 2)


def test_driver_flags_parse_and_default_off():
    sys.path.insert(0, REPO)
    try:
        import finetune as driver
    finally:
        sys.path.remove(REPO)
    base = ["--data_dir", "d", "--output_dir", "o", "--file_name", "f_{}"]
    a, r = driver.parse_args(base)
    assert r.do_retrieve is False and r.k3m_topk == 10 and r.k3m_retrieve_output == ""
    assert vars(a) == vars(driver.build_parser().parse_args(base))   # the other options: as without the new ones
    a, r = driver.parse_args(base[:2] + ["--do_retrieve", "--k3m_topk", "5"] + base[2:] +
                             ["--k3m_retrieve_output", "r.jsonl", "--do_pred"])
    assert r.do_retrieve is True and r.k3m_topk == 5 and r.k3m_retrieve_output == "r.jsonl"
    assert a.do_train is False and a.do_eval is False and a.do_pred is True and a.data_dir == "d"
    with pytest.raises(SystemExit):
        driver.parse_args(base + ["--k3m_no_such_option"])
