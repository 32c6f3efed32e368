"""k3m_amd.retrieve on the GPU: build_index over the forward-only item embeddings, ItemIndex.search
against a float64 reference of the stored rows, save / load, and the driver's --do_retrieve in a child process.
Items: k3m_amd.synthetic's (T 36, P 128, 37 regions), 6 of them in batches of 2."""
import json
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest
import torch

from golden_util import CFG_PATH, REPO

pytestmark = pytest.mark.gpu
TOL = 1e-5   # cosine: the fp32 kernel tolerance
SEED = 5
_EMBED = {"input_ids": "input_ids", "token_type_ids": "segment_ids", "attention_mask": "input_mask",
          "input_ids_pv": "input_ids_pv", "token_type_ids_pv": "segment_ids_pv", "attention_mask_pv": "input_mask_pv",
          "index_p": "index_p", "index_v": "index_v", "image_feat": "image_feat", "image_loc": "image_loc",
          "image_attention_mask": "image_mask"}


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda")


@pytest.fixture(scope="module")
def built(dev):
    """(model, item batches, the index built from them), once for the module"""
    from k3m_amd.config import finetune_config
    from k3m_amd.finetune import K3MForItemAlignment
    from k3m_amd.retrieve import build_index
    from k3m_amd.synthetic import synthetic_batch
    from k3m_amd.weights import param_values
    cfg = finetune_config(CFG_PATH, loss_type="cosine", if_pre_sampling=1)
    model = K3MForItemAlignment(cfg, dev)
    model.engine.fp.load(param_values(cfg, 7))
    batches = []
    for b in range(3):
        sb = synthetic_batch(cfg, 2, dev, seed=40 + b)
        batch = {dst: sb[src] for dst, src in _EMBED.items()}
        batch["item_ids"] = ["item-%d" % (2 * b), "item-%d" % (2 * b + 1)]
        batches.append(batch)
    index = build_index(model, batches, seed=SEED)
    torch.cuda.synchronize()
    return model, batches, index


def _reference(e, k):
    """float64 cosine neighbours of every stored row among the others: (scores [n, k], rows [n, k], all scores)"""
    e64 = e.astype(np.float64)
    n = np.linalg.norm(e64, axis=1)
    s = (e64 @ e64.T) / (n[:, None] * n[None, :])
    np.fill_diagonal(s, -np.inf)
    order = np.stack([np.lexsort((np.arange(len(e)), -s[i])) for i in range(len(e))])[:, :k]
    return np.take_along_axis(s, order, 1), order, s


def _check_search(index, e, got):
    scores, rows, ids = got
    scores, rows = scores.cpu().numpy(), rows.cpu().numpy()
    want_s, want_r, s = _reference(e, 3)
    assert scores.shape == rows.shape == (6, 3)
    for i in range(6):
        assert i not in rows[i] and len(set(rows[i].tolist())) == 3
        assert np.all(np.abs(scores[i] - s[i, rows[i]]) <= TOL)
        assert np.all(np.abs(scores[i] - want_s[i]) <= TOL)
        full = np.sort(s[i])[::-1]
        for p in range(3):   # the reference's neighbour wherever its float64 gaps are clear of the tolerance
            if (p == 0 or full[p - 1] - full[p] > 2 * TOL) and full[p] - full[p + 1] > 2 * TOL:
                assert rows[i, p] == want_r[i, p]
        assert ids[i] == [index.ids[r] for r in rows[i]]


def test_index_rows_are_item_embedding_bits(built):
    model, batches, index = built
    assert len(index) == 6 and index.ids == ["item-%d" % i for i in range(6)]
    stored = index.embeddings()
    assert stored.shape == (6, 768) and bool(torch.isfinite(stored).all())
    assert len({tuple(r) for r in stored.cpu().numpy().tolist()}) == 6   # six different items
    for b, batch in enumerate(batches):
        kw = {k: v for k, v in batch.items() if k != "item_ids"}
        _, cf = model.item_embedding(seed=SEED + b, **kw)
        assert torch.equal(stored[2 * b:2 * b + 2], cf)


def test_search_against_itself(built):
    from k3m_amd.retrieve import build_index
    model, batches, index = built
    e = index.embeddings()
    got = index.search(e, 3, query_ids=index.ids)
    torch.cuda.synchronize()
    _check_search(index, e.cpu().numpy(), got)
    again = build_index(model, batches, seed=SEED)
    assert torch.equal(again.embeddings(), e)
    got2 = again.search(again.embeddings(), 3, query_ids=again.ids)
    assert torch.equal(got2[0], got[0]) and torch.equal(got2[1], got[1]) and got2[2] == got[2]
    # stored in blocks of 4 + 2 rows: the same bits through the accumulate path
    from k3m_amd.retrieve import ItemIndex
    small = ItemIndex(device=index.device, block_rows=4)
    small.add(index.ids, e)
    assert [b.shape[0] for b in small.blocks] == [4, 2]
    got3 = small.search(e, 3, query_ids=index.ids)
    assert torch.equal(got3[0], got[0]) and torch.equal(got3[1], got[1]) and got3[2] == got[2]
    # k beyond the catalogue: padding maps to None
    _, rows, ids = index.search(e[:2], 8, query_ids=index.ids[:2])
    assert rows[:, 5:].eq(-1).all() and all(r[5:] == [None] * 3 and None not in r[:5] for r in ids)


def test_save_and_load(built, tmp_path):
    from k3m_amd.retrieve import ItemIndex
    _, _, index = built
    index.save(str(tmp_path / "idx"))
    assert all(f.endswith(".npy") for f in os.listdir(tmp_path / "idx"))
    back = ItemIndex.load(str(tmp_path / "idx"), device=index.device)
    assert back.ids == index.ids and back.metric == index.metric and len(back) == 6
    e = index.embeddings()
    assert torch.equal(back.embeddings(), e)
    a = index.search(e, 3, query_ids=index.ids)
    b = back.search(e, 3, query_ids=index.ids)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and a[2] == b[2]


def test_driver_do_retrieve(dev, tmp_path):
    """finetune.py --do_retrieve on the six-pair record directory of tests/test_gpu_finetune_driver.py."""
    from k3m_amd.loaders import read_raw_tsv, write_pair_records
    lines = []
    for i in range(12):
        pv = "#;#".join("p%d%d#:#v%d%d" % (i, j, j, i) for j in range(3 + i % 4))
        lines.append("%d\titem title %d with words\thttp://img/%d.jpg\t%s\tcat" % (1000 + i, i, i, pv))
    (tmp_path / "rows.tsv").write_text("\n".join(lines) + "\n", encoding="utf-8")
    recs = read_raw_tsv(str(tmp_path / "rows.tsv"), synthetic_regions=5)
    pairs = [(float(i % 2), recs[2 * i], recs[2 * i + 1]) for i in range(6)]
    write_pair_records(str(tmp_path / "pairs_valid"), pairs)
    out = tmp_path / "out"
    out.mkdir()
    shutil.copy(CFG_PATH, out / "bert_base_6layer_6conect.json")
    dest = tmp_path / "retrieved.jsonl"
    cmd = ["timeout", "-k", "10", "300", sys.executable, os.path.join(REPO, "finetune.py"), "--data_dir", str(tmp_path),
           "--output_dir", str(out), "--file_name", "pairs_{}", "--use_image", "--with_coattention", "--do_retrieve",
           "--k3m_topk", "3", "--k3m_retrieve_output", str(dest), "--k3m_char_tokenizer", "--eval_batch_size", "3",
           "--max_seq_length", "36", "--max_seq_length_pv", "128", "--max_num_pv", "20"]
    r = subprocess.run(cmd, cwd=str(tmp_path), capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    rows = [json.loads(l) for l in open(dest, encoding="utf-8")]
    assert len(rows) == 6 and all(list(x) == ["src_item_id", "tgt_item_ids", "scores"] for x in rows)
    tgt = {str(1000 + 2 * i + 1) for i in range(6)}
    assert [x["src_item_id"] for x in rows] == [str(1000 + 2 * i) for i in range(6)]
    for x in rows:
        assert len(x["tgt_item_ids"]) == 3 == len(x["scores"]) and len(set(x["tgt_item_ids"])) == 3
        assert set(x["tgt_item_ids"]) <= tgt
        assert all(-1.0 - TOL <= s <= 1.0 + TOL for s in x["scores"]) and x["scores"] == sorted(x["scores"], reverse=True)
    rank = [l for l in r.stdout.splitlines() if l.startswith("[Retrieval] Rank@1=")]
    assert len(rank) == 1 and "Rank@5=" in rank[0] and "Rank@10=" in rank[0]
    shares = [float(p.split("=")[1]) for p in rank[0][len("[Retrieval] "):].split(", ")]
    assert all(0.0 <= s <= 1.0 for s in shares) and shares == sorted(shares)
