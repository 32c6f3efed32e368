"""The classify.py driver on the GPU, in fresh child processes: --do_train --do_eval --do_pred on a 24-row product TSV
with three categories (one validation row has none), then evaluation and prediction alone from the files the training
run left (the epoch .bin through --file_state_dict, labels.json)."""
import json
import os
import shutil
import subprocess
import sys

import pytest
import torch

from golden_util import CFG_PATH, HERE, REPO

pytestmark = pytest.mark.gpu
CK_DIR = "k3m_bert-base-uncased_12l_12h"
CATES = ["bags", "hats", "shoes"]


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda")


def _run(tmp_path, *extra):
    out = tmp_path / "out"
    out.mkdir(exist_ok=True)
    shutil.copy(CFG_PATH, out / "bert_base_6layer_6conect.json")
    cmd = ["timeout", "-k", "10", "300", sys.executable, os.path.join(REPO, "classify.py"), "--data_dir", str(tmp_path),
           "--output_dir", str(out), "--file_name", "items_{}.tsv", "--use_image", "--with_coattention",
           "--k3m_char_tokenizer", "--k3m_synthetic_regions", "5", "--train_batch_size", "4", "--eval_batch_size", "4",
           "--max_seq_length", "36", "--max_seq_length_pv", "128", "--max_num_pv", "20", "--eval_topk", "2"] + list(extra)
    r = subprocess.run(cmd, cwd=str(tmp_path), capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    return out / CK_DIR, r


def _rows(lo, hi, blank=None):
    lines = []
    for i in range(lo, hi):
        pv = "#;#".join("p%d%d#:#v%d%d" % (i, j, j, i) for j in range(3 + i % 4))
        cate = "" if i == blank else CATES[i % 3]
        lines.append("%d\titem title %d with words\thttp://img/%d.jpg\t%s\t%s" % (1000 + i, i, i, pv, cate))
    return "\n".join(lines) + "\n"


def _eval_line(r):
    lines = [l for l in r.stdout.splitlines() if "accuracy@1=" in l]
    assert len(lines) == 1, r.stdout[-2000:]
    assert "accuracy@2=" in lines[0] and "macro_f1=" in lines[0] and "n=7," in lines[0] and "left_out=1" in lines[0]
    return lines[0]


def _predictions(path):
    rows = [json.loads(l) for l in open(path, encoding="utf-8")]
    assert [r["item_id"] for r in rows] == [str(1000 + i) for i in range(16, 24)]
    for r in rows:
        assert list(r) == ["item_id", "pred", "logp"]
        assert len(r["pred"]) == 2 and set(r["pred"]) <= set(CATES) and r["logp"][0] >= r["logp"][1]
    return rows


def test_train_eval_pred_on_a_product_tsv(dev, tmp_path):
    (tmp_path / "items_train.tsv").write_text(_rows(0, 16), encoding="utf-8")
    (tmp_path / "items_valid.tsv").write_text(_rows(16, 24, blank=19), encoding="utf-8")
    ck, r = _run(tmp_path, "--do_train", "--do_eval", "--do_pred", "--k3m_max_steps", "2", "--num_train_epochs", "1",
                 "--class_weights", "balanced", "--label_smoothing", "0.1")
    sd = torch.load(str(ck / "K3M_item_classification-1_epoch-0.bin"), map_location="cpu", weights_only=True)
    inv = json.load(open(os.path.join(HERE, "golden", "param_inventory_finetune.json")))
    assert set(sd) == set(inv["ce_state_dict_keys"])
    assert tuple(sd["classifier.out_proj.weight"].shape) == (3, 768)
    assert all(torch.isfinite(v).all() for v in sd.values())
    labels = json.load(open(ck / "labels.json", encoding="utf-8"))
    assert labels["names"] == CATES and sum(labels["counts"]) == 16
    _eval_line(r)
    first = _predictions(ck / "classification_top2.jsonl")
    # evaluation and prediction alone: labels.json and the .bin of the run above
    out = tmp_path / "again.jsonl"
    _, r2 = _run(tmp_path, "--do_eval", "--do_pred", "--file_state_dict",
                 str(ck / "K3M_item_classification-1_epoch-0.bin"), "--k3m_pred_output", str(out))
    os.remove(ck / "K3M_item_classification-1_epoch-0.bin")   # 1 GB: not left in the session's temporary directory
    _eval_line(r2)
    again = _predictions(out)
    assert [a["pred"] for a in again] == [b["pred"] for b in first]
