"""Host side of masked-position prediction, no GPU: predict.masked_metrics / MaskedEval on hand-made
results, the two train.py options, and the checkable shares of the fixture recomputed from the .npz."""
import json
import math
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(HERE, "golden"))


def _result():
    # three title rows: gold first; gold third; gold absent from the list.  One PV row without a gold (-1).
    t = {"pos": torch.tensor([[0, 1], [0, 4], [1, 2]]),
         "idx": torch.tensor([[7, 1, 2, 3, 4], [9, 8, 7, 6, 5], [1, 2, 3, 4, 5]]),
         "logprob": torch.full((3, 5), -1.0), "lse": torch.zeros(3),
         "gold": torch.tensor([7, 7, 7]), "gold_logprob": torch.tensor([-0.5, -1.5, -4.0])}
    pv = {"pos": torch.tensor([[0, 3], [1, 3]]), "idx": torch.tensor([[4, 5, 6, 7, 8], [4, 5, 6, 7, 8]]),
          "logprob": torch.full((2, 5), -2.0), "lse": torch.zeros(2),
          "gold": torch.tensor([-1, 5]), "gold_logprob": torch.tensor([-math.inf, -2.0])}
    v = {"pos": torch.tensor([[0, 0]]), "idx": torch.tensor([[3, 2, 1, 0, 9]]), "logprob": torch.full((1, 5), -3.0),
         "lse": torch.zeros(1)}   # no gold known: not scored
    return {"t": t, "pv": pv, "v": v}


def test_masked_metrics_by_hand():
    from k3m_amd import predict
    m = predict.masked_metrics(_result(), ks=(1, 3, 5))
    assert set(m) == {"t", "pv"}
    assert m["t"]["n"] == 3
    assert m["t"]["acc@1"] == pytest.approx(1 / 3) and m["t"]["acc@3"] == pytest.approx(2 / 3)
    assert m["t"]["acc@5"] == pytest.approx(2 / 3)
    assert m["t"]["nll"] == pytest.approx(2.0)
    assert m["pv"] == {"n": 1, "nll": pytest.approx(2.0), "acc@1": 0.0, "acc@3": 1.0, "acc@5": 1.0}
    with pytest.raises(ValueError):
        predict.masked_metrics(_result(), ks=(1, 10))   # a top-5 result has no accuracy@10
    empty = {"t": {"idx": torch.zeros((0, 5), dtype=torch.int64), "gold": torch.zeros((0,), dtype=torch.int64),
                   "gold_logprob": torch.zeros((0,))}}
    e = predict.masked_metrics(empty, ks=(1,))["t"]
    assert e["n"] == 0 and math.isnan(e["nll"]) and math.isnan(e["acc@1"])


def test_masked_eval_sums_batches_and_writes_lines(tmp_path):
    from k3m_amd import predict
    assert predict.eval_ks(5) == (1, 5) and predict.eval_ks(10) == (1, 5, 10) and predict.eval_ks(3) == (1, 3)
    path = tmp_path / "pred.jsonl"
    ev = predict.MaskedEval(5, str(path))
    ev.add(_result(), ["a", "b"])
    ev.add(_result(), ["c", "d"])
    ev.close()
    s = ev.summary()
    assert s["t"]["n"] == 6 and s["t"]["acc@1"] == pytest.approx(1 / 3) and s["t"]["nll"] == pytest.approx(2.0)
    assert s["pv"]["n"] == 2 and s["pv"]["acc@5"] == 1.0
    lines = [json.loads(ln) for ln in path.read_text().splitlines()]
    assert len(lines) == 12   # (3 title + 2 PV + 1 region) x 2 batches
    first = lines[0]
    assert first == {"item_id": "a", "stream": "t", "position": 1, "gold": 7,
                     "topk": [[7, -1.0], [1, -1.0], [2, -1.0], [3, -1.0], [4, -1.0]]}
    assert lines[2]["item_id"] == "b" and lines[5]["stream"] == "v" and lines[5]["gold"] is None
    assert lines[6]["item_id"] == "c"


def test_train_parser_options_and_defaults():
    sys.path.insert(0, REPO)
    import train
    base = ["--data_dir", "d", "--output_dir", "o", "--file_name", "f"]
    a = train.get_parser(base)
    assert a.k3m_eval_topk == 0 and a.k3m_pred_output == ""
    a = train.get_parser(base + ["--do_eval", "--k3m_eval_topk", "5", "--k3m_pred_output", "p.jsonl"])
    assert a.do_eval is True and a.k3m_eval_topk == 5 and a.k3m_pred_output == "p.jsonl"


def test_fixture_checkable_shares():
    """The positions that can be checked for index equality depend on the fixture alone: recomputed here, they are
    the counts the generator printed and stay over the generator's bars."""
    import make_masked_prediction_golden as M
    d = np.load(os.path.join(HERE, "golden", "golden_masked_prediction.npz"), allow_pickle=False)
    g = {k: d[k] for k in d.files}
    assert g["tok/top_id"].shape == (53, 64) and int(g["tok/n_title"]) == 15 and g["reg/top_id"].shape == (14, 64)
    for name in ("tok", "reg"):
        z = g[name + "/top_logit"].astype(np.float64)
        assert np.all(z[:, :-1] >= z[:, 1:])
        assert np.all(g[name + "/scale"] >= np.abs(z).max(1))
    assert int(M.checkable(g["tok/top_logit"], g["tok/scale"], 10).sum()) == 392
    assert int(M.checkable(g["tok/top_logit"], g["tok/scale"], 5).sum()) == 234
    assert int(M.checkable(g["reg/top_logit"], g["reg/scale"], 5).sum()) == 67
    sh = M.shares(g)
    for key, least in M.MIN_SHARE.items():
        assert sh[key] >= least, (key, sh[key])
    # the gold rows of the sibling fixture are these rows
    b = np.load(os.path.join(HERE, "golden", "golden_bs2_hard.npz"), allow_pickle=False)
    assert b["logit/mlm_label"].shape == (53,) and b["logit/img_rows"].shape[0] == 14
    lab = np.concatenate([b["in/lm_label_ids"].reshape(-1), b["in/lm_label_ids_pv"].reshape(-1)])
    assert np.array_equal(lab[lab != -1], g["tok/gold"])
    # "mask" mode rows: every [MASK] position; with the reference's masking they all carry a label
    assert len(g["mask/t"]) + len(g["mask/pv"]) <= 53
