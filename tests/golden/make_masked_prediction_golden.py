"""Fixture of masked-token and masked-region prediction — BUILD container only.

``golden_masked_prediction.npz``: what the reference's own heads predict at the masked positions of the ``bs2_hard``
case of make_golden.py (its inputs, read back from golden_bs2_hard.npz; the same weight seed and gumbel noise;
model.eval()), taken from ``prediction_scores_t / _pv / _v`` of BertPreTrainingHeads.forward (vilbert_k3m.py:1875-1909):

* ``tok/top_id``, ``tok/top_logit`` [53, 64]: per labelled row (15 title rows, then 38 PV rows, row-major: the order
  of ``logit/mlm_label`` / ``logit/mlm_lse`` of golden_bs2_hard.npz, which serve for the gold log-probabilities) the
  64 largest logits and their ids, ranked in float64, ties by ascending id; ``tok/scale`` [53]: the row's largest
  |logit|; ``tok/pos`` [53, 2]: (item, position); ``tok/n_title``; ``tok/gold`` [53].
* ``reg/*``: the same for the 14 masked regions (image_label == 1) over the 1601 classes, positions in
  seq_v[:, 1:]; ``reg/gold``: the argmax class of image_target.
* ``mask/t``, ``mask/pv`` [n, 2]: the positions whose token id is 103 ([MASK]), row-major: the rows of "mask" mode.

A position p of a row can be checked for index equality only where its logit is separated from both ranking
neighbours by more than 2 tol, tol = 1e-3 scale (the bar tests/test_gpu_parity.py puts on these logits).  The
generator asserts that at least 70 % of the token positions at k = 10, 85 % at k = 5 and 90 % of the region
positions at k = 5 are checkable, and refuses the fixture otherwise.  checkable() is that rule; the tests import it.

Usage:  python tests/golden/make_masked_prediction_golden.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
TOP = 64
TOL_REL = 1e-3
MIN_SHARE = {"tok10": 0.70, "tok5": 0.85, "reg5": 0.90}


def checkable(top_logit, scale, k):
    """bool [rows, k]: position p's float64 logit differs from those of positions p - 1 and p + 1 by more than
    2 * TOL_REL * scale[row]."""
    z = np.asarray(top_logit, np.float64)[:, :k + 1]
    gap = z[:, :-1] - z[:, 1:]                      # gap[p] between positions p and p + 1
    bar = 2.0 * TOL_REL * np.asarray(scale, np.float64)[:, None]
    below = gap[:, :k] > bar
    above = np.concatenate([np.ones((z.shape[0], 1), bool), gap[:, :k - 1] > bar], 1)
    return below & above


def shares(g):
    return {"tok10": float(checkable(g["tok/top_logit"], g["tok/scale"], 10).mean()),
            "tok5": float(checkable(g["tok/top_logit"], g["tok/scale"], 5).mean()),
            "reg5": float(checkable(g["reg/top_logit"], g["reg/scale"], 5).mean())}


def _top(rows):
    """rows [n, V] float64 -> (ids [n, TOP], logits [n, TOP] float32, scale [n] float32)"""
    ids = np.stack([np.lexsort((np.arange(rows.shape[1]), -r))[:TOP] for r in rows])
    return ids.astype(np.int64), np.take_along_axis(rows, ids, 1).astype(np.float32), \
        np.abs(rows).max(1).astype(np.float32)


def main():
    import torch
    sys.path.insert(0, HERE)
    sys.path.insert(0, REPO)
    import make_golden as MG
    MG._stub_imports()
    torch.set_num_threads(8)
    import vilbert_k3m.vilbert_k3m as K
    from k3m_amd.config import pretrain_config
    from k3m_amd.weights import param_values

    case = MG.CASES["bs2_hard"]
    d = np.load(os.path.join(HERE, "golden_bs2_hard.npz"), allow_pickle=False)
    batch = {k[3:]: d[k] for k in d.files if k.startswith("in/")}
    assert int(d["weight_seed"]) == case["weight_seed"] and int(d["noise_seed"]) == case["noise_seed"]
    cfg_path = os.path.join(REPO, "configs/bert_base_6layer_6conect.json")
    cfg = pretrain_config(cfg_path, if_pre_sampling=case["mode"])
    rcfg = K.BertConfig.from_json_file(cfg_path)
    for k in ("v_target_size", "visual_target", "with_coattention", "dynamic_attention", "if_pre_sampling",
              "num_negative"):
        setattr(rcfg, k, getattr(cfg, k))
    torch.manual_seed(0)
    model = K.BertForMultiModalPreTraining_tri_stru(rcfg)
    sd = {k: torch.from_numpy(v) for k, v in param_values(cfg, case["weight_seed"]).items()}
    sd["cls.predictions.decoder.weight"] = sd["embeddings.word_embeddings.weight"]
    model.load_state_dict(sd)
    model.tie_weights()
    model.eval()

    B, T = batch["input_ids"].shape
    P, R = batch["input_ids_pv"].shape[1], batch["image_feat"].shape[1]
    shapes = [("v", (B, R, 3, 1024)), ("t", (B, T, 3, 768)), ("pv", (B, P, 3, 768))]
    noise = {k: torch.from_numpy(v) for k, v in MG.gumbel_noise(case["noise_seed"], shapes).items()}

    def fake_gumbel(logits, tau=1.0, hard=False, eps=1e-10, dim=-1):
        key = "v" if logits.shape[-1] == 1024 else ("t" if logits.shape[1] == T else "pv")
        y = ((logits + noise[key]) / tau).softmax(dim)
        idx = y.max(dim, keepdim=True)[1]
        return torch.zeros_like(logits).scatter_(dim, idx, 1.0) - y.detach() + y
    K.F.gumbel_softmax = fake_gumbel
    cap = {}
    real_cls_forward = model.cls.forward

    def cls_capture(*a, **kw):
        r = real_cls_forward(*a, **kw)
        cap["t"], cap["v"], cap["pv"] = r[0].detach(), r[1].detach(), r[2].detach()
        return r
    model.cls.forward = cls_capture
    import random
    random.seed(case["neg_seed"])
    tb = {k: torch.from_numpy(np.asarray(v)) for k, v in batch.items()}
    with torch.no_grad():
        model(tb["input_ids"], tb["image_feat"], tb["image_loc"], tb["segment_ids"], tb["input_mask"],
              tb["image_mask"], tb["lm_label_ids"], tb["image_label"], tb["image_target"], tb["is_next"],
              input_ids_pv=tb["input_ids_pv"], token_type_ids_pv=tb["segment_ids_pv"],
              attention_mask_pv=tb["input_mask_pv"], masked_lm_labels_pv=tb["lm_label_ids_pv"],
              next_sentence_label_pv_v=tb["is_next_pv_v"], next_sentence_label_pv_t=tb["is_next_pv_t"],
              index_p=tb["index_p"], index_v=tb["index_v"], device=torch.device("cpu"))

    V = cap["t"].shape[-1]
    lt, lp = batch["lm_label_ids"], batch["lm_label_ids_pv"]
    pos_t, pos_p = np.argwhere(lt != -1), np.argwhere(lp != -1)
    rows = np.concatenate([cap["t"].reshape(-1, V).double().numpy()[(lt != -1).reshape(-1)],
                           cap["pv"].reshape(-1, V).double().numpy()[(lp != -1).reshape(-1)]])
    gold = np.concatenate([lt[lt != -1], lp[lp != -1]]).astype(np.int64)
    # the same run as golden_bs2_hard.npz: its label logits and log-sum-exps are these rows'
    assert np.allclose(rows[np.arange(len(gold)), gold], d["logit/mlm_label"], rtol=1e-4, atol=1e-4)
    res = {}
    res["tok/top_id"], res["tok/top_logit"], res["tok/scale"] = _top(rows)
    res["tok/pos"] = np.concatenate([pos_t, pos_p]).astype(np.int64)
    res["tok/n_title"] = np.array(len(pos_t))
    res["tok/gold"] = gold
    il = batch["image_label"]
    vr = cap["v"][:, 1:]
    rrows = vr.reshape(-1, vr.shape[-1]).double().numpy()[(il == 1).reshape(-1)]
    res["reg/top_id"], res["reg/top_logit"], res["reg/scale"] = _top(rrows)
    res["reg/pos"] = np.argwhere(il == 1).astype(np.int64)
    res["reg/gold"] = batch["image_target"].reshape(-1, batch["image_target"].shape[-1])[
        (il == 1).reshape(-1)].argmax(1).astype(np.int64)
    res["mask/t"] = np.argwhere(batch["input_ids"] == 103).astype(np.int64)
    res["mask/pv"] = np.argwhere(batch["input_ids_pv"] == 103).astype(np.int64)
    res["source"] = np.array("golden_bs2_hard")
    sh = shares(res)
    print("rows: %d title + %d PV, %d regions; checkable shares %s" % (len(pos_t), len(pos_p), len(rrows), sh))
    for key, least in MIN_SHARE.items():
        if sh[key] < least:
            print("refused: checkable share %s = %.3f under %.2f; nothing written" % (key, sh[key], least))
            return 1
    path = os.path.join(HERE, "golden_masked_prediction.npz")
    np.savez_compressed(path, **res)
    print("masked_prediction ->", path, os.path.getsize(path) // 1024, "KiB")
    return 0


if __name__ == "__main__":
    sys.exit(main())
