"""Golden vectors for the model without the image modality (use_image=False) — BUILD container only.

Runs the unmodified reference with ``config.use_image = False`` and ``image_feat / image_loc /
image_attention_mask = None`` (vilbert_k3m.py:1724-1743 encoder, :2331-2374 two-candidate gate with
``sequence_c1 = None``, :2725 c_initial, :1882-1883 NSP, :2815 image loss), fp32, if_pre_sampling 1, with the
stubs, tokenizer, batch builders and explicit-randomness hooks of make_golden.py / make_finetune_golden.py.
The records keep those generators' formats without the image arrays:

* ``golden_to_bs2.npz``, ``golden_to_bs3_zero_triple.npz``   pretraining step (make_golden.run_case's keys);
* ``golden_ft_to_ce.npz``, ``golden_ft_to_cosine.npz``       item-alignment pair step (model_case's keys);
* ``param_inventory_text_only.json``                         named_parameters() / state_dict keys of both models.

Gumbel noise: ``noise_seed`` over shapes t (B, T, 2, 768) then pv (B, P, 2, 768) (item alignment: noise_seed for
item 1, noise_seed + 1 for item 2).

Usage:  python tests/golden/make_text_only_golden.py [inventory|to_bs2|to_bs3_zero_triple|ft_to_ce|ft_to_cosine ...]
"""
import json
import os
import random
import re
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, REPO)
from make_golden import REF, CharTokenizer, _stub_imports, build_batch, gumbel_noise  # noqa: E402
from make_finetune_golden import build_pairs, rows as raw_rows  # noqa: E402

CFG = os.path.join(REPO, "configs/bert_base_6layer_6conect.json")
IMAGE_KEYS = ("image_feat", "image_loc", "image_target", "image_label", "image_mask")
FULL_GRADS = ["struc_w2.weight", "struc_w2.bias", "struc_w1.bias", "struc_w3.bias", "embeddings.LayerNorm.weight",
              "encoder.layer.0.attention.output.LayerNorm.bias", "encoder.layer.11.output.dense.bias",
              "encoder.c_layer_pv_t.0.biOutput.LayerNorm1.weight", "encoder.c_layer_pv_t.3.t_output.LayerNorm.bias",
              "encoder.c_layer_pv_t.5.biOutput.dense2.bias", "cls.predictions.transform.LayerNorm.weight",
              "score_self_t.bias", "score_cross2_pv.bias", "embeddings.token_type_embeddings.weight"]
SLICE_GRADS = ["encoder.layer.0.attention.self.query.weight", "encoder.layer.6.intermediate.dense.weight",
               "encoder.c_layer_pv_t.1.biattention.query1.weight", "encoder.c_layer_pv_t.2.biattention.key2.weight",
               "score_self_t.weight", "score_cross2_pv.weight", "struc_w1.weight",
               "cls.predictions.transform.dense.weight", "embeddings.word_embeddings.weight", "cls.predictions.bias"]
FT_GRADS = ["struc_w2.weight", "struc_w3.bias", "embeddings.LayerNorm.weight", "encoder.layer.11.output.dense.bias",
            "encoder.c_layer_pv_t.5.biOutput.dense2.bias", "score_self_t.bias", "score_cross2_pv.bias"]


def fake_gumbel_of(noise_of_call, T, order):
    """F.gumbel_softmax(hard=True) with the noise made explicit (first maximum wins, straight-through)."""
    def fake_gumbel(logits, tau=1.0, hard=False, eps=1e-10, dim=-1):
        assert logits.shape[2] == 2 and dim == 2, (tuple(logits.shape), dim)
        key = "t" if logits.shape[1] == T else "pv"
        g = noise_of_call(len(order))[key]
        order.append(key)
        y = ((logits + g) / tau).softmax(dim)
        idx = y.max(dim, keepdim=True)[1]
        hardv = torch.zeros_like(logits).scatter_(dim, idx, 1.0)
        return hardv - y.detach() + y
    return fake_gumbel


def pretrain_cfgs():
    import vilbert_k3m.vilbert_k3m as K
    from k3m_amd.config import pretrain_config
    cfg = pretrain_config(CFG, if_pre_sampling=1, use_image=False)
    rcfg = K.BertConfig.from_json_file(CFG)
    for k in ("v_target_size", "visual_target", "with_coattention", "dynamic_attention", "if_pre_sampling",
              "num_negative", "use_image"):
        setattr(rcfg, k, getattr(cfg, k))
    return cfg, rcfg


def ft_cfgs(loss_type):
    import vilbert_k3m.vilbert_k3m as K
    from k3m_amd.config import finetune_config
    cfg = finetune_config(CFG, loss_type=loss_type, use_image=False, if_pre_sampling=1)
    rcfg = K.BertConfig.from_json_file(CFG)
    for k in ("v_target_size", "visual_target", "model", "use_image", "with_coattention", "dynamic_attention",
              "if_pre_sampling", "num_negative_image", "loss_type"):
        setattr(rcfg, k, getattr(cfg, k))
    return cfg, rcfg


def grad_norms(model, res):
    names, gn = [], []
    for n, p in model.named_parameters():
        names.append(n)
        gn.append(np.nan if p.grad is None else float(p.grad.double().norm()))
    res["grad_norm_names"] = np.array(names)
    res["grad_norms"] = np.array(gn, np.float64)


def pretrain_case(name, row_ids, data_seed, weight_seed, noise_seed, neg_seed, T=36, P=128, NPV=20, drop_pv_of=()):
    import vilbert_k3m.vilbert_k3m as K
    from vilbert_k3m.datasets.concept_cap_dataset_struc import BertPreprocessBatch
    from k3m_amd.weights import param_values
    rows = [l.rstrip("\n").split("\t") for l in open(os.path.join(REF, "data/raw_multidata_of_product_preatrain.small_train"),
                                                        encoding="utf-8")]
    rows = [rows[i] for i in row_ids]
    for i in drop_pv_of:          # an item with no property-value triple (the zero-triple quirk)
        rows[i] = rows[i][:3] + ["no-properties-here"] + rows[i][4:]
    pre = BertPreprocessBatch(CharTokenizer(), max_seq_len=T, max_seq_len_pv=P, max_num_pv=NPV, max_region_len=36)
    batch = {k: v for k, v in build_batch(pre, rows, data_seed).items() if k not in IMAGE_KEYS}
    cfg, rcfg = pretrain_cfgs()
    torch.manual_seed(0)
    model = K.BertForMultiModalPreTraining_tri_stru(rcfg)
    sd = {k: torch.from_numpy(v) for k, v in param_values(cfg, weight_seed).items()}
    sd["cls.predictions.decoder.weight"] = sd["embeddings.word_embeddings.weight"]
    model.load_state_dict(sd)
    model.tie_weights()
    model.eval()

    B = batch["input_ids"].shape[0]
    noise = {k: torch.from_numpy(v) for k, v in
             gumbel_noise(noise_seed, [("t", (B, T, 2, 768)), ("pv", (B, P, 2, 768))]).items()}
    order = []
    K.F.gumbel_softmax = fake_gumbel_of(lambda i: noise, T, order)
    draws = []
    real_sample = random.sample

    def rec_sample(pop, k):
        r = real_sample(pop, k)
        draws.append(list(r))
        return r
    cap = {}
    real_cls_forward = model.cls.forward

    def cls_capture(*a, **kw):
        r = real_cls_forward(*a, **kw)
        cap["t"], cap["pv"], cap["nsp"] = r[0].detach(), r[2].detach(), r[6].detach()
        return r
    model.cls.forward = cls_capture
    random.seed(neg_seed)
    K.random.sample = rec_sample
    tb = {k: torch.from_numpy(np.asarray(v)) for k, v in batch.items()}
    try:
        # image_target only switches the loss branch on (:2739-2743); nothing reads it without the image modality
        out = model(tb["input_ids"], None, None, tb["segment_ids"], tb["input_mask"], None, tb["lm_label_ids"], None,
                    torch.zeros(1), tb["is_next"], input_ids_pv=tb["input_ids_pv"],
                    token_type_ids_pv=tb["segment_ids_pv"], attention_mask_pv=tb["input_mask_pv"],
                    masked_lm_labels_pv=tb["lm_label_ids_pv"], next_sentence_label_pv_v=tb["is_next_pv_v"],
                    next_sentence_label_pv_t=tb["is_next_pv_t"], index_p=tb["index_p"], index_v=tb["index_v"],
                    device=torch.device("cpu"))
    finally:
        K.random.sample = real_sample
    assert order == ["t", "pv"], order
    mlm_t, img, _, mlm_pv, _, _, nsp, c_init, c_final, lpm = out
    assert float(img) == 0.0
    loss = mlm_t + img + mlm_pv + lpm
    loss.backward()
    mlm_t, img, mlm_pv, lpm, nsp, loss = [x.detach() for x in (mlm_t, img, mlm_pv, lpm, nsp, loss)]

    ent = -np.ones((B, NPV, 2), np.int64)
    val = -np.ones((B, NPV, 2), np.int64)
    nvalid = [next((j for j in range(NPV) if batch["index_p"][i, j, 0] == 0), NPV) for i in range(B)]
    it = iter(draws)
    for i in range(B):
        for j in range(nvalid[i]):
            if B > 1:
                d = next(it)
                ent[i, j, :len(d)] = d
            if nvalid[i] > 1:
                d = next(it)
                val[i, j, :len(d)] = d
    assert next(it, None) is None

    res = {"losses": np.array([float(mlm_t), float(img), float(mlm_pv), float(lpm), float(nsp), float(loss)], np.float64),
           "c_initial": c_init.detach().numpy(), "c_final": c_final.detach().numpy(),
           "ent_neg": ent, "val_neg": val, "noise_seed": np.array(noise_seed), "weight_seed": np.array(weight_seed),
           "mode": np.array(1), "noise_order": np.array([-1, 0, 1])}
    grad_norms(model, res)
    params = dict(model.named_parameters())
    for n in FULL_GRADS:
        res["grad_full/" + n] = params[n].grad.numpy()
    for n in SLICE_GRADS:
        g = params[n].grad
        res["grad_slice/" + n] = (g[:4] if g.dim() == 2 else g[:256]).numpy()
    V = cap["t"].shape[-1]
    lt = cap["t"].reshape(-1, V)[torch.from_numpy(np.asarray(batch["lm_label_ids"]).reshape(-1) != -1)]
    lp = cap["pv"].reshape(-1, V)[torch.from_numpy(np.asarray(batch["lm_label_ids_pv"]).reshape(-1) != -1)]
    lab = np.concatenate([np.asarray(batch["lm_label_ids"]).reshape(-1), np.asarray(batch["lm_label_ids_pv"]).reshape(-1)])
    lab = lab[lab != -1]
    rows_m = torch.cat([lt, lp]).double()
    cols = np.unique(np.concatenate([np.arange(8), np.arange(100, 108), [131, 132],
                                     np.random.default_rng(2024).choice(V, 230, replace=False)]))[:256]
    res["logit/mlm_cols"] = cols.astype(np.int64)
    res["logit/mlm_rows"] = rows_m[:, torch.from_numpy(cols)].float().numpy()
    res["logit/mlm_label"] = rows_m[torch.arange(len(lab)), torch.from_numpy(lab)].float().numpy()
    res["logit/mlm_lse"] = torch.logsumexp(rows_m, 1).float().numpy()
    res["logit/nsp"] = cap["nsp"].numpy()
    for k, v in batch.items():
        res["in/" + k] = np.asarray(v)
    path = os.path.join(HERE, "golden_%s.npz" % name)
    np.savez_compressed(path, **res)
    print(name, "losses", res["losses"], "never-grad", int(np.isnan(res["grad_norms"]).sum()), "->", path,
          os.path.getsize(path) // 1024, "KiB")


def ft_case(name, loss_type, row0, labels, weight_seed, noise_seed, T=36, P=128, NPV=20):
    import vilbert_k3m.vilbert_k3m as K
    from vilbert_k3m.datasets.concept_cap_dataset_struc import K3MPreprocessBatch
    from k3m_amd.weights import param_values
    cfg, rcfg = ft_cfgs(loss_type)
    pre = K3MPreprocessBatch(CharTokenizer(), max_seq_len=T, max_seq_len_pv=P, max_num_pv=NPV, max_region_len=36)
    B = len(labels)
    res, cols = build_pairs(pre, raw_rows()[row0:row0 + 2 * B], labels, [36, 20, 9, 36], 2048, 1601, seed=row0)
    torch.manual_seed(0)
    model = K.K3MForItemAlignment(rcfg)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in param_values(cfg, weight_seed).items()}, strict=True)
    model.eval()
    shapes = [("t", (B, T, 2, 768)), ("pv", (B, P, 2, 768))]
    n1 = {k: torch.from_numpy(v) for k, v in gumbel_noise(noise_seed, shapes).items()}
    n2 = {k: torch.from_numpy(v) for k, v in gumbel_noise(noise_seed + 1, shapes).items()}
    calls = []
    K.F.gumbel_softmax = fake_gumbel_of(lambda i: n1 if i < 2 else n2, T, calls)
    tb = lambda k: torch.from_numpy(np.ascontiguousarray(cols[k]))  # noqa: E731
    args = [tb("labels")]
    for k in (1, 2):
        args += [tb("input_ids_%d" % k), tb("segment_ids_%d" % k), tb("input_mask_%d" % k), tb("input_ids_pv_%d" % k),
                 tb("segment_ids_pv_%d" % k), tb("input_mask_pv_%d" % k), tb("index_p_%d" % k), tb("index_v_%d" % k),
                 None, None, None]
    e1, e2, probs, loss = model(*args)
    loss.backward()
    assert calls == ["t", "pv", "t", "pv"], calls
    res["out/e1"], res["out/e2"] = e1.detach().numpy(), e2.detach().numpy()
    res["out/probs"], res["out/loss"] = probs.detach().numpy(), np.array(float(loss))
    res["noise_seed"], res["weight_seed"] = np.array(noise_seed), np.array(weight_seed)
    res["mode"], res["loss_type"] = np.array(1), np.array(loss_type)
    grad_norms(model, res)
    params = dict(model.named_parameters())
    for n in FT_GRADS + (["classifier.out_proj.weight", "classifier.out_proj.bias", "classifier.dense.bias"]
                         if loss_type == "ce" else []):
        res["grad_full/" + n] = params[n].grad.numpy()
    res = {k: v for k, v in res.items() if not k.startswith("in/")
           and not re.match(r"out/(coll_)?image_(feat|target|loc|mask)_\d|out/num_boxes_\d", k)}
    path = os.path.join(HERE, "golden_ft_%s.npz" % name)
    np.savez_compressed(path, **res)
    print(name, "loss", float(loss), "never-grad", int(np.isnan(res["grad_norms"]).sum()), "->", path,
          os.path.getsize(path) // 1024, "KiB")


def inventory():
    import vilbert_k3m.vilbert_k3m as K
    out = {}
    _, rcfg = pretrain_cfgs()
    m = K.BertForMultiModalPreTraining_tri_stru(rcfg)
    out["pretrain"] = [[n, list(p.shape)] for n, p in m.named_parameters()]
    out["pretrain_state_dict_keys"] = list(m.state_dict().keys())
    for lt in ("ce", "cosine"):
        _, rcfg = ft_cfgs(lt)
        m = K.K3MForItemAlignment(rcfg)
        out[lt] = [[n, list(p.shape)] for n, p in m.named_parameters()]
        out[lt + "_state_dict_keys"] = list(m.state_dict().keys())
    path = os.path.join(HERE, "param_inventory_text_only.json")
    json.dump(out, open(path, "w"))
    print("inventory ->", path, {k: len(v) for k, v in out.items()})


CASES = {
    "inventory": inventory,
    "to_bs2": lambda: pretrain_case("to_bs2", row_ids=[20, 23], data_seed=71, weight_seed=81, noise_seed=91,
                                    neg_seed=61),
    "to_bs3_zero_triple": lambda: pretrain_case("to_bs3_zero_triple", row_ids=[26, 22, 29], data_seed=72,
                                                weight_seed=82, noise_seed=92, neg_seed=62, drop_pv_of=(0,)),
    "ft_to_ce": lambda: ft_case("to_ce", "ce", row0=170, labels=[1, 0], weight_seed=83, noise_seed=93),
    "ft_to_cosine": lambda: ft_case("to_cosine", "cosine", row0=180, labels=[0, 1], weight_seed=84, noise_seed=94),
}


if __name__ == "__main__":
    _stub_imports()
    torch.set_num_threads(8)
    for name in (sys.argv[1:] or list(CASES)):
        CASES[name]()
