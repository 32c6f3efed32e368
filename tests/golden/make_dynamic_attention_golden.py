"""Golden vectors for dynamic image attention (``dynamic_attention=True``) — BUILD container only.

Runs the unmodified reference with ``config.dynamic_attention = True`` (BertImageSelfAttention,
vilbert_k3m.py:572-601: the image layers' Q and K scaled by 1 + sigmoid(dyLinear_*(masked mean of the text
partner))), fp32, if_pre_sampling 1, model.eval(), with the stubs, tokenizer, batch builders, fake gumbel noise and
recorded negatives of make_golden.py / make_finetune_golden.py.  Records:

* ``golden_da_bs2.npz``, ``golden_da_bs3_zero_triple.npz``   pretraining step (make_golden.run_case's keys);
* ``golden_ft_da_ce.npz``                                    ONE item-alignment pair (each item a batch of one in
                                                             the reference), model_case's keys;
* ``golden_ft_da_ce_bs2.npz``                                two pairs, as golden_ft_ce;
* ``param_inventory_dynamic_attention.json``                 named_parameters() of both models.

Beyond run_case's keys, for the dyLinear_* tensors of v_layer.0 and v_layer.5: ``grad_full/<bias>``, and of each
weight ``grad_sub/`` (every 16th row and column) and ``grad_rows/`` (the first two and last two rows in full, which
fix where the gradient lands); a full [1024, 768] weight gradient is 3 MB, the four of a layer pair 12 MB, and the
tensor's norm is in ``grad_norms``.  The image features and region targets are rounded to fp16 BEFORE the reference
runs and stored as fp16 (the recorded inputs are exactly what the model saw) to keep each file under 1 MiB.

Not blind.  Each case also runs the reference WITHOUT the flag on the same inputs and shared weights, records its
losses (``losses_without_flag`` / ``loss_without_flag``) and asserts of the reference alone:
* every dyLinear_* gradient norm is nonzero;
* the fine-tune cases: the loss moves by more than 10x its own parity bar (rtol 1e-3, atol 1e-4);
* the pretraining cases: the total loss moves by more than 10 x 1e-3 in loss units, at least one loss by more than
  10x its own parity bar, and the masked regions' logits (which come straight from the image streams; recorded as
  ``img_logit_move`` = [max move, max |logit|]) by more than 10x their 1e-3 bar.

The total loss.  The pretraining total does NOT move by 10x its OWN parity bar (about 0.25 of a total of 25), and no
choice of conditions makes it: the image streams reach the four loss terms through the co-attention only and the
terms' changes partly cancel.  Measured on da_bs2's inputs (total with / without the flag, forward only):

    weight std   unit noise                8x noise                   10x the total's bar
    0.02         23.193 / 23.185  0.0077   23.091 / 23.093  0.0020    0.23
    0.04         25.163 / 25.128  0.035    25.042 / 25.030  0.012     0.25
    0.06         27.878 / 27.736  0.14     28.446 / 28.502  0.056     0.28
    0.08         31.384 / 31.272  0.11     32.802 / 32.764  0.038     0.31
    0.10         36.954 / 37.307  0.35     36.682 / 37.168  0.49      0.37
    0.12                                   42.374 / 42.445  0.071     0.43

(da_bs3_zero_triple's inputs, 8x noise: 0.018 at std 0.08, 0.19 at 0.10, 0.13 at 0.12.)  At the conditions of
make_golden.run_case (std 0.02, unit noise) the move, 0.0077, is below even 0.01.  From std 0.06 on the move is
erratic: it comes from hard-gate choices that flip, not from the gate's smooth effect.  The witnesses that do see the
feature at 10x their bars are the ones asserted above, and the tests compare the dyLinear_* gradients themselves.

Weight scale.  At the scale of the other fixtures (param_values std 0.02) the image layers' attention is nearly
uniform, so these cases draw the weight matrices at ``weight_std`` 0.04 (recorded in the file; the tests pass it to
param_values), the smallest scale of the table at which the total passes 0.01.

Gumbel noise.  The recorded noise is NOISE_SCALE x gumbel(0, 1) (``noise_scale`` in the file).  The hard gate is an
argmax over sigmoid score + noise, and one flipped choice moves the pooled outputs (NSP, LPM, c_*) past the 1e-3
bars.  Counted in the reference at std 0.04 on da_bs2's inputs (327,680 choices; gap between the best and the second
candidate): with unit noise 5 choices lie within 1e-5 and 27 within 1e-4 of a tie, with 8x noise none and 3.  The fp32
differences between two correct implementations after 18 layers are taken to be of the order 1e-5 there (a
supposition, not measured), so unit noise leaves choices that no implementation is bound to reproduce; 8x noise
leaves none.  The gate's forward and straight-through
backward are exercised all the same.

Usage:  python tests/golden/make_dynamic_attention_golden.py [CASE ...]      (the keys of CASES; default: all)
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
from make_golden import REF, FULL_GRADS, SLICE_GRADS, CharTokenizer, _stub_imports, build_batch, gumbel_noise  # noqa: E402
from make_finetune_golden import build_pairs, rows as raw_rows  # noqa: E402

CFG = os.path.join(REPO, "configs/bert_base_6layer_6conect.json")
DY_LAYERS = (0, 5)
NOISE_SCALE = 8.0


def scaled_noise(seed, shapes):
    return {k: torch.from_numpy(v * np.float32(NOISE_SCALE)) for k, v in gumbel_noise(seed, shapes).items()}


def loss_bar(losses0):
    """10x the bar the parity tests put on a loss (rtol 1e-3, atol 1e-4)"""
    return 10 * (1e-3 * np.abs(np.asarray(losses0, np.float64)) + 1e-4)


def sensitive(losses, losses0, total_own_bar):
    """losses: the recorded loss vector, its last element the total.  total_own_bar (the fine-tune cases): the flag
    moves the total by more than 10x the total's own parity bar.  Otherwise (the pretraining cases, see "The total
    loss" in the module docstring): the total by more than 10 x 1e-3 in loss units, and at least one of the losses
    by more than 10x its own parity bar."""
    losses, losses0 = np.asarray(losses, np.float64), np.asarray(losses0, np.float64)
    d = np.abs(losses - losses0)
    if total_own_bar:
        return bool(d[-1] > loss_bar(losses0)[-1])
    return bool(d[-1] > 10 * 1e-3 and (d > loss_bar(losses0)).any())


def f16(a):
    return np.asarray(a, np.float32).astype(np.float16)


def pretrain_cfgs(dyn):
    import vilbert_k3m.vilbert_k3m as K
    from k3m_amd.config import pretrain_config
    cfg = pretrain_config(CFG, if_pre_sampling=1, dynamic_attention=dyn)
    rcfg = K.BertConfig.from_json_file(CFG)
    for k in ("v_target_size", "visual_target", "with_coattention", "dynamic_attention", "if_pre_sampling",
              "num_negative"):
        setattr(rcfg, k, getattr(cfg, k))
    return cfg, rcfg


def ft_cfgs(dyn):
    import vilbert_k3m.vilbert_k3m as K
    from k3m_amd.config import finetune_config
    cfg = finetune_config(CFG, loss_type="ce", if_pre_sampling=1, dynamic_attention=dyn)
    rcfg = K.BertConfig.from_json_file(CFG)
    for k in ("v_target_size", "visual_target", "model", "use_image", "with_coattention", "dynamic_attention",
              "if_pre_sampling", "num_negative_image", "loss_type"):
        setattr(rcfg, k, getattr(cfg, k))
    return cfg, rcfg


def fake_gumbel_of(noise_of_call, T, calls):
    def fake_gumbel(logits, tau=1.0, hard=False, eps=1e-10, dim=-1):
        key = "v" if logits.shape[-1] == 1024 else ("t" if logits.shape[1] == T else "pv")
        g = noise_of_call(len(calls))[key]
        calls.append(key)
        y = ((logits + g) / tau).softmax(dim)
        idx = y.max(dim, keepdim=True)[1]
        hardv = torch.zeros_like(logits).scatter_(dim, idx, 1.0)
        return hardv - y.detach() + y
    return fake_gumbel


def dy_names(model):
    return [n for n, _ in model.named_parameters() if ".dyLinear_" in n]


def record_grads(model, res, full, sliced):
    params = dict(model.named_parameters())
    names, gn = [], []
    for n, p in params.items():
        names.append(n)
        gn.append(np.nan if p.grad is None else float(p.grad.double().norm()))
    res["grad_norm_names"] = np.array(names)
    res["grad_norms"] = np.array(gn, np.float64)
    for n in full:
        g = params[n].grad
        res["grad_full/" + n] = np.zeros(tuple(params[n].shape), np.float32) if g is None else g.numpy()
    for n in sliced:
        g = params[n].grad
        if g is None:
            g = torch.zeros(tuple(params[n].shape))
        res["grad_slice/" + n] = (g[:4] if g.dim() == 2 else g[:256]).numpy()
    dy = dy_names(model)
    assert len(dy) == 24, len(dy)
    for n in dy:
        assert params[n].grad is not None and float(params[n].grad.double().norm()) > 0.0, n
        if int(n.split(".")[2]) in DY_LAYERS:
            g = params[n].grad
            if g.dim() == 1:
                res["grad_full/" + n] = g.numpy()
            else:
                res["grad_sub/" + n] = g[::16, ::16].contiguous().numpy()
                res["grad_rows/" + n] = torch.cat([g[:2], g[-2:]]).numpy()   # whole rows: where the gradient lands


def pretrain_run(dyn, batch, weight_seed, weight_std, noise_seed, neg_seed, T, P, NPV, R):
    import vilbert_k3m.vilbert_k3m as K
    from k3m_amd.weights import param_values
    cfg, rcfg = pretrain_cfgs(dyn)
    torch.manual_seed(0)
    model = K.BertForMultiModalPreTraining_tri_stru(rcfg)
    sd = {k: torch.from_numpy(v) for k, v in param_values(cfg, weight_seed, std=weight_std).items()}
    sd["cls.predictions.decoder.weight"] = sd["embeddings.word_embeddings.weight"]
    model.load_state_dict(sd)
    model.tie_weights()
    model.eval()
    B = batch["input_ids"].shape[0]
    shapes = [("v", (B, R + 1, 3, 1024)), ("t", (B, T, 3, 768)), ("pv", (B, P, 3, 768))]
    noise = scaled_noise(noise_seed, shapes)
    calls = []
    K.F.gumbel_softmax = fake_gumbel_of(lambda i: noise, T, calls)
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
        cap["t"], cap["v"], cap["pv"], cap["nsp"] = r[0].detach(), r[1].detach(), r[2].detach(), r[6].detach()
        return r
    model.cls.forward = cls_capture
    random.seed(neg_seed)
    K.random.sample = rec_sample
    tb = {k: torch.from_numpy(np.asarray(v)) for k, v in batch.items()}
    try:
        out = model(tb["input_ids"], tb["image_feat"], tb["image_loc"], tb["segment_ids"], tb["input_mask"],
                    tb["image_mask"], tb["lm_label_ids"], tb["image_label"], tb["image_target"], tb["is_next"],
                    input_ids_pv=tb["input_ids_pv"], token_type_ids_pv=tb["segment_ids_pv"],
                    attention_mask_pv=tb["input_mask_pv"], masked_lm_labels_pv=tb["lm_label_ids_pv"],
                    next_sentence_label_pv_v=tb["is_next_pv_v"], next_sentence_label_pv_t=tb["is_next_pv_t"],
                    index_p=tb["index_p"], index_v=tb["index_v"], device=torch.device("cpu"))
    finally:
        K.random.sample = real_sample
    return model, out, cap, draws, calls


def pretrain_case(name, row_ids, data_seed, weight_seed, weight_std, noise_seed, neg_seed, T=36, P=128, NPV=20, R=36,
                  drop_pv_of=()):
    from vilbert_k3m.datasets.concept_cap_dataset_struc import BertPreprocessBatch
    rows = raw_rows()
    rows = [rows[i] for i in row_ids]
    for i in drop_pv_of:          # an item with no property-value triple (the zero-triple quirk)
        rows[i] = rows[i][:3] + ["no-properties-here"] + rows[i][4:]
    pre = BertPreprocessBatch(CharTokenizer(), max_seq_len=T, max_seq_len_pv=P, max_num_pv=NPV, max_region_len=R)
    stored = build_batch(pre, rows, data_seed, nbox=R)
    stored["image_feat"], stored["image_target"] = f16(stored["image_feat"]), f16(stored["image_target"])
    batch = dict(stored, image_feat=stored["image_feat"].astype(np.float32),
                 image_target=stored["image_target"].astype(np.float32))
    nt, npv = batch["input_mask"].sum(1), batch["input_mask_pv"].sum(1)
    print(name, "title lengths", nt, "PV lengths", npv)

    _, out0, cap0, _, _ = pretrain_run(False, batch, weight_seed, weight_std, noise_seed, neg_seed, T, P, NPV, R)
    l0 = [float(out0[i].detach()) for i in (0, 1, 3, 9, 6)]
    losses0 = np.array(l0 + [float((out0[0] + out0[1] + out0[3] + out0[9]).detach())], np.float64)
    model, out, cap, draws, calls = pretrain_run(True, batch, weight_seed, weight_std, noise_seed, neg_seed, T, P, NPV, R)
    assert calls == ["v", "t", "pv"], calls
    mlm_t, img, _, mlm_pv, _, _, nsp, c_init, c_final, lpm = out
    loss = mlm_t + img + mlm_pv + lpm
    losses1 = np.array([float(x.detach()) for x in (mlm_t, img, mlm_pv, lpm, nsp, loss)], np.float64)
    print(name, "losses with the flag", losses1, "without", losses0)
    assert sensitive(losses1, losses0, total_own_bar=False), (losses1, losses0)
    # the masked regions' logits come straight from the image streams: their move against the 1e-3 logit bar
    sel = torch.from_numpy(np.asarray(batch["image_label"]).reshape(-1) == 1)
    rows1, rows0 = [c["v"][:, 1:].reshape(-1, c["v"].shape[-1])[sel].double() for c in (cap, cap0)]
    img_move = np.array([float((rows1 - rows0).abs().max()), float(rows0.abs().max())], np.float64)
    print(name, "masked-region logits move by %.4g of max %.4g" % tuple(img_move))
    assert img_move[0] > 10 * 1e-3 * img_move[1], img_move
    loss.backward()
    mlm_t, img, mlm_pv, lpm, nsp, loss = [x.detach() for x in (mlm_t, img, mlm_pv, lpm, nsp, loss)]

    B = batch["input_ids"].shape[0]
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
           "losses_without_flag": losses0, "img_logit_move": img_move,
           "c_initial": c_init.detach().numpy(), "c_final": c_final.detach().numpy(),
           "ent_neg": ent, "val_neg": val, "noise_seed": np.array(noise_seed), "weight_seed": np.array(weight_seed),
           "weight_std": np.array(weight_std, np.float64), "noise_scale": np.array(NOISE_SCALE, np.float64), "mode": np.array(1), "noise_order": np.array([0, 1, 2])}
    record_grads(model, res, FULL_GRADS, SLICE_GRADS)
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
    pv_ = cap["v"][:, 1:]
    res["logit/img_rows"] = pv_.reshape(-1, pv_.shape[-1])[
        torch.from_numpy(np.asarray(batch["image_label"]).reshape(-1) == 1)].numpy()
    res["logit/nsp"] = cap["nsp"].numpy()
    for k, v in stored.items():
        res["in/" + k] = np.asarray(v)
    path = os.path.join(HERE, "golden_%s.npz" % name)
    np.savez_compressed(path, **res)
    print(name, "losses", res["losses"], "->", path, os.path.getsize(path) // 1024, "KiB")
    assert os.path.getsize(path) < (1 << 20), "a committed file stays under 1 MiB"


def ft_run(dyn, cols, labels_n, weight_seed, weight_std, noise_seed, T, P):
    import vilbert_k3m.vilbert_k3m as K
    from k3m_amd.weights import param_values
    cfg, rcfg = ft_cfgs(dyn)
    B = labels_n
    torch.manual_seed(0)
    model = K.K3MForItemAlignment(rcfg)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in param_values(cfg, weight_seed, std=weight_std).items()},
                          strict=True)
    model.eval()
    shapes = [("v", (B, 37, 3, 1024)), ("t", (B, T, 3, 768)), ("pv", (B, P, 3, 768))]
    n1, n2 = scaled_noise(noise_seed, shapes), scaled_noise(noise_seed + 1, shapes)
    calls = []
    K.F.gumbel_softmax = fake_gumbel_of(lambda i: n1 if i < 3 else n2, T, calls)
    tb = lambda k: torch.from_numpy(np.ascontiguousarray(cols[k]).astype(  # noqa: E731
        np.float32 if cols[k].dtype == np.float16 else cols[k].dtype))
    args = [tb("labels")]
    for k in (1, 2):
        args += [tb("input_ids_%d" % k), tb("segment_ids_%d" % k), tb("input_mask_%d" % k), tb("input_ids_pv_%d" % k),
                 tb("segment_ids_pv_%d" % k), tb("input_mask_pv_%d" % k), tb("index_p_%d" % k), tb("index_v_%d" % k),
                 tb("coll_image_feat_%d" % k), tb("coll_image_loc_%d" % k), tb("coll_image_mask_%d" % k)]
    e1, e2, probs, loss = model(*args)
    assert calls == ["v", "t", "pv", "v", "t", "pv"], calls
    return model, e1, e2, probs, loss


def ft_case(name, row0, labels, weight_seed, weight_std, noise_seed, T=36, P=128, NPV=20):
    from vilbert_k3m.datasets.concept_cap_dataset_struc import K3MPreprocessBatch
    pre = K3MPreprocessBatch(CharTokenizer(), max_seq_len=T, max_seq_len_pv=P, max_num_pv=NPV, max_region_len=36)
    B = len(labels)
    res, cols = build_pairs(pre, raw_rows()[row0:row0 + 2 * B], labels, [36, 20, 9, 36], 2048, 1601, seed=row0)
    for k in (1, 2):
        cols["coll_image_feat_%d" % k] = f16(cols["coll_image_feat_%d" % k])
        res["out/coll_image_feat_%d" % k] = cols["coll_image_feat_%d" % k]
    _, _, _, _, loss0 = ft_run(False, cols, B, weight_seed, weight_std, noise_seed, T, P)
    model, e1, e2, probs, loss = ft_run(True, cols, B, weight_seed, weight_std, noise_seed, T, P)
    print(name, "loss with the flag %.6f, without %.6f" % (float(loss), float(loss0)))
    assert sensitive([float(loss)], [float(loss0)], total_own_bar=True), (float(loss), float(loss0))
    loss.backward()
    res["out/e1"], res["out/e2"] = e1.detach().numpy(), e2.detach().numpy()
    res["out/probs"], res["out/loss"] = probs.detach().numpy(), np.array(float(loss))
    res["loss_without_flag"] = np.array(float(loss0))
    res["noise_seed"], res["weight_seed"] = np.array(noise_seed), np.array(weight_seed)
    res["weight_std"], res["noise_scale"] = np.array(weight_std, np.float64), np.array(NOISE_SCALE, np.float64)
    res["mode"], res["loss_type"] = np.array(1), np.array("ce")
    record_grads(model, res, ["struc_w2.weight", "struc_w3.bias", "map_bi_to_individual.bias",
                              "embeddings.LayerNorm.weight", "encoder.layer.11.output.dense.bias",
                              "encoder.c_layer_pv_t.5.biOutput.dense2.bias", "v_embeddings.LayerNorm.bias",
                              "classifier.out_proj.weight", "classifier.out_proj.bias", "classifier.dense.bias"], [])
    res = {k: v for k, v in res.items() if not k.startswith("in/")
           and not re.match(r"out/image_(feat|target|loc|mask)_\d", k)}
    path = os.path.join(HERE, "golden_ft_%s.npz" % name)
    np.savez_compressed(path, **res)
    print(name, "loss", float(loss), "->", path, os.path.getsize(path) // 1024, "KiB")


def inventory():
    import vilbert_k3m.vilbert_k3m as K
    out = {}
    _, rcfg = pretrain_cfgs(True)
    m = K.BertForMultiModalPreTraining_tri_stru(rcfg)
    out["pretrain"] = [[n, list(p.shape)] for n, p in m.named_parameters()]
    _, rcfg = ft_cfgs(True)
    m = K.K3MForItemAlignment(rcfg)
    out["ce"] = [[n, list(p.shape)] for n, p in m.named_parameters()]
    path = os.path.join(HERE, "param_inventory_dynamic_attention.json")
    json.dump(out, open(path, "w"))
    print("inventory ->", path, {k: len(v) for k, v in out.items()})


CASES = {
    "inventory": inventory,
    "da_bs2": lambda: pretrain_case("da_bs2", row_ids=[30, 33], data_seed=73, weight_seed=85, weight_std=0.04, noise_seed=95,
                                    neg_seed=63),
    # fewer regions than da_bs2 (R = 20) keep the three items' region inputs small
    "da_bs3_zero_triple": lambda: pretrain_case("da_bs3_zero_triple", row_ids=[36, 32, 39], data_seed=74,
                                                weight_seed=86, weight_std=0.04, noise_seed=96, neg_seed=64, R=20, drop_pv_of=(0,)),
    # ONE pair: each item is a batch of one in the reference, the engine's stacked batch holds two sequences
    "ft_da_ce": lambda: ft_case("da_ce", row0=190, labels=[1], weight_seed=88, weight_std=0.04, noise_seed=97),
    "ft_da_ce_bs2": lambda: ft_case("da_ce_bs2", row0=190, labels=[1, 0], weight_seed=88, weight_std=0.04, noise_seed=97),
}


if __name__ == "__main__":
    _stub_imports()
    torch.set_num_threads(8)
    for name in (sys.argv[1:] or list(CASES)):
        CASES[name]()
