"""Golden vectors for masked-region feature regression (``visual_target=1``) — BUILD container only.

Runs the unmodified reference BertForMultiModalPreTraining_tri_stru with ``config.visual_target = 1`` and
``config.v_target_size = 2048`` (vilbert_k3m.py:2232-2237 selects nn.MSELoss(reduction="none"); :2745-2752 sum the
masked regions' squared errors and divide by max(masked regions * 2048, 1)), fp32, if_pre_sampling 1 (hard gate),
model.eval(), with the stubs, tokenizer, batch builder, recorded gumbel noise and recorded LPM negatives of
make_golden.py.  The batch comes from the reference's ``BertPreprocessBatch(..., visual_target=1,
v_target_size=2048)``, whose ``image_target`` is a copy of the region features before masking (dataset:584-601).
Records:

* ``golden_vt1_bs2.npz``                      one pretraining step of two items: make_golden.run_case's keys plus
                                              ``visual_target``;
* ``param_inventory_visual_target.json``      named_parameters() names and shapes of that model.

12 region boxes: the 2048-d features and targets are random floats that do not compress, and a committed file stays
under 1 MiB (asserted).

Not blind.  The fixture is written only if, of the reference and its inputs alone,
* each item has at least one masked region and the batch at least three (so the target-row gather of the compacted
  rows crosses items), and
* the gradient norm of ``cls.imagePredictions.decoder.weight`` is above 0, and
* no hard-gate choice lies within TIE_MARGIN of a tie (see TIE_MARGIN; ``gate_min_gap`` in the file).

Usage:  python tests/golden/make_visual_target_golden.py [CASE ...]      (keys of CASES; default: inventory vt1_bs2)
"""
import json
import os
import random
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, REPO)
from make_golden import REF, FULL_GRADS, SLICE_GRADS, CharTokenizer, _stub_imports, build_batch, gumbel_noise  # noqa: E402

CFG = os.path.join(REPO, "configs/bert_base_6layer_6conect.json")
VISUAL_TARGET = 1
V_TARGET_SIZE = 2048
DECODER = "cls.imagePredictions.decoder.weight"
# No hard-gate choice of the recorded step lies within this of a tie.  The gate is an argmax over sigmoid score +
# gumbel noise, and one flipped choice moves the pooled outputs (NSP, LPM, c_*) past the 1e-3 parity bars.  With unit
# noise about 1 choice in 60,000 lies within 1e-5 of a tie (make_dynamic_attention_golden.py counted 5 of 327,680), so
# of the 279,808 choices of this step a handful do for most seeds; fp32 differences between two correct
# implementations after 18 layers are taken to be of the order 1e-5 there (a supposition).  The scores do not depend
# on the noise, so the generator searches the noise seed (CASES "find") with the reference's scores alone, and the
# margin is four times that supposition.
TIE_MARGIN = 4e-5
# The recorded fp32 gradients (the recorded tensors by their max element, every tensor's norm) lie within this of the
# reference's own float64 run on the same inputs: a fifth of the tests' 5e-3 gradient bar.  The model is not smooth
# everywhere (F.relu on the three streams before the gate, :2336-2340).  Measured with weight_seed 61 (noise_seed
# 160): every loss of the fp32 reference agrees with its float64 run to 1e-7, but the title stream's gradients do
# not (encoder.layer.11.output.dense.bias 9.9e-3 of its max element, twice the bar; layer.6.intermediate.dense.weight
# 2.0e-3; token_type_embeddings 1.8e-3) while the image and PV sides agree to 1e-6: taken to be one title-stream
# activation so close to 0 that the two runs take different sides of the ReLU (a supposition).  Such a fixture would
# pin the reference's rounding, not the model; weight_seed 62 agrees to 5e-6.
OWN_ERROR = 1e-3


def cfgs():
    import vilbert_k3m.vilbert_k3m as K
    from k3m_amd.config import pretrain_config
    cfg = pretrain_config(CFG, if_pre_sampling=1, visual_target=VISUAL_TARGET)
    assert cfg.v_target_size == V_TARGET_SIZE
    rcfg = K.BertConfig.from_json_file(CFG)
    for k in ("v_target_size", "visual_target", "with_coattention", "dynamic_attention", "if_pre_sampling",
              "num_negative"):
        setattr(rcfg, k, getattr(cfg, k))
    return cfg, rcfg


def raw_rows():
    path = os.path.join(REF, "data/raw_multidata_of_product_preatrain.small_train")
    return [l.rstrip("\n").split("\t") for l in open(path, encoding="utf-8")]


def gate_gaps(scores, noise):
    """Of every hard-gate choice (argmax over the three candidates of sigmoid score + noise, :2362-2364): the gap
    between the best and the second candidate.  Returns the smallest gap and (choices within 1e-5, within 1e-4,
    all choices)."""
    gaps = []
    for k, sc in scores.items():
        top = torch.topk(sc + torch.as_tensor(noise[k]), 2, dim=2).values
        gaps.append((top[:, :, 0] - top[:, :, 1]).reshape(-1))
    gaps = torch.cat(gaps)
    return float(gaps.min()), (int((gaps < 1e-5).sum()), int((gaps < 1e-4).sum()), gaps.numel())


def pretrain_case(name, row_ids, data_seed, weight_seed, noise_seed, neg_seed, T=36, P=128, NPV=20, R=12,
                  find_from=21, double=False):
    """noise_seed None: return the first noise seed from ``find_from`` on that leaves no gate choice within
    TIE_MARGIN of a tie (nothing is written).  double: run the reference in float64 and return its gradients
    (nothing is written)."""
    import vilbert_k3m.vilbert_k3m as K
    from vilbert_k3m.datasets.concept_cap_dataset_struc import BertPreprocessBatch
    from k3m_amd.weights import param_values

    rows = raw_rows()
    rows = [rows[i] for i in row_ids]
    pre = BertPreprocessBatch(CharTokenizer(), max_seq_len=T, max_seq_len_pv=P, max_num_pv=NPV, max_region_len=R,
                              visual_target=VISUAL_TARGET, v_target_size=V_TARGET_SIZE)
    batch = build_batch(pre, rows, data_seed, nbox=R)
    B = batch["input_ids"].shape[0]
    assert batch["image_target"].shape == (B, R, V_TARGET_SIZE), batch["image_target"].shape
    masked = (np.asarray(batch["image_label"]) == 1).sum(1)
    print(name, "masked regions per item", masked)
    assert (masked >= 1).all() and masked.sum() >= 3, "the target-row gather must cross items: %s" % (masked,)

    cfg, rcfg = cfgs()
    torch.manual_seed(0)
    model = K.BertForMultiModalPreTraining_tri_stru(rcfg)
    sd = {k: torch.from_numpy(v) for k, v in param_values(cfg, weight_seed).items()}
    sd["cls.predictions.decoder.weight"] = sd["embeddings.word_embeddings.weight"]
    model.load_state_dict(sd)
    model.tie_weights()
    model.eval()
    if double:
        model.double()
    assert isinstance(model.vis_criterion, torch.nn.MSELoss)

    shapes = [("v", (B, R + 1, 3, 1024)), ("t", (B, T, 3, 768)), ("pv", (B, P, 3, 768))]
    order, scores = {}, {}
    if noise_seed is None:   # "find" mode: the gate scores do not depend on the noise (:2331-2364); one forward
        noise = {k: torch.zeros(sh) for k, sh in shapes}
    else:
        noise = {k: torch.from_numpy(v) for k, v in gumbel_noise(noise_seed, shapes).items()}
    if double:
        noise = {k: v.double() for k, v in noise.items()}

    def fake_gumbel(logits, tau=1.0, hard=False, eps=1e-10, dim=-1):
        key = "v" if logits.shape[-1] == 1024 else ("t" if logits.shape[1] == T else "pv")
        order.setdefault(key, len(order))
        scores[key] = logits.detach().clone()
        y = ((logits + noise[key]) / tau).softmax(dim)
        idx = y.max(dim, keepdim=True)[1]
        hardv = torch.zeros_like(logits).scatter_(dim, idx, 1.0)
        return hardv - y.detach() + y

    draws = []
    real_sample = random.sample

    def rec_sample(pop, k):
        r = real_sample(pop, k)
        draws.append(list(r))
        return r

    K.F.gumbel_softmax = fake_gumbel
    cap = {}
    real_cls_forward = model.cls.forward

    def cls_capture(*a, **kw):   # BertPreTrainingHeads.forward (vilbert_k3m.py:1875-1909): keep the head outputs
        r = real_cls_forward(*a, **kw)
        cap["t"], cap["v"], cap["pv"], cap["nsp"] = r[0].detach(), r[1].detach(), r[2].detach(), r[6].detach()
        return r
    model.cls.forward = cls_capture
    random.seed(neg_seed)
    K.random.sample = rec_sample
    tb = {k: torch.from_numpy(np.asarray(v)) for k, v in batch.items()}
    if double:
        tb = {k: v.double() if v.dtype == torch.float32 else v for k, v in tb.items()}
    try:
        out = model(tb["input_ids"], tb["image_feat"], tb["image_loc"], tb["segment_ids"], tb["input_mask"],
                    tb["image_mask"], tb["lm_label_ids"], tb["image_label"], tb["image_target"], tb["is_next"],
                    input_ids_pv=tb["input_ids_pv"], token_type_ids_pv=tb["segment_ids_pv"],
                    attention_mask_pv=tb["input_mask_pv"], masked_lm_labels_pv=tb["lm_label_ids_pv"],
                    next_sentence_label_pv_v=tb["is_next_pv_v"], next_sentence_label_pv_t=tb["is_next_pv_t"],
                    index_p=tb["index_p"], index_v=tb["index_v"], device=torch.device("cpu"))
    finally:
        K.random.sample = real_sample
    if noise_seed is None:
        for seed in range(find_from, find_from + 20000):
            gap, near = gate_gaps(scores, gumbel_noise(seed, shapes))
            if gap >= TIE_MARGIN:
                print(name, "noise_seed %d: smallest gate gap %.3g (%d seeds tried)" % (seed, gap, seed - find_from + 1))
                return seed
        raise RuntimeError("no noise seed without a near-tie found")
    gap, near = gate_gaps(scores, noise)
    print(name, "smallest gate gap %.3g; choices within 1e-5 / 1e-4 of a tie: %d / %d of %d" % ((gap,) + near))
    assert gap >= TIE_MARGIN, "a hard-gate choice within %g of a tie: pick another noise_seed (CASES: find)" % TIE_MARGIN
    mlm_t, img, _, mlm_pv, _, _, nsp, c_init, c_final, lpm = out
    loss = mlm_t + img + mlm_pv + lpm
    loss.backward()
    mlm_t, img, mlm_pv, lpm, nsp, loss = [x.detach() for x in (mlm_t, img, mlm_pv, lpm, nsp, loss)]
    if double:
        return {n: p.grad.clone() for n, p in model.named_parameters() if p.grad is not None}

    # the negative tables in the reference's draw order (:2472-2497)
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
           "mode": np.array(1), "visual_target": np.array(VISUAL_TARGET), "gate_min_gap": np.array(gap, np.float64),
           "noise_order": np.array([order.get(k, -1) for k in ("v", "t", "pv")])}
    params = dict(model.named_parameters())
    gn_names, gn = [], []
    for n, p in params.items():
        gn_names.append(n)
        gn.append(np.nan if p.grad is None else float(p.grad.double().norm()))
    res["grad_norm_names"] = np.array(gn_names)
    res["grad_norms"] = np.array(gn, np.float64)
    dec = float(res["grad_norms"][gn_names.index(DECODER)])
    print(name, DECODER, "gradient norm", dec)
    assert dec > 0.0, dec
    # the reference's own error: its float64 run on the same inputs, against the parity bars the tests apply
    g64 = pretrain_case(name, row_ids, data_seed, weight_seed, noise_seed, neg_seed, T, P, NPV, R, double=True)
    own = 0.0
    for n in FULL_GRADS + SLICE_GRADS:
        a, b = params[n].grad.double(), g64[n]
        if b.abs().max() > 1e-6:   # (struc_w2.bias: the softmax is shift invariant, its gradient is rounding only)
            own = max(own, float((a - b).abs().max() / b.abs().max()))
    for n, b in g64.items():
        bn = float(b.norm())
        if bn > 1e-6:
            own = max(own, abs(float(params[n].grad.double().norm()) - bn) / bn)
    print(name, "the fp32 reference's gradients against its float64 run: worst %.3g of the 5e-3 bar's scale" % own)
    assert own <= OWN_ERROR, "the fp32 reference is %.3g from its own float64 run: pick another weight_seed" % own
    res["ref_own_error"] = np.array(own, np.float64)
    for n in FULL_GRADS:
        g = params[n].grad
        res["grad_full/" + n] = np.zeros(tuple(params[n].shape), np.float32) if g is None else g.numpy()
    for n in SLICE_GRADS:
        g = params[n].grad
        if g is None:
            g = torch.zeros(tuple(params[n].shape))
        res["grad_slice/" + n] = (g[:4] if g.dim() == 2 else g[:256]).numpy()
    # head outputs as in make_golden.run_case; logit/img_rows: the masked regions' 2048-d predictions
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
    assert pv_.shape[-1] == V_TARGET_SIZE
    res["logit/img_rows"] = pv_.reshape(-1, pv_.shape[-1])[
        torch.from_numpy(np.asarray(batch["image_label"]).reshape(-1) == 1)].numpy()
    res["logit/nsp"] = cap["nsp"].numpy()
    for k, v in batch.items():
        res["in/" + k] = np.asarray(v)
    path = os.path.join(HERE, "golden_%s.npz" % name)
    np.savez_compressed(path, **res)
    print(name, "losses", res["losses"], "->", path, os.path.getsize(path) // 1024, "KiB")
    assert os.path.getsize(path) < (1 << 20), "a committed file stays under 1 MiB"


def inventory():
    import vilbert_k3m.vilbert_k3m as K
    _, rcfg = cfgs()
    m = K.BertForMultiModalPreTraining_tri_stru(rcfg)
    out = {"config": "bert_base_6layer_6conect", "visual_target": VISUAL_TARGET,
           "params": [[n, list(p.shape)] for n, p in m.named_parameters()]}   # param_inventory.json's layout
    path = os.path.join(HERE, "param_inventory_visual_target.json")
    json.dump(out, open(path, "w"))
    print("inventory ->", path, len(out["params"]))


CASES = {
    "inventory": inventory,
    # noise_seed 309: the first from 21 on that leaves no gate choice within TIE_MARGIN of a tie ("find").
    # data_seed 119 masks 2 + 3 of the 12 regions (mask_region draws with probability 0.15; many seeds leave an
    # item without a masked region, which the assertion above refuses)
    "find": lambda: pretrain_case("vt1_bs2", row_ids=[14, 17], data_seed=119, weight_seed=62, noise_seed=None,
                                  neg_seed=51),
    "vt1_bs2": lambda: pretrain_case("vt1_bs2", row_ids=[14, 17], data_seed=119, weight_seed=62, noise_seed=309,
                                     neg_seed=51),
}


if __name__ == "__main__":
    _stub_imports()
    torch.set_num_threads(8)
    for name in (sys.argv[1:] or ["inventory", "vt1_bs2"]):
        CASES[name]()
