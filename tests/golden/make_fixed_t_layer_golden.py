"""Golden vectors for frozen lower text layers (``fixed_t_layer``) — BUILD container only.

Runs the unmodified reference with ``config.fixed_t_layer = t_biattention_id[0] = 6`` on the shipped config
(train_concap_struc.py:206-207 sets it when ``--freeze`` exceeds that id; BertEncoder then runs text layers 0..5
under ``torch.no_grad()`` in all three pair passes, vilbert_k3m.py:1188-1193, :1366-1371, :1542-1547, :1558-1566),
fp32, if_pre_sampling 1 (hard gate), model.eval(), bs=2, with the stubs, tokenizer, batch builder, recorded gumbel
noise and recorded LPM negatives of make_golden.py.  Records:

* ``golden_ftl6_bs2.npz``               one pretraining step: make_golden.run_case's keys plus ``fixed_t_layer``; the
                                        gradient norms carry NaN where the reference leaves ``.grad is None``;
* ``none_grad_fixed_t_layer.json``      the names the reference leaves with ``.grad is None`` after one backward, with
                                        ``fixed_t_layer = 6``, for: pretraining with the hard gate (``pretrain_mode1``),
                                        interactive-only fusion (``pretrain_mode3``), without the image modality
                                        (``pretrain_text_only``), item alignment (``item_alignment``; interactive-only:
                                        ``item_alignment_mode3``), and the hard gate with the freeze list of
                                        ``--freeze 8`` (``pretrain_mode1_freeze8``).

The freeze list of ``--freeze 8``: the embeddings and text layers 0..8 of config/bert-base-uncased_weight_name.json
(train_concap_struc.py:245-253).  The reference's loop compares ``key[12:]`` of its own parameter names with that
list (:255-257), which matches no name of a model that is not wrapped, so on its own command line nothing is
frozen by ``requires_grad``; the inventory records the list applied by name (the rule's purpose, and what
k3m_amd's ``frozen_names`` argument takes), i.e. ``requires_grad = False`` on exactly those 149 tensors.

Not blind.  The generator searches the weight seed (and, for each, the first noise seed without a near-tie) until
* every loss equals the reference's own ``fixed_t_layer = 0`` run on the same inputs (the cut changes no forward
  value),
* the gradient of ``encoder.layer.6.intermediate.dense.weight`` and of the position embeddings is non-zero,
* the position-embedding gradient differs from the unfrozen run's by at least CUT_MARGIN = ten times the 5e-3
  gradient bar of tests/test_gpu_parity.py (of its max element), so a backward that forgets the cut cannot pass,
* no hard-gate choice lies within TIE_MARGIN of a tie, and
* the fp32 gradients agree with the reference's float64 run to OWN_ERROR, a fifth of the 5e-3 bar
  (make_visual_target_golden.py explains both margins).

Usage:  python tests/golden/make_fixed_t_layer_golden.py [inventory|ftl6_bs2 ...]
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
from make_visual_target_golden import OWN_ERROR, TIE_MARGIN, gate_gaps, raw_rows  # noqa: E402

CFG = os.path.join(REPO, "configs/bert_base_6layer_6conect.json")
FIXED = 6
POS = "embeddings.position_embeddings.weight"
ABOVE = "encoder.layer.6.intermediate.dense.weight"
CUT_MARGIN = 10 * 5e-3
T, P, NPV, R = 36, 128, 20, 12
# gradients below the cut or of the embeddings, recorded beside make_golden's lists
EXTRA_FULL = ["embeddings.LayerNorm.bias"]
EXTRA_SLICE = [POS]


def ref_cfgs(mode=1, use_image=True, fixed=FIXED):
    import vilbert_k3m.vilbert_k3m as K
    from k3m_amd.config import pretrain_config
    cfg = pretrain_config(CFG, if_pre_sampling=mode, use_image=use_image)
    rcfg = K.BertConfig.from_json_file(CFG)
    for k in ("v_target_size", "visual_target", "with_coattention", "dynamic_attention", "if_pre_sampling",
              "num_negative", "use_image"):
        setattr(rcfg, k, getattr(cfg, k))
    assert fixed <= rcfg.t_biattention_id[0]
    rcfg.fixed_t_layer = fixed
    return cfg, rcfg


def the_batch(row_ids, data_seed):
    from vilbert_k3m.datasets.concept_cap_dataset_struc import BertPreprocessBatch
    rows = raw_rows()
    pre = BertPreprocessBatch(CharTokenizer(), max_seq_len=T, max_seq_len_pv=P, max_num_pv=NPV, max_region_len=R)
    return build_batch(pre, [rows[i] for i in row_ids], data_seed, nbox=R)


def step(batch, fixed, weight_seed, noise, neg_seed, mode=1, use_image=True, double=False, freeze=None):
    """One forward + backward of the reference's summed loss.  noise: {v,t,pv} arrays, or None for zeros (the gate
    scores do not depend on it).  Returns (model, outputs, gate scores, noise order, LPM draws, head capture)."""
    import vilbert_k3m.vilbert_k3m as K
    from k3m_amd.weights import param_values
    cfg, rcfg = ref_cfgs(mode, use_image, fixed)
    torch.manual_seed(0)
    model = K.BertForMultiModalPreTraining_tri_stru(rcfg)
    sd = {k: torch.from_numpy(v) for k, v in param_values(cfg, weight_seed).items()}
    sd["cls.predictions.decoder.weight"] = sd["embeddings.word_embeddings.weight"]
    model.load_state_dict(sd)
    model.tie_weights()
    model.eval()
    if double:
        model.double()
    if freeze is not None:
        for n, p in model.named_parameters():
            if n in freeze:
                p.requires_grad = False
    B = batch["input_ids"].shape[0]
    nc = 3 if use_image else 2
    shapes = ([("v", (B, R + 1, nc, 1024))] if use_image else []) + [("t", (B, T, nc, 768)), ("pv", (B, P, nc, 768))]
    nz = {k: torch.zeros(sh) if noise is None else torch.from_numpy(noise[k]) for k, sh in shapes}
    if double:
        nz = {k: v.double() for k, v in nz.items()}
    order, scores, draws, cap = {}, {}, [], {}

    def fake_gumbel(logits, tau=1.0, hard=False, eps=1e-10, dim=-1):
        key = "v" if logits.shape[-1] == 1024 else ("t" if logits.shape[1] == T else "pv")
        order.setdefault(key, len(order))
        scores[key] = logits.detach().clone()
        y = ((logits + nz[key]) / tau).softmax(dim)
        idx = y.max(dim, keepdim=True)[1]
        hardv = torch.zeros_like(logits).scatter_(dim, idx, 1.0)
        return hardv - y.detach() + y

    real_sample = random.sample

    def rec_sample(pop, k):
        r = real_sample(pop, k)
        draws.append(list(r))
        return r
    real_gumbel = K.F.gumbel_softmax
    K.F.gumbel_softmax = fake_gumbel
    real_cls_forward = model.cls.forward

    def cls_capture(*a, **kw):
        r = real_cls_forward(*a, **kw)
        cap["t"], cap["pv"], cap["nsp"] = r[0].detach(), r[2].detach(), r[6].detach()
        if use_image:
            cap["v"] = r[1].detach()
        return r
    model.cls.forward = cls_capture
    random.seed(neg_seed)
    K.random.sample = rec_sample
    tb = {k: torch.from_numpy(np.asarray(v)) for k, v in batch.items()}
    if double:
        tb = {k: v.double() if v.dtype == torch.float32 else v for k, v in tb.items()}
    img = [tb["image_feat"], tb["image_loc"]] if use_image else [None, None]
    try:
        out = model(tb["input_ids"], img[0], img[1], tb["segment_ids"], tb["input_mask"],
                    tb["image_mask"] if use_image else None, tb["lm_label_ids"],
                    tb["image_label"] if use_image else None, tb["image_target"] if use_image else torch.zeros(1),
                    tb["is_next"], input_ids_pv=tb["input_ids_pv"], token_type_ids_pv=tb["segment_ids_pv"],
                    attention_mask_pv=tb["input_mask_pv"], masked_lm_labels_pv=tb["lm_label_ids_pv"],
                    next_sentence_label_pv_v=tb["is_next_pv_v"], next_sentence_label_pv_t=tb["is_next_pv_t"],
                    index_p=tb["index_p"], index_v=tb["index_v"], device=torch.device("cpu"))
    finally:
        K.random.sample = real_sample
        K.F.gumbel_softmax = real_gumbel
    mlm_t, img_l, _, mlm_pv, _, _, nsp, c_init, c_final, lpm = out
    (mlm_t + img_l + mlm_pv + lpm).backward()
    return model, out, scores, order, draws, cap


def none_grads(model):
    return [n for n, p in model.named_parameters() if p.grad is None]


def freeze_list(model, freeze):
    bw = json.load(open(os.path.join(REF, "config/bert-base-uncased_weight_name.json"), encoding="utf-8"))
    keep = {n for n in bw if "embeddings" in n or ("encoder" in n and int(n.split(".")[2]) <= freeze)}
    return sorted(n for n, _ in model.named_parameters() if n in keep)


def item_alignment_none_grads(mode=1):
    """K3MForItemAlignment (loss_type "ce", with the image modality) with fixed_t_layer = 6."""
    import vilbert_k3m.vilbert_k3m as K
    from vilbert_k3m.datasets.concept_cap_dataset_struc import K3MPreprocessBatch
    from make_finetune_golden import build_pairs, ref_cfg, rows
    from k3m_amd.weights import param_values
    cfg, rcfg = ref_cfg("ce", mode)
    rcfg.fixed_t_layer = FIXED
    pre = K3MPreprocessBatch(CharTokenizer(), max_seq_len=T, max_seq_len_pv=P, max_num_pv=NPV, max_region_len=36)
    labels = [1, 0]
    _, cols = build_pairs(pre, rows()[120:124], labels, [36, 20, 9, 36], 2048, 1601, seed=120)
    torch.manual_seed(0)
    model = K.K3MForItemAlignment(rcfg)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in param_values(cfg, 5).items()}, strict=True)
    model.eval()
    tb = lambda k: torch.from_numpy(np.ascontiguousarray(cols[k]))  # noqa: E731
    args = [tb("labels")]
    for k in (1, 2):
        args += [tb("input_ids_%d" % k), tb("segment_ids_%d" % k), tb("input_mask_%d" % k), tb("input_ids_pv_%d" % k),
                 tb("segment_ids_pv_%d" % k), tb("input_mask_pv_%d" % k), tb("index_p_%d" % k), tb("index_v_%d" % k),
                 tb("coll_image_feat_%d" % k), tb("coll_image_loc_%d" % k), tb("coll_image_mask_%d" % k)]
    torch.manual_seed(1)   # (the gumbel draw: which candidate wins does not change who gets a gradient)
    model(*args)[3].backward()
    return none_grads(model)


def inventory():
    batch = the_batch([14, 17], 119)
    out = {"config": "bert_base_6layer_6conect", "fixed_t_layer": FIXED}
    m = step(batch, FIXED, 62, None, 51, mode=1)[0]
    out["pretrain_mode1"] = none_grads(m)
    fl = freeze_list(m, 8)
    out["freeze8_names"] = fl
    out["pretrain_mode1_freeze8"] = none_grads(step(batch, FIXED, 62, None, 51, mode=1, freeze=set(fl))[0])
    out["pretrain_mode3"] = none_grads(step(batch, FIXED, 62, None, 51, mode=3)[0])
    out["pretrain_text_only"] = none_grads(step(batch, FIXED, 62, None, 51, mode=1, use_image=False)[0])
    out["item_alignment"] = item_alignment_none_grads()
    out["item_alignment_mode3"] = item_alignment_none_grads(3)
    # the same runs without the cut, so a reader sees what the cut adds
    out["pretrain_mode1_unfrozen"] = none_grads(step(batch, 0, 62, None, 51, mode=1)[0])
    path = os.path.join(HERE, "none_grad_fixed_t_layer.json")
    json.dump(out, open(path, "w"), indent=0)
    print("inventory ->", path, {k: len(v) for k, v in out.items() if isinstance(v, list)})


def parity_case(name="ftl6_bs2", row_ids=(14, 17), data_seed=119, neg_seed=51, weight_seeds=range(62, 82)):
    batch = the_batch(list(row_ids), data_seed)
    B = batch["input_ids"].shape[0]
    shapes = [("v", (B, R + 1, 3, 1024)), ("t", (B, T, 3, 768)), ("pv", (B, P, 3, 768))]
    for weight_seed in weight_seeds:
        _, _, scores, _, _, _ = step(batch, FIXED, weight_seed, None, neg_seed)
        noise_seed = next((s for s in range(21, 20021) if gate_gaps(scores, gumbel_noise(s, shapes))[0] >= TIE_MARGIN),
                          None)
        if noise_seed is None:
            print(name, "weight_seed", weight_seed, "no noise seed without a near-tie")
            continue
        noise = gumbel_noise(noise_seed, shapes)
        model, out, scores, order, draws, cap = step(batch, FIXED, weight_seed, noise, neg_seed)
        gap, near = gate_gaps(scores, noise)
        assert gap >= TIE_MARGIN
        m0, out0 = step(batch, 0, weight_seed, noise, neg_seed)[:2]
        m64 = step(batch, FIXED, weight_seed, noise, neg_seed, double=True)[0]
        params, p0, p64 = dict(model.named_parameters()), dict(m0.named_parameters()), dict(m64.named_parameters())
        same = all(float(out[i]) == float(out0[i]) for i in (0, 1, 3, 6, 9))
        gpos, gpos0 = params[POS].grad, p0[POS].grad
        cut = float((gpos - gpos0).abs().max() / gpos.abs().max())
        own = 0.0
        for n in FULL_GRADS + SLICE_GRADS + EXTRA_FULL + EXTRA_SLICE:
            if params[n].grad is None:
                assert p64[n].grad is None, n
                continue
            a, b = params[n].grad.double(), p64[n].grad
            if b.abs().max() > 1e-6:
                own = max(own, float((a - b).abs().max() / b.abs().max()))
        for n, p in p64.items():
            assert (p.grad is None) == (params[n].grad is None), n
            if p.grad is not None and float(p.grad.norm()) > 1e-6:
                own = max(own, abs(float(params[n].grad.double().norm()) - float(p.grad.norm())) / float(p.grad.norm()))
        print(name, "weight_seed %d noise_seed %d: gate gap %.3g, losses equal the unfrozen run's: %s, position-"
              "embedding gradient %.3g from the unfrozen run's (of its max), own error %.3g"
              % (weight_seed, noise_seed, gap, same, cut, own))
        ok = (same and float(params[ABOVE].grad.abs().max()) > 0 and float(gpos.abs().max()) > 0
              and cut >= CUT_MARGIN and own <= OWN_ERROR)
        if ok:
            break
    else:
        raise RuntimeError("no seed satisfies the checks")

    mlm_t, img, mlm_pv, nsp, c_init, c_final, lpm = [out[i].detach() for i in (0, 1, 3, 6, 7, 8, 9)]
    loss = mlm_t + img + mlm_pv + lpm
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
           "c_initial": c_init.numpy(), "c_final": c_final.numpy(), "ent_neg": ent, "val_neg": val,
           "noise_seed": np.array(noise_seed), "weight_seed": np.array(weight_seed), "mode": np.array(1),
           "fixed_t_layer": np.array(FIXED), "gate_min_gap": np.array(gap, np.float64),
           "ref_own_error": np.array(own, np.float64), "cut_margin_seen": np.array(cut, np.float64),
           "noise_order": np.array([order.get(k, -1) for k in ("v", "t", "pv")])}
    names, gn = [], []
    for n, p in params.items():
        names.append(n)
        gn.append(np.nan if p.grad is None else float(p.grad.double().norm()))
    res["grad_norm_names"] = np.array(names)
    res["grad_norms"] = np.array(gn, np.float64)
    for n in FULL_GRADS + EXTRA_FULL:
        g = params[n].grad
        res["grad_full/" + n] = np.zeros(tuple(params[n].shape), np.float32) if g is None else g.numpy()
    for n in SLICE_GRADS + EXTRA_SLICE:
        g = params[n].grad
        if g is None:
            g = torch.zeros(tuple(params[n].shape))
        res["grad_slice/" + n] = (g[:4] if g.dim() == 2 else g[:256]).numpy()
    for k, v in batch.items():
        res["in/" + k] = np.asarray(v)
    path = os.path.join(HERE, "golden_%s.npz" % name)
    np.savez_compressed(path, **res)
    print(name, "losses", res["losses"], "never-grad", int(np.isnan(res["grad_norms"]).sum()), "->", path,
          os.path.getsize(path) // 1024, "KiB")
    assert os.path.getsize(path) < (1 << 20), "a committed file stays under 1 MiB"


CASES = {"inventory": inventory, "ftl6_bs2": parity_case}


if __name__ == "__main__":
    _stub_imports()
    torch.set_num_threads(8)
    for name in (sys.argv[1:] or list(CASES)):
        CASES[name]()
