"""Item classification on the GPU: K3MForItemClassification through libk3m_hip against the CPU oracle.

The batch is the "ce" fine-tune golden's two pairs as four single items (item 1 rows, then item 2 rows; the gumbel
noise concatenated the same way), C = 5, labels [2, 0, -1, 4], weights from param_values, dropout probabilities 0.
The CPU side is oracle.encode -> oracle.structure_aggregator -> a torch head (oracle.linear, torch.tanh,
F.cross_entropy(ignore_index=-1)) under autograd; the encoder graph is built once for the module and both loss
variants differentiate it.  Bars as tests/test_gpu_finetune.py: loss rtol 1e-3, logits rtol 1e-3 / atol 1e-4 (its
embedding bar), gradients err <= 5e-3 max|ref| + 1e-6, the AdamW update rtol 1e-6.

Without the image modality the oracle has no encoder, so that case takes the reference's own c_final of the four
items from the text-only cosine golden (its e1 / e2 are c_final; the weights are name-keyed, so the encoder's are the
same) and runs the torch head on it: loss and the four classifier gradients.
"""
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from golden_util import CFG_PATH, ft_noise, ft_pair, load_ft_case

pytestmark = pytest.mark.gpu
C = 5
LABELS = [2, 0, -1, 4]
NAMES = ["classifier.out_proj.weight", "classifier.dense.weight", "classifier.dense.bias", "struc_w1.weight",
         "encoder.layer.0.output.dense.bias", "embeddings.LayerNorm.weight", "v_embeddings.image_embeddings.weight",
         "t_pooler.dense.weight"]
CLASS_WEIGHT = np.array([0.5, 2.0, 1.0, 0.0, 1.5], np.float32)
VARIANTS = {"plain": (0.0, None), "smoothed_weighted": (0.1, CLASS_WEIGHT)}


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda")


def _config(g, eps=0.0, **kw):
    from k3m_amd.config import classify_config
    cfg = classify_config(CFG_PATH, C, if_pre_sampling=int(g["mode"]), label_smoothing=eps, **kw)
    cfg.hidden_dropout_prob = cfg.attention_probs_dropout_prob = 0.0
    cfg.v_hidden_dropout_prob = cfg.v_attention_probs_dropout_prob = 0.0
    return cfg


def _items(g):
    """(batch of the 4 single items with labels, their gumbel noise), on the host"""
    from oracle import k3m_oracle as O
    pair = ft_pair(g)
    a, b = O.item_batch(pair, 1), O.item_batch(pair, 2)
    batch = {k: torch.cat([a[k], b[k]]) for k in a}
    batch["labels"] = torch.tensor(LABELS, dtype=torch.int64)
    n1, n2 = ft_noise(g)
    return batch, {k: torch.cat([n1[k], n2[k]]) for k in n1}


def _to(d, dev):
    return {k: v.to(dev) for k, v in d.items()}


@pytest.fixture(scope="module")
def case():
    """The golden, the host batch and noise, the weights and, per variant, the oracle's (loss, logits, gradients)."""
    from k3m_amd.weights import param_values
    from oracle import k3m_oracle as O
    g = load_ft_case("ce")
    cfg = _config(g)
    batch, noise = _items(g)
    vals = param_values(cfg, int(g["weight_seed"]))
    torch.set_num_threads(16)
    P = {k: torch.from_numpy(v).requires_grad_(True) for k, v in vals.items()}
    enc = O.encode(P, cfg, batch, noise)
    cf, _ = O.structure_aggregator(P, enc["c_init"], enc["seq_pv"], batch["index_p"], batch["index_v"], None, None, 0.0)
    logits = O.linear(P, "classifier.out_proj", torch.tanh(O.linear(P, "classifier.dense", cf)))
    ref = {}
    for name, (eps, w) in VARIANTS.items():
        loss = F.cross_entropy(logits, batch["labels"], weight=None if w is None else torch.from_numpy(w),
                               ignore_index=-1, label_smoothing=eps)
        grads = torch.autograd.grad(loss, [P[n] for n in NAMES], retain_graph=True, allow_unused=True)
        ref[name] = (float(loss.detach()), dict(zip(NAMES, grads)))
    return {"g": g, "batch": batch, "noise": noise, "vals": vals, "logits": logits.detach().numpy(), "ref": ref}


def _model(case, dev, eps=0.0, w=None):
    from k3m_amd.classify import K3MForItemClassification
    model = K3MForItemClassification(_config(case["g"], eps), dev, class_weight=None if w is None else torch.from_numpy(w))
    model.engine.fp.load(case["vals"])
    return model


def _check_grads(G, ref):
    for n in NAMES:
        r = ref[n]
        if r is None:
            assert n == "t_pooler.dense.weight" and float(G[n].abs().max()) == 0.0, n
        else:
            err = (G[n].cpu() - r).abs().max().item()
            print(n, "err", err, "max |ref|", r.abs().max().item())
            assert err <= 5e-3 * r.abs().max().item() + 1e-6, (n, err)


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_forward_backward_match_the_oracle(dev, case, variant):
    eps, w = VARIANTS[variant]
    model = _model(case, dev, eps, w)
    logits, loss = model(_to(case["batch"], dev), train=True, noise=_to(case["noise"], dev))
    model.backward()
    torch.cuda.synchronize()
    ref_loss, ref_grads = case["ref"][variant]
    print(variant, "loss", float(loss), ref_loss)
    np.testing.assert_allclose(float(loss), ref_loss, rtol=1e-3)
    np.testing.assert_allclose(logits.cpu().numpy(), case["logits"], rtol=1e-3, atol=1e-4)
    assert np.array_equal(model.pred.cpu().numpy(), logits.argmax(1).cpu().numpy().astype(np.int32))
    _check_grads(model.engine.fp.g, ref_grads)
    with pytest.raises(RuntimeError):
        model.backward()   # the ctx is consumed


def test_trainer_step_matches_adamw_restatement(dev, case):
    """One ItemClassificationTrainer.step: the update against oracle.adamw_torch_step on the GPU's own gradients
    (taken as the step hands them to the optimizer)."""
    from k3m_amd.classify import ItemClassificationTrainer
    from k3m_amd.params import is_frozen, is_no_decay
    from oracle import k3m_oracle as O
    lr = 1e-4
    tr = ItemClassificationTrainer(_config(case["g"]), dev, lr=lr, warmup_steps=0, total_steps=100, init=False)
    tr.engine.fp.load(case["vals"])
    G = {}
    step = tr.optimizer_step

    def snapshot(**kw):
        G.update({n: tr.engine.fp.g[n].cpu().clone() for n in NAMES})
        return step(**kw)

    tr.optimizer_step = snapshot
    out = tr.step(_to(case["batch"], dev), noise=_to(case["noise"], dev))
    torch.cuda.synchronize()
    assert sorted(out) == ["logits", "loss", "pred"] and tr.global_step == 1
    ref_loss, ref_grads = case["ref"]["plain"]
    np.testing.assert_allclose(float(out["loss"]), ref_loss, rtol=1e-3)
    assert np.array_equal(out["pred"].cpu().numpy(), out["logits"].argmax(1).cpu().numpy().astype(np.int32))
    _check_grads(G, ref_grads)
    assert float(tr.engine.fp.grad.abs().max()) == 0.0   # zeroed by the step
    for n in NAMES:
        p = torch.from_numpy(case["vals"][n]).clone()
        if not is_frozen(n):
            m, v = torch.zeros_like(p), torch.zeros_like(p)
            O.adamw_torch_step(p, G[n], m, v, 1, lr, 0.0 if is_no_decay(n) else 0.01)
        np.testing.assert_allclose(tr.engine.fp.p[n].cpu().numpy(), p.numpy(), rtol=1e-6, atol=1e-7 * lr / 1e-4,
                                   err_msg=n)
    tr.finish()


def test_predict_matches_forward_and_keeps_a_pending_ctx(dev, case):
    from k3m_amd import ops
    model = _model(case, dev)
    batch, noise = _to(case["batch"], dev), _to(case["noise"], dev)
    logits, _ = model(batch, train=False, noise=noise)
    fp = model.engine.fp
    fp.grad.normal_()
    before = fp.grad.clone()
    r = model.predict(batch, k=3, noise=noise)
    torch.cuda.synchronize()
    assert torch.equal(fp.grad, before)
    assert r["ids"].shape == (4, 3) and r["ids"].dtype == torch.int64 and r["logp"].shape == (4, 3)
    assert torch.equal(r["ids"][:, 0], logits.argmax(1))
    lp = torch.log_softmax(logits.double(), 1)
    np.testing.assert_allclose(r["logp"].cpu().numpy(), lp.gather(1, r["ids"]).cpu().numpy(), rtol=1e-3, atol=1e-5)
    np.testing.assert_allclose(r["lse"].cpu().numpy(), torch.logsumexp(logits.double(), 1).cpu().numpy(), rtol=1e-3,
                               atol=1e-5)
    gold = r["gold_logp"].cpu().numpy()
    assert gold[2] == -np.inf
    rows = [0, 1, 3]
    np.testing.assert_allclose(gold[rows], lp.cpu().numpy()[rows, [LABELS[i] for i in rows]], rtol=1e-3, atol=1e-5)
    nolab = {k: v for k, v in batch.items() if k != "labels"}
    r2 = model.predict(nolab, k=C + 2, noise=noise)     # no labels: no gold; slots past C hold (-inf, -1)
    assert "gold_logp" not in r2
    assert bool((r2["ids"][:, C:] == -1).all()) and bool(torch.isinf(r2["logp"][:, C:]).all())
    assert torch.equal(r2["ids"][:, :3], r["ids"])
    with pytest.raises(ValueError):
        model.predict(batch, k=ops.TOPK_LOGITS_MAX_K + 1, noise=noise)
    fp.grad.zero_()
    model.backward()                                     # the pending forward's backward still runs
    torch.cuda.synchronize()
    assert float(fp.g["classifier.out_proj.weight"].abs().max()) > 0.0
    with pytest.raises(ValueError):
        model.engine.predict_masked(batch)               # no prediction heads in this engine


def test_train_mode_dropout_follows_the_seed(dev, case):
    from k3m_amd.classify import K3MForItemClassification
    from k3m_amd.config import classify_config
    cfg = classify_config(CFG_PATH, C, if_pre_sampling=int(case["g"]["mode"]))
    assert cfg.hidden_dropout_prob == pytest.approx(0.1)
    model = K3MForItemClassification(cfg, dev)
    model.engine.fp.load(case["vals"])
    batch = _to(case["batch"], dev)
    losses = []
    for seed in (3, 3, 4):
        _, loss = model(batch, train=True, seed=seed)
        model._ctx = None
        losses.append(float(loss))
    print("train-mode losses", losses)
    assert np.isfinite(losses).all() and losses[0] == losses[1] and losses[0] != losses[2]


def test_bad_label_is_nan_and_debug_mode_names_the_field(dev, case):
    from k3m_amd import debug
    model = _model(case, dev)
    batch, noise = _to(case["batch"], dev), _to(case["noise"], dev)
    batch["labels"] = torch.tensor([2, C, -1, 4], dtype=torch.int64, device=dev)
    _, loss = model(batch, train=False, noise=noise)
    model._ctx = None
    assert np.isnan(float(loss))
    old = debug.ON
    debug.set_debug(True)
    try:
        with pytest.raises(debug.K3mIndexError, match="labels"):
            model(batch, train=False, noise=noise)
    finally:
        debug.set_debug(old)
    with pytest.raises(ValueError):
        model(dict(batch, labels=batch["labels"].float()), train=False, noise=noise)
    with pytest.raises(ValueError):
        model.set_class_weight(torch.tensor([1.0, -1.0, 1.0, 1.0, 1.0]))


def test_text_only_matches_the_reference_embeddings(dev):
    """use_image=False: the model's loss and classifier gradients against a torch head on the reference's c_final."""
    from k3m_amd.classify import K3MForItemClassification
    from k3m_amd.weights import param_values
    from oracle import k3m_oracle as O
    g = load_ft_case("to_cosine")
    cfg = _config(g, use_image=False)
    model = K3MForItemClassification(cfg, dev)
    vals = param_values(cfg, int(g["weight_seed"]))
    model.engine.fp.load(vals)
    t = lambda k: torch.from_numpy(np.ascontiguousarray(g["out/" + k]))  # noqa: E731
    keys = [("input_ids", "input_ids"), ("segment_ids", "segment_ids"), ("input_mask", "input_mask"),
            ("input_ids_pv", "input_ids_pv"), ("segment_ids_pv", "segment_ids_pv"), ("input_mask_pv", "input_mask_pv"),
            ("index_p", "index_p"), ("index_v", "index_v")]
    batch = {dst: torch.cat([t("%s_1" % src), t("%s_2" % src)]) for src, dst in keys}
    assert bool((batch["index_p"][:, 0, 0] != 0).all())   # no zero-triple item: the two pairs' batches do not interact
    batch["labels"] = torch.tensor(LABELS, dtype=torch.int64)
    B, T = g["out/input_ids_1"].shape
    P = g["out/input_ids_pv_1"].shape[1]
    nz = []
    for s in (int(g["noise_seed"]), int(g["noise_seed"]) + 1):
        rng = np.random.default_rng(s)
        nz.append({k: torch.from_numpy((-np.log(rng.standard_exponential(sh))).astype(np.float32))
                   for k, sh in [("t", (B, T, 2, 768)), ("pv", (B, P, 2, 768))]})
    noise = {k: torch.cat([nz[0][k], nz[1][k]]) for k in nz[0]}
    logits, loss = model(_to(batch, dev), train=True, noise=_to(noise, dev))
    model.backward()
    torch.cuda.synchronize()
    names = ["classifier.dense.weight", "classifier.dense.bias", "classifier.out_proj.weight", "classifier.out_proj.bias"]
    Pm = {n: torch.from_numpy(vals[n]).requires_grad_(True) for n in names}
    cf = torch.from_numpy(np.concatenate([g["out/e1"], g["out/e2"]]))
    ref_logits = O.linear(Pm, "classifier.out_proj", torch.tanh(O.linear(Pm, "classifier.dense", cf)))
    ref_loss = F.cross_entropy(ref_logits, batch["labels"], ignore_index=-1)
    ref_loss.backward()
    ref = float(ref_loss.detach())
    print("text-only loss", float(loss), ref)
    np.testing.assert_allclose(float(loss), ref, rtol=1e-3)
    np.testing.assert_allclose(logits.cpu().numpy(), ref_logits.detach().numpy(), rtol=1e-3, atol=1e-4)
    G = model.engine.fp.g
    for n in names:
        r = Pm[n].grad
        err = (G[n].cpu() - r).abs().max().item()
        assert err <= 5e-3 * r.abs().max().item() + 1e-6, (n, err)
    assert float(G["encoder.layer.0.output.dense.bias"].abs().max()) > 0.0
    assert float(G["t_pooler.dense.weight"].abs().max()) == 0.0


def test_save_model_and_load_encoder(dev, case, tmp_path):
    from k3m_amd.classify import load_encoder, save_model
    from k3m_amd.data import LabelVocab
    model = _model(case, dev)
    batch, noise = _to(case["batch"], dev), _to(case["noise"], dev)
    vocab = LabelVocab(["a", "b", "c", "d", "e"], [3, 1, 2, 2, 4])
    path = str(tmp_path / "K3M_item_classification-1_epoch-0.bin")
    save_model(model, path, vocab)
    sd = torch.load(path, map_location="cpu", weights_only=True)
    assert len(sd) == 989 and tuple(sd["classifier.out_proj.weight"].shape) == (C, 768)
    assert tuple(sd["classifier.dense.weight"].shape) == (768, 768)
    assert json.load(open(os.path.join(str(tmp_path), "labels.json"), encoding="utf-8"))["names"] == vocab.names
    logits, _ = model(batch, train=False, noise=noise)
    model._ctx = None
    other = _model(case, dev)
    other.engine.fp.data.mul_(0.5)
    assert load_encoder(other, sd) == []
    got, _ = other(batch, train=False, noise=noise)
    torch.cuda.synchronize()
    os.remove(path)   # 1 GB: not left in the session's temporary directory
    assert torch.equal(got, logits)
