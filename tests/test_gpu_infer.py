"""Item-embedding inference on the GPU: K3MEngine.embed, K3MForItemAlignment.item_embedding / predict.

* dedup off: embed is torch.equal to forward(train=False) on the same batch, noise and seed (the forward-only kernel
  forms are bit-identical and the launches are the same), fp32 and bf16, every accepted model switch;
* dedup on (the default): predict against the reference goldens at the bars of tests/test_gpu_finetune.py;
* dedup on against dedup off: measured distances (narrow GEMMs may take other tiles), bounded by the distance of the
  same arithmetic from its reference;
* reproducibility by seed; no training state (gradients untouched, backward() raises, peak memory).
Fixtures: the bs-2 goldens (T 36, P 128, 37 regions)."""
import numpy as np
import pytest
import torch

from golden_util import CFG_PATH, case_batch, case_config, case_noise, ft_config, ft_noise, ft_pair, load_case, load_ft_case

pytestmark = pytest.mark.gpu
CASES = ["ce", "cosine", "ce_soft", "da_ce_bs2", "to_ce", "noco_ce"]
OUT_KEYS = ("c_initial", "c_final", "pooled_t", "pooled_pv", "pooled_v")


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda")


def _case_config(case, g):
    from k3m_amd.config import finetune_config
    if case == "da_ce_bs2":
        return finetune_config(CFG_PATH, loss_type="ce", if_pre_sampling=1, dynamic_attention=True)
    if case == "to_ce":
        return finetune_config(CFG_PATH, loss_type=str(g["loss_type"]), use_image=False, if_pre_sampling=int(g["mode"]))
    if case == "noco_ce":
        return finetune_config(CFG_PATH, loss_type="ce", with_coattention=False, if_pre_sampling=int(g["mode"]))
    return ft_config(g)


def _case_inputs(case, g, dev):
    """(pair dict, noise pair) on the device"""
    if case == "da_ce_bs2":   # stored as fp16
        g["out/coll_image_feat_1"] = g["out/coll_image_feat_1"].astype(np.float32)
        g["out/coll_image_feat_2"] = g["out/coll_image_feat_2"].astype(np.float32)
    if case == "to_ce":
        t = lambda k: torch.from_numpy(np.ascontiguousarray(g["out/" + k]))  # noqa: E731
        pair = {"labels": t("labels")}
        for k in (1, 2):
            for a, b in (("input_ids", "input_ids"), ("token_type_ids", "segment_ids"), ("attention_mask", "input_mask"),
                         ("input_ids_pv", "input_ids_pv"), ("token_type_ids_pv", "segment_ids_pv"),
                         ("attention_mask_pv", "input_mask_pv"), ("index_p", "index_p"), ("index_v", "index_v")):
                pair["%s_%d" % (a, k)] = t("%s_%d" % (b, k))
        B, T = pair["input_ids_1"].shape
        P = pair["input_ids_pv_1"].shape[1]
        noise = []
        for s in (int(g["noise_seed"]), int(g["noise_seed"]) + 1):
            rng = np.random.default_rng(s)
            noise.append({k: torch.from_numpy((-np.log(rng.standard_exponential(sh))).astype(np.float32))
                          for k, sh in [("t", (B, T, 2, 768)), ("pv", (B, P, 2, 768))]})
    else:
        pair, noise = ft_pair(g), ft_noise(g)
    ns = float(g["noise_scale"]) if "noise_scale" in g else 1.0
    pair = {k: v.to(dev) for k, v in pair.items()}
    noise = tuple({k: (v * ns).to(dev) if ns != 1.0 else v.to(dev) for k, v in nz.items()} for nz in noise)
    return pair, noise


_MODELS = {}


def _model(case, dtype, dev):
    """(model, golden, pair, noise), built once per (case, dtype); a test sets engine.infer_dedup itself"""
    from k3m_amd.finetune import K3MForItemAlignment
    from k3m_amd.weights import param_values
    key = (case, dtype)
    if key not in _MODELS:
        g = load_ft_case(case)
        cfg = _case_config(case, g)
        model = K3MForItemAlignment(cfg, dev, dtype=dtype)
        # (the dynamic-attention fixture records its own weight scale and noise scale)
        std = {"std": float(g["weight_std"])} if "weight_std" in g else {}
        model.engine.fp.load(param_values(cfg, int(g["weight_seed"]), **std))
        pair, noise = _case_inputs(case, g, dev)
        _MODELS.clear()   # one model on the device at a time
        _MODELS[key] = (model, g, pair, noise)
    m = _MODELS[key]
    m[0].engine.infer_dedup = True
    return m


def _stacked(model, pair, noise):
    from k3m_amd.finetune import _pair_args
    _, batch, nz, _ = model._stacked((), _pair_args(pair, model.engine.use_image), noise)
    return batch, nz


def _dist(a, b):
    return float((a.double() - b.double()).abs().max())


# ---------------------------------------------------------------- dedup off: the bits of forward(train=False)
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("case", CASES)
def test_embed_equals_eval_forward_without_dedup(dev, case, dtype):
    model, g, pair, noise = _model(case, dtype, dev)
    eng = model.engine
    batch, nz = _stacked(model, pair, noise)
    eng.infer_dedup = False
    for kw in (dict(noise=nz, seed=3), dict(noise=None, seed=5)):   # explicit noise, then the Philox draw
        ref, ctx = eng.forward(batch, train=False, groups=2, **kw)
        del ctx
        got = eng.embed(batch, groups=2, **kw)
        torch.cuda.synchronize()
        assert set(got) == set(OUT_KEYS)
        for k in OUT_KEYS:
            if ref[k] is None:
                assert got[k] is None and not eng.use_image
            else:
                assert torch.isfinite(got[k]).all() and torch.equal(got[k], ref[k]), (k, _dist(got[k], ref[k]))


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_no_coattention_with_dynamic_attention(dev, dtype):
    """with_coattention=False + dynamic_attention: the one configuration whose image stream splits in the middle of
    the encoder (at image layer 0, one buffer copied into the wide one) while the text stream never splits, so the
    fusion sees a wide image stream beside a single text buffer.  Dedup off equals forward(train=False) bit for bit;
    dedup on is compared with it: the image layers then run the same rows, the text layers half of them, whose
    products are row-independent -- measured, and bounded by the dtype's rounding of the outputs' scale (fp32
    2^-20, bf16 2^-6: a few ulps of the encoder dtype), both with explicit noise and with the Philox draw."""
    from k3m_amd.config import finetune_config
    from k3m_amd.finetune import K3MForItemAlignment
    from k3m_amd.infer import infer_plan
    from k3m_amd.weights import param_values
    _MODELS.clear()
    g = load_ft_case("noco_ce")
    cfg = finetune_config(CFG_PATH, loss_type="ce", with_coattention=False, dynamic_attention=True)
    plan = infer_plan(cfg)
    assert any(e.kind == "v" and e.image == "split" and e.text == "merged" for e in plan)
    model = K3MForItemAlignment(cfg, dev, dtype=dtype)
    model.engine.fp.load(param_values(cfg, int(g["weight_seed"]), std=0.04))   # a scale at which the gate matters
    pair, noise = _case_inputs("noco_ce", g, dev)
    eng = model.engine
    assert eng.dyn_attn and not eng.coattn
    batch, nz = _stacked(model, pair, noise)
    for kw in (dict(noise=nz, seed=3), dict(noise=None, seed=5)):
        ref, ctx = eng.forward(batch, train=False, groups=2, **kw)
        del ctx
        eng.infer_dedup = False
        off = eng.embed(batch, groups=2, **kw)
        eng.infer_dedup = True
        on = eng.embed(batch, groups=2, **kw)
        torch.cuda.synchronize()
        for k in OUT_KEYS:
            assert torch.isfinite(on[k]).all() and torch.equal(off[k], ref[k]), k
            d, scale = _dist(on[k], ref[k]), float(ref[k].abs().max())
            print(dtype, "noise" if kw["noise"] is not None else "philox", k, "|on - off| %.3e of max %.3e" % (d, scale))
            assert d <= (2.0 ** -20 if dtype == "fp32" else 2.0 ** -6) * scale, (k, d, scale)


def test_embed_one_group_equals_eval_forward_without_dedup(dev):
    """groups=1 over the same stacked rows (the zero-triple fallback then crosses the whole batch)"""
    model, g, pair, noise = _model("ce", "fp32", dev)
    eng = model.engine
    batch, nz = _stacked(model, pair, noise)
    eng.infer_dedup = False
    ref, ctx = eng.forward(batch, train=False, noise=nz, seed=3, groups=1)
    del ctx
    got = eng.embed(batch, noise=nz, seed=3, groups=1)
    torch.cuda.synchronize()
    for k in OUT_KEYS:
        assert torch.equal(got[k], ref[k]), k


def test_dedup_knob_is_read_when_the_engine_is_built(dev, monkeypatch):
    from k3m_amd.config import finetune_config
    from k3m_amd.engine import K3MEngine
    cfg = finetune_config(CFG_PATH, loss_type="ce")
    _MODELS.clear()
    assert K3MEngine(cfg, dev).infer_dedup is True
    monkeypatch.setenv("K3M_INFER_DEDUP", "0")
    assert K3MEngine(cfg, dev).infer_dedup is False


# ---------------------------------------------------------------- dedup on: the reference goldens
@pytest.mark.parametrize("case", CASES)
def test_predict_matches_reference_golden(dev, case):
    from k3m_amd.finetune import ARG_NAMES, _pair_args
    model, g, pair, noise = _model(case, "fp32", dev)
    assert model.engine.infer_dedup
    if model.engine.use_image:
        e1, e2, probs, loss = model.predict(*[pair[k] for k in ARG_NAMES], noise=noise)
    else:
        e1, e2, probs, loss = model.predict(**_pair_args(pair, False), noise=noise)
    torch.cuda.synchronize()
    print(case, "loss", float(loss), float(g["out/loss"]), "e1", _dist(e1.cpu(), torch.from_numpy(g["out/e1"])),
          "e2", _dist(e2.cpu(), torch.from_numpy(g["out/e2"])))
    np.testing.assert_allclose(float(loss), float(g["out/loss"]), rtol=1e-3, atol=1e-5)
    np.testing.assert_allclose(e1.cpu().numpy(), g["out/e1"], rtol=1e-3, atol=1e-4)
    np.testing.assert_allclose(e2.cpu().numpy(), g["out/e2"], rtol=1e-3, atol=1e-4)
    np.testing.assert_allclose(probs.cpu().numpy(), g["out/probs"], rtol=1e-3, atol=1e-5)


def test_item_embedding_matches_reference_golden(dev):
    """c_initial / c_final of both items against the reference's own item_embedding on golden_ft_ce's inputs and
    weights (tests/golden/golden_item_embedding.npz), at the bars of tests/test_gpu_finetune.py; dedup on."""
    import os
    from golden_util import HERE
    model, g, pair, _ = _model("ce", "fp32", dev)
    z = np.load(os.path.join(HERE, "golden", "golden_item_embedding.npz"), allow_pickle=False)
    assert float(z["gate_min_gap"]) >= 4e-5 and model.engine.infer_dedup
    assert int(z["weight_seed"]) == int(g["weight_seed"])
    # the fixture's own noise (golden_ft_ce's has a gate choice 4.8e-7 from a tie, which its generator refuses)
    g2 = dict(g, noise_seed=z["noise_seed"])
    noise = tuple({k: (v * float(z["noise_scale"])).to(dev) for k, v in nz.items()} for nz in ft_noise(g2))
    for k in (1, 2):
        ci, cf = model.item_embedding(
            pair["input_ids_%d" % k], pair["image_feat_%d" % k], pair["image_loc_%d" % k],
            token_type_ids=pair["token_type_ids_%d" % k], attention_mask=pair["attention_mask_%d" % k],
            image_attention_mask=pair["image_attention_mask_%d" % k], input_ids_pv=pair["input_ids_pv_%d" % k],
            token_type_ids_pv=pair["token_type_ids_pv_%d" % k], attention_mask_pv=pair["attention_mask_pv_%d" % k],
            index_p=pair["index_p_%d" % k], index_v=pair["index_v_%d" % k], noise=noise[k - 1])
        torch.cuda.synchronize()
        print("item", k, "c_initial", _dist(ci.cpu(), torch.from_numpy(z["c_initial_%d" % k])), "c_final",
              _dist(cf.cpu(), torch.from_numpy(z["c_final_%d" % k])))
        np.testing.assert_allclose(ci.cpu().numpy(), z["c_initial_%d" % k], rtol=1e-3, atol=1e-4)
        np.testing.assert_allclose(cf.cpu().numpy(), z["c_final_%d" % k], rtol=1e-3, atol=1e-4)
    with pytest.raises(TypeError):
        model.item_embedding(pair["input_ids_1"], pair["image_feat_1"], pair["image_loc_1"])


# ---------------------------------------------------------------- dedup on against dedup off (measured)
def _cosine_c_final(dev, dtype, dedup):
    model, g, pair, noise = _model("cosine", dtype, dev)
    batch, nz = _stacked(model, pair, noise)
    model.engine.infer_dedup = dedup
    cf = model.engine.embed(batch, noise=nz, groups=2)["c_final"].clone()
    torch.cuda.synchronize()
    return cf, torch.from_numpy(np.concatenate([g["out/e1"], g["out/e2"]])).to(dev)


def test_dedup_distance(dev):
    """Mean fusion (no gate to flip).  fp32: dedup on is no farther from dedup off than dedup off is from the
    reference golden (both are rounding noise of the same arithmetic).  bf16: dedup on is at most twice as far from
    the fp32 dedup-off result as the bf16 dedup-off result is (two draws of the same rounding noise)."""
    off32, ref = _cosine_c_final(dev, "fp32", False)
    on32, _ = _cosine_c_final(dev, "fp32", True)
    d_on_off, d_off_ref = _dist(on32, off32), _dist(off32, ref)
    print("fp32 cosine c_final: |on - off| %.3e  |off - golden| %.3e" % (d_on_off, d_off_ref))
    off16, _ = _cosine_c_final(dev, "bf16", False)
    on16, _ = _cosine_c_final(dev, "bf16", True)
    d16_on, d16_off = _dist(on16, off32), _dist(off16, off32)
    print("bf16 cosine c_final: |on16 - off32| %.3e  |off16 - off32| %.3e" % (d16_on, d16_off))
    assert d_on_off <= d_off_ref
    assert d16_on <= 2 * d16_off


# ---------------------------------------------------------------- reproducibility
def test_seed_reproducibility(dev):
    for case, moves in (("ce", True), ("cosine", False)):   # hard gate; mean fusion (no draw)
        model, g, pair, noise = _model(case, "fp32", dev)
        batch, _ = _stacked(model, pair, None)
        a = model.engine.embed(batch, seed=11, groups=2)
        b = model.engine.embed(batch, seed=11, groups=2)
        c = model.engine.embed(batch, seed=12, groups=2)
        torch.cuda.synchronize()
        for k in ("c_initial", "c_final"):
            assert torch.equal(a[k], b[k]), (case, k)
            assert torch.equal(a[k], c[k]) != moves, (case, k)


# ---------------------------------------------------------------- no training state
def test_no_training_state(dev):
    from k3m_amd.finetune import _pair_args
    model, g, pair, noise = _model("ce", "fp32", dev)
    eng = model.engine
    eng.fp.grad.zero_()
    model._ctx = None
    model.predict(**_pair_args(pair, True), noise=noise)
    assert model._ctx is None   # predict makes no ctx ...
    sentinel = model._ctx = {"pending": True}
    model.predict(**_pair_args(pair, True), noise=noise)
    assert model._ctx is sentinel   # ... and leaves a pending forward's alone
    model._ctx = None
    model.item_embedding(pair["input_ids_1"], pair["image_feat_1"], pair["image_loc_1"], pair["token_type_ids_1"],
                         pair["attention_mask_1"], pair["image_attention_mask_1"], False, pair["input_ids_pv_1"],
                         pair["token_type_ids_pv_1"], pair["attention_mask_pv_1"], pair["index_p_1"], pair["index_v_1"])
    torch.cuda.synchronize()
    assert model._ctx is None
    assert int(torch.count_nonzero(eng.fp.grad)) == 0
    with pytest.raises(RuntimeError, match="without a preceding forward"):
        model.backward()
    # peak memory above the pre-call level at bs 8: the saving path keeps a dozen row-widths for each of 36 layer
    # bodies, embed none
    batch, _ = _stacked(model, pair, None)
    batch8 = {k: torch.cat([v, v]).contiguous() for k, v in batch.items()}   # 2 pairs x 2 items x 2 = 8 items
    assert batch8["input_ids"].shape[0] == 8

    def peak(fn):
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        keep = fn()
        torch.cuda.synchronize()
        p = torch.cuda.max_memory_allocated() - base
        del keep
        return p
    peak(lambda: eng.embed(batch8, seed=1))   # warm the side allocations (masks, workspaces) of both paths
    p_embed = peak(lambda: eng.embed(batch8, seed=1))
    p_fwd = peak(lambda: eng.forward(batch8, train=False, seed=1))
    print("peak above the pre-call level at bs 8 fp32: embed %.1f MB, forward(train=False) holding ctx %.1f MB"
          % (p_embed / 2 ** 20, p_fwd / 2 ** 20))
    assert p_embed < 0.5 * p_fwd


# ---------------------------------------------------------------- pretraining engine
def test_pretrain_engine_embed(dev):
    from k3m_amd.engine import K3MEngine
    from k3m_amd.weights import param_values
    _MODELS.clear()
    g = load_case("bs2_hard")
    cfg = case_config(g)
    eng = K3MEngine(cfg, dev)
    eng.fp.load(param_values(cfg, int(g["weight_seed"])))
    batch = {k: v.to(dev) for k, v in case_batch(g).items()}
    noise = {k: v.to(dev) for k, v in case_noise(g).items()}
    ref, ctx = eng.forward(batch, train=False, noise=noise, seed=2)
    del ctx
    eng.infer_dedup = False
    got = eng.embed(batch, noise=noise, seed=2)
    for k in ("c_initial", "c_final"):
        assert torch.equal(got[k], ref[k]), k
    # no label field is read; with dedup on the values are the golden's at the engine test's bar
    eng.infer_dedup = True
    bare = {k: v for k, v in batch.items() if "label" not in k and not k.startswith("is_next") and k != "image_target"}
    assert len(bare) < len(batch)
    got = eng.embed(bare, noise=noise, seed=2)
    torch.cuda.synchronize()
    for k in ("c_initial", "c_final"):
        np.testing.assert_allclose(got[k].cpu().numpy(), ref[k].cpu().numpy(), rtol=1e-3, atol=1e-4)


# ---------------------------------------------------------------- prediction file and evaluation
def _parse(field):
    assert field[0] == "[" and field[-1] == "]"
    return np.array([float(x) for x in field[1:-1].split(",")], np.float32)


def test_write_predictions_and_forward_only_evaluate(dev, tmp_path):
    import json
    from k3m_amd.finetune import evaluate, write_predictions
    keys = ["src_item_id", "src_item_emb", "tgt_item_id", "tgt_item_emb", "threshold"]   # finetune.py:1204-1206
    # ce, the reference's layout: the two "embeddings" are the class probabilities
    model, g, pair, noise = _model("ce", "fp32", dev)
    batch = dict(pair, item_ids_1=["a1", "a2"], item_ids_2=["b1", "b2"])
    path = str(tmp_path / "deepAI_result_threshold=0.5.jsonl")
    assert write_predictions(model, [batch], path, 0.5, noise=[noise]) == 2
    rows = [json.loads(l) for l in open(path, encoding="utf-8")]
    assert [list(r) for r in rows] == [keys, keys]
    assert [r["src_item_id"] for r in rows] == ["a1", "a2"] and [r["tgt_item_id"] for r in rows] == ["b1", "b2"]
    assert all(r["threshold"] == 0.5 for r in rows)
    e1 = np.concatenate([_parse(r["src_item_emb"]) for r in rows])
    e2 = np.concatenate([_parse(r["tgt_item_emb"]) for r in rows])
    np.testing.assert_allclose(e1, g["out/e1"], rtol=1e-3, atol=1e-4)
    np.testing.assert_allclose(e2, g["out/e2"], rtol=1e-3, atol=1e-4)
    assert rows[0]["src_item_emb"] == "[%s]" % str(np.float32(e1[0]))   # a scalar field, as str(np.float32)
    # forward-only evaluation (evaluate passes no explicit noise: the gate's draw is the engine's own, so the metrics'
    # shapes and ranges are checked, not values against the golden)
    metrics, probs, labels = evaluate(model, [pair, pair], forward_only=True)
    assert len(metrics) == 9 and probs.shape == (4,) and labels.shape == (4,) and model._ctx is None
    assert all(0.0 <= m["f1"] <= 1.0 for m in metrics) and np.isfinite(probs).all()
    # cosine, output="embedding": c_final of both items, 768 values each
    model, g, pair, noise = _model("cosine", "fp32", dev)
    batch = dict(pair, item_ids_1=[1, 2], item_ids_2=[3, 4])
    path = str(tmp_path / "emb.jsonl")
    assert write_predictions(model, [batch], path, 0.3, output="embedding", noise=[noise]) == 2
    rows = [json.loads(l) for l in open(path, encoding="utf-8")]
    e1 = np.stack([_parse(r["src_item_emb"]) for r in rows])
    e2 = np.stack([_parse(r["tgt_item_emb"]) for r in rows])
    assert e1.shape == e2.shape == (2, 768)
    np.testing.assert_allclose(e1, g["out/e1"], rtol=1e-3, atol=1e-4)
    np.testing.assert_allclose(e2, g["out/e2"], rtol=1e-3, atol=1e-4)
    with pytest.raises(ValueError):
        write_predictions(model, [batch], path, 0.3, output="logits")
