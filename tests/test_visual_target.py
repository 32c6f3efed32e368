"""Masked-region feature regression (visual_target=1) without a GPU: the float64 restatement
(tests/visual_target_ref.py) against the reference's formula and the recorded reference fixture, the configuration
check, the parameter layout, the checkpoint shape check and the synthetic batch."""
import json
import os
import types

import numpy as np
import pytest
import torch

import visual_target_ref as VR
from golden_util import CFG_PATH, HERE, load_case


def _reference_formula(pred, target, label):
    """vilbert_k3m.py:2232-2237 and :2745-2752 as written, in float64 with autograd."""
    crit = torch.nn.MSELoss(reduction="none")
    pred = pred.clone().requires_grad_(True)
    img_loss = crit(pred, target)
    loss = torch.sum(img_loss * (label == 1).unsqueeze(2).float()) / max(
        torch.sum((label == 1).unsqueeze(2).expand_as(img_loss)), 1)
    loss.backward()
    return float(loss.detach()), pred.grad.numpy()


def _random_case(seed=0):
    g = torch.Generator().manual_seed(seed)
    pred = torch.randn((2, 5, 7), generator=g, dtype=torch.float64)
    target = torch.randn((2, 5, 7), generator=g, dtype=torch.float64)
    label = torch.tensor([[1, -1, 1, 0, -1], [-1, -1, 1, 1, 0]])   # 0: a label the loss must not count
    return pred, target, label


def test_restatement_equals_the_reference_formula():
    pred, target, label = _random_case()
    want, want_g = _reference_formula(pred, target, label)
    got, got_g = VR.dense_loss(pred.numpy(), target.numpy(), label.numpy())
    assert want > 0
    np.testing.assert_allclose(got, want, rtol=1e-12)
    np.testing.assert_allclose(got_g, want_g, rtol=1e-12, atol=1e-15)
    trow, sc = VR.compact(label.numpy())
    assert list(trow) == [0, 2, 7, 8] and np.allclose(sc, 0.25)
    assert np.abs(got_g.reshape(10, 7)[[1, 3, 4, 5, 6, 9]]).max() == 0.0


def test_no_masked_region_gives_zero_loss_and_zero_gradient():
    pred, target, label = _random_case(1)
    label = torch.full_like(label, -1)
    want, want_g = _reference_formula(pred, target, label)
    got, got_g = VR.dense_loss(pred.numpy(), target.numpy(), label.numpy())
    assert want == 0.0 and got == 0.0
    assert np.abs(want_g).max() == 0.0 and np.abs(got_g).max() == 0.0


def test_restatement_gradient_agrees_with_central_differences():
    pred, target, label = _random_case(2)
    p, t, lab = pred.numpy(), target.numpy(), label.numpy()
    _, grad = VR.dense_loss(p, t, lab)
    h = 1e-6
    num = np.zeros_like(p)
    for i in np.ndindex(*p.shape):
        hi, lo = p.copy(), p.copy()
        hi[i] += h
        lo[i] -= h
        num[i] = (VR.dense_loss(hi, t, lab)[0] - VR.dense_loss(lo, t, lab)[0]) / (2 * h)
    # the loss is quadratic in pred: central differences are exact up to rounding, ~1e-16 / h = 1e-10
    np.testing.assert_allclose(grad, num, rtol=1e-7, atol=1e-9)


def test_restatement_reproduces_the_recorded_reference_loss():
    g = load_case("vt1_bs2")
    assert int(g["visual_target"]) == 1 and g["in/image_target"].shape == (2, 12, 2048)
    lab = g["in/image_label"]
    assert ((lab == 1).sum(1) >= 1).all() and (lab == 1).sum() >= 3
    assert np.array_equal(g["in/image_target"][lab != 1], g["in/image_feat"][:, 1:][lab != 1])   # unmasked: untouched
    loss, _ = VR.masked_img_loss(g["logit/img_rows"], g["in/image_target"], lab)
    print("restated", loss, "recorded", g["losses"][1])
    np.testing.assert_allclose(loss, g["losses"][1], rtol=1e-6)


def test_validate_config():
    from k3m_amd.config import finetune_config, pretrain_config
    from k3m_amd.engine import K3MEngine, validate_config
    for vt in (0, 1):
        validate_config(pretrain_config(CFG_PATH, visual_target=vt))
        validate_config(finetune_config(CFG_PATH, loss_type="ce", visual_target=vt))
    cfg = pretrain_config(CFG_PATH, visual_target=2)
    with pytest.raises(ValueError, match="visual_target.*num_negative"):
        validate_config(cfg)
    with pytest.raises(ValueError, match="visual_target"):   # before any device work
        K3MEngine(cfg, torch.device("cpu"))
    for bad in (3, -1):
        cfg = pretrain_config(CFG_PATH, visual_target=1)
        cfg.visual_target = bad
        with pytest.raises(ValueError, match="visual_target"):
            validate_config(cfg)


def test_param_layout_equals_reference_inventory():
    from k3m_amd.config import pretrain_config
    from k3m_amd.params import param_spec
    inv = json.load(open(os.path.join(HERE, "golden", "param_inventory_visual_target.json")))["params"]
    spec = param_spec(pretrain_config(CFG_PATH, visual_target=1))
    assert [(n, list(s)) for n, s in spec] == [(n, list(s)) for n, s in inv]
    base = json.load(open(os.path.join(HERE, "golden", "param_inventory.json")))["params"]
    assert [n for n, _ in inv] == [n for n, _ in base]
    differ = [n for (n, s), (_, s0) in zip(inv, base) if s != s0]
    assert differ == ["cls.imagePredictions.decoder.weight", "cls.imagePredictions.decoder.bias"]
    assert dict((n, s) for n, s in inv)["cls.imagePredictions.decoder.weight"] == [2048, 1024]


def _tiny(visual_target):
    """The shrunken model of tests/test_text_only.py, with the two decoder widths kept apart."""
    from k3m_amd.config import pretrain_config
    cfg = pretrain_config(CFG_PATH, visual_target=visual_target)
    cfg.num_hidden_layers, cfg.v_num_hidden_layers = 2, 1
    cfg.v_biattention_id, cfg.t_biattention_id = [0], [1]
    cfg.vocab_size, cfg.hidden_size, cfg.intermediate_size = 97, 64, 128
    cfg.v_hidden_size = cfg.bi_hidden_size = cfg.v_intermediate_size = 64
    cfg.v_feature_size, cfg.max_position_embeddings = 32, 40
    cfg.v_target_size = 17 if visual_target == 0 else 32
    return cfg


def _fake_trainer(cfg, seed, step):
    from k3m_amd.engine import FlatParams
    fp = FlatParams(cfg, torch.device("cpu"))
    g = torch.Generator().manual_seed(seed)
    fp.data.copy_(torch.randn(fp.total, generator=g))
    nopt = fp.segments["frozen"][0]
    t = types.SimpleNamespace(engine=types.SimpleNamespace(fp=fp, step_count=step), global_step=step,
                              m=torch.randn(nopt, generator=g), v=torch.rand(nopt, generator=g),
                              lr=1e-4, warmup=10, t_total=1000, beta1=0.9, beta2=0.98, eps=1e-8, wd=0.01)
    t.current_lr = lambda: t.lr * min(1.0, t.global_step / t.warmup)
    return t


@pytest.mark.parametrize("src_vt,dst_vt", [(0, 1), (1, 0)])
def test_cross_target_state_dict_is_refused_by_shape_and_loads_nothing(src_vt, dst_vt, tmp_path):
    from k3m_amd import checkpoint as C
    src = _fake_trainer(_tiny(src_vt), 1, step=3)
    dst = _fake_trainer(_tiny(dst_vt), 2, step=0)
    dst.engine.fp.grad = torch.zeros_like(dst.engine.fp.data)
    before = dst.engine.fp.data.clone()
    sd = C.model_state_dict(src.engine.fp)
    with pytest.raises(ValueError, match=r"cls\.imagePredictions\.decoder\.weight: shape"):
        C.load_model_state_dict(dst.engine.fp, sd)
    with pytest.raises(ValueError, match=r"cls\.imagePredictions\.decoder\.weight: shape"):
        C.load_model_state_dict(dst.engine.fp, sd, strict=False)
    tar = str(tmp_path / "k.tar")
    C.save_checkpoint(src, tar_path=tar)
    with pytest.raises(ValueError, match=r"cls\.imagePredictions\.decoder\.weight: shape"):
        C.load_checkpoint(dst, tar)
    assert torch.equal(dst.engine.fp.data, before)


def test_synthetic_batch_targets_are_the_region_features():
    from k3m_amd.config import pretrain_config
    from k3m_amd.synthetic import synthetic_batch
    cfg1 = pretrain_config(CFG_PATH, visual_target=1)
    b1 = synthetic_batch(cfg1, 3, "cpu", seed=5, n_boxes=9)
    assert b1["image_target"].shape == (3, 9, 2048) and b1["image_target"].dtype == torch.float32
    assert torch.equal(b1["image_target"], b1["image_feat"][:, 1:])
    assert b1["image_target"].data_ptr() != b1["image_feat"].data_ptr()
    # every other field is drawn as for target 0 up to the target itself
    b0 = synthetic_batch(pretrain_config(CFG_PATH), 3, "cpu", seed=5, n_boxes=9)
    assert b0["image_target"].shape == (3, 9, 1601)
    np.testing.assert_allclose(b0["image_target"].sum(-1).numpy(), 1.0, rtol=1e-5)
    for k in ("input_ids", "lm_label_ids", "input_ids_pv", "image_feat", "image_loc"):
        assert torch.equal(b0[k], b1[k]), k
