"""The model without the image modality (cfg.use_image false) — host side: parameter inventories and never-grad
sets against the reference's records (tests/golden/make_text_only_golden.py), the flat layout of the two-candidate
gate, the refused fusion modes and the checkpoint surface.  No GPU."""
import json
import os
import types

import numpy as np
import pytest
import torch

from golden_util import CFG_PATH, HERE, load_case, load_ft_case


def _inv():
    return json.load(open(os.path.join(HERE, "golden", "param_inventory_text_only.json")))


def _cfg(task, use_image=False, **kw):
    from k3m_amd.config import finetune_config, pretrain_config
    if task == "pretrain":
        return pretrain_config(CFG_PATH, use_image=use_image, **kw)
    return finetune_config(CFG_PATH, loss_type=task, use_image=use_image, **kw)


def test_pretrain_config_default_keeps_the_image_modality():
    from k3m_amd.config import pretrain_config
    assert pretrain_config(CFG_PATH).use_image is True
    assert pretrain_config(CFG_PATH, use_image=False).use_image is False


@pytest.mark.parametrize("task,count,keys", [("pretrain", 444, 445), ("ce", 441, 441), ("cosine", 437, 437)])
def test_param_spec_equals_reference_inventory(task, count, keys):
    from k3m_amd.params import param_spec
    inv = _inv()
    spec = param_spec(_cfg(task))
    assert [(n, list(s)) for n, s in spec] == [(n, list(s)) for n, s in inv[task]]   # names, order, shapes
    assert len(spec) == count and len(inv[task + "_state_dict_keys"]) == keys
    names = [n for n, _ in spec]
    assert not [n for n in names if n.startswith(("v_embeddings", "v_pooler", "encoder.v_layer", "encoder.c_layer.",
                                                   "encoder.c_layer_pv_v", "cls.imagePredictions", "map_"))
                or n.split(".")[0].endswith("_v")]
    assert dict(spec)["score_self_t.weight"] == (768, 1536)


@pytest.mark.parametrize("task,case,count", [("pretrain", "to_bs2", 36), ("pretrain", "to_bs3_zero_triple", 36),
                                             ("ce", "to_ce", 34), ("cosine", "to_cosine", 34)])
def test_frozen_names_equal_the_references_never_grad_set(task, case, count):
    from k3m_amd.params import frozen_names
    g = load_case(case) if task == "pretrain" else load_ft_case(case)
    never = {str(n) for n, v in zip(g["grad_norm_names"], g["grad_norms"]) if np.isnan(v)}
    got = frozen_names(_cfg(task))
    assert got == never and len(got) == count
    assert {"score_cross1_t.weight", "score_cross1_t.bias", "score_cross1_pv.weight", "score_cross1_pv.bias"} <= got


@pytest.mark.parametrize("task", ["pretrain", "ce"])
def test_flat_layout_of_the_two_candidate_gate(task):
    from k3m_amd.params import flat_layout, frozen_names
    cfg = _cfg(task)
    spec, off, seg, total, shapes = flat_layout(cfg)
    n = {k: int(np.prod(s)) for k, s in spec}
    for m in ("t", "pv"):
        for kind in ("weight", "bias"):
            a, b = "score_self_%s.%s" % (m, kind), "score_cross2_%s.%s" % (m, kind)
            assert off[b] == off[a] + n[a], (a, b)       # one [2H, 2H] weight / [2H] bias view
    lo, hi = seg["frozen"]
    fz = frozen_names(cfg)
    for name, _ in spec:
        inside = lo <= off[name] and off[name] + n[name] <= hi
        assert inside == (name in fz), name
    # optimizer runs and DDP buckets read the same set: nothing of it below the frozen segment
    from k3m_amd.trainer import block_runs, optimizer_runs
    fp = types.SimpleNamespace(spec=spec, offsets=off, frozen=fz)
    assert max(a + k for a, k, _, _ in optimizer_runs(fp)) <= lo + 4
    assert max(a + k for runs in block_runs(fp).values() for a, k, _, _ in runs) <= lo + 4


def test_default_layout_and_frozen_set_are_unchanged():
    """use_image=True (the default everywhere): the 86 never-grad tensors and the three-scorer groups as before."""
    from k3m_amd.config import pretrain_config
    from k3m_amd.params import flat_layout, frozen_names, is_frozen, param_spec
    cfg = pretrain_config(CFG_PATH)
    spec, off, seg, total, shapes = flat_layout(cfg)
    assert spec == param_spec(cfg) and len(spec) == 998
    fz = frozen_names(cfg)
    assert fz == {n for n, _ in spec if is_frozen(n)} and len(fz) == 86
    assert "score_cross1_t.weight" not in fz
    n = {k: int(np.prod(s)) for k, s in spec}
    for m in ("v", "t", "pv"):
        a, b, c = ["score_%s_%s.weight" % (k, m) for k in ("self", "cross1", "cross2")]
        assert off[b] == off[a] + n[a] and off[c] == off[b] + n[b]
    ref = json.load(open(os.path.join(HERE, "golden", "param_inventory.json")))["params"]
    assert [(k, list(s)) for k, s in spec] == [(k, list(s)) for k, s in ref]


@pytest.mark.parametrize("mode", [0, 2, 3])
@pytest.mark.parametrize("task", ["pretrain", "ce"])
def test_engine_refuses_the_undefined_fusion_modes(task, mode):
    """Raised before any device work (no GPU and no library needed)."""
    from k3m_amd.engine import K3MEngine, validate_config
    cfg = _cfg(task, if_pre_sampling=mode)
    with pytest.raises(ValueError, match="hard gate"):
        validate_config(cfg)
    with pytest.raises(ValueError, match="hard gate"):
        K3MEngine(cfg, torch.device("cpu"))
    validate_config(_cfg(task, if_pre_sampling=1))
    validate_config(_cfg(task, use_image=True, if_pre_sampling=mode))


# ---------------------------------------------------------------- checkpoints
def _tiny(task, use_image):
    cfg = _cfg(task, use_image=use_image)
    cfg.num_hidden_layers, cfg.v_num_hidden_layers = 2, 1
    cfg.v_biattention_id, cfg.t_biattention_id = [0], [1]
    cfg.vocab_size, cfg.hidden_size, cfg.intermediate_size = 97, 64, 128
    cfg.v_hidden_size = cfg.bi_hidden_size = cfg.v_intermediate_size = 64
    cfg.v_feature_size, cfg.v_target_size, cfg.max_position_embeddings = 32, 17, 40
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


@pytest.mark.parametrize("task", ["pretrain", "ce"])
def test_checkpoint_round_trip_and_key_sets(task, tmp_path):
    from k3m_amd import checkpoint as C
    from k3m_amd.params import is_no_decay, param_spec
    inv = _inv()
    full = [n for n, _ in param_spec(_cfg(task))] + ([C.DECODER_KEY] if task == "pretrain" else [])
    assert sorted(full) == sorted(inv[task + "_state_dict_keys"]) and len(full) == (445 if task == "pretrain" else 441)
    cfg = _tiny(task, False)
    src = _fake_trainer(cfg, 1, step=5)
    tar, binp = str(tmp_path / "k.tar"), str(tmp_path / "k.bin")
    C.save_checkpoint(src, tar_path=tar, bin_path=binp)
    names = [n for n, _ in src.engine.fp.spec]
    sd = torch.load(binp, weights_only=True)
    assert list(sd) == names + ([C.DECODER_KEY] if task == "pretrain" else [])
    ck = torch.load(tar, map_location="cpu", weights_only=True)
    order = [n for n in names if not is_no_decay(n)] + [n for n in names if is_no_decay(n)]
    fz = src.engine.fp.frozen
    assert set(ck["optimizer_state_dict"]["state"]) == {i for i, n in enumerate(order) if n not in fz}
    assert "score_cross1_t.weight" in fz
    dst = _fake_trainer(cfg, 2, step=0)
    dst.engine.fp.grad = torch.zeros_like(dst.engine.fp.data)
    assert C.load_checkpoint(dst, tar) == 5
    for n in names:
        assert torch.equal(src.engine.fp.p[n], dst.engine.fp.p[n]), n
        if n not in fz:
            o, k = src.engine.fp.offsets[n], src.engine.fp.p[n].numel()
            assert torch.equal(src.m[o:o + k], dst.m[o:o + k]) and torch.equal(src.v[o:o + k], dst.v[o:o + k]), n


@pytest.mark.parametrize("task", ["pretrain", "ce"])
def test_cross_loading_is_refused_and_loads_nothing(task, tmp_path):
    from k3m_amd import checkpoint as C
    tri = _fake_trainer(_tiny(task, True), 1, step=3)
    txt = _fake_trainer(_tiny(task, False), 2, step=0)
    tar_tri, tar_txt = str(tmp_path / "tri.tar"), str(tmp_path / "txt.tar")
    C.save_checkpoint(tri, tar_path=tar_tri)
    C.save_checkpoint(txt, tar_path=tar_txt)
    for dst, tar, other in ((txt, tar_tri, "tri-modal"), (tri, tar_txt, "without the image modality")):
        dst.engine.fp.grad = torch.zeros_like(dst.engine.fp.data)
        before = dst.engine.fp.data.clone()
        with pytest.raises(ValueError, match=other):
            C.load_checkpoint(dst, tar)
        sd = torch.load(tar, map_location="cpu", weights_only=True)["model_state_dict"]
        with pytest.raises(ValueError, match=other):
            C.load_model_state_dict(dst.engine.fp, sd, strict=False)   # the drivers' non-strict load as well
        assert torch.equal(dst.engine.fp.data, before) and dst.global_step in (0, 3)


@pytest.mark.parametrize("use_image", [True, False])
def test_wrong_shape_is_refused_before_the_first_copy(use_image):
    """A file of the right modality with one wrongly shaped tensor (the last one, so that a check made while
    copying would already have overwritten the others) loads nothing."""
    from k3m_amd import checkpoint as C
    fp = _fake_trainer(_tiny("pretrain", use_image), 1, step=0).engine.fp
    sd = {n: torch.full_like(fp.p[n], 3.0) for n, _ in fp.spec}
    last = fp.spec[-1][0]
    sd[last] = torch.full((5,) + tuple(fp.shapes[last]), 3.0)
    before = fp.data.clone()
    with pytest.raises(ValueError, match=last.replace(".", r"\.") + ": shape"):
        C.load_model_state_dict(fp, sd)
    assert torch.equal(fp.data, before)


def test_pair_arguments_only_the_image_ones_may_be_left_out():
    """ItemAlignmentTrainer.step / finetune.evaluate take the forward's arguments out of a pair dict: a missing
    key is a KeyError, as it always was, except the image arguments of a model without the image modality."""
    from k3m_amd.finetune import ARG_NAMES, _pair_args
    full = {k: i for i, k in enumerate(ARG_NAMES)}
    text = {k: v for k, v in full.items() if not k.startswith("image_")}
    assert len(full) - len(text) == 6
    assert _pair_args(full, True) == full
    assert _pair_args(text, False) == text and _pair_args(full, False) == full
    with pytest.raises(KeyError, match="image_feat_1"):
        _pair_args(text, True)
    for use_image in (True, False):
        with pytest.raises(KeyError, match="index_v_2"):
            _pair_args({k: v for k, v in (full if use_image else text).items() if k != "index_v_2"}, use_image)
