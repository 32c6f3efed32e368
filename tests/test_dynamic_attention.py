"""Dynamic image attention (cfg.dynamic_attention) — host side: the parameter inventory against the reference's
record (tests/golden/make_dynamic_attention_golden.py), the flat layout of the fused dyLinear_q | dyLinear_k gate,
the checkpoint surface, and the numpy restatement of the four kernels (tests/dynattn_ref.py) against float64 finite
differences.  No GPU."""
import json
import os

import numpy as np
import pytest
import torch

import dynattn_ref as R
from golden_util import CFG_PATH, HERE
from test_text_only import _fake_trainer, _tiny


def _inv():
    return json.load(open(os.path.join(HERE, "golden", "param_inventory_dynamic_attention.json")))


def _cfg(task, **kw):
    from k3m_amd.config import finetune_config, pretrain_config
    if task == "pretrain":
        return pretrain_config(CFG_PATH, **kw)
    return finetune_config(CFG_PATH, loss_type=task, **kw)


@pytest.mark.parametrize("task,count", [("pretrain", 1022), ("ce", 1013)])
def test_param_spec_equals_reference_inventory(task, count):
    from k3m_amd.params import param_spec
    inv = _inv()
    spec = param_spec(_cfg(task, dynamic_attention=True))
    assert [(n, list(s)) for n, s in spec] == [(n, list(s)) for n, s in inv[task]]   # names, order, shapes
    assert len(spec) == count
    dy = [(n, s) for n, s in spec if ".dyLinear_" in n]
    assert len(dy) == 24
    names = [n for n, _ in spec]
    for i in range(6):
        p = "encoder.v_layer.%d.attention.self." % i
        j = names.index(p + "value.bias")
        assert names[j + 1:j + 5] == [p + "dyLinear_q.weight", p + "dyLinear_q.bias", p + "dyLinear_k.weight",
                                      p + "dyLinear_k.bias"]
        assert dict(spec)[p + "dyLinear_q.weight"] == (1024, 768) and dict(spec)[p + "dyLinear_k.bias"] == (1024,)


@pytest.mark.parametrize("task", ["pretrain", "ce", "cosine"])
def test_flag_off_inventories_and_layouts_are_unchanged(task):
    """dynamic_attention=False and a config without the attribute give the same spec, offsets, segments and never-grad
    set; the pretraining spec is the committed inventory of the model as it was."""
    from k3m_amd.params import flat_layout, frozen_names, fused_groups, param_spec
    off = _cfg(task, dynamic_attention=False)
    bare = _cfg(task)
    del bare.dynamic_attention
    assert flat_layout(off) == flat_layout(bare) and frozen_names(off) == frozen_names(bare)
    assert fused_groups(off) == fused_groups(bare)
    assert not [n for n, _ in param_spec(off) if "dyLinear" in n]
    if task == "pretrain":
        ref = json.load(open(os.path.join(HERE, "golden", "param_inventory.json")))["params"]
        assert [(k, list(s)) for k, s in param_spec(off)] == [(k, list(s)) for k, s in ref]
    else:
        ref = json.load(open(os.path.join(HERE, "golden", "param_inventory_finetune.json")))[task]
        assert [(k, list(s)) for k, s in param_spec(off)] == [(k, list(s)) for k, s in ref]
    # the flag only adds tensors: every other tensor keeps its place in the order
    on = param_spec(_cfg(task, dynamic_attention=True))
    assert [(n, s) for n, s in on if "dyLinear" not in n] == param_spec(off)


@pytest.mark.parametrize("task", ["pretrain", "ce"])
def test_without_the_image_modality_the_flag_changes_nothing(task):
    from k3m_amd.params import flat_layout, frozen_names, param_spec
    inv = json.load(open(os.path.join(HERE, "golden", "param_inventory_text_only.json")))
    on, off = _cfg(task, use_image=False, dynamic_attention=True), _cfg(task, use_image=False)
    assert [(n, list(s)) for n, s in param_spec(on)] == [(n, list(s)) for n, s in inv[task]]
    assert flat_layout(on) == flat_layout(off) and frozen_names(on) == frozen_names(off)


@pytest.mark.parametrize("task", ["pretrain", "ce"])
def test_flat_layout_fuses_the_gate_and_keeps_qkv(task):
    from k3m_amd.ddp import _block_of
    from k3m_amd.params import flat_layout, frozen_names, is_no_decay, segment_of
    cfg = _cfg(task, dynamic_attention=True)
    spec, off, seg, total, shapes = flat_layout(cfg)
    n = {k: int(np.prod(s)) for k, s in spec}
    for i in range(cfg.v_num_hidden_layers):
        p = "encoder.v_layer.%d.attention.self." % i
        for kind in ("weight", "bias"):
            q, k, v = [p + "%s.%s" % (x, kind) for x in ("query", "key", "value")]
            assert off[k] == off[q] + n[q] and off[v] == off[k] + n[k]            # the fused QKV Lin still holds
            a, b = p + "dyLinear_q." + kind, p + "dyLinear_k." + kind
            assert off[b] == off[a] + n[a] and off[a] % 4 == 0                    # one [2 Hv, H] Lin
            assert segment_of(a, cfg) == ("no_decay" if kind == "bias" else "decay") and is_no_decay(a) == (kind == "bias")
            assert _block_of(a) == ("v", i)                                       # DDP: the v_layer block's range
    assert not [x for x in frozen_names(cfg) if "dyLinear" in x]
    assert len(frozen_names(cfg)) == len(frozen_names(_cfg(task)))


def _tiny_da(task, dyn):
    cfg = _tiny(task, True)
    cfg.dynamic_attention = dyn
    return cfg


@pytest.mark.parametrize("task", ["pretrain", "ce"])
def test_checkpoint_round_trip(task, tmp_path):
    from k3m_amd import checkpoint as C
    from k3m_amd.params import is_no_decay
    cfg = _tiny_da(task, True)
    src = _fake_trainer(cfg, 1, step=5)
    tar, binp = str(tmp_path / "k.tar"), str(tmp_path / "k.bin")
    C.save_checkpoint(src, tar_path=tar, bin_path=binp)
    names = [n for n, _ in src.engine.fp.spec]
    assert len([n for n in names if "dyLinear" in n]) == 4
    sd = torch.load(binp, weights_only=True)
    assert list(sd) == names + ([C.DECODER_KEY] if task == "pretrain" else [])
    ck = torch.load(tar, map_location="cpu", weights_only=True)
    order = [n for n in names if not is_no_decay(n)] + [n for n in names if is_no_decay(n)]
    fz = src.engine.fp.frozen
    assert set(ck["optimizer_state_dict"]["state"]) == {i for i, n in enumerate(order) if n not in fz}
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
    dyn = _fake_trainer(_tiny_da(task, True), 1, step=3)
    plain = _fake_trainer(_tiny_da(task, False), 2, step=0)
    tar_dyn, tar_plain = str(tmp_path / "dyn.tar"), str(tmp_path / "plain.tar")
    C.save_checkpoint(dyn, tar_path=tar_dyn)
    C.save_checkpoint(plain, tar_path=tar_plain)
    for dst, tar, what in ((plain, tar_dyn, "built without dynamic_attention"),
                           (dyn, tar_plain, "built with dynamic_attention=True")):
        dst.engine.fp.grad = torch.zeros_like(dst.engine.fp.data)
        before = dst.engine.fp.data.clone()
        with pytest.raises(ValueError, match=what):
            C.load_checkpoint(dst, tar)
        sd = torch.load(tar, map_location="cpu", weights_only=True)["model_state_dict"]
        assert "dyLinear" in str(pytest.raises(ValueError, C.load_model_state_dict, dst.engine.fp, sd, False).value)
        assert torch.equal(dst.engine.fp.data, before) and dst.global_step in (0, 3)
    # an encoder-only file (no image layers) still loads non-strictly into the model with the gates
    sd = {k: v for k, v in torch.load(tar_plain, map_location="cpu", weights_only=True)["model_state_dict"].items()
          if k.startswith("encoder.layer.")}
    assert "encoder.v_layer.0.attention.self.dyLinear_q.weight" in C.load_model_state_dict(dyn.engine.fp, sd, strict=False)


# ---------------------------------------------------------------- the kernels' formulas
def _problem(seed=0, nseq=2, L=5, Rr=3, H=8):
    """Hv = H; qkv has the V block and four trailing columns of a wider buffer"""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((nseq, L, H))
    mask = np.array([[1, 1, 0, 1, 0], [1, 0, 0, 0, 0]], np.float64)[:nseq, :L]
    W = rng.standard_normal((2 * H, H)) * 0.7
    b = rng.standard_normal(2 * H)
    qkv = rng.standard_normal((nseq, Rr, 3 * H + 4))
    gout = rng.standard_normal(qkv.shape)
    return x, mask, W, b, qkv, gout


def _loss_of_z(z, qkv, gout):
    return float((R.scale_fwd(qkv, z) * gout).sum())


def _loss_of_x(x, mask, W, b, qkv, gout):
    pool, _ = R.pool_fwd(x, mask)
    return _loss_of_z(pool @ W.T + b, qkv, gout)


def _fd(f, a, eps=1e-6):
    g = np.zeros_like(a)
    it = np.nditer(a, flags=["multi_index"])
    for _ in it:
        i = it.multi_index
        hi, lo = a.copy(), a.copy()
        hi[i] += eps
        lo[i] -= eps
        g[i] = (f(hi) - f(lo)) / (2 * eps)
    return g


def test_restatement_matches_finite_differences():
    """nseq 2, L 5, R 3, H 8, float64: dz of scale_bwd from the GATED qkv (the S / g identity), the in-place
    rescaling of dqkv, and dX through the gate GEMM and pool_bwd."""
    x, mask, W, b, qkv, gout = _problem()
    pool, ic = R.pool_fwd(x, mask)
    np.testing.assert_allclose(ic, [1 / 3, 1.0])
    np.testing.assert_allclose(pool[1], x[1, 0])
    z = pool @ W.T + b
    gated = R.scale_fwd(qkv, z)
    assert np.array_equal(gated[:, :, 16:], qkv[:, :, 16:])                       # V and beyond untouched
    dz, dq = R.scale_bwd(gout, gated, z)
    np.testing.assert_allclose(dz, _fd(lambda zz: _loss_of_z(zz, qkv, gout), z), rtol=1e-7, atol=1e-8)
    np.testing.assert_allclose(dq, _fd(lambda qq: _loss_of_z(z, qq, gout), qkv), rtol=1e-7, atol=1e-8)
    dx0 = np.random.default_rng(5).standard_normal(x.shape)                        # pool_bwd accumulates
    dx = R.pool_bwd(dz @ W, mask, ic, dx0)
    np.testing.assert_allclose(dx - dx0, _fd(lambda xx: _loss_of_x(xx, mask, W, b, qkv, gout), x), rtol=1e-6,
                               atol=1e-8)
    assert np.array_equal((dx - dx0)[mask == 0], np.zeros_like(dx)[mask == 0])     # masked tokens get nothing


def test_restatement_empty_sequence_is_zero_not_nan():
    x = np.ones((1, 4, 8))
    pool, ic = R.pool_fwd(x, np.zeros((1, 4)))
    assert np.array_equal(pool, np.zeros((1, 8))) and ic[0] == 0.0
    assert np.array_equal(R.pool_bwd(np.ones((1, 8)), np.zeros((1, 4)), ic, x), x)


def test_engine_builds_the_gate():
    """Host side of the engine: constructing it no longer refuses the flag (the parent asserted), every image layer
    carries a fused [2 Hv, H] gate, no text layer does, and without the image modality nothing changes."""
    from k3m_amd.engine import K3MEngine
    eng = K3MEngine(_tiny_da("pretrain", True), torch.device("cpu"))
    assert eng.dyn_attn and all(op.dyn is not None and tuple(op.dyn.lin.W.shape) == (128, 64) for op in eng.image)
    assert all(op.dyn is None for op in eng.text)
    off = K3MEngine(_tiny_da("pretrain", False), torch.device("cpu"))
    assert not off.dyn_attn and all(op.dyn is None for op in off.image)
    cfg = _tiny("pretrain", False)
    cfg.dynamic_attention = True
    assert not K3MEngine(cfg, torch.device("cpu")).dyn_attn


def test_step_graph_is_ineligible_with_the_flag():
    """StepGraphs.eligible: the same trainer state is eligible without the flag and not with it (the step with
    dynamic attention runs eagerly, as the step without the image modality does)."""
    import types
    from k3m_amd.graph import StepGraphs

    def trainer(dyn_attn):
        eng = types.SimpleNamespace(fp=types.SimpleNamespace(data=types.SimpleNamespace(is_cuda=True)),
                                    use_image=True, dyn_attn=dyn_attn)
        return types.SimpleNamespace(ddp=None, accum_steps=1, micro=0, ADAMW=None, lr_schedule="warmup_linear",
                                     objective=0, engine=eng)
    batch = {"_label_counts": (1, 1, 1)}
    assert StepGraphs(trainer(False)).eligible(batch)
    assert not StepGraphs(trainer(True)).eligible(batch)


def test_surface_class_accepts_the_flag():
    """vilbert_k3m.BertForMultiModalPreTraining_tri_stru takes a config with the flag: its named_parameters() hold
    the gate tensors directly after value.bias, and a state dict without them is refused before any copy."""
    from k3m_amd.vilbert_k3m import BertForMultiModalPreTraining_tri_stru
    model = BertForMultiModalPreTraining_tri_stru(_tiny_da("pretrain", True), device="cpu")
    names = [n for n, _ in model.named_parameters()]
    p = "encoder.v_layer.0.attention.self."
    j = names.index(p + "value.bias")
    assert names[j + 1:j + 5] == [p + "dyLinear_q.weight", p + "dyLinear_q.bias", p + "dyLinear_k.weight",
                                  p + "dyLinear_k.bias"]
    assert model.engine.dyn_attn and set(names) <= set(model.state_dict())
    plain = BertForMultiModalPreTraining_tri_stru(_tiny_da("pretrain", False), device="cpu")
    before = plain.engine.fp.data.clone()
    with pytest.raises(ValueError, match="dynamic_attention"):
        plain.load_state_dict(model.state_dict())
    assert torch.equal(plain.engine.fp.data, before)
