"""Frozen lower text layers (fixed_t_layer) end to end on the GPU: parity with the fixture recorded from
the reference with ``fixed_t_layer = 6`` (tests/golden/make_fixed_t_layer_golden.py), the cut against the uncut step,
the K3M_FROZEN_NOSAVE knob, memory, --freeze on top of the cut, item alignment, the model without the image modality,
the train.py driver and the hipGraph step.  Bars: those of tests/test_gpu_parity.py."""
import json
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest
import torch

from golden_util import CFG_PATH, HERE, REPO, load_case, case_batch, case_noise, ft_pair, load_ft_case

pytestmark = pytest.mark.gpu
CASE = "ftl6_bs2"
FIXED = 6
LOSS_KEYS = ("masked_lm_loss", "masked_img_loss", "masked_lm_loss_pv", "loss_lpm", "next_sentence_loss", "loss")
INVENTORY = json.load(open(os.path.join(HERE, "golden", "none_grad_fixed_t_layer.json")))


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda")


@pytest.fixture()
def deterministic():
    from k3m_amd import ops
    old = ops.DETERMINISTIC
    ops.set_deterministic(True)
    yield
    ops.set_deterministic(old)


_VALUES = {}


def _values(cfg, seed):
    """param_values(cfg, seed), generated once per model and seed (the values do not depend on fixed_t_layer)."""
    from k3m_amd.weights import param_values
    key = (seed, getattr(cfg, "use_image", True), getattr(cfg, "task", "pretrain"),
           bool(getattr(cfg, "dynamic_attention", False)))
    if key not in _VALUES:
        _VALUES[key] = param_values(cfg, seed)
    return _VALUES[key]


def _config(fixed=FIXED, **kw):
    from k3m_amd.config import pretrain_config
    return pretrain_config(CFG_PATH, if_pre_sampling=1, fixed_t_layer=fixed, **kw)


def _golden_step(dev, dtype, fixed=FIXED):
    from k3m_amd.engine import K3MEngine
    g = load_case(CASE)
    assert int(g["fixed_t_layer"]) == FIXED and int(g["mode"]) == 1
    cfg = _config(fixed)
    eng = K3MEngine(cfg, dev, dtype=dtype)
    eng.fp.load(_values(cfg, int(g["weight_seed"])))
    batch = {k: v.to(dev) for k, v in case_batch(g).items()}
    noise = {k: v.to(dev) for k, v in case_noise(g).items()}
    out, ctx = eng.forward(batch, train=False, noise=noise, ent_neg=torch.from_numpy(g["ent_neg"]),
                           val_neg=torch.from_numpy(g["val_neg"]))
    assert not any(kind == "t" and i < fixed for kind, i, _ in ctx["enc"])   # nothing of the frozen layers is kept
    eng.backward(ctx)
    torch.cuda.synchronize()
    return g, eng, out, np.array([float(out[k]) for k in LOSS_KEYS])


def test_engine_matches_reference_golden(dev):
    g, eng, out, got = _golden_step(dev, "fp32")
    print("losses", got, g["losses"])
    np.testing.assert_allclose(got, g["losses"], rtol=1e-3, atol=1e-4)
    np.testing.assert_allclose(out["c_initial"].cpu().numpy(), g["c_initial"], rtol=1e-3, atol=1e-4)
    np.testing.assert_allclose(out["c_final"].cpu().numpy(), g["c_final"], rtol=1e-3, atol=1e-4)
    G = eng.fp.g
    for k in g:
        if k.startswith("grad_full/") or k.startswith("grad_slice/"):
            n = k.split("/", 1)[1]
            gr = G[n]
            if k.startswith("grad_slice/"):
                gr = gr[:4] if gr.dim() == 2 else gr[:256]
            ref = g[k]
            err = np.abs(gr.cpu().numpy() - ref).max()
            print("grad", n, "err %.3g of max %.3g" % (err, np.abs(ref).max()))
            assert err <= 5e-3 * np.abs(ref).max() + 1e-6, (n, err, np.abs(ref).max())
    never = 0
    for n, ref in zip(list(g["grad_norm_names"]), g["grad_norms"]):
        gn = float(G[n].double().norm())
        if np.isnan(ref):
            never += 1
            assert gn == 0.0, n
            assert str(n) in eng.fp.frozen, n
        else:
            assert str(n) not in eng.fp.frozen, n
            assert abs(gn - ref) <= 5e-3 * ref + 1e-6, (n, gn, ref)
    assert never == len(INVENTORY["pretrain_mode1"]) == 182
    # the fixture is not blind to the cut: the uncut engine's position-embedding gradient misses the bar
    _, eng0, _, got0 = _golden_step(dev, "fp32", fixed=0)
    np.testing.assert_allclose(got0, g["losses"], rtol=1e-3, atol=1e-4)
    ref = g["grad_slice/embeddings.position_embeddings.weight"]
    err0 = np.abs(eng0.fp.g["embeddings.position_embeddings.weight"][:4].cpu().numpy() - ref).max()
    assert err0 > 5e-3 * np.abs(ref).max() + 1e-6


def test_bf16_engine_close_to_reference_golden(dev):
    from test_gpu_parity import BF16_LOSS_RTOL, BF16_GRAD_COS, BF16_GRAD_NORM_RTOL, BF16_GLOBAL_COS
    g, eng, out, got = _golden_step(dev, "bf16")
    rel = np.abs(got - g["losses"]) / np.maximum(np.abs(g["losses"]), 1e-3)
    print("bf16 loss rel err", rel)
    assert (rel <= BF16_LOSS_RTOL).all(), (got, g["losses"])
    G = eng.fp.g
    bad = []
    dot = na = nb2 = 0.0
    for k in g:
        if k.startswith("grad_full/"):
            n = k.split("/", 1)[1]
            a = G[n].double().cpu().numpy().ravel()
            b = g[k].astype(np.float64).ravel()
            nb = np.linalg.norm(b)
            if nb < 1e-6:
                assert n in eng.fp.frozen or np.linalg.norm(a) < 1e-3, n
                continue
            cos = float(a @ b / (np.linalg.norm(a) * nb + 1e-30))
            nr = abs(np.linalg.norm(a) - nb) / nb
            dot, na, nb2 = dot + float(a @ b), na + float(a @ a), nb2 + float(b @ b)
            print("bf16 grad", n, "cos %.5f norm rel %.4f" % (cos, nr))
            if not (cos >= BF16_GRAD_COS and nr <= BF16_GRAD_NORM_RTOL):
                bad.append((n, cos, nr))
    assert not bad, bad
    assert dot / np.sqrt(na * nb2) >= BF16_GLOBAL_COS
    for n, ref in zip(list(g["grad_norm_names"]), g["grad_norms"]):
        if np.isnan(ref):
            assert float(G[n].abs().max()) == 0.0, n


def test_trainer_step_leaves_never_grad_tensors_alone(dev):
    """After a Trainer.step on the parity case: the never-grad tensors have an all-zero gradient, unchanged values and
    no optimizer state (the moment buffers end before the frozen segment); the others moved."""
    from k3m_amd.trainer import Trainer
    g = load_case(CASE)
    tr = Trainer(_config(), dev, lr=1e-3, warmup_steps=0, total_steps=20, seed=9)
    tr.graph = False
    fp = tr.engine.fp
    assert fp.frozen == set(INVENTORY["pretrain_mode1"])
    batch = {k: v.to(dev) for k, v in case_batch(g).items()}
    start = fp.data.clone()
    out = tr.step(batch)
    torch.cuda.synchronize()
    assert np.isfinite(float(out["loss"]))
    f0, f1 = fp.segments["frozen"]
    assert all(f0 <= fp.offsets[n] < f1 for n in fp.frozen)
    assert tr.m.numel() <= f0 + 4 and tr.v.numel() <= f0 + 4
    assert torch.equal(fp.data[f0:f1], start[f0:f1])
    assert float(fp.grad[f0:f1].abs().max()) == 0.0
    for n in ("encoder.layer.6.attention.self.query.weight", "embeddings.position_embeddings.weight",
              "embeddings.LayerNorm.bias", "embeddings.word_embeddings.weight", "encoder.layer.11.output.dense.bias"):
        o = fp.offsets[n]
        assert not torch.equal(fp.p[n].reshape(-1), start[o:o + fp.p[n].numel()]), n
    tr.finish()


def _train_step(dev, dtype, fixed, seed=5, nosave_env=None, monkeypatch=None, cfg_kw=None, B=2):
    from k3m_amd.engine import K3MEngine, label_counts
    from k3m_amd.synthetic import synthetic_batch
    if monkeypatch is not None and nosave_env is not None:
        monkeypatch.setenv("K3M_FROZEN_NOSAVE", nosave_env)
    cfg = _config(fixed, **(cfg_kw or {}))
    eng = K3MEngine(cfg, dev, dtype=dtype, seed=77)
    eng.fp.load(_values(cfg, 4321))
    batch = synthetic_batch(cfg, B, dev, seed=3)
    batch["_label_counts"] = label_counts(batch)
    out, ctx = eng.forward(batch, train=True, seed=seed)
    assert eng.p_h > 0 and eng.p_a > 0   # dropout is on
    eng.backward(ctx)
    torch.cuda.synchronize()
    return eng, out


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_cut_changes_no_forward_value_and_no_gradient_above_it(dev, dtype, deterministic, monkeypatch):
    """Train mode, dropout on, same weights / batch / seed: the losses and c_final of fixed_t_layer = 6 are torch.equal
    to those of fixed_t_layer = 0, and so is the gradient of every tensor above the cut: the same launches on the same
    inputs.  The text embeddings are not above it (they lose the gradient that came down through the layers) and
    differ; the layers below it have none.  K3M_FROZEN_NOSAVE=0 (the saving kernels, the backward still skipped) gives
    the bits of the default."""
    e0, o0 = _train_step(dev, dtype, 0)
    e6, o6 = _train_step(dev, dtype, FIXED)
    assert e6.frozen_nosave
    for k in LOSS_KEYS + ("c_final", "c_initial"):
        assert torch.equal(o0[k], o6[k]), k
    below = e6.cut_frozen
    assert len(below) == 16 * FIXED
    same = differ = 0
    for n, _ in e6.fp.spec:
        a, b = e0.fp.g[n], e6.fp.g[n]
        if n in below:
            assert float(b.abs().max()) == 0.0 and float(a.abs().max()) > 0.0, n
        elif n.startswith("embeddings."):
            differ += int(not torch.equal(a, b))
        else:
            assert torch.equal(a, b), n
            same += 1
    assert differ == 5 and same == len(e6.fp.spec) - len(below) - 5
    es, os_ = _train_step(dev, dtype, FIXED, nosave_env="0", monkeypatch=monkeypatch)
    assert not es.frozen_nosave
    for k in LOSS_KEYS + ("c_final",):
        assert torch.equal(os_[k], o6[k]), k
    assert torch.equal(es.fp.grad, e6.fp.grad)


def test_frozen_step_peak_memory(dev):
    """The peak of the frozen step lies below the unfrozen step's by at least the frozen layers' GELU pre-activation
    buffers, fixed_t_layer x M x intermediate_size x itemsize (M: the rows of the wide text buffer)."""
    from k3m_amd.engine import K3MEngine, label_counts
    from k3m_amd.synthetic import synthetic_batch
    B = 2
    peaks = {}
    for fixed in (0, FIXED):
        cfg = _config(fixed)
        eng = K3MEngine(cfg, dev)
        eng.fp.load(_values(cfg, 4321))
        batch = synthetic_batch(cfg, B, dev, seed=3)
        batch["_label_counts"] = label_counts(batch)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats(dev)
        base = torch.cuda.memory_allocated(dev)
        out, ctx = eng.forward(batch, train=True, seed=1)
        eng.backward(ctx)
        torch.cuda.synchronize()
        peaks[fixed] = torch.cuda.max_memory_allocated(dev) - base
        M = 2 * B * (batch["input_ids"].shape[1] + batch["input_ids_pv"].shape[1])
        del out, ctx, eng, batch
    need = FIXED * M * cfg.intermediate_size * 4
    print("peak bytes above the parameters: unfrozen %d, frozen %d, difference %d, pre-activations %d"
          % (peaks[0], peaks[FIXED], peaks[0] - peaks[FIXED], need))
    assert peaks[0] - peaks[FIXED] >= need


def test_freeze_on_top_of_the_cut(dev):
    """--freeze 8 semantics (frozen_names: the embeddings and text layers 0..8) plus fixed_t_layer = 6: layers 6..8
    pass the gradient down (layer 6 gets one, and the layers above the list are unaffected by it) but are not updated;
    what the reference leaves without a gradient in that configuration stays as it was."""
    from k3m_amd.engine import K3MEngine
    from k3m_amd.trainer import Trainer
    g = load_case(CASE)
    freeze = INVENTORY["freeze8_names"]
    assert len(freeze) == 149 and "encoder.layer.8.output.dense.weight" in freeze
    cfg = _config()
    batch = {k: v.to(dev) for k, v in case_batch(g).items()}
    eng = K3MEngine(cfg, dev)
    eng.fp.load(_values(cfg, int(g["weight_seed"])))
    out, ctx = eng.forward(batch, train=False)
    eng.backward(ctx)
    for n in ("encoder.layer.6.attention.self.query.weight", "encoder.layer.8.output.dense.weight"):
        assert float(eng.fp.g[n].abs().max()) > 0.0, n   # computed on the way down
    del eng, out, ctx
    tr = Trainer(cfg, dev, lr=1e-3, warmup_steps=0, total_steps=20, seed=9, frozen_names=freeze)
    tr.graph = False
    fp = tr.engine.fp
    start = {n: fp.p[n].clone() for n, _ in fp.spec}
    tr.step(batch)
    torch.cuda.synchronize()
    none_grad = set(INVENTORY["pretrain_mode1_freeze8"])
    assert none_grad == set(freeze) | fp.frozen
    for n, _ in fp.spec:
        if n in none_grad:
            assert torch.equal(fp.p[n], start[n]), n
            assert float(fp.g[n].abs().max()) == 0.0, n
    for n in ("encoder.layer.9.attention.self.query.weight", "encoder.layer.9.output.dense.bias",
              "encoder.c_layer_pv_t.0.biattention.query2.weight", "struc_w1.weight"):
        assert not torch.equal(fp.p[n], start[n]), n
    tr.finish()


def _moved(fp, start):
    return {n for n, _ in fp.spec if not torch.equal(fp.p[n], start[n])}


def _check_moved(fp, start, inventory, extra):
    """No tensor of the recorded inventory changes; every other decayed weight does (AdamW moves a tensor that has a
    gradient), and so do the named no-decay tensors."""
    from k3m_amd.params import is_no_decay
    moved = _moved(fp, start)
    assert fp.frozen == set(inventory)
    assert not (moved & set(inventory)), sorted(moved & set(inventory))[:5]
    still = [n for n, _ in fp.spec if n not in inventory and n not in moved and not is_no_decay(n)]
    assert not still, still[:5]
    for n in extra:
        assert n in moved, n


def test_item_alignment_step(dev):
    from k3m_amd.config import finetune_config
    from k3m_amd.finetune import ItemAlignmentTrainer
    g = load_ft_case("ce")
    cfg = finetune_config(CFG_PATH, loss_type="ce", if_pre_sampling=1, fixed_t_layer=FIXED)
    tr = ItemAlignmentTrainer(cfg, dev, lr=1e-3, warmup_steps=0, total_steps=10, seed=19)
    fp = tr.engine.fp
    start = {n: fp.p[n].clone() for n, _ in fp.spec}
    pair = {k: v.to(dev) for k, v in ft_pair(g).items()}
    loss = float(tr.step(pair)["loss"])
    torch.cuda.synchronize()
    assert np.isfinite(loss)
    _check_moved(fp, start, INVENTORY["item_alignment"],
                 ("embeddings.LayerNorm.bias", "encoder.layer.6.output.dense.bias", "classifier.out_proj.bias"))


def test_text_only_step(dev):
    from k3m_amd.engine import label_counts
    from k3m_amd.synthetic import synthetic_batch
    from k3m_amd.trainer import Trainer
    cfg = _config(use_image=False)
    batch = synthetic_batch(cfg, 2, dev, seed=31, n_triples=6)
    for k in ("image_feat", "image_loc", "image_target", "image_label", "image_mask"):
        batch.pop(k, None)
    batch["_label_counts"] = label_counts(batch)
    tr = Trainer(cfg, dev, lr=1e-3, warmup_steps=0, total_steps=10, seed=17)
    tr.graph = False
    fp = tr.engine.fp
    start = {n: fp.p[n].clone() for n, _ in fp.spec}
    loss = float(tr.step(batch)["loss"])
    torch.cuda.synchronize()
    assert np.isfinite(loss)
    _check_moved(fp, start, INVENTORY["pretrain_text_only"],
                 ("embeddings.LayerNorm.bias", "encoder.layer.6.output.dense.bias", "cls.predictions.bias"))
    tr.finish()


def test_interactive_only_fusion_leaves_the_text_embeddings_alone(dev):
    """if_pre_sampling = 3 has no individual candidate: below the cut nothing reaches the text embeddings but the tied
    MLM decoder's gradient of the word embeddings (the recorded pretrain_mode3 inventory)."""
    from k3m_amd.engine import K3MEngine, label_counts
    from k3m_amd.synthetic import synthetic_batch
    from k3m_amd.config import pretrain_config
    cfg = pretrain_config(CFG_PATH, if_pre_sampling=3, fixed_t_layer=FIXED)
    eng = K3MEngine(cfg, dev)
    assert eng.fp.frozen == set(INVENTORY["pretrain_mode3"])
    eng.fp.load(_values(cfg, 4321))
    batch = synthetic_batch(cfg, 2, dev, seed=3)
    batch["_label_counts"] = label_counts(batch)
    out, ctx = eng.forward(batch, train=True, seed=2)
    eng.backward(ctx)
    torch.cuda.synchronize()
    for n in eng.fp.frozen:
        assert float(eng.fp.g[n].abs().max()) == 0.0, n
    assert float(eng.fp.g["embeddings.word_embeddings.weight"].abs().max()) > 0.0
    assert float(eng.fp.g["encoder.layer.6.output.dense.weight"].abs().max()) > 0.0


def test_drop_in_module_reports_no_gradient_below_the_cut(dev):
    from vilbert_k3m.vilbert_k3m import BertForMultiModalPreTraining_tri_stru
    g = load_case(CASE)
    cfg = _config()
    model = BertForMultiModalPreTraining_tri_stru(cfg, device=dev)
    assert not model.load_state_dict({k: torch.from_numpy(v) for k, v in _values(cfg, int(g["weight_seed"])).items()})
    model.eval()
    tb = {k: v.to(dev) for k, v in case_batch(g).items()}
    noise = {k: v.to(dev) for k, v in case_noise(g).items()}
    outs = model(tb["input_ids"], tb["image_feat"], tb["image_loc"], tb["segment_ids"], tb["input_mask"],
                 tb["image_mask"], tb["lm_label_ids"], tb["image_label"], tb["image_target"], tb["is_next"],
                 input_ids_pv=tb["input_ids_pv"], token_type_ids_pv=tb["segment_ids_pv"],
                 attention_mask_pv=tb["input_mask_pv"], masked_lm_labels_pv=tb["lm_label_ids_pv"],
                 next_sentence_label_pv_v=tb["is_next_pv_v"], next_sentence_label_pv_t=tb["is_next_pv_t"],
                 index_p=tb["index_p"], index_v=tb["index_v"], device=dev, gumbel_noise=noise,
                 ent_neg=torch.from_numpy(g["ent_neg"]), val_neg=torch.from_numpy(g["val_neg"]))
    (outs[0] + outs[1] + outs[3] + outs[9]).backward()
    named = dict(model.named_parameters())
    for n, ref in zip(list(g["grad_norm_names"]), g["grad_norms"]):
        n = str(n)
        if n.startswith("encoder.layer.") and int(n.split(".")[2]) < FIXED:
            assert np.isnan(ref) and named[n].grad is None, n
        elif not np.isnan(ref):
            assert named[n].grad is not None, n
            assert abs(float(named[n].grad.double().norm()) - ref) <= 5e-3 * ref + 1e-6, n


def test_train_py_freeze_above_the_first_coattention_block(dev, tmp_path):
    """train.py --freeze 8 (> t_biattention_id[0] = 6) sets config.fixed_t_layer = 6 as the reference driver does and
    runs two steps on the parity case; the text layers below the cut keep their values, layer 6 moves."""
    g = load_case(CASE)
    out = tmp_path / "out"
    out.mkdir()
    shutil.copy(CFG_PATH, out / "bert_base_6layer_6conect.json")
    vals = _values(_config(), int(g["weight_seed"]))
    torch.save({k: torch.from_numpy(v) for k, v in vals.items()}, str(tmp_path / "w.bin"))
    log = tmp_path / "loss.jsonl"
    r = subprocess.run([sys.executable, os.path.join(REPO, "train.py"), "--data_dir", str(tmp_path), "--output_dir",
                        str(out), "--file_name", "unused", "--do_train", "--with_coattention", "--train_batch_size", "2",
                        "--num_train_epochs", "1", "--if_pre_sampling", "1", "--freeze", "8", "--file_state_dict",
                        str(tmp_path / "w.bin"), "--k3m_parity_case",
                        os.path.join(HERE, "golden", "golden_%s.npz" % CASE), "--k3m_max_steps", "2",
                        "--k3m_loss_log", str(log)], cwd=str(tmp_path), capture_output=True, text=True, timeout=400)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    rows = [json.loads(l) for l in log.read_text().splitlines()]
    assert len(rows) == 2
    got = np.array([rows[0][k] for k in ("masked_lm_loss", "masked_img_loss", "masked_lm_loss_pv", "loss_lpm",
                                         "next_sentence_loss", "loss")])
    np.testing.assert_allclose(got, g["losses"], rtol=1e-3, atol=1e-4)   # (lr = 0 on the first step)
    sd = torch.load(str(out / "k3m_bert-base-uncased_12l_12h" / "K3M_struc_presample-1_epoch-0.bin"),
                    map_location="cpu", weights_only=True)
    for n in ("encoder.layer.0.attention.self.query.weight", "encoder.layer.5.output.LayerNorm.bias"):
        assert torch.equal(sd[n], torch.from_numpy(vals[n])), n
    for n in ("encoder.layer.6.attention.self.query.weight", "embeddings.position_embeddings.weight"):
        assert not torch.equal(sd[n], torch.from_numpy(vals[n])), n


def test_graph_step_captures_the_frozen_step(dev):
    """a frozen step is captured like any other (the forward-only launches and the shorter backward
    are ordinary graph nodes).  The body of test_gpu_graph.test_graph_step_matches_eager at fixed_t_layer = 6: fp32,
    B = 2, three steps (one capture, two replays), the same bars; the frozen segment never moves."""
    from k3m_amd.engine import label_counts
    from k3m_amd.synthetic import synthetic_batch
    from k3m_amd.trainer import Trainer
    cfg = _config()
    batch = synthetic_batch(cfg, 2, dev, seed=23)
    batch["_label_counts"] = label_counts(batch)
    lr = 1e-3
    ta = Trainer(cfg, dev, lr=lr, warmup_steps=0, total_steps=20, seed=9)
    tb = Trainer(cfg, dev, lr=lr, warmup_steps=0, total_steps=20, seed=9)
    ta.graph, tb.graph = False, True
    f0, f1 = tb.engine.fp.segments["frozen"]
    frozen0 = tb.engine.fp.data[f0:f1].clone()
    for k in range(3):
        fa, fb = ta.engine.fp, tb.engine.fp
        fb.data.copy_(fa.data)
        tb.m.copy_(ta.m)
        tb.v.copy_(ta.v)
        tb.global_step = ta.global_step
        oa, ob = ta.step(batch), tb.step(batch)
        for key in ("loss", "masked_img_loss", "masked_lm_loss", "masked_lm_loss_pv", "loss_lpm"):
            assert float(oa[key]) == float(ob[key]), (k, key, float(oa[key]), float(ob[key]))
        d = (fa.data - fb.data).abs()
        mean_d, frac = float(d.mean()), float((d > 0.05 * lr).float().mean())
        print("step %d: mean |dp| %.3e, fraction > 0.05 lr %.2e" % (k, mean_d, frac))
        assert mean_d <= 1e-3 * lr and frac <= 1e-3, (k, mean_d, frac)
        assert float(fb.grad.abs().max()) == 0.0
    assert torch.equal(tb.engine.fp.data[f0:f1], frozen0)
    gs = tb._graphs
    assert gs.captures == 1 and gs.replays == 2, (gs.captures, gs.replays)
    tb.finish()


@pytest.mark.parametrize("group_tv", [False, True], ids=["unpaired", "K3M_GROUP_TV"])
def test_dynamic_attention_below_and_above_the_cut(dev, deterministic, group_tv):
    """dynamic_attention with fixed_t_layer = t_biattention_id[0], on a schedule that runs image layer 0 before the
    first co-attention block (v_biattention_id[0] = 1): that layer's gate reads frozen text, so its pool gradient is
    dropped, while its dyLinear tensors keep theirs; the image layer after the last block pairs with text layer 11 in
    the lock step (K3M_GROUP_TV).  Every gradient above the cut is torch.equal to the uncut step's, and one
    Trainer.step moves the dyLinear tensors and leaves the frozen segment alone."""
    from k3m_amd import engine as E
    from k3m_amd.engine import K3MEngine, label_counts
    from k3m_amd.synthetic import synthetic_batch
    from k3m_amd.trainer import Trainer

    def config(fixed):
        cfg = _config(fixed, dynamic_attention=True)
        cfg.v_biattention_id = [1, 2, 3, 4, 5, 5]
        return cfg
    old = E.GROUP_TV
    E.GROUP_TV = bool(group_tv) and E.GROUPED
    try:
        engs = {}
        for fixed in (0, FIXED):
            cfg = config(fixed)
            eng = K3MEngine(cfg, dev, seed=77)
            assert ("v", 0) in eng.schedule[:eng.schedule.index(("c", 0))]
            eng.fp.load(_values(cfg, 4321))
            batch = synthetic_batch(cfg, 2, dev, seed=3)
            batch["_label_counts"] = label_counts(batch)
            out, ctx = eng.forward(batch, train=True, seed=5)
            eng.backward(ctx)
            torch.cuda.synchronize()
            engs[fixed] = (eng, out)
        (e0, o0), (e6, o6) = engs[0], engs[FIXED]
        for k in LOSS_KEYS + ("c_final",):
            assert torch.equal(o0[k], o6[k]), k
        for n, _ in e6.fp.spec:
            if n in e6.cut_frozen:
                assert float(e6.fp.g[n].abs().max()) == 0.0, n
            elif not n.startswith("embeddings."):
                assert torch.equal(e0.fp.g[n], e6.fp.g[n]), n
        for n in ("encoder.v_layer.0.attention.self.dyLinear_q.weight", "encoder.v_layer.5.attention.self.dyLinear_k.bias"):
            assert float(e6.fp.g[n].abs().max()) > 0.0, n
        del engs, e0, e6
        cfg = config(FIXED)
        tr = Trainer(cfg, dev, lr=1e-3, warmup_steps=0, total_steps=20, seed=9)
        tr.graph = False
        fp = tr.engine.fp
        start = fp.data.clone()
        tr.step(batch)
        torch.cuda.synchronize()
        f0, f1 = fp.segments["frozen"]
        assert torch.equal(fp.data[f0:f1], start[f0:f1]) and float(fp.grad[f0:f1].abs().max()) == 0.0
        for n, _ in fp.spec:
            if "dyLinear" in n:
                o = fp.offsets[n]
                assert not torch.equal(fp.p[n].reshape(-1), start[o:o + fp.p[n].numel()]), n
        tr.finish()
    finally:
        E.GROUP_TV = old
