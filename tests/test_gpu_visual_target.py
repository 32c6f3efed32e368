"""Masked-region feature regression (visual_target=1) end to end on the GPU, against the fixture recorded from the
reference model with that objective (tests/golden/make_visual_target_golden.py) and the float64 restatement of
tests/visual_target_ref.py: the fp32 and bf16 engines, a batch without a masked region, train mode, the Trainer, the
hipGraph step, the train.py driver, K3MForItemAlignment and the drop-in module.  Assertions and tolerances are those
of the tests they mirror (tests/test_gpu_fusion_modes.py, test_gpu_parity.py, test_gpu_finetune.py,
test_gpu_train_driver.py, test_gpu_graph.py)."""
import json
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest
import torch

import visual_target_ref as VR
from golden_util import (CFG_PATH, REPO, load_case, case_batch, case_noise, check_logits, check_img_logits, ft_noise,
                         ft_pair, load_ft_case)

pytestmark = pytest.mark.gpu
CASE = "vt1_bs2"
LOSS_KEYS = ("masked_lm_loss", "masked_img_loss", "masked_lm_loss_pv", "loss_lpm", "next_sentence_loss", "loss")
DECODER = "cls.imagePredictions.decoder.weight"


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda")


def _config(g):
    from k3m_amd.config import pretrain_config
    assert int(g["visual_target"]) == 1
    return pretrain_config(CFG_PATH, if_pre_sampling=int(g["mode"]), visual_target=1)


def _run_case(dev, dtype, train=False, image_label=None, backward=True):
    from k3m_amd.engine import K3MEngine
    from k3m_amd.weights import param_values
    g = load_case(CASE)
    cfg = _config(g)
    eng = K3MEngine(cfg, dev, dtype=dtype)
    eng.fp.load(param_values(cfg, int(g["weight_seed"])))
    batch = {k: v.to(dev) for k, v in case_batch(g).items()}
    if image_label is not None:
        batch["image_label"] = torch.full_like(batch["image_label"], image_label)
    noise = {k: v.to(dev) for k, v in case_noise(g).items()}
    eng.capture_logits = True
    out, ctx = eng.forward(batch, train=train, noise=noise, ent_neg=torch.from_numpy(g["ent_neg"]),
                           val_neg=torch.from_numpy(g["val_neg"]))
    if backward:
        eng.backward(ctx)
    torch.cuda.synchronize()
    got = np.array([float(out[k]) for k in LOSS_KEYS])
    return g, eng, out, got


@pytest.fixture(scope="module")
def fp32_run(dev):
    return _run_case(dev, "fp32")


def test_engine_matches_reference_golden(fp32_run):
    g, eng, out, got = fp32_run
    print("losses", got, g["losses"])
    np.testing.assert_allclose(got, g["losses"], rtol=1e-3, atol=1e-4)
    assert out["img_logits"].shape == (int((g["in/image_label"] == 1).sum()), 2048)
    check_logits(g, out["mlm_logits"].cpu().numpy(), g["logit/img_rows"], 1e-3, CASE)
    check_img_logits(g, out["img_logits"].cpu().numpy(), 1e-3, CASE)
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
            assert err <= 5e-3 * np.abs(ref).max() + 1e-6, (n, err, np.abs(ref).max())
    for n, ref in zip(list(g["grad_norm_names"]), g["grad_norms"]):
        gn = float(G[n].double().norm())
        if np.isnan(ref):
            assert gn == 0.0, n
            assert str(n) in eng.fp.frozen, n
        else:
            assert abs(gn - ref) <= 5e-3 * ref + 1e-6, (n, gn, ref)
    assert tuple(G[DECODER].shape) == (2048, 1024) and float(G[DECODER].abs().max()) > 0.0


# The one exception to the bf16 bars of tests/test_gpu_parity.py, at most twice the measured value (MI355X; the fp32
# run of the same fixture passes every fp32 bar).  out["img_logits"], the masked regions' predictions: the largest
# per-COLUMN mean error is 0.0250 of the row's max |prediction| (column 1115), against BF16_LOGIT_COLMEAN = 0.02.
# That bar was set from fixtures whose column means average 8 to 30 masked regions over 1601 columns (worst
# 0.0147, bs2_hard); this fixture has 5 masked regions (12 boxes keep the file under 1 MiB) and 2048 columns, so each
# column mean averages fewer errors and the maximum is taken over more columns.  The per-element, mean and
# 99th-percentile bars hold as they are.
BF16_IMG_COLMEAN_BAR = 0.04


def test_bf16_engine_close_to_reference_golden(dev):
    """The bars are those of tests/test_gpu_parity.py, with the one exception above."""
    from test_gpu_parity import (BF16_LOSS_RTOL, BF16_GRAD_COS, BF16_GRAD_NORM_RTOL, BF16_GLOBAL_COS, BF16_LOGIT_RTOL,
                                 BF16_LOGIT_MEAN, BF16_LOGIT_P99, BF16_LOGIT_COLMEAN, BF16_LSE_ATOL)
    g, eng, out, got = _run_case(dev, "bf16")
    check_logits(g, out["mlm_logits"].cpu().numpy(), g["logit/img_rows"], BF16_LOGIT_RTOL, CASE + " bf16",
                 mean_rtol=BF16_LOGIT_MEAN, p99=BF16_LOGIT_P99, col_mean=BF16_LOGIT_COLMEAN, lse_atol=BF16_LSE_ATOL)
    assert BF16_LOGIT_COLMEAN < BF16_IMG_COLMEAN_BAR <= 2 * 0.0250
    check_img_logits(g, out["img_logits"].cpu().numpy(), BF16_LOGIT_RTOL, CASE + " bf16", mean_rtol=BF16_LOGIT_MEAN,
                     p99=BF16_LOGIT_P99, col_mean=BF16_IMG_COLMEAN_BAR)
    rel = np.abs(got - g["losses"]) / np.maximum(np.abs(g["losses"]), 1e-3)
    print("bf16 loss rel err", rel)
    assert (rel <= BF16_LOSS_RTOL).all(), (got, g["losses"])
    G = eng.fp.g
    worst_cos, worst_norm, bad = 1.0, 0.0, []
    dot = na = nb2 = 0.0
    for k in g:
        if k.startswith("grad_full/"):
            n = k.split("/", 1)[1]
            a = G[n].double().cpu().numpy().ravel()
            b = g[k].astype(np.float64).ravel()
            nb = np.linalg.norm(b)
            if nb < 1e-6:
                continue
            cos = float(a @ b / (np.linalg.norm(a) * nb + 1e-30))
            nr = abs(np.linalg.norm(a) - nb) / nb
            dot, na, nb2 = dot + float(a @ b), na + float(a @ a), nb2 + float(b @ b)
            worst_cos, worst_norm = min(worst_cos, cos), max(worst_norm, nr)
            print("bf16 grad", n, "cos %.5f norm rel %.4f" % (cos, nr))
            if not (cos >= BF16_GRAD_COS and nr <= BF16_GRAD_NORM_RTOL):
                bad.append((n, cos, nr))
    gcos = dot / np.sqrt(na * nb2)
    print("bf16 grads: worst cos %.5f worst norm rel %.4f global cos %.6f" % (worst_cos, worst_norm, gcos))
    assert not bad, bad
    assert gcos >= BF16_GLOBAL_COS, gcos
    for n, ref in zip(list(g["grad_norm_names"]), g["grad_norms"]):
        if np.isnan(ref):
            assert float(G[n].abs().max()) == 0.0, n


def test_no_masked_region_gives_zero_loss_and_no_image_head_gradient(dev):
    """The clamped denominator (vilbert_k3m.py:2750-2752): 0.0, where the KL of visual_target 0 gives 0/0."""
    g, eng, out, got = _run_case(dev, "fp32", image_label=-1)
    print("losses", got, g["losses"])
    assert got[1] == 0.0
    assert out["img_logits"].shape[0] == 0
    for n, t in eng.fp.g.items():
        if n.startswith("cls.imagePredictions."):
            assert float(t.abs().max()) == 0.0, n
    keep = [0, 2, 3, 4]   # the encoder's inputs are unchanged: the other losses are those of the unmodified run
    np.testing.assert_allclose(got[keep], g["losses"][keep], rtol=1e-3, atol=1e-4)
    np.testing.assert_allclose(got[5], g["losses"][5] - g["losses"][1], rtol=1e-3, atol=1e-4)
    assert float(eng.fp.g["struc_w1.weight"].abs().max()) > 0.0


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_train_mode_loss_equals_restatement_of_its_own_predictions(dev, dtype):
    g, eng, out, got = _run_case(dev, dtype, train=True, backward=False)
    assert eng.p_vh > 0   # dropout is on
    want, _ = VR.masked_img_loss(out["img_logits"].cpu().numpy(), g["in/image_target"], g["in/image_label"])
    print(dtype, "masked_img_loss", got[1], "restated", want)
    np.testing.assert_allclose(got[1], want, rtol=1e-5)
    assert abs(got[1] - g["losses"][1]) > 1e-5 * g["losses"][1]   # not the eval-mode value: dropout did act


def _synthetic(dev, B, seed):
    from k3m_amd.config import pretrain_config
    from k3m_amd.engine import label_counts
    from k3m_amd.synthetic import synthetic_batch
    cfg = pretrain_config(CFG_PATH, visual_target=1)
    batch = synthetic_batch(cfg, B, dev, seed=seed)
    assert batch["image_target"].shape == (B, 36, 2048)
    batch["_label_counts"] = label_counts(batch)
    return cfg, batch


def test_trainer_step_moves_the_decoder(dev):
    from k3m_amd.trainer import Trainer
    cfg, batch = _synthetic(dev, 2, 21)
    tr = Trainer(cfg, dev, lr=1e-3, warmup_steps=0, total_steps=20, seed=9, loss_img_weight=0.5)
    tr.graph = False
    before = tr.engine.fp.p[DECODER].clone()
    assert tuple(before.shape) == (2048, 1024)
    out = tr.step(batch)
    torch.cuda.synchronize()
    parts = [float(out[k]) for k in ("masked_lm_loss", "masked_img_loss", "masked_lm_loss_pv", "loss_lpm")]
    assert np.isfinite(float(out["loss"])) and all(np.isfinite(parts)) and parts[1] > 0
    np.testing.assert_allclose(float(out["loss"]), parts[0] + 0.5 * parts[1] + parts[2] + parts[3], rtol=1e-5)
    assert not torch.equal(tr.engine.fp.p[DECODER], before)
    tr.finish()


def test_graph_step_matches_eager(dev):
    """The body of test_gpu_graph.test_graph_step_matches_eager with visual_target = 1: fp32, B = 2, three steps (one
    capture, two replays), the same bars."""
    from k3m_amd.trainer import Trainer
    cfg, batch = _synthetic(dev, 2, 23)
    lr = 1e-3
    ta = Trainer(cfg, dev, lr=lr, warmup_steps=0, total_steps=20, seed=9)
    tb = Trainer(cfg, dev, lr=lr, warmup_steps=0, total_steps=20, seed=9)
    ta.graph, tb.graph = False, True
    assert ta.dropout and tb.dropout
    start = tb.engine.fp.p[DECODER][:4].clone()
    for k in range(3):
        fa, fb = ta.engine.fp, tb.engine.fp
        fb.data.copy_(fa.data)
        tb.m.copy_(ta.m)
        tb.v.copy_(ta.v)
        tb.global_step = ta.global_step
        oa, ob = ta.step(batch), tb.step(batch)
        for key in ("loss", "masked_img_loss", "masked_lm_loss", "masked_lm_loss_pv", "loss_lpm"):
            assert float(oa[key]) == float(ob[key]), (k, key, float(oa[key]), float(ob[key]))
        assert ta.global_step == tb.global_step == k + 1
        d = (fa.data - fb.data).abs()
        mean_d, frac = float(d.mean()), float((d > 0.05 * lr).float().mean())
        print("step %d: mean |dp| %.3e, fraction > 0.05 lr %.2e" % (k, mean_d, frac))
        assert mean_d <= 1e-3 * lr and frac <= 1e-3, (k, mean_d, frac)
        assert float(fb.grad.abs().max()) == 0.0
    assert not torch.equal(tb.engine.fp.p[DECODER][:4], start)
    gs = tb._graphs
    assert gs.captures == 1 and gs.replays == 2, (gs.captures, gs.replays)
    tb.finish()


def test_train_py_visual_target_1_trains_evaluates_and_saves(dev, tmp_path):
    from vilbert_k3m.vilbert_k3m import BertForMultiModalPreTraining_tri_stru
    from k3m_amd.config import pretrain_config
    out = tmp_path / "out"
    out.mkdir()
    shutil.copy(CFG_PATH, out / "bert_base_6layer_6conect.json")
    rows = []
    for i in range(6):
        pv = "#;#".join("p%d%d#:#v%d%d" % (i, j, j, i) for j in range(3 + i))
        rows.append("%d\titem title %d with words\thttp://img/%d.jpg\t%s\tcat" % (1000 + i, i, i, pv))
    for name in ("rows_train+valid.tsv", "rows_valid.tsv"):
        (tmp_path / name).write_text("\n".join(rows) + "\n", encoding="utf-8")
    log = tmp_path / "loss.jsonl"
    r = subprocess.run([sys.executable, os.path.join(REPO, "train.py"), "--data_dir", str(tmp_path), "--output_dir",
                        str(out), "--file_name", "rows_{}.tsv", "--do_train", "--do_eval", "--with_coattention",
                        "--visual_target", "1", "--train_batch_size", "3", "--eval_batch_size", "3",
                        "--num_train_epochs", "1", "--k3m_char_tokenizer", "--k3m_synthetic_regions", "3",
                        "--k3m_loss_log", str(log)], cwd=str(tmp_path), capture_output=True, text=True, timeout=400)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    steps = [json.loads(l) for l in log.read_text().splitlines()]
    assert len(steps) == 2 and all(np.isfinite(s["loss"]) and np.isfinite(s["masked_img_loss"]) for s in steps)
    assert "[Eval] [Epoch-0] loss:" in r.stderr
    sd = torch.load(str(out / "k3m_bert-base-uncased_12l_12h" / "K3M_struc_presample-1_epoch-0.bin"),
                    map_location="cpu", weights_only=True)
    cfg1 = pretrain_config(CFG_PATH, visual_target=1)
    assert tuple(sd[DECODER].shape) == (2048, cfg1.v_hidden_size)
    assert tuple(sd["cls.imagePredictions.decoder.bias"].shape) == (2048,)
    m1 = BertForMultiModalPreTraining_tri_stru(cfg1, device=dev)
    assert not m1.load_state_dict(sd)
    assert torch.equal(dict(m1.named_parameters())[DECODER].detach().cpu(), sd[DECODER])
    del m1
    m0 = BertForMultiModalPreTraining_tri_stru(pretrain_config(CFG_PATH), device=dev)
    with pytest.raises(ValueError, match=r"cls\.imagePredictions\.decoder\.weight: shape"):
        m0.load_state_dict(sd)


def test_item_alignment_with_visual_target_1_matches_reference_golden(dev):
    """The item-alignment task has no image head: the recorded outputs of golden_ft_ce apply as they are."""
    from k3m_amd.config import finetune_config
    from k3m_amd.finetune import ARG_NAMES, K3MForItemAlignment
    from k3m_amd.weights import param_values
    g = load_ft_case("ce")
    cfg = finetune_config(CFG_PATH, loss_type="ce", if_pre_sampling=int(g["mode"]), visual_target=1)
    assert cfg.visual_target == 1 and cfg.v_target_size == 2048
    model = K3MForItemAlignment(cfg, dev)
    model.engine.fp.load(param_values(cfg, int(g["weight_seed"])))
    pair = {k: v.to(dev) for k, v in ft_pair(g).items()}
    n1, n2 = ft_noise(g)
    noise = ({k: v.to(dev) for k, v in n1.items()}, {k: v.to(dev) for k, v in n2.items()})
    e1, e2, probs, loss = model(*[pair[k] for k in ARG_NAMES], train=False, noise=noise)
    model.backward()
    torch.cuda.synchronize()
    np.testing.assert_allclose(float(loss), float(g["out/loss"]), rtol=1e-3, atol=1e-5)
    np.testing.assert_allclose(e1.cpu().numpy(), g["out/e1"], rtol=1e-3, atol=1e-4)
    np.testing.assert_allclose(e2.cpu().numpy(), g["out/e2"], rtol=1e-3, atol=1e-4)
    np.testing.assert_allclose(probs.cpu().numpy(), g["out/probs"], rtol=1e-3, atol=1e-5)
    G = model.engine.fp.g
    for k in g:
        if k.startswith("grad_full/"):
            n = k.split("/", 1)[1]
            ref = g[k]
            err = np.abs(G[n].cpu().numpy() - ref).max()
            assert err <= 5e-3 * np.abs(ref).max() + 1e-6, (n, err, np.abs(ref).max())
    for n, ref in zip(list(g["grad_norm_names"]), g["grad_norms"]):
        gn = float(G[n].double().norm())
        if np.isnan(ref):
            assert gn == 0.0, n
        else:
            assert abs(gn - ref) <= 5e-3 * ref + 1e-6, (n, gn, ref)


def test_drop_in_module_returns_the_engines_losses(dev, fp32_run):
    from vilbert_k3m.vilbert_k3m import BertForMultiModalPreTraining_tri_stru
    from k3m_amd.weights import param_values
    g, _, _, eng_losses = fp32_run
    cfg = _config(g)
    model = BertForMultiModalPreTraining_tri_stru(cfg, device=dev)
    assert not model.load_state_dict({k: torch.from_numpy(v) for k, v in param_values(cfg, int(g["weight_seed"])).items()})
    model.eval()
    tb = {k: v.to(dev) for k, v in case_batch(g).items()}
    noise = {k: v.to(dev) for k, v in case_noise(g).items()}
    outs = model(tb["input_ids"], tb["image_feat"], tb["image_loc"], tb["segment_ids"], tb["input_mask"],
                 tb["image_mask"], tb["lm_label_ids"], tb["image_label"], tb["image_target"], tb["is_next"],
                 output_all_attention_masks=False, input_ids_pv=tb["input_ids_pv"],
                 token_type_ids_pv=tb["segment_ids_pv"], attention_mask_pv=tb["input_mask_pv"],
                 masked_lm_labels_pv=tb["lm_label_ids_pv"], next_sentence_label_pv_v=tb["is_next_pv_v"],
                 next_sentence_label_pv_t=tb["is_next_pv_t"], index_p=tb["index_p"], index_v=tb["index_v"],
                 device=dev, gumbel_noise=noise, ent_neg=torch.from_numpy(g["ent_neg"]),
                 val_neg=torch.from_numpy(g["val_neg"]))
    assert len(outs) == 10
    mlm_t, img, _, mlm_pv, _, _, nsp, c_init, c_final, lpm = outs
    loss = mlm_t + img * 1.0 + mlm_pv + lpm
    got = np.array([float(x.detach()) for x in (mlm_t, img, mlm_pv, lpm, nsp, loss)])
    # the same kernels on the same inputs; only the backward's float atomics are order dependent, not the forward
    np.testing.assert_allclose(got, eng_losses, rtol=1e-6)
    np.testing.assert_allclose(got, g["losses"], rtol=1e-3, atol=1e-4)
    loss.backward()
    p = dict(model.named_parameters())[DECODER]
    ref = float(g["grad_norms"][list(g["grad_norm_names"]).index(DECODER)])
    assert abs(float(p.grad.double().norm()) - ref) <= 5e-3 * ref + 1e-6
