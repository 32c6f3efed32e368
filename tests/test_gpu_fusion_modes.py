"""The soft (if_pre_sampling 2) and interactive-only (3) fusion modes end to end on the GPU, against
fixtures recorded from the reference model in those modes (tests/golden/make_fusion_golden.py):
the fp32 and bf16 engines, K3MForItemAlignment, the train.py driver, the hipGraph step and train mode.
Assertions and tolerances are those of the mode-0/1 tests they mirror (tests/test_gpu_parity.py,
test_gpu_finetune.py, test_gpu_train_driver.py, test_gpu_graph.py)."""
import json
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest
import torch

from golden_util import (CFG_PATH, HERE, REPO, load_case, case_config, case_batch, check_logits, check_img_logits,
                         ft_config, ft_noise, ft_pair, load_ft_case)

pytestmark = pytest.mark.gpu
FUSION_CASES = ["bs2_soft", "bs2_inter"]


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda")


def _run_case(case, dev, dtype):
    from k3m_amd.engine import K3MEngine
    from k3m_amd.weights import param_values
    g = load_case(case)
    cfg = case_config(g)
    assert cfg.if_pre_sampling == {"bs2_soft": 2, "bs2_inter": 3}[case]
    eng = K3MEngine(cfg, dev, dtype=dtype)
    eng.fp.load(param_values(cfg, int(g["weight_seed"])))
    batch = {k: v.to(dev) for k, v in case_batch(g).items()}
    eng.capture_logits = True
    # neither mode draws gumbel noise: none is passed
    out, ctx = eng.forward(batch, train=False, noise=None, ent_neg=torch.from_numpy(g["ent_neg"]),
                           val_neg=torch.from_numpy(g["val_neg"]))
    eng.backward(ctx)
    torch.cuda.synchronize()
    got = np.array([float(out[k]) for k in ("masked_lm_loss", "masked_img_loss", "masked_lm_loss_pv", "loss_lpm",
                                           "next_sentence_loss", "loss")])
    return g, eng, out, got


@pytest.mark.parametrize("case", FUSION_CASES)
def test_engine_matches_reference_golden(dev, case):
    g, eng, out, got = _run_case(case, dev, "fp32")
    print("losses", case, got, g["losses"])
    np.testing.assert_allclose(got, g["losses"], rtol=1e-3, atol=1e-4)
    check_logits(g, out["mlm_logits"].cpu().numpy(), g["logit/img_rows"], 1e-3, case)
    check_img_logits(g, out["img_logits"].cpu().numpy(), 1e-3, case)
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
    if case == "bs2_soft":   # the new trainable tensors carry a real gradient
        for m in ("v", "t", "pv"):
            assert float(G["soft_%s.weight" % m].abs().max()) > 0.0 and float(G["soft_%s.bias" % m].abs().max()) > 0.0


# Per-fixture exceptions to BF16_GRAD_NORM_RTOL (2e-2), each at most twice the measured value.
# bs2_inter (MI355X, fp32 run of the same fixture passes at 5e-3): struc_w2.weight has gradient-norm
# relative error 0.0251 at cosine 0.99807; every other recorded tensor of the fixture is within 0.0020 and
# cosine >= 0.99985, the global cosine is 0.99988.  Without the individual stream (the fp32 embedding
# output) the fused sequence consists of bf16 encoder outputs only, and the aggregator's score vector
# struc_w2 sees a softmax over few triples: its error vector (|d| ~ 0.06 |g|, like the worst mode-1 tensors,
# cosine 0.9961) happens to lie along the gradient.  bs2_soft stays inside the common bars (worst 0.0078).
BF16_NORM_BAR = {"bs2_inter": 5e-2}


@pytest.mark.parametrize("case", FUSION_CASES)
def test_bf16_engine_close_to_reference_golden(dev, case):
    """The bars are those of tests/test_gpu_parity.py (set about 2x above the five mode-0/1 fixtures)."""
    from test_gpu_parity import (BF16_LOSS_RTOL, BF16_GRAD_COS, BF16_GRAD_NORM_RTOL, BF16_GLOBAL_COS, BF16_LOGIT_RTOL,
                                 BF16_LOGIT_MEAN, BF16_LOGIT_P99, BF16_LOGIT_COLMEAN, BF16_LSE_ATOL)
    g, eng, out, got = _run_case(case, dev, "bf16")
    check_logits(g, out["mlm_logits"].cpu().numpy(), g["logit/img_rows"], BF16_LOGIT_RTOL, case + " bf16",
                 mean_rtol=BF16_LOGIT_MEAN, p99=BF16_LOGIT_P99, col_mean=BF16_LOGIT_COLMEAN, lse_atol=BF16_LSE_ATOL)
    check_img_logits(g, out["img_logits"].cpu().numpy(), BF16_LOGIT_RTOL, case + " bf16", mean_rtol=BF16_LOGIT_MEAN,
                     p99=BF16_LOGIT_P99, col_mean=BF16_LOGIT_COLMEAN)
    rel = np.abs(got - g["losses"]) / np.maximum(np.abs(g["losses"]), 1e-3)
    print("bf16 loss rel err", case, rel)
    assert (rel <= BF16_LOSS_RTOL).all(), (got, g["losses"])
    G = eng.fp.g
    norm_bar = BF16_NORM_BAR.get(case, BF16_GRAD_NORM_RTOL)
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
            if not (cos >= BF16_GRAD_COS and nr <= norm_bar):
                bad.append((n, cos, nr))
    gcos = dot / np.sqrt(na * nb2)
    print("bf16 grads: worst cos %.5f worst norm rel %.4f global cos %.6f" % (worst_cos, worst_norm, gcos))
    assert not bad, bad
    assert gcos >= BF16_GLOBAL_COS, gcos
    for n, ref in zip(list(g["grad_norm_names"]), g["grad_norms"]):
        if np.isnan(ref):
            assert float(G[n].abs().max()) == 0.0, n


def test_item_alignment_matches_reference_golden(dev):
    from k3m_amd.finetune import ARG_NAMES, K3MForItemAlignment
    from k3m_amd.weights import param_values
    g = load_ft_case("ce_soft")
    cfg = ft_config(g)
    assert cfg.if_pre_sampling == 2
    model = K3MForItemAlignment(cfg, dev)
    model.engine.fp.load(param_values(cfg, int(g["weight_seed"])))
    pair = {k: v.to(dev) for k, v in ft_pair(g).items()}
    n1, n2 = ft_noise(g)   # ignored by the soft gate; passed as the mode-1 test passes it
    noise = ({k: v.to(dev) for k, v in n1.items()}, {k: v.to(dev) for k, v in n2.items()})
    e1, e2, probs, loss = model(*[pair[k] for k in ARG_NAMES], train=False, noise=noise)
    model.backward()
    torch.cuda.synchronize()
    print("ft ce soft loss", float(loss), float(g["out/loss"]))
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


# ---------------------------------------------------------------- train.py
def _train_py_parity(case, mode, tmp_path):
    from k3m_amd.weights import param_values
    g = load_case(case)
    out = tmp_path / "out"
    out.mkdir()
    shutil.copy(CFG_PATH, out / "bert_base_6layer_6conect.json")
    vals = param_values(case_config(g), int(g["weight_seed"]))
    torch.save({k: torch.from_numpy(v) for k, v in vals.items()}, str(tmp_path / "w.bin"))
    log = tmp_path / "loss.jsonl"
    r = subprocess.run([sys.executable, os.path.join(REPO, "train.py"), "--data_dir", str(tmp_path), "--output_dir",
                        str(out), "--file_name", "unused", "--do_train", "--with_coattention", "--train_batch_size", "2",
                        "--num_train_epochs", "1", "--if_pre_sampling", str(mode), "--file_state_dict",
                        str(tmp_path / "w.bin"), "--k3m_parity_case",
                        os.path.join(HERE, "golden", "golden_%s.npz" % case), "--k3m_max_steps", "2",
                        "--k3m_loss_log", str(log)], cwd=str(tmp_path), capture_output=True, text=True, timeout=400)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    rows = [json.loads(l) for l in log.read_text().splitlines()]
    assert len(rows) == 2
    for row in rows:   # lr = 0 on the first step, so both steps see the fixture's weights
        got = np.array([row["masked_lm_loss"], row["masked_img_loss"], row["masked_lm_loss_pv"], row["loss_lpm"],
                        row["next_sentence_loss"], row["loss"]])
        np.testing.assert_allclose(got, g["losses"], rtol=1e-3, atol=1e-4)
    ck_dir = out / "k3m_bert-base-uncased_12l_12h"
    base = "K3M_struc_presample-%d_epoch-0" % mode
    ck = torch.load(str(ck_dir / (base + ".tar")), map_location="cpu", weights_only=True)
    sd = torch.load(str(ck_dir / (base + ".bin")), map_location="cpu", weights_only=True)
    assert ck["global_step"] == 2 and len(sd) == 999
    return vals, ck, sd


def _state_names(ck, cfg):
    """Names that carry optimizer state in a two-group reference-layout .tar."""
    from k3m_amd.params import is_no_decay, param_spec
    names = [n for n, _ in param_spec(cfg)]
    order = [n for n in names if not is_no_decay(n)] + [n for n in names if is_no_decay(n)]
    return {order[int(i)] for i in ck["optimizer_state_dict"]["state"]}


def test_train_py_soft_mode_two_steps_match_golden(tmp_path):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    vals, ck, sd = _train_py_parity("bs2_soft", 2, tmp_path)
    have = _state_names(ck, case_config(load_case("bs2_soft")))
    assert "soft_t.weight" in have and "score_self_t.weight" in have and "t_pooler.dense.weight" not in have
    assert not torch.equal(sd["soft_t.weight"], torch.from_numpy(vals["soft_t.weight"]))
    assert not torch.equal(sd["struc_w1.weight"], torch.from_numpy(vals["struc_w1.weight"]))


def test_train_py_interactive_only_leaves_gate_tensors_untouched(tmp_path):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    vals, ck, sd = _train_py_parity("bs2_inter", 3, tmp_path)
    have = _state_names(ck, case_config(load_case("bs2_inter")))
    assert "soft_t.weight" not in have and "score_self_t.weight" not in have and "struc_w1.weight" in have
    for n in ("score_self_t.weight", "soft_t.weight"):
        assert torch.equal(sd[n], torch.from_numpy(vals[n])), n
    assert not torch.equal(sd["struc_w1.weight"], torch.from_numpy(vals["struc_w1.weight"]))


# ---------------------------------------------------------------- hipGraph step, train mode
def test_graph_step_matches_eager_soft_mode(dev):
    """The body of test_gpu_graph.test_graph_step_matches_eager at if_pre_sampling = 2: fp32, B = 4, three
    steps (one capture, two replays), the same bars."""
    from k3m_amd.config import pretrain_config
    from k3m_amd.engine import label_counts
    from k3m_amd.synthetic import synthetic_batch
    from k3m_amd.trainer import Trainer
    cfg = pretrain_config(CFG_PATH, if_pre_sampling=2)
    batch = synthetic_batch(cfg, 4, dev, seed=21)
    batch["_label_counts"] = label_counts(batch)
    lr = 1e-3
    ta = Trainer(cfg, dev, lr=lr, warmup_steps=0, total_steps=20, seed=9)
    tb = Trainer(cfg, dev, lr=lr, warmup_steps=0, total_steps=20, seed=9)
    ta.graph, tb.graph = False, True
    assert ta.dropout and tb.dropout
    o = ta.engine.fp.offsets["soft_t.weight"]
    start = ta.engine.fp.data[o:o + 64].clone()
    for k in range(3):
        fa, fb = ta.engine.fp, tb.engine.fp
        fb.data.copy_(fa.data)
        tb.m.copy_(ta.m)
        tb.v.copy_(ta.v)
        tb.global_step = ta.global_step
        la = float(ta.step(batch)["loss"])
        lb = float(tb.step(batch)["loss"])
        assert la == lb, (k, la, lb)
        assert ta.global_step == tb.global_step == k + 1
        d = (fa.data - fb.data).abs()
        mean_d, frac = float(d.mean()), float((d > 0.05 * lr).float().mean())
        print("step %d: mean |dp| %.3e, fraction > 0.05 lr %.2e" % (k, mean_d, frac))
        assert mean_d <= 1e-3 * lr and frac <= 1e-3, (k, mean_d, frac)
        assert float(fb.grad.abs().max()) == 0.0
    assert not torch.equal(tb.engine.fp.data[o:o + 64], start)   # the replayed AdamW table reaches soft_*
    gs = tb._graphs
    assert gs.captures == 1 and gs.replays == 2, (gs.captures, gs.replays)
    tb.finish()


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("mode", [2, 3])
def test_train_mode_step_is_finite_and_learns(dev, mode, dtype):
    from k3m_amd.config import pretrain_config
    from k3m_amd.trainer import Trainer
    from k3m_amd.synthetic import synthetic_batch
    cfg = pretrain_config(CFG_PATH, if_pre_sampling=mode)
    tr = Trainer(cfg, dev, lr=2e-4, warmup_steps=0, total_steps=100, seed=3, dtype=dtype)
    batch = synthetic_batch(cfg, 8, dev, seed=5)
    losses = []
    for _ in range(6):
        out = tr.step(batch)
        losses.append(float(out["loss"]))
    print("mode", mode, dtype, losses)
    assert all(np.isfinite(losses)), losses
    assert losses[-1] < losses[0], losses
