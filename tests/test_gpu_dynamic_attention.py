"""Dynamic image attention (cfg.dynamic_attention) end to end on the GPU, against fixtures recorded from the reference
with the flag on (tests/golden/make_dynamic_attention_golden.py): the fp32 and bf16 engines, the text + image lock
step (GROUP_TV) on and off, K3MForItemAlignment, a Trainer in train mode, the train.py --dynamic_attention driver, and
the first-step loss of the model WITHOUT the flag against the value of the commit before the feature.

Bars: those of tests/test_gpu_parity.py (fp32: losses, logits and c_* rtol 1e-3 / atol 1e-4, gradient tensors
within 5e-3 of their max + 1e-6, norms within 5e-3; bf16: the common BF16_* bars, as tests/test_gpu_text_only.py
applies them to its bs2 case).  The fixtures draw the weights at the ``weight_std`` they record (see the
generator).  Train-mode (dropout) parity against an external reference is not covered: the committed oracle has no
dynamic attention."""
import json
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest
import torch

from golden_util import (CFG_PATH, HERE, REPO, load_case, case_batch, case_noise, check_logits, check_img_logits,
                         load_ft_case, ft_noise, ft_pair)

pytestmark = pytest.mark.gpu
CASES = ["da_bs2", "da_bs3_zero_triple"]
LOSS_KEYS = ("masked_lm_loss", "masked_img_loss", "masked_lm_loss_pv", "loss_lpm", "next_sentence_loss", "loss")


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda")


@pytest.fixture
def deterministic():
    from k3m_amd import ops
    old = ops.DETERMINISTIC
    ops.set_deterministic(True)
    yield
    ops.set_deterministic(old)


def da_config(dyn=True):
    from k3m_amd.config import pretrain_config
    return pretrain_config(CFG_PATH, if_pre_sampling=1, dynamic_attention=dyn)


def da_batch(g, dev):
    """the fixture stores the region features and targets as fp16 (exactly what the reference was fed)"""
    return {k: (v.float() if v.dtype == torch.float16 else v).to(dev) for k, v in case_batch(g).items()}


def dy_names(fp):
    return [n for n, _ in fp.spec if ".dyLinear_" in n]


_RUNS = {}


def _run_case(case, dev, dtype, group_tv=False):
    """forward + backward of one fixture; cached per (case, dtype, pairing) — the runs are shared, not repeated"""
    key = (case, dtype, group_tv)
    if key in _RUNS:
        return _RUNS[key]
    from k3m_amd import engine as E
    from k3m_amd.weights import param_values
    g = load_case(case)
    cfg = da_config()
    eng = E.K3MEngine(cfg, dev, dtype=dtype)
    eng.fp.load(param_values(cfg, int(g["weight_seed"]), std=float(g["weight_std"])))
    batch = da_batch(g, dev)
    noise = {k: (v * float(g["noise_scale"])).to(dev) for k, v in case_noise(g).items()}   # as the generator fed it
    eng.capture_logits = True
    old = E.GROUP_TV
    E.GROUP_TV = bool(group_tv) and E.GROUPED
    try:
        out, ctx = eng.forward(batch, train=False, noise=noise, ent_neg=torch.from_numpy(g["ent_neg"]),
                               val_neg=torch.from_numpy(g["val_neg"]))
        eng.backward(ctx)
    finally:
        E.GROUP_TV = old
    torch.cuda.synchronize()
    got = np.array([float(out[k]) for k in LOSS_KEYS])
    out = {k: v.detach().clone() for k, v in out.items() if torch.is_tensor(v)}
    res = (g, eng.fp.grad.clone(), {n: eng.fp.g[n] for n, _ in eng.fp.spec}, out, got, eng)
    if len(_RUNS) >= 2:   # two engines' worth of buffers at most
        _RUNS.pop(next(iter(_RUNS)))
    _RUNS[key] = res
    return res


def _check_fp32(g, G, out, got, what):
    print("losses", what, got, g["losses"])
    np.testing.assert_allclose(got, g["losses"], rtol=1e-3, atol=1e-4)
    check_logits(g, out["mlm_logits"].cpu().numpy(), g["logit/img_rows"], 1e-3, what)
    check_img_logits(g, out["img_logits"].cpu().numpy(), 1e-3, what)
    np.testing.assert_allclose(out["c_initial"].cpu().numpy(), g["c_initial"], rtol=1e-3, atol=1e-4)
    np.testing.assert_allclose(out["c_final"].cpu().numpy(), g["c_final"], rtol=1e-3, atol=1e-4)
    seen = 0
    for k in g:
        kind, _, n = k.partition("/")
        if kind not in ("grad_full", "grad_slice", "grad_sub", "grad_rows"):
            continue
        gr = G[n]
        if kind == "grad_slice":
            gr = gr[:4] if gr.dim() == 2 else gr[:256]
        elif kind == "grad_sub":
            gr = gr[::16, ::16]
        elif kind == "grad_rows":      # the first and last two rows in full
            gr = torch.cat([gr[:2], gr[-2:]])
        ref = g[k]
        err = np.abs(gr.cpu().numpy() - ref).max()
        assert err <= 5e-3 * np.abs(ref).max() + 1e-6, (n, err, np.abs(ref).max())
        seen += "dyLinear" in n
    assert seen == 12               # dyLinear_q / dyLinear_k of v_layer.0 and v_layer.5: bias, weight grid, weight rows
    dyn = 0
    for n, ref in zip(list(g["grad_norm_names"]), g["grad_norms"]):
        gn = float(G[n].double().norm())
        if np.isnan(ref):
            assert gn == 0.0, n
        else:
            assert abs(gn - ref) <= 5e-3 * ref + 1e-6, (n, gn, ref)
            if "dyLinear" in str(n):
                assert ref > 0.0 and gn > 0.0
                dyn += 1
    assert dyn == 24


@pytest.mark.parametrize("case", CASES)
def test_engine_matches_reference_golden(dev, case):
    g, _, G, out, got, eng = _run_case(case, dev, "fp32")
    assert eng.dyn_attn and len(dy_names(eng.fp)) == 24
    # a fixture that cannot be blind: what the reference gives WITHOUT the flag (recorded by the generator) is
    # outside the bars below — the total by more than 0.01, at least one loss by more than 10x its own bar, the
    # masked regions' logits by more than 10x theirs.  (The total does NOT move by 10x its own bar, about 0.25: in
    # the reference the flag moves it by 3e-4 to 1e-2 of its value at any weight scale, see the generator.)
    d = np.abs(g["losses_without_flag"] - g["losses"])
    print("flag moves the losses by", d, "the masked-region logits by", g["img_logit_move"])
    assert d[5] > 1e-2 and (d > 10 * (1e-3 * np.abs(g["losses_without_flag"]) + 1e-4)).any(), d
    assert g["img_logit_move"][0] > 10 * 1e-3 * g["img_logit_move"][1]
    _check_fp32(g, G, out, got, case)


@pytest.fixture
def same_split_policy():
    """The k-split heuristics that apply to UNGROUPED GEMM launches only (ops.small_splitk, ops.SPLITK_FILL) change a
    product's summation order by design, so a layer run alone and the same layer in a grouped launch differ in the
    last bits with or without dynamic attention.  Off for both runs of the comparison below."""
    from k3m_amd import ops
    old = ops.SMALL_SPLITK, ops.SPLITK_FILL
    ops.SMALL_SPLITK = ops.SPLITK_FILL = False
    yield
    ops.SMALL_SPLITK, ops.SPLITK_FILL = old


def _lock_step_runs(case, dev):
    _RUNS.clear()   # the runs of these tests are made in deterministic mode
    r0 = _run_case(case, dev, "fp32", group_tv=False)
    r1 = _run_case(case, dev, "fp32", group_tv=True)
    _RUNS.clear()
    return r0, r1


@pytest.mark.parametrize("case", CASES)
def test_lock_step_pairing_gives_the_same_forward_under_one_split_policy(dev, deterministic, same_split_policy, case):
    """GROUP_TV on: the image layers after the last co-attention block run in lock step with the text layers that
    follow them, the (text, image) positions before a block do not.  Forward and gradients equal the fixture either
    way, and the forward is bit-identical between the two."""
    (g, flat0, G0, out0, got0, _), (_, flat1, G1, out1, got1, eng) = _lock_step_runs(case, dev)
    sched = eng.schedule
    pairs = [(a, b) for a, b in zip(sched, sched[1:]) if {a[0], b[0]} == {"t", "v"}]
    assert [p for p in pairs if p[0][0] == "v"] and [p for p in pairs if p[0][0] == "t"]   # both kinds occur
    _check_fp32(g, G0, out0, got0, case + " unpaired")
    _check_fp32(g, G1, out1, got1, case + " paired")
    assert (got0 == got1).all()
    assert torch.equal(out0["c_final"], out1["c_final"]) and torch.equal(out0["mlm_logits"], out1["mlm_logits"])
    assert torch.equal(out0["img_logits"], out1["img_logits"])


@pytest.mark.parametrize("case", CASES)
def test_lock_step_pairing_gradients_are_bit_identical_under_one_split_policy(dev, deterministic, same_split_policy,
                                                                              case):
    """Gradients bit-identical with the pairing on and off in deterministic mode, GIVEN one GEMM split policy: with
    the default ops.SMALL_SPLITK / ops.SPLITK_FILL an ungrouped launch picks another k-split than the same product
    in a grouped launch, and the property does not hold (with or without dynamic attention).  With
    dynamic attention the lock step launches the one product whose bits depend on its launch partners (the dGELU
    input gradient with fused bias column sums) on its own (BertLayerOp.bwd_steps exact)."""
    (g, flat0, _, _, _, _), (_, flat1, _, _, _, _) = _lock_step_runs(case, dev)
    dg = (flat0 - flat1).abs()
    print("paired vs unpaired", case, "grad max abs diff", float(dg.max()), "of max", float(flat0.abs().max()),
          "differing elements", int((dg != 0).sum()), "of", dg.numel())
    assert torch.equal(flat0, flat1)


def test_bf16_engine_close_to_reference_golden(dev):
    """The common bf16 bars of tests/test_gpu_parity.py on da_bs2, as tests/test_gpu_text_only.py applies them to
    its bs2 case; the gate GEMM and z stay fp32, the pool reads the bf16 text rows."""
    from test_gpu_parity import (BF16_LOSS_RTOL, BF16_GRAD_COS, BF16_GRAD_NORM_RTOL, BF16_GLOBAL_COS, BF16_LOGIT_RTOL,
                                 BF16_LOGIT_MEAN, BF16_LOGIT_P99, BF16_LOGIT_COLMEAN, BF16_LSE_ATOL)
    case = "da_bs2"
    g, _, G, out, got, _ = _run_case(case, dev, "bf16")
    rel = np.abs(got - g["losses"]) / np.maximum(np.abs(g["losses"]), 1e-3)
    print("bf16 loss rel err", case, rel)
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
    check_logits(g, out["mlm_logits"].cpu().numpy(), g["logit/img_rows"], BF16_LOGIT_RTOL, case + " bf16",
                 mean_rtol=BF16_LOGIT_MEAN, p99=BF16_LOGIT_P99, col_mean=BF16_LOGIT_COLMEAN, lse_atol=BF16_LSE_ATOL)
    check_img_logits(g, out["img_logits"].cpu().numpy(), BF16_LOGIT_RTOL, case + " bf16", mean_rtol=BF16_LOGIT_MEAN,
                     p99=BF16_LOGIT_P99, col_mean=BF16_LOGIT_COLMEAN)
    assert (rel <= BF16_LOSS_RTOL).all(), (got, g["losses"])
    assert not bad, bad
    assert gcos >= BF16_GLOBAL_COS, gcos
    for n in dy_names(_RUNS[(case, "bf16", False)][5].fp):
        assert float(G[n].abs().max()) > 0.0, n


@pytest.mark.parametrize("case,npairs", [("da_ce", 1), ("da_ce_bs2", 2)])
def test_item_alignment_matches_reference_golden(dev, case, npairs):
    """golden_ft_da_ce (ONE pair: the reference runs each item as a batch of one, the engine's stacked batch holds
    two sequences and a gate GEMM four pools) and golden_ft_da_ce_bs2 (two pairs) at the bars of
    tests/test_gpu_finetune.py."""
    from k3m_amd.config import finetune_config
    from k3m_amd.finetune import ARG_NAMES, K3MForItemAlignment
    from k3m_amd.weights import param_values
    g = load_ft_case(case)
    d = abs(float(g["loss_without_flag"]) - float(g["out/loss"]))       # not blind: 10x the loss's own bar
    assert d > 10 * (1e-3 * abs(float(g["loss_without_flag"])) + 1e-4), d
    g["out/coll_image_feat_1"] = g["out/coll_image_feat_1"].astype(np.float32)   # stored as fp16
    g["out/coll_image_feat_2"] = g["out/coll_image_feat_2"].astype(np.float32)
    cfg = finetune_config(CFG_PATH, loss_type="ce", if_pre_sampling=1, dynamic_attention=True)
    model = K3MForItemAlignment(cfg, dev)
    assert model.engine.dyn_attn
    model.engine.fp.load(param_values(cfg, int(g["weight_seed"]), std=float(g["weight_std"])))
    pair = {k: v.to(dev) for k, v in ft_pair(g).items()}
    assert pair["input_ids_1"].shape[0] == npairs
    n1, n2 = ft_noise(g)
    ns = float(g["noise_scale"])
    noise = ({k: (v * ns).to(dev) for k, v in n1.items()}, {k: (v * ns).to(dev) for k, v in n2.items()})
    e1, e2, probs, loss = model(*[pair[k] for k in ARG_NAMES], train=False, noise=noise)
    model.backward()
    torch.cuda.synchronize()
    print("ft da_ce loss", float(loss), float(g["out/loss"]), "without the flag", float(g["loss_without_flag"]))
    np.testing.assert_allclose(float(loss), float(g["out/loss"]), rtol=1e-3, atol=1e-5)
    np.testing.assert_allclose(e1.cpu().numpy(), g["out/e1"], rtol=1e-3, atol=1e-4)
    np.testing.assert_allclose(e2.cpu().numpy(), g["out/e2"], rtol=1e-3, atol=1e-4)
    np.testing.assert_allclose(probs.cpu().numpy(), g["out/probs"], rtol=1e-3, atol=1e-5)
    G = model.engine.fp.g
    for k in g:
        kind, _, n = k.partition("/")
        if kind in ("grad_full", "grad_sub", "grad_rows"):
            ref = g[k]
            gr = G[n]
            gr = gr[::16, ::16] if kind == "grad_sub" else torch.cat([gr[:2], gr[-2:]]) if kind == "grad_rows" else gr
            err = np.abs(gr.cpu().numpy() - ref).max()
            assert err <= 5e-3 * np.abs(ref).max() + 1e-6, (n, err, np.abs(ref).max())
    dyn, worst = 0, (0.0, None)
    for n, ref in zip(list(g["grad_norm_names"]), g["grad_norms"]):
        gn = float(G[n].double().norm())
        if np.isnan(ref):
            assert gn == 0.0, n
        else:
            assert abs(gn - ref) <= 5e-3 * ref + 1e-6, (n, gn, ref)
            dyn += "dyLinear" in str(n)
            if ref > 1e-4:      # where the absolute term is under 1 % of the bar
                worst = max(worst, (abs(gn - ref) / ref, str(n)))
    print("ft", case, "worst gradient-norm error among norms > 1e-4: %.2e %s" % worst)
    assert dyn == 24


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_trainer_learns_and_moves_every_gate(dev, dtype):
    """Three train-mode steps (dropout, device gumbel noise and negatives, AdamW) at batch 2: finite losses, the
    summed loss goes down, every dyLinear_* tensor changes; the step is not captured into a graph."""
    from k3m_amd.engine import label_counts
    from k3m_amd.synthetic import synthetic_batch
    from k3m_amd.trainer import Trainer
    cfg = da_config()
    tr = Trainer(cfg, dev, lr=2e-4, warmup_steps=0, total_steps=100, seed=3, dtype=dtype)
    tr.graph = True    # asked for, but the step with dynamic attention is not eligible: eager
    assert tr.dropout
    batch = synthetic_batch(cfg, 2, dev, seed=5)
    batch["_label_counts"] = label_counts(batch)
    fp = tr.engine.fp
    start = {n: fp.p[n].clone() for n in dy_names(fp)}
    assert len(start) == 24
    losses = [float(tr.step(batch)["loss"]) for _ in range(3)]
    tr.finish()
    torch.cuda.synchronize()
    print("dynamic attention trainer", dtype, losses)
    assert all(np.isfinite(losses)), losses
    assert losses[-1] < losses[0], losses
    assert tr._graphs is None or tr._graphs.captures == 0
    for n, v in start.items():
        assert not torch.equal(fp.p[n], v), n
        assert bool(torch.isfinite(fp.p[n]).all()), n


# the first-step loss of the model WITHOUT the flag, measured on the commit before this feature (MI355X, fp32,
# Trainer(seed=3), synthetic_batch(cfg, 2, seed=5), train mode): the flag off changes no launch
PARENT_FIRST_LOSS = "0x1.5fc78a0000000p+4"   # 21.986215591430664


def test_flag_off_first_step_loss_is_the_parents(dev):
    from k3m_amd.synthetic import synthetic_batch
    from k3m_amd.trainer import Trainer
    cfg = da_config(dyn=False)
    tr = Trainer(cfg, dev, lr=2e-4, warmup_steps=0, total_steps=100, seed=3)
    assert not tr.engine.dyn_attn and not dy_names(tr.engine.fp)
    loss = float(tr.step(synthetic_batch(cfg, 2, dev, seed=5))["loss"])
    tr.finish()
    print("flag-off first-step loss", loss.hex(), loss)
    assert loss.hex() == PARENT_FIRST_LOSS, (loss, loss.hex())


# ---------------------------------------------------------------- train.py --dynamic_attention
def test_train_py_dynamic_attention_loader_loop_with_eval_and_reload(tmp_path):
    """Raw product rows through the native loader (char tokenizer, synthetic regions), train mode, two steps and the
    evaluation pass with the flag; the checkpoint holds the 24 gate tensors, reloads into a Trainer built with the
    flag and is refused by one built without it."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
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
                        "--dynamic_attention", "--train_batch_size", "3", "--eval_batch_size", "3",
                        "--num_train_epochs", "1", "--seed", "42", "--k3m_char_tokenizer", "--k3m_synthetic_regions",
                        "3", "--k3m_loss_log", str(log)], cwd=str(tmp_path), capture_output=True, text=True,
                       timeout=400)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    steps = [json.loads(l) for l in log.read_text().splitlines()]
    assert len(steps) == 2 and all(np.isfinite(s[k]) for s in steps for k in LOSS_KEYS), steps
    assert "[Eval] [Epoch-0] loss:" in r.stderr
    ck_dir = out / "k3m_bert-base-uncased_12l_12h"
    tar = str(ck_dir / "K3M_struc_presample-1_epoch-0.tar")
    sd = torch.load(str(ck_dir / "K3M_struc_presample-1_epoch-0.bin"), map_location="cpu", weights_only=True)
    assert len(sd) == 1023 and len([k for k in sd if ".dyLinear_" in k]) == 24
    assert all(bool(torch.isfinite(v).all()) for v in sd.values())
    from k3m_amd.trainer import Trainer
    dev = torch.device("cuda")
    tr = Trainer(da_config(), dev, lr=1e-4, warmup_steps=0, total_steps=2, seed=42, init=True)
    start = {n: tr.engine.fp.p[n].clone() for n in dy_names(tr.engine.fp)}
    assert tr.load_checkpoint(tar) == 2
    for n, v in start.items():   # the run's start weights were these (same seed): step 2 (lr > 0) moved the gates
        assert torch.equal(tr.engine.fp.p[n].cpu(), sd[n]) and not torch.equal(tr.engine.fp.p[n], v), n
    del tr
    plain = Trainer(da_config(dyn=False), dev, lr=1e-4, warmup_steps=0, total_steps=2, seed=42, init=True)
    before = plain.engine.fp.data.clone()
    with pytest.raises(ValueError, match="built without dynamic_attention"):
        plain.load_checkpoint(tar)
    assert torch.equal(plain.engine.fp.data, before)
