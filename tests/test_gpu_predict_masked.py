"""K3MEngine.predict_masked on the GPU: against the reference's own predictions
(tests/golden/golden_masked_prediction.npz, recorded from the bs2_hard case), against the engine's own captured
logits, across the row-selection modes, the model variants, the bf16 engine and the train.py driver.

tol = 1e-3 x the row's largest |logit| is the bar tests/test_gpu_parity.py puts on these logits; a position is
checked for index equality only where the fixture's float64 logit is more than 2 tol from both ranking neighbours
(make_masked_prediction_golden.checkable: 392 of 530 token positions at k = 10, 67 of 70 region positions at k = 5)."""
import json
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest
import torch

from golden_util import CFG_PATH, HERE, REPO, load_case, case_batch, case_noise

sys.path.insert(0, os.path.join(HERE, "golden"))
import make_masked_prediction_golden as M  # noqa: E402

pytestmark = pytest.mark.gpu
CASE = "bs2_hard"
LABEL_KEYS = ("lm_label_ids", "lm_label_ids_pv", "image_label", "image_target")


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda")


@pytest.fixture(scope="module")
def fix():
    d = np.load(os.path.join(HERE, "golden", "golden_masked_prediction.npz"), allow_pickle=False)
    return {k: d[k] for k in d.files}


_ENG = {}


def _engine(dev, dtype="fp32", **kw):
    """(engine, golden, batch, noise) of the bs2_hard case under the config switches kw; one engine at a time"""
    from k3m_amd.config import pretrain_config
    from k3m_amd.engine import K3MEngine
    from k3m_amd.weights import param_values
    key = (dtype,) + tuple(sorted(kw.items()))
    if key not in _ENG:
        _ENG.clear()
        g = load_case(CASE)
        cfg = pretrain_config(CFG_PATH, if_pre_sampling=int(g["mode"]), **kw)
        eng = K3MEngine(cfg, dev, dtype=dtype)
        eng.fp.load(param_values(cfg, int(g["weight_seed"])))
        batch = {k: v.to(dev) for k, v in case_batch(g).items()}
        noise = {k: v.to(dev) for k, v in case_noise(g).items()}
        if not cfg.use_image:   # two candidates per position, no image field
            rng = np.random.default_rng(int(g["noise_seed"]))
            B, T = batch["input_ids"].shape
            P = batch["input_ids_pv"].shape[1]
            noise = {k: torch.from_numpy((-np.log(rng.standard_exponential(s))).astype(np.float32)).to(dev)
                     for k, s in [("t", (B, T, 2, 768)), ("pv", (B, P, 2, 768))]}
            batch = {k: v for k, v in batch.items() if not k.startswith("image_")}
        _ENG[key] = (eng, g, batch, noise)
    eng = _ENG[key][0]
    eng.fp.grad.zero_()
    return _ENG[key]


def _np(r):
    return {k: v.cpu().numpy() for k, v in r.items()}


def _tokens(res):
    """title rows then PV rows of a result, as numpy"""
    t, pv = _np(res["t"]), _np(res["pv"])
    return {k: np.concatenate([t[k], pv[k]]) for k in t}


def _check_against_fixture(got, top_id, top_logit, scale, k_check, what):
    """got: {idx, logprob, lse} [n, k] numpy.  Every returned id inside the fixture's top-64 and its logit within tol;
    no fixture entry better than the returned k-th by more than 2 tol missing; the index equal at every checkable
    position of the first k_check."""
    idx, score = got["idx"], got["logprob"].astype(np.float64) + got["lse"].astype(np.float64)[:, None]
    n, k = idx.shape
    tol = 1e-3 * scale.astype(np.float64)
    ok = M.checkable(top_logit, scale, k_check)
    worst = 0.0
    for i in range(n):
        where = {int(j): p for p, j in enumerate(top_id[i])}
        for p in range(k):
            assert int(idx[i, p]) in where, (what, i, p, "outside the fixture's top-64")
            err = abs(score[i, p] - float(top_logit[i, where[int(idx[i, p])]]))
            worst = max(worst, err / tol[i])
            assert err <= tol[i], (what, i, p, err, tol[i])
        kth = score[i, k - 1]
        have = set(int(j) for j in idx[i])
        for p in range(top_id.shape[1]):
            if float(top_logit[i, p]) > kth + 2 * tol[i]:
                assert int(top_id[i, p]) in have, (what, i, p, "a better entry is missing")
        for p in range(k_check):
            if ok[i, p]:
                assert idx[i, p] == top_id[i, p], (what, i, p)
    print("%s: worst logit error %.3g tol; %d of %d positions checked for the index" % (what, worst, int(ok.sum()), ok.size))


def _own_reference(logits, hl, W):
    """(s [n, v] float64 of the engine's captured logits, order, tol = 1e-5 |h| |e|)"""
    s = logits.double().cpu().numpy()
    tol = 1e-5 * hl.double().norm(dim=1).cpu().numpy()[:, None] * W.double().norm(dim=1).cpu().numpy()[None, :]
    order = np.stack([np.lexsort((np.arange(s.shape[1]), -s[i])) for i in range(s.shape[0])])
    return s, order, tol


def _check_against_own(got, s, order, tol, what):
    idx, score = got["idx"], got["logprob"].astype(np.float64) + got["lse"].astype(np.float64)[:, None]
    n, k = idx.shape
    skipped = 0
    for i in range(n):
        # (+ 2e-6: logprob = score - lse was rounded to fp32 at |lse| ~ 10, two ulps of which are 1.9e-6)
        assert np.all(np.abs(score[i] - s[i, idx[i]]) <= tol[i, idx[i]] + 2e-6), (what, i)
        rs, rt = s[i, order[i, :k + 1]], tol[i, order[i, :k + 1]]
        for p in range(k):
            t = max(rt[max(p - 1, 0)], rt[p], rt[p + 1])
            if (p == 0 or rs[p - 1] - rs[p] > t) and rs[p] - rs[p + 1] > t:
                assert idx[i, p] == order[i, p], (what, i, p)
            else:
                skipped += 1
    print("%s: %d of %d positions under the gap" % (what, skipped, n * k))
    return skipped


def _captured(eng, g, batch, noise):
    eng.capture_logits = True
    try:
        out, ctx = eng.forward(batch, train=False, noise=noise, ent_neg=torch.from_numpy(g["ent_neg"]),
                               val_neg=torch.from_numpy(g["val_neg"]))
    finally:
        eng.capture_logits = False
    return out, ctx


# ---------------------------------------------------------------- the reference's predictions
def test_fp32_engine_against_the_fixture(dev, fix):
    eng, g, batch, noise = _engine(dev)
    res = eng.predict_masked(batch, k=10, rows="labels", noise=noise)
    torch.cuda.synchronize()
    assert set(res) == {"t", "pv", "v"}
    nt = int(fix["tok/n_title"])
    tok = _tokens(res)
    assert res["t"]["idx"].shape == (nt, 10) and tok["idx"].shape == (53, 10)
    assert np.array_equal(tok["pos"], fix["tok/pos"]) and np.array_equal(tok["gold"], fix["tok/gold"])
    _check_against_fixture(tok, fix["tok/top_id"], fix["tok/top_logit"], fix["tok/scale"], 10, "tokens")
    np.testing.assert_allclose(tok["lse"], g["logit/mlm_lse"], rtol=1e-3, atol=1e-3)
    np.testing.assert_allclose(tok["gold_logprob"], g["logit/mlm_label"] - g["logit/mlm_lse"], rtol=1e-3, atol=1e-3)
    v = _np(res["v"])
    assert np.array_equal(v["pos"], fix["reg/pos"]) and np.array_equal(v["gold"], fix["reg/gold"])
    _check_against_fixture(v, fix["reg/top_id"], fix["reg/top_logit"], fix["reg/scale"], 5, "regions")
    rows = g["logit/img_rows"].astype(np.float64)
    m = rows.max(1)
    lse = m + np.log(np.exp(rows - m[:, None]).sum(1))
    np.testing.assert_allclose(v["lse"], lse, rtol=1e-3, atol=1e-3)
    np.testing.assert_allclose(v["gold_logprob"], rows[np.arange(len(lse)), fix["reg/gold"]] - lse, rtol=1e-3, atol=1e-3)


# ---------------------------------------------------------------- the engine's own logits
@pytest.mark.parametrize("variant", ["full", "no_image", "no_coattention"])
def test_against_the_engines_own_logits(dev, variant):
    kw = {"full": {}, "no_image": {"use_image": False}, "no_coattention": {"with_coattention": False}}[variant]
    eng, g, batch, noise = _engine(dev, **kw)
    out, ctx = _captured(eng, g, batch, noise)
    res = eng.predict_masked(batch, k=10, rows="labels", noise=noise)
    torch.cuda.synchronize()
    tok = _tokens(res)
    hl = ctx["mlm"][4]
    s, order, tol = _own_reference(out["mlm_logits"], hl, eng.fp.p["embeddings.word_embeddings.weight"])
    skipped = _check_against_own(tok, s, order, tol, variant + " tokens")
    assert skipped <= 0.05 * tok["idx"].size
    for name, key in (("t", "masked_lm_loss"), ("pv", "masked_lm_loss_pv")):
        nll = float(-res[name]["gold_logprob"].double().mean())
        print(variant, key, float(out[key]), "mean -gold_logprob", nll)
        assert nll == pytest.approx(float(out[key]), rel=1e-5)
    if variant == "no_image":
        assert "v" not in res and "img_logits" not in out
    else:
        s, order, tol = _own_reference(out["img_logits"], ctx["img"][4], eng.fp.p["cls.imagePredictions.decoder.weight"])
        _check_against_own(_np(res["v"]), s, order, tol, variant + " regions")
    del ctx


# ---------------------------------------------------------------- row-selection modes, determinism
def test_mask_mode_and_explicit_positions_equal_labels_mode(dev, fix):
    eng, g, batch, noise = _engine(dev)
    lab = eng.predict_masked(batch, k=10, rows="labels", noise=noise)
    bare = {k: v for k, v in batch.items() if k not in LABEL_KEYS}
    msk = eng.predict_masked(bare, k=10, rows="mask", noise=noise)   # no label field to read
    torch.cuda.synchronize()
    assert set(msk) == {"t", "pv"} and "gold" not in msk["t"]
    assert np.array_equal(msk["t"]["pos"].cpu().numpy(), fix["mask/t"])
    assert np.array_equal(msk["pv"]["pos"].cpu().numpy(), fix["mask/pv"])
    for name in ("t", "pv"):
        at = {tuple(p): i for i, p in enumerate(lab[name]["pos"].tolist())}
        sel = torch.tensor([at[tuple(p)] for p in msk[name]["pos"].tolist()], device=dev)
        assert len(sel) > 0
        for key in ("idx", "logprob", "lse"):
            assert torch.equal(msk[name][key], lab[name][key][sel]), (name, key)
    with_v = eng.predict_masked({**bare, "image_label": batch["image_label"]}, k=10, rows="mask", noise=noise)
    assert torch.equal(with_v["v"]["idx"], lab["v"]["idx"]) and "gold" not in with_v["v"]
    # explicit positions: those of the labels
    rows = {name: lab[name]["pos"].clone() for name in ("t", "pv", "v")}
    exp = eng.predict_masked(batch, k=10, rows=rows, noise=noise)
    torch.cuda.synchronize()
    for name in ("t", "pv", "v"):
        assert set(exp[name]) == set(lab[name])
        for key in lab[name]:
            assert torch.equal(exp[name][key], lab[name][key]), (name, key)
    with pytest.raises(ValueError):
        eng.predict_masked(batch, rows={"t": torch.tensor([[0, 99]])})
    with pytest.raises(ValueError):
        eng.predict_masked(batch, rows="everything")
    with pytest.raises(ValueError):
        eng.predict_masked(batch, k=33)


def test_same_seed_same_bits(dev):
    eng, g, batch, _ = _engine(dev)
    a = eng.predict_masked(batch, k=5, seed=17)   # the gumbel draw comes from the seed
    b = eng.predict_masked(batch, k=5, seed=17)
    torch.cuda.synchronize()
    for name in a:
        for key in a[name]:
            assert torch.equal(a[name][key], b[name][key]), (name, key)


# ---------------------------------------------------------------- no training state
def test_gradients_untouched_and_pending_ctx_survives(dev):
    from k3m_amd import ops
    eng, g, batch, noise = _engine(dev)
    old = ops.DETERMINISTIC
    ops.set_deterministic(True)   # the fixed-order backward sums: two backward passes of one ctx give the same bits
    try:
        out, ctx = _captured(eng, g, batch, noise)
        eng.backward(ctx)
        want = eng.fp.grad.clone()
        eng.fp.grad.zero_()
        out, ctx = _captured(eng, g, batch, noise)
        eng.predict_masked(batch, k=10, noise=noise)
        assert not bool(eng.fp.grad.any())
        eng.backward(ctx)
        torch.cuda.synchronize()
        assert bool(want.any()) and torch.equal(eng.fp.grad, want)
    finally:
        ops.set_deterministic(old)
        eng.fp.grad.zero_()


# ---------------------------------------------------------------- variants without a region head
def test_visual_target_1_has_no_region_stream(dev):
    eng, g, batch, noise = _engine(dev, visual_target=1)
    res = eng.predict_masked(batch, k=5, noise=noise)
    torch.cuda.synchronize()
    assert set(res) == {"t", "pv"} and res["t"]["idx"].shape[1] == 5
    assert bool(torch.isfinite(res["pv"]["logprob"]).all())


def test_item_alignment_engine_raises(dev):
    from k3m_amd.config import finetune_config
    from k3m_amd.engine import K3MEngine
    _ENG.clear()
    eng = K3MEngine(finetune_config(CFG_PATH, loss_type="ce"), dev)
    with pytest.raises(ValueError):
        eng.predict_masked({})


# ---------------------------------------------------------------- bf16 encoder
def test_bf16_engine_against_the_fixture(dev, fix):
    from test_gpu_parity import BF16_LOGIT_RTOL, BF16_LSE_ATOL
    eng, g, batch, noise = _engine(dev, dtype="bf16")
    res = eng.predict_masked(batch, k=10, noise=noise)
    torch.cuda.synchronize()
    tok = _tokens(res)
    lse_err = np.abs(tok["lse"] - g["logit/mlm_lse"]).max()
    gold = tok["gold_logprob"].astype(np.float64) + tok["lse"]
    gold_err = (np.abs(gold - g["logit/mlm_label"]) / fix["tok/scale"]).max()
    print("bf16: lse error %.3g (bar %.3g), gold logit error %.3g of the row scale (bar %.3g)"
          % (lse_err, BF16_LSE_ATOL, gold_err, BF16_LOGIT_RTOL))
    assert lse_err <= BF16_LSE_ATOL and gold_err <= BF16_LOGIT_RTOL
    assert np.array_equal(tok["pos"], fix["tok/pos"]) and set(res) == {"t", "pv", "v"}


# ---------------------------------------------------------------- train.py --do_eval --k3m_eval_topk
def test_train_py_eval_topk(tmp_path):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    _ENG.clear()
    torch.cuda.empty_cache()
    out = tmp_path / "out"
    out.mkdir()
    shutil.copy(CFG_PATH, out / "bert_base_6layer_6conect.json")
    rows = []
    for i in range(4):
        pv = "#;#".join("p%d%d#:#v%d%d" % (i, j, j, i) for j in range(3 + i))
        rows.append("%d\titem title %d with words\thttp://img/%d.jpg\t%s\tcat" % (1000 + i, i, i, pv))
    for name in ("rows_train+valid.tsv", "rows_valid.tsv"):
        (tmp_path / name).write_text("\n".join(rows) + "\n", encoding="utf-8")
    pred = tmp_path / "pred.jsonl"

    def run(extra, log):
        try:
            r = subprocess.run([sys.executable, os.path.join(REPO, "train.py"), "--data_dir", str(tmp_path),
                                "--output_dir", str(out), "--file_name", "rows_{}.tsv", "--do_train", "--do_eval",
                                "--with_coattention", "--train_batch_size", "2", "--eval_batch_size", "2",
                                "--num_train_epochs", "1", "--seed", "42", "--k3m_char_tokenizer",
                                "--k3m_synthetic_regions", "3", "--k3m_max_steps", "1", "--k3m_loss_log", str(log)] + extra,
                               cwd=str(tmp_path), capture_output=True, text=True, timeout=400,
                               env=dict(os.environ, K3M_DETERMINISTIC="1"))   # fixed-order backward sums
        finally:
            # the epoch's checkpoint (.bin and .tar with the optimizer state, several GB for the tri-modal fp32 model)
            # is not what this test is about: it must not stay on the disk for the rest of the session
            shutil.rmtree(str(out / "k3m_bert-base-uncased_12l_12h"), ignore_errors=True)
        assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
        ev = [re.sub(r"^.*\[Eval\]", "[Eval]", ln) for ln in r.stderr.splitlines() if "[Eval] [Epoch-0]" in ln]
        return ev, [json.loads(ln) for ln in log.read_text().splitlines()]
    ev, steps = run(["--k3m_eval_topk", "5", "--k3m_pred_output", str(pred)], tmp_path / "a.jsonl")
    acc = [ln for ln in ev if " acc@1: " in ln]
    assert [ln.split()[2] for ln in acc] == ["title", "pv", "region"], ev
    assert all(" acc@5: " in ln and " nll: " in ln for ln in acc)
    lines = [json.loads(ln) for ln in pred.read_text().splitlines()]
    n_rows = sum(int(ln.rsplit("rows: ", 1)[1]) for ln in acc)
    assert len(lines) == n_rows > 0
    assert {ln["stream"] for ln in lines} == {"t", "pv", "v"}
    assert all(len(ln["topk"]) == 5 and ln["gold"] is not None and str(ln["item_id"]) in ("1000", "1001", "1002", "1003")
               for ln in lines)
    # without the option: the parent's output
    ev0, steps0 = run([], tmp_path / "b.jsonl")
    assert ev0 == [ln for ln in ev if " acc@1: " not in ln] and len(ev0) == 2
    assert steps0 == steps
