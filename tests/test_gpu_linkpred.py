"""Link-prediction evaluation on the GPU: K3MEngine.triples, k3m_amd/linkpred.py and the train.py driver.

* triples against the CPU oracle (oracle.k3m_oracle.encode + structure_aggregator's endpoint means) on the bs2_hard
  and bs3_zero_triple goldens, fp32 at the bars tests/test_gpu_infer.py puts on c_final (rtol 1e-3, atol 1e-4); the
  bf16 engine at that file's bf16 bars, against its own eval-mode forward (test_bf16_triples says why);
* the text-only and no-co-attention models, for which the oracle has no encoder: c_final, p, v and nvalid against
  the engine's own eval-mode forward (bits without the stream dedup, the same bars with it);
* triples against the engine itself (the X buffer forward(train=False) keeps), no training state;
* rank_values / rank_entities against a float64 restatement over the pool's own vectors, by the list and rank rules
  of tests/test_gpu_lprank_kernels.py; filtered against raw ranking;
* train.py --do_eval --k3m_eval_lpm."""
import json
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest
import torch

from golden_util import CFG_PATH, REPO, case_batch, case_config, case_noise, load_case
import test_gpu_lprank_kernels as K

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda")


_ENG = {}


def _engine(dev, case, dtype="fp32"):
    """(engine, golden, batch, noise, weights) of a pretraining golden; one engine per dtype, one dtype at a time"""
    from k3m_amd.engine import K3MEngine
    from k3m_amd.weights import param_values
    g = load_case(case)
    cfg = case_config(g)
    if dtype not in _ENG:
        _ENG.clear()
        _ENG[dtype] = K3MEngine(cfg, dev, dtype=dtype)
    eng = _ENG[dtype]
    vals = param_values(cfg, int(g["weight_seed"]))
    eng.fp.load(vals)
    eng.fp.grad.zero_()
    eng.infer_dedup = True
    batch = {k: v.to(dev) for k, v in case_batch(g).items()}
    noise = {k: v.to(dev) for k, v in case_noise(g).items()}
    return eng, g, batch, noise, vals


_ORACLE = {}


def _oracle(case):
    """{c_final [B, H], p, v [B, NPV, H] (zero past nvalid), nvalid [B]} of the CPU oracle, computed once per case"""
    if case not in _ORACLE:
        from k3m_amd.weights import param_values
        from oracle import k3m_oracle as O
        g = load_case(case)
        cfg = case_config(g)
        P = {k: torch.from_numpy(v) for k, v in param_values(cfg, int(g["weight_seed"])).items()}
        batch, noise = case_batch(g), case_noise(g)
        with torch.no_grad():
            enc = O.encode(P, cfg, batch, noise)
            c_final, _ = O.structure_aggregator(P, enc["c_init"], enc["seq_pv"], batch["index_p"], batch["index_v"],
                                                None, None, 1.0)
        ip, iv = batch["index_p"], batch["index_v"]
        B, NPV = ip.shape[:2]
        H = c_final.shape[1]
        p, v = torch.zeros((B, NPV, H)), torch.zeros((B, NPV, H))
        nvalid = []
        for i in range(B):
            j = 0
            while j < NPV and int(ip[i, j, 0]) != 0:
                p[i, j] = enc["seq_pv"][i].index_select(0, ip[i, j]).mean(0)
                v[i, j] = enc["seq_pv"][i].index_select(0, iv[i, j]).mean(0)
                j += 1
            nvalid.append(j)
        _ORACLE[case] = {"c_final": c_final.numpy(), "p": p.numpy(), "v": v.numpy(), "nvalid": nvalid}
    return _ORACLE[case]


def _valid(t, nvalid):
    """the rows of the valid triples of a [B, NPV, H] array, item by item"""
    return np.concatenate([t[i, :n] for i, n in enumerate(nvalid)])


@pytest.mark.parametrize("case", ["bs2_hard", "bs3_zero_triple"])
def test_triples_against_the_oracle(dev, case):
    eng, g, batch, noise, _ = _engine(dev, case)
    ref = _oracle(case)
    got = eng.triples(batch, noise=noise)
    emb = eng.embed(batch, noise=noise)
    torch.cuda.synchronize()
    B, NPV = batch["index_p"].shape[:2]
    assert set(got) == {"c_final", "p", "v", "nvalid"}
    assert got["p"].shape == (B, NPV, eng.H) and got["v"].shape == (B, NPV, eng.H)
    assert got["nvalid"].dtype == torch.int32 and got["nvalid"].tolist() == ref["nvalid"]
    assert torch.equal(got["c_final"], emb["c_final"])
    for name in ("p", "v"):
        a, b = _valid(got[name].cpu().numpy(), ref["nvalid"]), _valid(ref[name], ref["nvalid"])
        print(case, name, "largest distance from the oracle %.3e of %.3e" % (np.abs(a - b).max(), np.abs(b).max()))
        np.testing.assert_allclose(a, b, rtol=1e-3, atol=1e-4)
    np.testing.assert_allclose(got["c_final"].cpu().numpy(), ref["c_final"], rtol=1e-3, atol=1e-4)
    if case == "bs3_zero_triple":   # the zero-triple item is an entity and asks no query
        from k3m_amd.linkpred import TriplePool, property_keys, value_keys
        assert ref["nvalid"][0] == 0
        pool = TriplePool()
        pool.add(got, (value_keys(batch), property_keys(batch)), ["a", "b", "c"])
        t = pool.tensors()
        assert pool.n_items == 3 and pool.n_triples == sum(ref["nvalid"]) and t["c_final"].shape[0] == 3
        assert int(t["item_row"].min()) == 1 and bool((t["value_key"] >= 0).all())


@pytest.mark.parametrize("case", ["bs2_hard", "bs3_zero_triple"])
def test_bf16_triples(dev, case):
    """The bf16 engine at tests/test_gpu_infer.py's bf16 bars, applied as that file applies them, to the bf16 engine's
    own eval-mode forward: without the stream dedup the bits of forward(train=False) (c_final, and p / v against the
    thirds of its X buffer); with it c_final within 2^-6 of the tensor's largest magnitude of the dedup-off value (the
    file's bar on the pooled outputs).  No element-wise bar against the fp32 oracle: the hard gate chooses one of three
    candidates per element, and bf16 rounding moves a near-tie to another candidate, which changes that element of a
    p / v row by the distance between two candidates.  Measured against the oracle (printed below): c_final within
    1.8e-2 of 1.47 (bs2_hard) and 2.2e-2 of 1.32 (bs3_zero_triple); the worst element of p 0.98 of 2.93."""
    eng, g, batch, noise, _ = _engine(dev, case, dtype="bf16")
    ref = _oracle(case)
    H = eng.H
    out, ctx = eng.forward(batch, train=False, noise=noise)
    X3 = ctx["struct"][0].view(batch["input_ids"].shape[0], -1, 3 * H).clone()
    want_cf = out["c_final"].clone()
    del ctx, out
    nv = ref["nvalid"]
    eng.infer_dedup = False
    off = eng.triples(batch, noise=noise)
    eng.infer_dedup = True
    on = eng.triples(batch, noise=noise)
    emb = eng.embed(batch, noise=noise)
    torch.cuda.synchronize()
    assert off["nvalid"].tolist() == nv == on["nvalid"].tolist()
    assert torch.equal(off["c_final"], want_cf) and torch.equal(on["c_final"], emb["c_final"])
    for name, lo in (("p", H), ("v", 2 * H)):
        assert off[name].dtype == torch.float32 and bool(torch.isfinite(on[name]).all())
        assert np.array_equal(_valid(off[name].cpu().numpy(), nv), _valid(X3[:, :, lo:lo + H].cpu().numpy(), nv)), name
    d, scale = float((on["c_final"] - off["c_final"]).abs().max()), float(off["c_final"].abs().max())
    print(case, "bf16 c_final: |dedup on - dedup off| %.3e of %.3e" % (d, scale))
    assert d <= 2.0 ** -6 * scale
    pairs = [("c_final", on["c_final"].cpu().numpy(), ref["c_final"])]
    pairs += [(n, _valid(on[n].cpu().numpy(), nv), _valid(ref[n], nv)) for n in "pv"]
    for name, a, b in pairs:
        err = np.abs(a - b)
        print(case, "bf16", name, "distance from the fp32 oracle: largest %.3e, mean %.3e, of %.3e"
              % (err.max(), err.mean(), np.abs(b).max()))


@pytest.mark.parametrize("case", ["to_ce", "noco_ce"])
def test_triples_of_the_text_only_and_no_coattention_models(dev, case):
    """The item-alignment goldens recorded without the image modality / without co-attention (the oracle encodes the
    full model only): c_final, p, v and nvalid against the engine's own eval-mode forward and its X buffer, the same
    bits without the stream dedup, tests/test_gpu_infer.py's bars with it (single items through the model class)."""
    import test_gpu_infer as I
    _ENG.clear()
    model, g, pair, noise = I._model(case, "fp32", dev)
    eng = model.engine
    batch, nz = I._stacked(model, pair, noise)
    H = eng.H
    out, ctx = eng.forward(batch, train=False, noise=nz, seed=3, groups=2)
    X, nvalid = ctx["struct"][0].clone(), ctx["struct"][1].clone()
    del ctx, out
    B = batch["input_ids"].shape[0]
    X3 = X.view(B, -1, 3 * H)
    nv = nvalid.tolist()
    eng.infer_dedup = False
    off = eng.triples(batch, noise=nz, seed=3, groups=2)
    assert off["nvalid"].tolist() == nv and sum(nv) > 0
    assert torch.equal(off["c_final"], eng.embed(batch, noise=nz, seed=3, groups=2)["c_final"])
    for name, lo in (("p", H), ("v", 2 * H)):   # (rows past nvalid are never written)
        assert np.array_equal(_valid(off[name].cpu().numpy(), nv), _valid(X3[:, :, lo:lo + H].cpu().numpy(), nv)), name
    eng.infer_dedup = True
    on = model.triples(**{k[:-2]: v for k, v in pair.items() if k.endswith("_1")}, noise=noise[0])
    torch.cuda.synchronize()
    half = B // 2
    assert on["nvalid"].tolist() == nv[:half]
    np.testing.assert_allclose(on["c_final"].cpu().numpy(), off["c_final"][:half].cpu().numpy(), rtol=1e-3, atol=1e-4)
    for name in ("p", "v"):
        a, b = _valid(on[name].cpu().numpy(), nv[:half]), _valid(off[name][:half].cpu().numpy(), nv[:half])
        np.testing.assert_allclose(a, b, rtol=1e-3, atol=1e-4, err_msg=name)
    I._MODELS.clear()


def test_triples_against_the_engines_own_forward_and_no_training_state(dev):
    from k3m_amd import ops
    eng, g, batch, noise, _ = _engine(dev, "bs2_hard")
    H = eng.H
    old = ops.DETERMINISTIC
    ops.set_deterministic(True)   # the fixed-order backward sums: two backward passes of one ctx give the same bits
    try:
        out, ctx = eng.forward(batch, train=False, noise=noise)
        X3 = ctx["struct"][0].view(batch["input_ids"].shape[0], -1, 3 * H)
        nv = ctx["struct"][1].tolist()
        eng.infer_dedup = False   # the launches of forward(train=False): the same bits
        off = eng.triples(batch, noise=noise)
        eng.infer_dedup = True    # one buffer per stream until the copies diverge: tests/test_gpu_infer.py's bars
        on = eng.triples(batch, noise=noise)
        assert off["nvalid"].tolist() == nv == on["nvalid"].tolist()
        for name, lo in (("p", H), ("v", 2 * H)):
            a, b = _valid(on[name].cpu().numpy(), nv), _valid(X3[:, :, lo:lo + H].cpu().numpy(), nv)
            assert np.array_equal(_valid(off[name].cpu().numpy(), nv), b), name   # (rows past nvalid: never written)
            print(name, "dedup on: largest distance from forward(train=False) %.3e of %.3e"
                  % (np.abs(a - b).max(), np.abs(b).max()))
            np.testing.assert_allclose(a, b, rtol=1e-3, atol=1e-4, err_msg=name)
        eng.backward(ctx)
        want = eng.fp.grad.clone()
        eng.fp.grad.zero_()
        out, ctx = eng.forward(batch, train=False, noise=noise)
        eng.triples(batch, noise=noise)
        assert not bool(eng.fp.grad.any())
        eng.backward(ctx)
        torch.cuda.synchronize()
        assert bool(want.any()) and torch.equal(eng.fp.grad, want)
    finally:
        ops.set_deterministic(old)
        eng.fp.grad.zero_()


def _pool_reference(q, c, gold, gid, sign=1.0):
    return K._reference(q, c, gold, gid, gid, sign=sign)


def _check_ranking(res, q, c, gold, gid, k, what):
    """a rank_values / rank_entities result against float64 over the same stored vectors"""
    ref = _pool_reference(q, c, gold, gid)
    d2 = (res["dist"].double() ** 2).cpu().numpy()
    gold_d2 = (res["gold_dist"].double() ** 2).cpu().numpy()
    idx, rank = res["idx"].cpu().numpy(), res["rank"].cpu().numpy()
    # the square root and its square move a distance by a few ulp: the list rule's own bar on d2 covers it
    skipped, total = K._check_list(d2, idx, ref, k)
    loose = K._check_rank(rank, gold_d2, gold, ref)
    print("%s: index check skipped %d of %d positions, ranks with lo != hi: %d of %d"
          % (what, skipped, total, loose, len(rank)))
    for i in range(len(rank)):
        if 1 <= rank[i] <= k:
            assert idx[i, rank[i] - 1] == gold[i] and res["dist"][i, rank[i] - 1] == res["gold_dist"][i]
    return ref


def test_rankings_over_a_pool_of_two_batches(dev):
    from k3m_amd import linkpred as LP
    k = 32
    pool = LP.TriplePool()
    twins = None
    for case, ids in (("bs2_hard", [10, 11]), ("bs3_zero_triple", ["x", "y", "z"])):
        eng, g, batch, noise, _ = _engine(dev, case)
        if case == "bs2_hard":
            # one value occurs twice: the tokens (and their labels) of a value span of item 0 also stand in a span of
            # the same length of item 1
            iv = batch["index_v"].cpu()
            a0, a1 = int(iv[0, 0, 0]), int(iv[0, 0, 1])
            j1 = next(j for j in range(10) if int(iv[1, j, 1] - iv[1, j, 0]) == a1 - a0)
            b0 = int(iv[1, j1, 0])
            batch = {k_: v.clone() for k_, v in batch.items()}
            for name in ("input_ids_pv", "lm_label_ids_pv"):
                batch[name][1, b0:b0 + a1 - a0 + 1] = batch[name][0, a0:a1 + 1]
            twins = (0, 4 + j1)   # rows of the pool: item 0 holds 4 triples
        pool.add(eng.triples(batch, noise=noise), (LP.value_keys(batch), LP.property_keys(batch)), ids)
    t = pool.tensors()
    n = pool.n_triples
    assert n == 32 and pool.n_items == 5 and pool.item_ids == [10, 11, "x", "y", "z"]
    vk = t["value_key"].cpu().numpy()
    assert vk[twins[0]] == vk[twins[1]]
    dup = np.array([int((vk == x).sum()) > 1 for x in vk])
    assert dup.sum() == 2 and dup[list(twins)].all()
    cf, p, v = (t[name].cpu().numpy() for name in ("c_final", "p", "v"))
    item = t["item_row"].cpu().numpy()
    qv = (t["c_final"][t["item_row"]] + t["p"]).cpu().numpy()   # the op's own fp32 queries
    qe = (t["v"] - t["p"]).cpu().numpy()
    own = np.arange(n, dtype=np.int64)
    filt = LP.rank_values(pool, k)
    raw = LP.rank_values(pool, k, filtered=False)
    ent = LP.rank_entities(pool, k)
    torch.cuda.synchronize()
    _check_ranking(filt, qv, v, own, vk, k, "values, filtered")
    _check_ranking(raw, qv, v, own, None, k, "values, raw")
    _check_ranking(ent, qe, cf, item, None, k, "entities")
    assert ent["idx"].shape == (n, k) and bool((ent["idx"][:, 5:] == -1).all()) and bool((ent["idx"][:, :5] >= 0).all())
    # filtered against raw: the same bits except on the two triples whose value occurs twice, which lose each other
    for i in range(n):
        same = all(torch.equal(filt[name][i], raw[name][i]) for name in ("rank", "gold_dist", "idx", "dist"))
        assert same != bool(dup[i]), i
    for a, b in (twins, twins[::-1]):
        assert b in raw["idx"][a].tolist() and b not in filt["idx"][a].tolist()
        assert int(filt["rank"][a]) <= int(raw["rank"][a])
    # farthest first reverses the order of the distances
    far = LP.rank_values(pool, k, farthest=True, filtered=False)
    assert bool((far["dist"][:, :-1] >= far["dist"][:, 1:]).all())
    m = LP.link_metrics(filt["rank"], ks=(1, 3, 10))
    assert m["n"] == n and m["skipped"] == 0 and 1.0 <= m["mr"] <= n and 0.0 < m["mrr"] <= 1.0


def test_link_eval_file(dev, tmp_path):
    from k3m_amd import linkpred as LP
    eng, g, batch, noise, _ = _engine(dev, "bs3_zero_triple")
    path = tmp_path / "lpm.jsonl"
    ev = LP.LinkEval(3, str(path))
    ev.add(eng, batch, [7, 8, 9], noise=noise)
    ev.close()
    s = ev.summary()
    assert set(s) == {"value", "entity"} and ev.ks == (1, 3)
    lines = [json.loads(ln) for ln in path.read_text().splitlines()]
    assert len(lines) == 18 == s["value"]["n"] == s["entity"]["n"]
    assert {ln["item_id"] for ln in lines} == {8, 9}
    assert all(1 <= ln["value_rank"] <= 18 and 1 <= ln["entity_rank"] <= 3 and len(ln["value_topk"]) == 3
               and all(a in (8, 9) for a, _ in ln["value_topk"]) for ln in lines)
    for m in s.values():
        assert m["gold_dist"] >= m["top1_dist"] > 0.0 and 0.0 <= m["hits@1"] <= m["hits@3"] <= 1.0


# ---------------------------------------------------------------- train.py --do_eval --k3m_eval_lpm
def test_train_py_eval_lpm(tmp_path):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    _ENG.clear()
    torch.cuda.empty_cache()
    out = tmp_path / "out"
    out.mkdir()
    shutil.copy(CFG_PATH, out / "bert_base_6layer_6conect.json")
    rows = []
    for i in range(4):   # the four raw rows of tests/test_gpu_predict_masked.py's driver test: 3 + i triples each
        pv = "#;#".join("p%d%d#:#v%d%d" % (i, j, j, i) for j in range(3 + i))
        rows.append("%d\titem title %d with words\thttp://img/%d.jpg\t%s\tcat" % (1000 + i, i, i, pv))
    for name in ("rows_train+valid.tsv", "rows_valid.tsv"):
        (tmp_path / name).write_text("\n".join(rows) + "\n", encoding="utf-8")
    lpm = tmp_path / "lpm.jsonl"

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
            shutil.rmtree(str(out / "k3m_bert-base-uncased_12l_12h"), ignore_errors=True)   # the epoch's checkpoint
        assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
        ev = [re.sub(r"^.*\[Eval\]", "[Eval]", ln) for ln in r.stderr.splitlines() if "[Eval] [Epoch-0]" in ln]
        return ev, [json.loads(ln) for ln in log.read_text().splitlines()]
    ev, steps = run(["--k3m_eval_lpm", "3", "--k3m_lpm_output", str(lpm)], tmp_path / "a.jsonl")
    n = sum(3 + i for i in range(4))
    mine = [ln for ln in ev if " mr: " in ln or " gold distance: " in ln]
    assert [ln.split()[2] for ln in mine] == ["value", "value", "entity", "entity"], ev
    for ln in mine[0::2]:
        assert all(" %s: " % key in ln for key in ("mr", "mrr", "hits@1", "hits@3")) and ln.endswith(" n: %d" % n), ln
    for ln in mine[1::2]:
        assert " rank-1 distance: " in ln and ln.endswith(" n: %d" % n), ln
    lines = [json.loads(ln) for ln in lpm.read_text().splitlines()]
    assert len(lines) == n
    assert sorted((str(ln["item_id"]), ln["triple"]) for ln in lines) == [(str(1000 + i), j) for i in range(4)
                                                                           for j in range(3 + i)]
    assert all(1 <= ln["value_rank"] <= n and 1 <= ln["entity_rank"] <= 4 and len(ln["value_topk"]) == 3 for ln in lines)
    # without the option: the parent's output
    ev0, steps0 = run([], tmp_path / "b.jsonl")
    assert ev0 == [ln for ln in ev if ln not in mine] and len(ev0) == 2
    assert steps0 == steps
