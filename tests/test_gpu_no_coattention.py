"""The model without co-attention (with_coattention=False) end to end on the GPU: parity with the
fixtures recorded from the reference with the flag off (tests/golden/make_no_coattention_golden.py), the two copies of
every stream in eval and in train mode, every accepted combination of switches against its recorded never-grad
inventory, deterministic repeats (also behind the load-time grouping knobs), Trainer / ItemAlignmentTrainer, the
hipGraph step, two-rank DDP, the drop-in module and the train.py driver on its default command line.
Bars: those of tests/test_gpu_parity.py, tests/test_gpu_finetune.py and tests/test_gpu_graph.py."""
import json
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest
import torch

from golden_util import CFG_PATH, HERE, REPO, load_case, case_batch, case_noise, ft_noise, ft_pair, load_ft_case

pytestmark = pytest.mark.gpu
CASE = "noco_bs2"
LOSS_KEYS = ("masked_lm_loss", "masked_img_loss", "masked_lm_loss_pv", "loss_lpm", "next_sentence_loss", "loss")
INV = json.load(open(os.path.join(HERE, "golden", "inventory_no_coattention.json")))
PROBE = "encoder.layer.11.output.dense.weight"


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
    """param_values(cfg, seed), generated once per inventory and seed."""
    from k3m_amd.weights import param_values
    key = (seed, getattr(cfg, "use_image", True), getattr(cfg, "task", "pretrain"),
           bool(getattr(cfg, "dynamic_attention", False)), bool(cfg.with_coattention), cfg.v_target_size)
    if key not in _VALUES:
        _VALUES[key] = param_values(cfg, seed)
    return _VALUES[key]


def _config(with_coattention=False, **kw):
    from k3m_amd.config import pretrain_config
    kw.setdefault("if_pre_sampling", 1)
    return pretrain_config(CFG_PATH, with_coattention=with_coattention, **kw)


def _golden_step(dev, dtype, with_coattention=False):
    from k3m_amd.engine import K3MEngine
    g = load_case(CASE)
    assert int(g["with_coattention"]) == 0 and int(g["mode"]) == 1
    cfg = _config(with_coattention)
    eng = K3MEngine(cfg, dev, dtype=dtype)
    eng.fp.load(_values(cfg, int(g["weight_seed"])))
    batch = {k: v.to(dev) for k, v in case_batch(g).items()}
    noise = {k: v.to(dev) for k, v in case_noise(g).items()}
    out, ctx = eng.forward(batch, train=False, noise=noise, ent_neg=torch.from_numpy(g["ent_neg"]),
                           val_neg=torch.from_numpy(g["val_neg"]))
    assert with_coattention or not any(kind == "c" for kind, _, _ in ctx["enc"])
    eng.backward(ctx)
    torch.cuda.synchronize()
    return g, eng, out, np.array([float(out[k]) for k in LOSS_KEYS])


def test_engine_matches_reference_golden(dev):
    g, eng, out, got = _golden_step(dev, "fp32")
    print("losses", got, g["losses"])
    assert len(eng.fp.spec) == len(g["grad_norm_names"]) == 350
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
    assert never == len(INV["pretrain_mode1"]["grad_none"]) == 14


def test_the_fixture_is_not_blind_to_the_flag(dev):
    """The engine with the connection blocks, on the fixture's inputs and the weights the two models share, misses the
    fixture's loss bar and meets the with-co-attention losses the generator recorded beside it."""
    g, eng, out, got = _golden_step(dev, "fp32", with_coattention=True)
    assert len(eng.fp.spec) == 998
    on = g["losses_with_coattention"]   # mlm_t, img, mlm_pv, lpm, nsp
    np.testing.assert_allclose(got[:5], on, rtol=1e-3, atol=1e-4)
    rel = np.abs(got[:4] - g["losses"][:4]) / np.abs(g["losses"][:4])
    print("relative distance of the with-co-attention losses from the fixture", rel)
    assert rel.max() >= 10 * 1e-3


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


def test_item_alignment_matches_reference_golden(dev):
    from k3m_amd.config import finetune_config
    from k3m_amd.finetune import ARG_NAMES, K3MForItemAlignment
    g = load_ft_case("noco_ce")
    assert int(g["with_coattention"]) == 0 and str(g["loss_type"]) == "ce"
    cfg = finetune_config(CFG_PATH, loss_type="ce", with_coattention=False, if_pre_sampling=int(g["mode"]))
    model = K3MForItemAlignment(cfg, dev)
    assert len(model.engine.fp.spec) == len(INV["item_alignment"]["named_parameters"])
    model.engine.fp.load(_values(cfg, int(g["weight_seed"])))
    pair = {k: v.to(dev) for k, v in ft_pair(g).items()}
    n1, n2 = ft_noise(g)
    noise = ({k: v.to(dev) for k, v in n1.items()}, {k: v.to(dev) for k, v in n2.items()})
    e1, e2, probs, loss = model(*[pair[k] for k in ARG_NAMES], train=False, noise=noise)
    model.backward()
    torch.cuda.synchronize()
    print("loss", float(loss), float(g["out/loss"]))
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
    never = set()
    for n, ref in zip(list(g["grad_norm_names"]), g["grad_norms"]):
        gn = float(G[n].double().norm())
        if np.isnan(ref):
            never.add(str(n))
            assert gn == 0.0, n
        else:
            assert abs(gn - ref) <= 5e-3 * ref + 1e-6, (n, gn, ref)
    assert never == set(INV["item_alignment"]["grad_none"]) == model.engine.fp.frozen


def _synthetic_step(dev, cfg, dtype="fp32", train=True, seed=5, B=2, eng_seed=77):
    from k3m_amd.engine import K3MEngine, label_counts
    from k3m_amd.synthetic import synthetic_batch
    eng = K3MEngine(cfg, dev, dtype=dtype, seed=eng_seed)
    eng.fp.load(_values(cfg, 4321))
    batch = synthetic_batch(cfg, B, dev, seed=3)
    if not eng.use_image:
        for k in ("image_feat", "image_loc", "image_target", "image_label", "image_mask"):
            batch.pop(k, None)
    batch["_label_counts"] = label_counts(batch)
    out, ctx = eng.forward(batch, train=train, seed=seed)
    return eng, batch, out, ctx


@pytest.mark.parametrize("dyn", [False, True], ids=["plain", "dynamic_attention"])
def test_the_two_copies_of_a_stream(dev, dyn):
    """Eval mode: without a connection block nothing distinguishes the two copies of a stream (the same arithmetic in
    other rows of the wide buffer): rtol 1e-5, the bar for the same arithmetic at another tile position.  The image
    copies agree only without dynamic attention (with it, copy 1 is gated by the title and copy 2 by the PV).  Train
    mode with the shipped dropout: the copies draw per-row counters and differ, as the reference's two invocations do."""
    cfg = _config(dynamic_attention=dyn)
    eng, batch, out, ctx = _synthetic_step(dev, cfg, train=False)
    B, T, P, R = ctx["B"], ctx["T"], ctx["P"], ctx["R"]
    BT, BP, BR = B * T, B * P, B * R
    XT, XV = ctx["XT"], ctx["XV"]
    assert XT.shape[0] == 2 * BT + 2 * BP and XV.shape[0] == 2 * BR

    def close(a, b):
        print("copies: max |a - b| %.3g of max |b| %.3g, equal %s" % (float((a - b).abs().max()), float(b.abs().max()),
                                                                     torch.equal(a, b)))
        return torch.allclose(a, b, rtol=1e-5, atol=0.0)
    assert close(XT[0:BT], XT[BT:2 * BT])
    assert close(XT[2 * BT:2 * BT + BP], XT[2 * BT + BP:])
    if dyn:
        assert not close(XV[0:BR], XV[BR:])
    else:
        assert close(XV[0:BR], XV[BR:])
    eng.backward(ctx)
    eng, batch, out, ctx = _synthetic_step(dev, cfg, train=True)
    assert eng.p_h > 0 and eng.p_a > 0 and eng.p_vh > 0
    XT, XV = ctx["XT"], ctx["XV"]
    assert not close(XT[0:BT], XT[BT:2 * BT])
    assert not close(XT[2 * BT:2 * BT + BP], XT[2 * BT + BP:])
    assert not close(XV[0:BR], XV[BR:])
    eng.backward(ctx)
    torch.cuda.synchronize()


COMBOS = [
    ("mode0", dict(if_pre_sampling=0), "pretrain_mode1"),   # mode 0 keeps mode 1's never-grad set (params.is_frozen)
    ("mode2", dict(if_pre_sampling=2), "pretrain_mode2"),
    ("mode3", dict(if_pre_sampling=3), "pretrain_mode3"),
    ("text_only", dict(use_image=False), "pretrain_text_only"),
    ("dynamic_attention", dict(dynamic_attention=True), "pretrain_dynamic_attention"),
    ("visual_target1", dict(visual_target=1), "pretrain_mode1"),
    ("fixed_t_layer6", dict(fixed_t_layer=6), "pretrain_fixed_t_layer6"),
    ("dynamic_attention+fixed_t_layer6+mode2", dict(dynamic_attention=True, fixed_t_layer=6, if_pre_sampling=2), None),
]


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("combo", COMBOS, ids=[c[0] for c in COMBOS])
def test_switch_combinations_run_and_keep_the_inventory(dev, combo, dtype):
    _, kw, inv = combo
    cfg = _config(**kw)
    eng, batch, out, ctx = _synthetic_step(dev, cfg, dtype=dtype)
    eng.backward(ctx)
    torch.cuda.synchronize()
    for k in LOSS_KEYS:
        assert np.isfinite(float(out[k])), k
    assert float(eng.fp.g[PROBE].abs().max()) > 0.0
    assert torch.isfinite(eng.fp.grad).all()
    if inv is not None:
        assert eng.fp.frozen == set(INV[inv]["grad_none"])
    zero = {n for n, _ in eng.fp.spec if float(eng.fp.g[n].abs().max()) == 0.0}
    assert eng.fp.frozen <= zero
    if kw.get("if_pre_sampling", 1) != 0:   # (mode 0 keeps the unused score_* trainable with a zero gradient)
        assert zero == eng.fp.frozen, sorted(zero ^ eng.fp.frozen)[:6]


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_deterministic_repeats(dev, dtype, deterministic):
    cfg = _config()
    runs = []
    for _ in range(2):
        eng, batch, out, ctx = _synthetic_step(dev, cfg, dtype=dtype)
        eng.backward(ctx)
        torch.cuda.synchronize()
        runs.append(([out[k].clone() for k in LOSS_KEYS], eng.fp.grad.clone()))
    for a, b in zip(runs[0][0], runs[1][0]):
        assert torch.equal(a, b)
    assert torch.equal(runs[0][1], runs[1][1])
    assert float(runs[0][1].abs().max()) > 0


_CHILD = r'''
import sys, torch
sys.path.insert(0, sys.argv[1])
from k3m_amd import engine as E, ops
from k3m_amd.config import pretrain_config
from k3m_amd.engine import K3MEngine, label_counts
from k3m_amd.synthetic import synthetic_batch
from k3m_amd.weights import param_values
ops.set_deterministic(True)
dev = torch.device("cuda")
want = sys.argv[3]
assert (want == "tv") == E.GROUP_TV and (want == "ungrouped") == (not E.GROUPED), (want, E.GROUPED, E.GROUP_TV)
for dyn in (False, True):
    cfg = pretrain_config(sys.argv[2], with_coattention=False, dynamic_attention=dyn)
    vals = param_values(cfg, 4321)
    for dtype in ("fp32", "bf16"):
        runs = []
        for _ in range(2):
            eng = K3MEngine(cfg, dev, dtype=dtype, seed=77)
            eng.fp.load(vals)
            batch = synthetic_batch(cfg, 2, dev, seed=3)
            batch["_label_counts"] = label_counts(batch)
            out, ctx = eng.forward(batch, train=True, seed=5)
            eng.backward(ctx)
            torch.cuda.synchronize()
            runs.append((out["loss"].clone(), out["c_final"].clone(), eng.fp.grad.clone()))
        for a, b in zip(*runs):
            assert torch.equal(a, b) and torch.isfinite(a).all(), (dyn, dtype)
        assert float(runs[0][2].abs().max()) > 0
        print("loss", dyn, dtype, float(runs[0][0]))
print("ok", want)
'''


@pytest.mark.parametrize("case", [("ungrouped", {"K3M_GROUPED": "0"}), ("tv", {"K3M_GROUP_TV": "1"}),
                                  ("branch", {"K3M_BRANCH_STREAMS": "4"})], ids=["K3M_GROUPED=0", "K3M_GROUP_TV=1",
                                                                               "K3M_BRANCH_STREAMS=4"])
def test_deterministic_repeats_behind_the_grouping_knobs(dev, tmp_path, case):
    """The knobs are read when the package loads, so each runs in a fresh child process: two train-mode steps from one
    seed are bit-equal in loss, c_final and the whole gradient buffer, for both dtypes, with and without dynamic
    attention.  K3M_GROUP_TV=1 pairs every image layer with a text layer on the shorter schedule (text layer 6 + k with
    image layer k; with dynamic attention image layer k with text layer 7 + k, which reads the state before the pair)."""
    name, knobs = case
    script = tmp_path / "child.py"
    script.write_text(_CHILD)
    r = subprocess.run([sys.executable, str(script), REPO, CFG_PATH, name], env=dict(os.environ, **knobs),
                       capture_output=True, text=True, timeout=240)
    assert r.returncode == 0 and ("ok " + name) in r.stdout, (r.stdout[-2000:], r.stderr[-3000:])


def test_group_tv_pairs_match_the_unpaired_step(dev, deterministic):
    """Dynamic attention makes the t / v order observable: the lock-step pairs of K3M_GROUP_TV on the shorter schedule
    (image layer k with text layer 7 + k) give the unpaired step's bits, forward and backward (exact=True).  As in
    tests/test_gpu_dynamic_attention.py: eval mode (in train mode the lock step takes the dropout counters of the two
    layers in another order, so the masks differ), deterministic mode, and the k-split heuristics of ungrouped
    launches off for both runs (a layer run alone picks another k-split than the same product in a grouped launch)."""
    from k3m_amd import engine as E, ops
    cfg = _config(dynamic_attention=True)
    old = E.GROUP_TV, ops.SMALL_SPLITK, ops.SPLITK_FILL
    ops.SMALL_SPLITK = ops.SPLITK_FILL = False
    res = {}
    try:
        for tv in (False, True):
            E.GROUP_TV = tv and E.GROUPED
            eng, batch, out, ctx = _synthetic_step(dev, cfg, train=False)
            kinds = [k for k, _, _ in ctx["enc"]]
            assert kinds == ["t"] * 7 + ["v", "t"] * 4 + ["v", "v", "t"]
            eng.backward(ctx)
            torch.cuda.synchronize()
            res[tv] = (out["loss"].clone(), out["c_final"].clone(), eng.fp.grad.clone())
    finally:
        E.GROUP_TV, ops.SMALL_SPLITK, ops.SPLITK_FILL = old
    for a, b in zip(res[False], res[True]):
        assert torch.equal(a, b)


def test_trainer_step(dev):
    from k3m_amd.trainer import Trainer
    g = load_case(CASE)
    tr = Trainer(_config(), dev, lr=1e-3, warmup_steps=0, total_steps=20, seed=9)
    tr.graph = False
    fp = tr.engine.fp
    assert fp.frozen == set(INV["pretrain_mode1"]["grad_none"])
    batch = {k: v.to(dev) for k, v in case_batch(g).items()}
    start = fp.data.clone()
    out = tr.step(batch)
    torch.cuda.synchronize()
    assert np.isfinite(float(out["loss"]))
    f0, f1 = fp.segments["frozen"]
    assert tr.m.numel() <= f0 + 4 and tr.v.numel() <= f0 + 4
    assert torch.equal(fp.data[f0:f1], start[f0:f1]) and float(fp.grad[f0:f1].abs().max()) == 0.0
    for n in ("encoder.layer.0.attention.self.query.weight", "encoder.v_layer.5.output.dense.bias", PROBE,
              "embeddings.word_embeddings.weight", "struc_w1.weight"):
        o = fp.offsets[n]
        assert not torch.equal(fp.p[n].reshape(-1), start[o:o + fp.p[n].numel()]), n
    tr.finish()


def test_trainer_step_with_accumulation_and_objective_1(dev):
    from k3m_amd.engine import label_counts
    from k3m_amd.synthetic import synthetic_batch
    from k3m_amd.trainer import Trainer
    cfg = _config()
    tr = Trainer(cfg, dev, lr=1e-3, warmup_steps=0, total_steps=20, seed=9, accum_steps=2, objective=1)
    tr.graph = False
    batch = synthetic_batch(cfg, 2, dev, seed=23)
    batch["_label_counts"] = label_counts(batch)
    start = tr.engine.fp.p[PROBE].clone()
    for _ in range(2):
        out = tr.step(batch)
    torch.cuda.synchronize()
    assert np.isfinite(float(out["loss"])) and tr.global_step == 1
    assert not torch.equal(tr.engine.fp.p[PROBE], start)
    tr.finish()


def test_freeze_list(dev):
    """--freeze semantics (frozen_names) on the model without co-attention: the listed tensors compute their gradient
    on the way down and are not updated; the rest move."""
    from k3m_amd.engine import label_counts
    from k3m_amd.synthetic import synthetic_batch
    from k3m_amd.trainer import Trainer
    cfg = _config()
    freeze = [n for n, _ in INV["pretrain_mode1"]["named_parameters"]
              if n.startswith("embeddings.") or (n.startswith("encoder.layer.") and int(n.split(".")[2]) <= 2)]
    assert len(freeze) == 5 + 3 * 16
    tr = Trainer(cfg, dev, lr=1e-3, warmup_steps=0, total_steps=20, seed=9, frozen_names=freeze)
    tr.graph = False
    fp = tr.engine.fp
    batch = synthetic_batch(cfg, 2, dev, seed=23)
    batch["_label_counts"] = label_counts(batch)
    start = {n: fp.p[n].clone() for n, _ in fp.spec}
    assert np.isfinite(float(tr.step(batch)["loss"]))
    torch.cuda.synchronize()
    moved = {n for n, _ in fp.spec if not torch.equal(fp.p[n], start[n])}
    assert not (moved & (set(freeze) | fp.frozen))
    for n in ("encoder.layer.3.attention.self.query.weight", PROBE, "encoder.v_layer.0.output.dense.weight"):
        assert n in moved, n
    tr.finish()


def test_item_alignment_trainer_step(dev):
    from k3m_amd.config import finetune_config
    from k3m_amd.finetune import ItemAlignmentTrainer
    g = load_ft_case("noco_ce")
    cfg = finetune_config(CFG_PATH, loss_type="ce", with_coattention=False)
    tr = ItemAlignmentTrainer(cfg, dev, lr=1e-3, warmup_steps=0, total_steps=10, seed=19)
    fp = tr.engine.fp
    assert fp.frozen == set(INV["item_alignment"]["grad_none"])
    start = {n: fp.p[n].clone() for n, _ in fp.spec}
    pair = {k: v.to(dev) for k, v in ft_pair(g).items()}
    loss = float(tr.step(pair)["loss"])
    torch.cuda.synchronize()
    assert np.isfinite(loss)
    moved = {n for n, _ in fp.spec if not torch.equal(fp.p[n], start[n])}
    assert not (moved & fp.frozen)
    for n in (PROBE, "classifier.out_proj.bias", "encoder.v_layer.0.attention.self.query.weight"):
        assert n in moved, n


def test_graph_step_captures_and_matches_eager(dev):
    """The body of test_gpu_graph.test_graph_step_matches_eager for the model without co-attention: fp32, B = 2, three
    steps (one capture, two replays), the same bars."""
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
    ta.finish()
    tb.finish()


def test_two_rank_engine_allreduce():
    """Two ranks over gloo sharing GPU 0, in child processes (scripts/ddp_engine_check.py --no_coattention): bucket
    order = the grad-ready order of the shorter backward, reduced gradient = sum of the ranks' gradients."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    r = subprocess.run([sys.executable, os.path.join(REPO, "scripts", "ddp_engine_check.py"), "--world", "2",
                        "--backend", "gloo", "--dtype", "fp32", "--no_coattention"], capture_output=True, text=True,
                       timeout=280, env=env, cwd=REPO)
    line = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert line, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    res = json.loads(line[-1])
    print(res)
    assert res["with_coattention"] is False and res["blocks"] == 12 + 6 + 2
    assert res["order_ok"], res
    assert res["ranks_bitwise_equal"] and res["max_rel_err_vs_sum_of_local"] < res["tolerance"], res
    assert res["params_equal_after_step"] and res["world_seen"] == 2, res
    assert r.returncode == 0 and res["ok"], res


def test_drop_in_module(dev):
    from vilbert_k3m.vilbert_k3m import BertForMultiModalPreTraining_tri_stru
    g = load_case(CASE)
    cfg = _config()
    model = BertForMultiModalPreTraining_tri_stru(cfg, device=dev)
    names = [n for n, _ in model.named_parameters()]
    assert names == [n for n, _ in INV["pretrain_mode1"]["named_parameters"]] and len(names) == 350
    sd = model.state_dict()
    assert len(sd) == 351 and set(sd) == set(names) | {"cls.predictions.decoder.weight"}
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
    assert len(outs) == 10
    got = np.array([float(outs[i].detach()) for i in (0, 1, 3, 9, 6)])
    np.testing.assert_allclose(got, g["losses"][:5], rtol=1e-3, atol=1e-4)
    (outs[0] + outs[1] + outs[3] + outs[9]).backward()
    named = dict(model.named_parameters())
    none = {n for n, p in named.items() if p.grad is None}
    assert none == set(INV["pretrain_mode1"]["grad_none"]) and len(none) == 14
    for n, ref in zip(list(g["grad_norm_names"]), g["grad_norms"]):
        if not np.isnan(ref):
            assert abs(float(named[str(n)].grad.double().norm()) - ref) <= 5e-3 * ref + 1e-6, n


def test_train_py_default_command_line(dev, tmp_path):
    """train.py without --with_coattention (the reference drivers' default) on the parity case: the first step meets
    the fixture's losses, the second is finite, and the epoch's .bin is the 351-key state dict, which reloads.  On the
    parent commit this command ended with the engine constructor's AssertionError."""
    from k3m_amd import checkpoint as C
    from k3m_amd.engine import FlatParams
    g = load_case(CASE)
    out = tmp_path / "out"
    out.mkdir()
    shutil.copy(CFG_PATH, out / "bert_base_6layer_6conect.json")
    cfg = _config()
    vals = _values(cfg, int(g["weight_seed"]))
    torch.save({k: torch.from_numpy(v) for k, v in vals.items()}, str(tmp_path / "w.bin"))
    log = tmp_path / "loss.jsonl"
    r = subprocess.run([sys.executable, os.path.join(REPO, "train.py"), "--data_dir", str(tmp_path), "--output_dir",
                        str(out), "--file_name", "unused", "--do_train", "--train_batch_size", "2",
                        "--num_train_epochs", "1", "--if_pre_sampling", "1", "--file_state_dict",
                        str(tmp_path / "w.bin"), "--k3m_parity_case",
                        os.path.join(HERE, "golden", "golden_%s.npz" % CASE), "--k3m_max_steps", "2",
                        "--k3m_loss_log", str(log)], cwd=str(tmp_path), capture_output=True, text=True, timeout=400)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    rows = [json.loads(l) for l in log.read_text().splitlines()]
    assert len(rows) == 2
    got = np.array([rows[0][k] for k in LOSS_KEYS])
    np.testing.assert_allclose(got, g["losses"], rtol=1e-3, atol=1e-4)   # (lr = 0 on the first step)
    assert np.isfinite(rows[1]["loss"])
    sd = torch.load(str(out / "k3m_bert-base-uncased_12l_12h" / "K3M_struc_presample-1_epoch-0.bin"),
                    map_location="cpu", weights_only=True)
    assert len(sd) == 351 and not [k for k in sd if ".c_layer" in k]
    fp = FlatParams(cfg, torch.device("cpu"))
    assert not C.load_model_state_dict(fp, sd)
    assert torch.equal(fp.p[PROBE], sd[PROBE])
    assert not torch.equal(sd[PROBE], torch.from_numpy(vals[PROBE]))   # the second step moved it
