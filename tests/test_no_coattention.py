"""The model without co-attention (with_coattention=False) on the host: the parameter inventories, the
never-grad bookkeeping and the fused views against the records taken from the reference
(tests/golden/inventory_no_coattention.json, written by tests/golden/make_no_coattention_golden.py), the configurations
accepted and refused, the schedule, the checkpoint surface, the DDP bucket plan and the train.py argument path.
No GPU."""
import json
import os
import types

import pytest
import torch

from golden_util import CFG_PATH, HERE
from test_text_only import _fake_trainer

INV = json.load(open(os.path.join(HERE, "golden", "inventory_no_coattention.json")))
CASE_NAMES = ["pretrain_mode1", "pretrain_mode2", "pretrain_mode3", "pretrain_text_only", "pretrain_dynamic_attention",
              "pretrain_fixed_t_layer6", "item_alignment"]


def _cases(with_coattention=False):
    from k3m_amd.config import finetune_config, pretrain_config
    kw = dict(with_coattention=with_coattention)
    return {
        "pretrain_mode1": pretrain_config(CFG_PATH, if_pre_sampling=1, **kw),
        "pretrain_mode2": pretrain_config(CFG_PATH, if_pre_sampling=2, **kw),
        "pretrain_mode3": pretrain_config(CFG_PATH, if_pre_sampling=3, **kw),
        "pretrain_text_only": pretrain_config(CFG_PATH, if_pre_sampling=1, use_image=False, **kw),
        "pretrain_dynamic_attention": pretrain_config(CFG_PATH, if_pre_sampling=1, dynamic_attention=True, **kw),
        "pretrain_fixed_t_layer6": pretrain_config(CFG_PATH, if_pre_sampling=1, fixed_t_layer=6, **kw),
        "item_alignment": finetune_config(CFG_PATH, loss_type="ce", **kw),
    }


def _tiny(task="pretrain", with_coattention=False, use_image=True):
    from k3m_amd.config import finetune_config, pretrain_config
    cfg = (pretrain_config(CFG_PATH, with_coattention=with_coattention, use_image=use_image) if task == "pretrain" else
           finetune_config(CFG_PATH, loss_type=task, with_coattention=with_coattention, use_image=use_image))
    cfg.num_hidden_layers, cfg.v_num_hidden_layers = 2, 1
    cfg.v_biattention_id, cfg.t_biattention_id = [0], [1]
    cfg.vocab_size, cfg.hidden_size, cfg.intermediate_size = 97, 64, 128
    cfg.v_hidden_size = cfg.bi_hidden_size = cfg.v_intermediate_size = 64
    cfg.v_feature_size, cfg.v_target_size, cfg.max_position_embeddings = 32, 17, 40
    return cfg


def test_the_inventory_records_every_case():
    assert INV["with_coattention"] is False
    for case in CASE_NAMES:
        assert "named_parameters" in INV[case] or "error" in INV[case], case


def test_default_case_counts():
    """350 parameters, 351 state-dict keys (the tied decoder), 14 never-grad tensors — against 998 / 999 / 86 with the
    connection blocks.  The 14: the two poolers, the NSP head, map_individual_to_bi and the three soft_* (the 72
    q_dense* of the connection blocks left with them)."""
    from k3m_amd.params import frozen_names, param_spec
    cfg = _cases()["pretrain_mode1"]
    rec = INV["pretrain_mode1"]
    assert len(param_spec(cfg)) == len(rec["named_parameters"]) == 350
    assert rec["state_dict_keys"] == 351
    assert len(frozen_names(cfg)) == len(rec["grad_none"]) == 14
    want = {p + s for p in ("t_pooler.dense", "v_pooler.dense", "cls.seq_relationship", "map_individual_to_bi", "soft_v",
                            "soft_t", "soft_pv") for s in (".weight", ".bias")}
    assert frozen_names(cfg) == want
    on = _cases(True)["pretrain_mode1"]
    assert len(param_spec(on)) == 998 and len(frozen_names(on)) == 86
    # the flag only removes tensors: every other one keeps its place in the order
    assert [(n, s) for n, s in param_spec(on) if ".c_layer" not in n] == param_spec(cfg)


@pytest.mark.parametrize("case", CASE_NAMES)
def test_bookkeeping_equals_the_recorded_inventory(case):
    """param_spec / item_alignment_spec (names, order, shapes), is_frozen, the segments, the fused q|k|v views and the
    optimizer runs, for every case the reference ran; a case it could not run must be refused by validate_config."""
    from k3m_amd.engine import validate_config
    from k3m_amd.params import flat_layout, frozen_names, fused_groups, param_spec
    from k3m_amd.trainer import block_runs, optimizer_runs
    cfg = _cases()[case]
    rec = INV[case]
    if "error" in rec:
        with pytest.raises(ValueError):
            validate_config(cfg)
        return
    validate_config(cfg)
    spec = param_spec(cfg)
    assert [(n, list(s)) for n, s in spec] == [(n, list(s)) for n, s in rec["named_parameters"]]
    assert not [n for n, _ in spec if ".c_layer" in n]
    tied = 1 if getattr(cfg, "task", "pretrain") == "pretrain" else 0
    assert rec["state_dict_keys"] == len(spec) + tied
    want = set(rec["grad_none"])
    assert frozen_names(cfg) == want
    spec, offsets, segs, total, shapes = flat_layout(cfg)
    numel = {n: int(torch.Size(s).numel()) for n, s in spec}
    f0, f1 = segs["frozen"]
    for n, _ in spec:
        assert (f0 <= offsets[n] < f1) == (n in want), n
    groups = fused_groups(cfg)
    assert not [n for g in groups for n in g if ".c_layer" in n]
    qkv = [g for g in groups if g[0].endswith("attention.self.query.weight")]
    assert len(qkv) == cfg.num_hidden_layers + (cfg.v_num_hidden_layers if cfg.use_image else 0)
    for grp in groups:
        for a, b in zip(grp, grp[1:]):
            assert offsets[b] == offsets[a] + numel[a], (a, b)
    fp = types.SimpleNamespace(spec=spec, offsets=offsets, segments=segs, total=total, shapes=shapes, frozen=want)
    covered = [(off, off + n) for off, n, _, _ in optimizer_runs(fp)]
    blocks = block_runs(fp)
    assert not [b for b in blocks if b[0] == "c"]
    inblock = [(off, off + n) for runs in blocks.values() for off, n, _, _ in runs]
    for n, _ in spec:
        a, b = offsets[n], offsets[n] + numel[n]
        if n in want:
            assert not any(x < b and a < y for x, y in covered + inblock), n
        else:
            assert any(x <= a and b <= y for x, y in covered), n
            assert any(x <= a and b <= y for x, y in inblock), n


def test_validate_config_accepts_the_flag_and_refuses_with_value_errors():
    from k3m_amd.config import pretrain_config
    from k3m_amd.engine import K3MEngine, validate_config
    for cfg in _cases().values():
        validate_config(cfg)
    for mode in (0, 1, 2, 3):
        for vt in (0, 1):
            for ft in range(0, 7):
                validate_config(pretrain_config(CFG_PATH, with_coattention=False, if_pre_sampling=mode, visual_target=vt,
                                                fixed_t_layer=ft))
    for key, what in (("in_batch_pairs", "in_batch_pairs=True is not built"), ("fast_mode", "fast_mode=True is not built")):
        for co in (False, True):
            cfg = pretrain_config(CFG_PATH, with_coattention=co)
            setattr(cfg, key, True)
            with pytest.raises(ValueError, match=what):
                validate_config(cfg)
            with pytest.raises(ValueError, match=what):   # the constructor refuses before it builds anything
                K3MEngine(cfg, torch.device("cpu"))
    cfg = pretrain_config(CFG_PATH, with_coattention=False)
    cfg.model = "albert"
    with pytest.raises(ValueError, match="model='albert'"):
        validate_config(cfg)
    # the refusals that held with co-attention hold without it
    with pytest.raises(ValueError, match="use_image=False with if_pre_sampling=2"):
        validate_config(pretrain_config(CFG_PATH, with_coattention=False, use_image=False, if_pre_sampling=2))
    with pytest.raises(ValueError, match="visual_target=2"):
        validate_config(pretrain_config(CFG_PATH, with_coattention=False, visual_target=2))
    with pytest.raises(ValueError, match="fixed_t_layer=7"):
        validate_config(pretrain_config(CFG_PATH, with_coattention=False, fixed_t_layer=7))


def _schedule(cfg):
    from k3m_amd.engine import K3MEngine
    return K3MEngine(cfg, torch.device("cpu")).schedule


def test_schedule_is_the_default_one_without_its_c_entries():
    off, on = _schedule(_tiny(with_coattention=False)), _schedule(_tiny(with_coattention=True))
    assert ("c", 0) in on and not [s for s in off if s[0] == "c"]
    assert off == [s for s in on if s[0] != "c"]
    # the shipped config's order, from the loop of the reference (vilbert_k3m.py:1185-1290) with the block skipped:
    # image layer k after text layer 6 + k, image layer 5 after text layer 10 and before text layer 11
    from k3m_amd.engine import K3MEngine
    sched = {}
    for co in (False, True):
        eng = types.SimpleNamespace(cfg=_cases(co)["pretrain_mode1"], coattn=co)
        sched[co] = K3MEngine._schedule(eng)
    assert sched[False] == [s for s in sched[True] if s[0] != "c"]
    assert sched[False] == ([("t", i) for i in range(7)] + [("v", 0), ("t", 7), ("v", 1), ("t", 8), ("v", 2), ("t", 9),
                                                            ("v", 3), ("t", 10), ("v", 4), ("v", 5), ("t", 11)])
    assert len([s for s in sched[True] if s[0] == "c"]) == 6


def test_engine_builds_no_connection_op():
    from k3m_amd.engine import K3MEngine
    eng = K3MEngine(_tiny(with_coattention=False), torch.device("cpu"))
    assert not eng.coattn and eng.co_tt == [] and eng.co_tv == [] and eng.co_pv == []
    assert len(eng.text) == 2 and len(eng.image) == 1
    on = K3MEngine(_tiny(with_coattention=True), torch.device("cpu"))
    assert on.coattn and len(on.co_tt) == len(on.co_tv) == len(on.co_pv) == 1
    txt = K3MEngine(_tiny(with_coattention=False, use_image=False), torch.device("cpu"))
    assert txt.co_tt == [] and txt.schedule == [("t", 0), ("t", 1)]


@pytest.mark.parametrize("task", ["pretrain", "ce"])
def test_checkpoint_round_trip_and_cross_loads(task, tmp_path):
    from k3m_amd import checkpoint as C
    from k3m_amd.params import param_spec
    full = [n for n, _ in param_spec(_cases()["pretrain_mode1"])] + [C.DECODER_KEY]
    assert len(full) == 351 and not [k for k in full if ".c_layer" in k]
    src = _fake_trainer(_tiny(task, False), 1, step=5)
    tar, binp = str(tmp_path / "k.tar"), str(tmp_path / "k.bin")
    C.save_checkpoint(src, tar_path=tar, bin_path=binp)
    sd = torch.load(binp, map_location="cpu", weights_only=True)
    names = [n for n, _ in src.engine.fp.spec]
    assert sorted(sd) == sorted(names + ([C.DECODER_KEY] if task == "pretrain" else []))
    dst = _fake_trainer(_tiny(task, False), 2, step=0)
    dst.engine.fp.grad = torch.zeros_like(dst.engine.fp.data)
    assert C.load_checkpoint(dst, tar) == 5
    for n in names:
        assert torch.equal(dst.engine.fp.p[n], src.engine.fp.p[n]), n
    # both cross-loads are refused before the first copy
    co = _fake_trainer(_tiny(task, True), 3, step=0)
    tar_co = str(tmp_path / "co.tar")
    C.save_checkpoint(co, tar_path=tar_co)
    for to, path, what in ((dst, tar_co, r"built without co-attention \(with_coattention=False\)"),
                           (co, tar, r"built with co-attention \(with_coattention=True\)")):
        to.engine.fp.grad = torch.zeros_like(to.engine.fp.data)
        before = to.engine.fp.data.clone()
        with pytest.raises(ValueError, match=what):
            C.load_checkpoint(to, path)
        file_sd = torch.load(path, map_location="cpu", weights_only=True)["model_state_dict"]
        with pytest.raises(ValueError, match="c_layer"):
            C.load_model_state_dict(to.engine.fp, file_sd, strict=False)
        assert torch.equal(to.engine.fp.data, before)
    # an encoder-only file (a BERT checkpoint for --pretrained_model_path) loads non-strictly into both
    bert = {k: v for k, v in sd.items() if k.startswith("encoder.layer.") or k.startswith("embeddings.")}
    assert "struc_w1.weight" in C.load_model_state_dict(dst.engine.fp, bert, strict=False)
    assert C.COATT_KEY in C.load_model_state_dict(co.engine.fp, bert, strict=False)


def test_surface_class_follows_the_inventory():
    from k3m_amd.vilbert_k3m import BertForMultiModalPreTraining_tri_stru
    model = BertForMultiModalPreTraining_tri_stru(_tiny(with_coattention=False), device="cpu")
    names = [n for n, _ in model.named_parameters()]
    assert names == [n for n, _ in model.engine.fp.spec] and not [n for n in names if ".c_layer" in n]
    assert len(model.state_dict()) == len(names) + 1
    co = BertForMultiModalPreTraining_tri_stru(_tiny(with_coattention=True), device="cpu")
    before = model.engine.fp.data.clone()
    with pytest.raises(ValueError, match="with_coattention=False"):
        model.load_state_dict(co.state_dict())
    assert torch.equal(model.engine.fp.data, before)
    with pytest.raises(ValueError, match="with_coattention=True"):
        co.load_state_dict(model.state_dict(), strict=False)


def test_ddp_bucket_plan(monkeypatch):
    """Every tensor with a gradient lies in exactly one bucket, no never-grad tensor in any, no block is a connection
    block, and the grad-ready order of the shorter backward (no ('c', i) hand-off) reduces every element once."""
    import torch.distributed as dist
    from k3m_amd import ddp
    from k3m_amd.engine import K3MEngine
    from k3m_amd.params import flat_layout
    cfg = _cases()["pretrain_mode1"]
    spec, offsets, segs, total, shapes = flat_layout(cfg)
    frozen = set(INV["pretrain_mode1"]["grad_none"])
    fp = types.SimpleNamespace(spec=spec, offsets=offsets, segments=segs, total=total, shapes=shapes, frozen=frozen)
    monkeypatch.setattr(dist, "get_world_size", lambda group=None: 2)
    fp.grad = torch.zeros(total)
    calls = []

    class Work(object):
        def wait(self):
            calls.append("wait")

    def all_reduce(t, op=None, group=None, async_op=False):
        calls.append((t.storage_offset(), t.storage_offset() + t.numel()))
        t += 1.0
        return Work()
    monkeypatch.setattr(dist, "all_reduce", all_reduce)
    red = ddp.GradAllReducer(fp)
    assert not [b for b in red.blocks if b[0] == "c"]
    assert set(red.blocks) == ({("t", i) for i in range(12)} | {("v", i) for i in range(6)} | {("head", 0), ("emb", 0)})
    red.begin(None)
    sched = K3MEngine._schedule(types.SimpleNamespace(cfg=cfg, coattn=False))
    order = list(reversed(sched)) + [("emb", 0)]
    assert order[:3] == [("t", 11), ("v", 5), ("v", 4)]
    for kind, i in order:
        red.grad_ready(kind, i)
    assert red.done == set(red.blocks)   # nothing is left for finish() to sweep up
    red.finish()
    assert not red.pending
    f0, f1 = segs["frozen"]
    assert float(fp.grad[f0:f1].abs().max()) == 0.0
    for n, _ in spec:
        g = fp.grad[offsets[n]:offsets[n] + int(torch.Size(shapes[n]).numel())]
        assert float(g.min()) == float(g.max()) == (0.0 if n in frozen else 1.0), n


def test_graph_eligibility_is_unchanged():
    from k3m_amd.graph import StepGraphs

    def trainer(**eng):
        e = types.SimpleNamespace(fp=types.SimpleNamespace(data=types.SimpleNamespace(is_cuda=True)), use_image=True,
                                  dyn_attn=False, coattn=False)
        for k, v in eng.items():
            setattr(e, k, v)
        return types.SimpleNamespace(ddp=None, accum_steps=1, micro=0, ADAMW=None, lr_schedule="warmup_linear",
                                     objective=2, engine=e)
    batch = {"_label_counts": (3, 2)}
    assert StepGraphs(trainer()).eligible(batch)
    assert not StepGraphs(trainer(use_image=False)).eligible(batch)
    assert not StepGraphs(trainer(dyn_attn=True)).eligible(batch)


def test_train_py_leaves_the_flag_off_by_default(monkeypatch, tmp_path):
    """The argument path of train.py: without --with_coattention the config reaches the Trainer with the flag False
    (the reference drivers' default, train_concap_struc.py:104), with it True."""
    import shutil
    import sys
    sys.path.insert(0, os.path.dirname(HERE))
    import train
    import k3m_amd.trainer as T
    out = tmp_path / "out"
    out.mkdir()
    shutil.copy(CFG_PATH, out / "bert_base_6layer_6conect.json")
    seen = {}

    class Stop(Exception):
        pass

    def fake_trainer(config, *a, **kw):
        seen["flag"] = config.with_coattention
        raise Stop()
    monkeypatch.setattr(T, "Trainer", fake_trainer)
    monkeypatch.setattr("torch.cuda.device_count", lambda: 1)
    monkeypatch.setattr("torch.cuda.manual_seed_all", lambda s: None)
    base = ["--data_dir", str(tmp_path), "--output_dir", str(out), "--file_name", "unused", "--train_batch_size", "2",
            "--k3m_char_tokenizer"]
    assert train.get_parser(base).with_coattention is False
    assert train.get_parser(base + ["--with_coattention"]).with_coattention is True
    for extra, want in (([], False), (["--with_coattention"], True)):
        with pytest.raises(Stop):
            train.main(base + extra)
        assert seen["flag"] is want, (extra, seen)
