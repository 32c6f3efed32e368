"""fixed_t_layer on the host: the configurations accepted and refused, the never-grad bookkeeping (frozen_names, the
optimizer runs, the DDP bucket layout, the flat layout's fused views) against the inventories recorded from the
reference (tests/golden/none_grad_fixed_t_layer.json), and the train.py argument path."""
import json
import os
import types

import pytest

from golden_util import CFG_PATH, HERE

INV = json.load(open(os.path.join(HERE, "golden", "none_grad_fixed_t_layer.json")))
FIXED = 6


def _cases():
    from k3m_amd.config import finetune_config, pretrain_config
    return {
        "pretrain_mode1": pretrain_config(CFG_PATH, if_pre_sampling=1, fixed_t_layer=FIXED),
        "pretrain_mode3": pretrain_config(CFG_PATH, if_pre_sampling=3, fixed_t_layer=FIXED),
        "pretrain_text_only": pretrain_config(CFG_PATH, if_pre_sampling=1, use_image=False, fixed_t_layer=FIXED),
        "item_alignment": finetune_config(CFG_PATH, loss_type="ce", fixed_t_layer=FIXED),
        "item_alignment_mode3": finetune_config(CFG_PATH, loss_type="ce", if_pre_sampling=3, fixed_t_layer=FIXED),
        "pretrain_mode1_unfrozen": pretrain_config(CFG_PATH, if_pre_sampling=1),
    }


def test_validate_config_accepts_and_refuses():
    from k3m_amd.config import pretrain_config
    from k3m_amd.engine import validate_config
    assert INV["fixed_t_layer"] == FIXED
    cfg = pretrain_config(CFG_PATH)
    assert cfg.fixed_t_layer == 0 and cfg.t_biattention_id[0] == 6
    for ft in range(0, 7):
        validate_config(pretrain_config(CFG_PATH, fixed_t_layer=ft))
    with pytest.raises(ValueError, match=r"fixed_t_layer=7: the reference asserts fixed_t_layer <= t_biattention_id\[0\] = 6"):
        validate_config(pretrain_config(CFG_PATH, fixed_t_layer=7))
    with pytest.raises(ValueError, match="fixed_t_layer=-1"):
        validate_config(pretrain_config(CFG_PATH, fixed_t_layer=-1))
    cfg.fixed_v_layer = 1
    with pytest.raises(ValueError, match="fixed_v_layer=1: no driver of the reference sets it"):
        validate_config(cfg)


@pytest.mark.parametrize("case", ["pretrain_mode1", "pretrain_mode3", "pretrain_text_only", "item_alignment",
                                  "item_alignment_mode3", "pretrain_mode1_unfrozen"])
def test_never_grad_bookkeeping_equals_the_recorded_inventory(case):
    from k3m_amd.params import flat_layout, frozen_names, fused_groups, param_spec
    from k3m_amd.trainer import block_runs, optimizer_runs
    cfg = _cases()[case]
    want = set(INV[case])
    assert frozen_names(cfg) == want
    spec, offsets, segs, total, shapes = flat_layout(cfg)
    numel = {n: 1 for n, _ in spec}
    for n, sh in spec:
        for d in sh:
            numel[n] *= d
    f0, f1 = segs["frozen"]
    for n, _ in spec:
        assert (f0 <= offsets[n] < f1) == (n in want), n
    # fused views stay contiguous wherever their members land (the frozen layers' q|k|v move as one)
    for grp in fused_groups(cfg):
        for a, b in zip(grp, grp[1:]):
            assert offsets[b] == offsets[a] + numel[a], (a, b)
    fp = types.SimpleNamespace(spec=spec, offsets=offsets, segments=segs, total=total, shapes=shapes, frozen=want)
    covered = []
    for off, n, wd, mult in optimizer_runs(fp):
        covered.append((off, off + n))
        assert off + n <= f0 + 4
    trainable = sorted((offsets[n], offsets[n] + numel[n]) for n, _ in spec if n not in want)
    for a, b in trainable:   # every trainable tensor lies inside one optimizer run
        assert any(x <= a and b <= y for x, y in covered), (a, b)
    blocks = block_runs(fp)
    inblock = [(off, off + n) for runs in blocks.values() for off, n, _, _ in runs]
    for a, b in trainable:
        assert any(x <= a and b <= y for x, y in inblock), (a, b)
    for n in want:   # and no run reaches a never-grad tensor
        a, b = offsets[n], offsets[n] + numel[n]
        assert not any(x < b and a < y for x, y in covered + inblock), n
    if cfg.fixed_t_layer:
        assert not any(("t", i) in blocks for i in range(FIXED))
        assert ("t", FIXED) in blocks


def test_ddp_bucket_layout_skips_the_frozen_layers(monkeypatch):
    import torch.distributed as dist
    from k3m_amd import ddp
    from k3m_amd.params import flat_layout
    cfg = _cases()["pretrain_mode1"]
    spec, offsets, segs, total, shapes = flat_layout(cfg)
    fp = types.SimpleNamespace(spec=spec, offsets=offsets, segments=segs, total=total, shapes=shapes,
                               frozen=set(INV["pretrain_mode1"]))
    monkeypatch.setattr(dist, "get_world_size", lambda group=None: 2)
    red = ddp.GradAllReducer(fp)
    f0, f1 = segs["frozen"]
    for i in range(FIXED):
        assert ("t", i) not in red.blocks
    assert ("t", FIXED) in red.blocks and ("emb", 0) in red.blocks
    for rs in red.blocks.values():
        for a, b in rs:
            assert b <= f0 or a >= f1
    # the real _launch / finish path on the CPU all-reduce branch, with a recording stand-in for the collective:
    # grad_ready in the order the frozen backward fires it (no text block below the cut), then finish()
    import torch
    fp.grad = torch.zeros(total)
    calls = []

    class Work(object):
        def wait(self):
            calls.append("wait")

    def all_reduce(t, op=None, group=None, async_op=False):
        o = t.storage_offset()
        calls.append((o, o + t.numel()))
        t += 1.0
        return Work()
    monkeypatch.setattr(dist, "all_reduce", all_reduce)
    red = ddp.GradAllReducer(fp)
    red.begin(None)
    for kind, i in [("t", 11), ("c", 5), ("v", 5), ("t", FIXED), ("c", 0), ("emb", 0)]:
        red.grad_ready(kind, i)
    assert red.done == {("head", 0), ("t", 11), ("c", 5), ("v", 5), ("t", FIXED), ("c", 0), ("emb", 0)}
    red.finish()
    assert set(red.done) == set(red.blocks) and not red.pending
    ranges = [c for c in calls if c != "wait"]
    assert calls.count("wait") == len(ranges) == sum(len(r) for r in red.blocks.values())
    # every trainable element was reduced exactly once, no element of the frozen segment at all
    assert float(fp.grad[f0:f1].abs().max()) == 0.0
    numel = lambda n: int(torch.Size(shapes[n]).numel())  # noqa: E731
    for n, _ in spec:
        g = fp.grad[offsets[n]:offsets[n] + numel(n)]
        assert float(g.min()) == float(g.max()) == (0.0 if n in fp.frozen else 1.0), n


def test_freeze_list_on_top_of_the_cut():
    from k3m_amd.params import frozen_names, param_spec
    cfg = _cases()["pretrain_mode1"]
    freeze = set(INV["freeze8_names"])
    names = {n for n, _ in param_spec(cfg)}
    assert freeze <= names
    assert set(INV["pretrain_mode1_freeze8"]) == freeze | frozen_names(cfg)


def test_train_py_sets_fixed_t_layer(monkeypatch, tmp_path):
    """The argument path of train.py: --freeze above t_biattention_id[0] sets config.fixed_t_layer to that id (the
    reference driver, train_concap_struc.py:206-207) where it used to exit; at or below it the config keeps 0."""
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
        seen["fixed"] = config.fixed_t_layer
        seen["frozen_names"] = kw.get("frozen_names")
        raise Stop()
    monkeypatch.setattr(T, "Trainer", fake_trainer)
    monkeypatch.setattr("torch.cuda.device_count", lambda: 1)
    monkeypatch.setattr("torch.cuda.manual_seed_all", lambda s: None)
    base = ["--data_dir", str(tmp_path), "--output_dir", str(out), "--file_name", "unused", "--with_coattention",
            "--train_batch_size", "2", "--k3m_char_tokenizer"]
    for freeze, want in ((8, 6), (7, 6), (6, 0), (-1, 0)):
        with pytest.raises(Stop):
            train.main(base + ["--freeze", str(freeze)])
        assert seen["fixed"] == want, (freeze, seen)
