"""infer_plan(cfg): the merge rule of K3MEngine.embed as a pure function of the config (no device).
Two copies of a stream stay one buffer until the first op whose inputs differ between them: a co-attention block,
or (image stream) a layer with dynamic attention."""
import copy

from golden_util import CFG_PATH


def _cfg(**kw):
    from k3m_amd.config import finetune_config
    return finetune_config(CFG_PATH, loss_type="ce", **kw)


def _plan(cfg, **kw):
    from k3m_amd.infer import infer_plan
    return infer_plan(cfg, **kw)


def test_plan_follows_the_engine_schedule():
    from k3m_amd.engine import schedule
    for kw in ({}, {"with_coattention": False}, {"dynamic_attention": True}):
        cfg = _cfg(**kw)
        assert [(e.kind, e.index) for e in _plan(cfg)] == schedule(cfg)


def test_shipped_config_merges_text_layers_0_to_5():
    cfg = _cfg()
    assert cfg.t_biattention_id[0] == 6 and cfg.v_biattention_id[0] == 0
    plan = _plan(cfg)
    text = {e.index: e.text for e in plan if e.kind == "t"}
    assert text == {i: ("merged" if i < 6 else "split") for i in range(12)}
    first_c = next(e for e in plan if e.kind == "c")
    assert (first_c.index, first_c.text, first_c.image) == (0, "merged", "merged")   # reads the single buffers
    assert all(e.text == "split" and e.image == "split" for e in plan[plan.index(first_c) + 1:])
    assert all(e.image == "split" for e in plan if e.kind == "v")   # every image layer comes after block 0


def test_without_coattention_everything_stays_merged():
    plan = _plan(_cfg(with_coattention=False))
    assert not any(e.kind == "c" for e in plan)
    assert {e.kind for e in plan} == {"t", "v"}
    assert all(e.text == "merged" and e.image == "merged" for e in plan)


def test_without_coattention_dynamic_attention_splits_the_image_stream_at_layer_0():
    plan = _plan(_cfg(with_coattention=False, dynamic_attention=True))
    assert all(e.text == "merged" for e in plan)
    assert all(e.image == "split" for e in plan if e.kind == "v")
    v0 = next(k for k, e in enumerate(plan) if e.kind == "v")
    assert plan[v0].index == 0
    assert all(e.image == "merged" for e in plan[:v0]) and all(e.image == "split" for e in plan[v0:])


def test_dynamic_attention_splits_an_image_layer_before_the_first_block():
    cfg = copy.copy(_cfg(dynamic_attention=True))
    cfg.v_biattention_id = [1] + list(cfg.v_biattention_id[1:])
    plan = _plan(cfg)
    k = next(k for k, e in enumerate(plan) if e.kind == "v")
    c0 = next(k for k, e in enumerate(plan) if e.kind == "c")
    assert k < c0 and plan[k].index == 0 and plan[k].image == "split"   # image layer 0 is already split
    assert plan[k].text == "merged" and plan[c0].text == "merged" and plan[c0].image == "split"
    # the same schedule without dynamic attention keeps that layer merged
    cfg2 = copy.copy(_cfg())
    cfg2.v_biattention_id = list(cfg.v_biattention_id)
    assert _plan(cfg2)[k].image == "merged"


def test_text_only_has_nothing_to_merge():
    plan = _plan(_cfg(use_image=False))
    assert plan and not any(e.kind == "v" for e in plan)
    assert all(e.text == "split" and e.image is None for e in plan)


def test_dedup_off_is_wide_from_the_start():
    for kw in ({}, {"with_coattention": False}):
        assert all(e.text == "split" and e.image == "split" for e in _plan(_cfg(**kw), dedup=False))
