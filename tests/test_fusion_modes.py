"""Host-side bookkeeping of the soft (if_pre_sampling 2) and interactive-only (3) fusion modes: which
tensors never get a gradient, where they land in the flat layout, and that the optimizer runs, the
checkpoint's optimizer state and the gradient all-reduce ranges follow the mode.  CPU only."""
import math
import os
import types

import numpy as np
import pytest
import torch

from golden_util import CFG_PATH, load_case

MODS = ("v", "t", "pv")
SOFT = ["soft_%s.%s" % (m, w) for m in MODS for w in ("weight", "bias")]
SCORE = ["score_%s_%s.%s" % (k, m, w) for m in MODS for k in ("self", "cross1", "cross2") for w in ("weight", "bias")]


def _cfg(mode):
    from k3m_amd.config import pretrain_config
    return pretrain_config(CFG_PATH, if_pre_sampling=mode)


def _tiny(mode):
    cfg = _cfg(mode)
    cfg.num_hidden_layers, cfg.v_num_hidden_layers = 2, 1
    cfg.v_biattention_id, cfg.t_biattention_id = [0], [1]
    cfg.vocab_size, cfg.hidden_size, cfg.intermediate_size = 97, 64, 128
    cfg.v_hidden_size = cfg.bi_hidden_size = cfg.v_intermediate_size = 64
    cfg.v_feature_size, cfg.v_target_size, cfg.max_position_embeddings = 32, 17, 40
    return cfg


def _covered(runs, fp, name):
    """How many runs [(offset, length, ...)] contain the whole tensor."""
    o, n = fp.offsets[name], math.prod(fp.shapes[name])
    return sum(1 for r in runs if r[0] <= o and o + n <= r[0] + r[1])


def _touched(runs, fp, name):
    o, n = fp.offsets[name], math.prod(fp.shapes[name])
    return any(r[0] < o + n and o < r[0] + r[1] for r in runs)


# ---------------------------------------------------------------- never-grad sets
@pytest.mark.parametrize("mode,case,count", [(2, "bs2_soft", 80), (3, "bs2_inter", 104)])
def test_never_grad_set_matches_reference_fixture(mode, case, count):
    from k3m_amd.params import frozen_names, is_frozen, param_spec
    cfg = _cfg(mode)
    fz = frozen_names(cfg)
    assert len(fz) == count
    assert fz == {n for n, _ in param_spec(cfg) if is_frozen(n, cfg)}
    g = load_case(case)
    assert int(g["mode"]) == mode
    nan = {str(n) for n, v in zip(g["grad_norm_names"], g["grad_norms"]) if np.isnan(v)}
    assert fz == nan
    assert set(SOFT) <= fz if mode == 3 else not (set(SOFT) & fz)
    assert (set(SCORE) <= fz) == (mode == 3)


def test_never_grad_set_of_modes_0_and_1_is_unchanged():
    from k3m_amd.params import frozen_names, is_frozen, param_spec, segment_of
    for mode in (0, 1):
        cfg = _cfg(mode)
        old = {n for n, _ in param_spec(cfg) if is_frozen(n)}   # the one-argument form
        assert len(old) == 86 and frozen_names(cfg) == old
        for n, _ in param_spec(cfg):
            assert segment_of(n, cfg) == segment_of(n)


def test_item_alignment_never_grad_set_follows_the_mode():
    from k3m_amd.config import finetune_config
    from k3m_amd.params import frozen_names
    fz = {m: frozen_names(finetune_config(CFG_PATH, loss_type="ce", if_pre_sampling=m)) for m in (1, 2, 3)}
    assert fz[2] == fz[1] - set(SOFT) and fz[3] == fz[1] | set(SCORE)
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "golden_ft_ce_soft.npz"))
    nan = {str(n) for n, v in zip(g["grad_norm_names"], g["grad_norms"]) if np.isnan(v)}
    assert int(g["mode"]) == 2 and fz[2] == nan


# ---------------------------------------------------------------- flat layout
def test_layout_soft_mode_moves_soft_tensors_into_the_trained_segments():
    from k3m_amd.params import flat_layout, fused_groups
    cfg = _cfg(2)
    spec, off, seg, total, shapes = flat_layout(cfg)

    def seg_of(n):
        return next(s for s, (a, b) in seg.items() if a <= off[n] < b)
    for m in MODS:
        assert seg_of("soft_%s.weight" % m) == "decay"
        assert seg_of("soft_%s.bias" % m) == "no_decay"
    for grp in fused_groups(cfg):
        for a, b in zip(grp, grp[1:]):
            assert off[b] == off[a] + math.prod(shapes[a]), (a, b)
    # mode 3: the scorers join the frozen segment, still adjacent
    spec3, off3, seg3, _, _ = flat_layout(_cfg(3))
    for n in SCORE + SOFT:
        assert seg3["frozen"][0] <= off3[n] < seg3["frozen"][1], n
    for grp in fused_groups(_cfg(3)):
        for a, b in zip(grp, grp[1:]):
            assert off3[b] == off3[a] + math.prod(shapes[a]), (a, b)


def test_layout_of_mode_1_is_the_one_argument_layout():
    """A config object without the attribute goes through the old one-argument path (is_frozen(name))."""
    from k3m_amd.params import flat_layout
    cfg = _cfg(1)
    bare = _cfg(1)
    del bare.if_pre_sampling
    new, old = flat_layout(cfg), flat_layout(bare)
    assert new[1] == old[1] and new[2] == old[2] and new[3] == old[3]
    assert flat_layout(_cfg(0))[1] == old[1]
    from k3m_amd.params import segment_of
    for n, _ in new[0]:
        assert new[2][segment_of(n)][0] <= new[1][n] < new[2][segment_of(n)][1], n


# ---------------------------------------------------------------- optimizer runs, checkpoint
def _fake_trainer(cfg, seed, step):
    from k3m_amd.engine import FlatParams
    fp = FlatParams(cfg, torch.device("cpu"))
    g = torch.Generator().manual_seed(seed)
    fp.data.copy_(torch.randn(fp.total, generator=g))
    nopt = fp.segments["frozen"][0]
    t = types.SimpleNamespace(engine=types.SimpleNamespace(fp=fp, step_count=step), global_step=step,
                              m=torch.randn(nopt, generator=g), v=torch.rand(nopt, generator=g),
                              lr=1e-4, warmup=10, t_total=1000, beta1=0.9, beta2=0.98, eps=1e-8, wd=0.01)
    t.current_lr = lambda: t.lr * min(1.0, t.global_step / t.warmup)
    return t


def test_optimizer_runs_follow_the_mode():
    from k3m_amd.engine import FlatParams
    from k3m_amd.trainer import block_runs, optimizer_runs
    fp2 = FlatParams(_tiny(2), torch.device("cpu"))
    assert fp2.frozen == {n for n in fp2.frozen if n in dict(fp2.spec)} and not (set(SOFT) & fp2.frozen)
    runs = optimizer_runs(fp2)
    head = block_runs(fp2)[("head", 0)]
    for n in SOFT + SCORE:
        assert _covered(runs, fp2, n) == 1, n
        assert _covered(head, fp2, n) == 1, n
    wd = {n: next(r[2] for r in runs if r[0] <= fp2.offsets[n] < r[0] + r[1]) for n in SOFT}
    assert all(wd[n] == (0.01 if n.endswith(".weight") else 0.0) for n in SOFT), wd
    for n in fp2.frozen:
        assert not _touched(runs, fp2, n), n
    fp3 = FlatParams(_tiny(3), torch.device("cpu"))
    runs3 = optimizer_runs(fp3)
    all3 = [r for rs in block_runs(fp3).values() for r in rs]
    for n in SOFT + SCORE:
        assert n in fp3.frozen and not _touched(runs3, fp3, n) and not _touched(all3, fp3, n), n
    assert _covered(runs3, fp3, "struc_w1.weight") == 1


def test_soft_mode_optimizer_state_round_trip(tmp_path):
    from k3m_amd import checkpoint as C
    from k3m_amd.params import is_no_decay
    cfg = _tiny(2)
    src = _fake_trainer(cfg, 1, step=5)
    tar = str(tmp_path / "soft.tar")
    C.save_checkpoint(src, tar_path=tar)
    ck = torch.load(tar, map_location="cpu", weights_only=True)
    names = [n for n, _ in src.engine.fp.spec]
    order = [n for n in names if not is_no_decay(n)] + [n for n in names if is_no_decay(n)]
    state = ck["optimizer_state_dict"]["state"]
    fz = src.engine.fp.frozen
    assert set(state) == {i for i, n in enumerate(order) if n not in fz}
    fs = src.engine.fp
    for n in SOFT:
        st = state[order.index(n)]
        o, k = fs.offsets[n], fs.p[n].numel()
        assert st["step"] == 5 and torch.equal(st["exp_avg"].reshape(-1), src.m[o:o + k])
    dst = _fake_trainer(cfg, 2, step=0)
    dst.engine.fp.grad = torch.zeros_like(dst.engine.fp.data)
    assert C.load_checkpoint(dst, tar) == 5
    for n in SOFT + SCORE:
        o, k = fs.offsets[n], fs.p[n].numel()
        assert torch.equal(src.m[o:o + k], dst.m[o:o + k]) and torch.equal(src.v[o:o + k], dst.v[o:o + k]), n
        assert torch.equal(fs.p[n], dst.engine.fp.p[n])


# ---------------------------------------------------------------- DDP ranges (gloo, CPU)
def test_allreduce_ranges_follow_the_mode(tmp_path):
    import torch.distributed as dist
    from k3m_amd.ddp import GradAllReducer
    from k3m_amd.engine import FlatParams
    dist.init_process_group("gloo", init_method="file://" + str(tmp_path / "store"), rank=0, world_size=1)
    try:
        for mode in (2, 3):
            fp = FlatParams(_tiny(mode), torch.device("cpu"))
            red = GradAllReducer(fp, max_bucket_elems=50000)
            every = [r for rs in red.blocks.values() for r in rs]
            cover = torch.zeros(fp.total, dtype=torch.int32)
            for a, b in every:
                cover[a:b] += 1
            assert int(cover.max()) == 1
            for n, sh in fp.spec:
                o, k = fp.offsets[n], math.prod(sh)
                want = 0 if n in fp.frozen else 1
                assert bool((cover[o:o + k] == want).all()), (mode, n)
            head = torch.zeros(fp.total, dtype=torch.int32)
            for a, b in red.blocks[("head", 0)]:
                head[a:b] += 1
            for n in SOFT + SCORE:
                o, k = fp.offsets[n], math.prod(fp.shapes[n])
                assert bool((head[o:o + k] == (1 if mode == 2 else 0)).all()), (mode, n)
            # the exchange itself: a world of one leaves the trainable gradients as they are
            fp.grad.copy_(torch.randn(fp.total, generator=torch.Generator().manual_seed(mode)))
            want = fp.grad.clone()
            red.begin(None)
            for blk in [("head", 0), ("t", 1), ("t", 0), ("v", 0), ("c", 0), ("emb", 0)]:
                red.grad_ready(*blk)
            red.finish()
            assert torch.equal(fp.grad, want)
    finally:
        dist.destroy_process_group()
