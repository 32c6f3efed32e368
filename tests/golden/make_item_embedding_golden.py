"""Fixtures of item-embedding inference and of the fine-tuning driver's command line — BUILD container only.

* ``golden_item_embedding.npz``: ``c_initial`` / ``c_final`` of both items from the reference's own
  ``K3MForItemAlignment.item_embedding`` (vilbert_k3m/vilbert_k3m.py:3329-3377), called once per item on the inputs,
  and weights (``weight_seed``) of ``golden_ft_ce.npz``, model.eval(), explicit gumbel noise per item.  The generator
  refuses a fixture in which any hard-gate choice lies within TIE_MARGIN of a tie (make_visual_target_golden.py
  explains the margin): such a fixture would pin rounding, not the model.  golden_ft_ce's own noise IS refused: of its
  655,360 choices the closest lies 4.8e-7 from a tie (printed by the first pass below), and one flipped choice moves a
  pooled output by about |candidate difference| / (3 L), past the 1e-4 bar.  At that size unit noise leaves about a
  dozen choices within the margin for any seed, so, as make_dynamic_attention_golden.py does, the recorded noise is
  NOISE_SCALE x gumbel(0, 1) and the generator takes the first ``noise_seed`` from golden_ft_ce's on (item 1: seed,
  item 2: seed + 1) that leaves no choice within the margin; it exits non-zero and writes nothing if there is none
  among SEEDS.  ``noise_seed``, ``noise_scale`` and the smallest gap (``gate_min_gap``) are recorded.
* ``finetune_cli.json``: the options of the reference's ``finetune.py`` parser (:1223-1288) as data: option string,
  dest, type name, default, required, and whether it is a flag.  The parser is imported and built at run time; none of
  its text is embedded here.

Usage:  python tests/golden/make_item_embedding_golden.py [item_embedding] [cli]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, REPO)
from make_golden import REF, _stub_imports, gumbel_noise  # noqa: E402
from make_finetune_golden import ref_cfg  # noqa: E402
from make_visual_target_golden import TIE_MARGIN  # noqa: E402

NOISE_SCALE = 8.0
SEEDS = 400


def item_embedding_case():
    import vilbert_k3m.vilbert_k3m as K
    from k3m_amd.weights import param_values
    d = np.load(os.path.join(HERE, "golden_ft_ce.npz"), allow_pickle=False)
    g = {k: d[k] for k in d.files}
    cfg, rcfg = ref_cfg(str(g["loss_type"]), int(g["mode"]))
    torch.manual_seed(0)
    model = K.K3MForItemAlignment(rcfg)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in param_values(cfg, int(g["weight_seed"])).items()},
                          strict=True)
    model.eval()
    B, T = g["out/input_ids_1"].shape
    P = g["out/input_ids_pv_1"].shape[1]
    R = g["out/coll_image_feat_1"].shape[1]
    shapes = [("v", (B, R, 3, 1024)), ("t", (B, T, 3, 768)), ("pv", (B, P, 3, 768))]
    state = {"noise": None, "calls": [], "gaps": [], "scores": []}

    def gaps_of(z, dim):
        top = torch.topk(z, 2, dim=dim).values
        return (top.select(dim, 0) - top.select(dim, 1)).reshape(-1)

    def fake_gumbel(logits, tau=1.0, hard=False, eps=1e-10, dim=-1):
        key = "v" if logits.shape[-1] == 1024 else ("t" if logits.shape[1] == T else "pv")
        state["calls"].append(key)
        state["scores"].append((key, dim, logits.detach().clone()))   # (do not depend on the noise)
        z = logits + state["noise"][key]
        state["gaps"].append(gaps_of(z, dim))
        y = (z / tau).softmax(dim)
        idx = y.max(dim, keepdim=True)[1]
        return torch.zeros_like(logits).scatter_(dim, idx, 1.0) - y.detach() + y

    K.F.gumbel_softmax = fake_gumbel
    t = lambda k: torch.from_numpy(np.ascontiguousarray(g["out/" + k]))  # noqa: E731

    def noise_of(seed, scale):
        return {n: torch.from_numpy(v * np.float32(scale)) for n, v in gumbel_noise(seed, shapes).items()}

    def run(seed, scale):
        state["calls"], state["gaps"], state["scores"] = [], [], []
        out = {}
        with torch.no_grad():
            for k in (1, 2):
                state["noise"] = noise_of(seed + k - 1, scale)
                ci, cf = model.item_embedding(
                    t("input_ids_%d" % k), t("coll_image_feat_%d" % k), t("coll_image_loc_%d" % k),
                    token_type_ids=t("segment_ids_%d" % k), attention_mask=t("input_mask_%d" % k),
                    image_attention_mask=t("coll_image_mask_%d" % k), input_ids_pv=t("input_ids_pv_%d" % k),
                    token_type_ids_pv=t("segment_ids_pv_%d" % k), attention_mask_pv=t("input_mask_pv_%d" % k),
                    index_p=t("index_p_%d" % k), index_v=t("index_v_%d" % k))
                out["c_initial_%d" % k], out["c_final_%d" % k] = ci.numpy(), cf.numpy()
        assert state["calls"] == ["v", "t", "pv", "v", "t", "pv"], state["calls"]
        return out, float(torch.cat(state["gaps"]).min())

    seed0 = int(g["noise_seed"])
    _, gap0 = run(seed0, 1.0)
    print("golden_ft_ce's own noise: smallest hard-gate gap %.3e (TIE_MARGIN %.0e): %s"
          % (gap0, TIE_MARGIN, "refused" if gap0 < TIE_MARGIN else "accepted"))
    scores = list(state["scores"])   # three per item, in call order

    def min_gap(seed):
        m = float("inf")
        for item in (0, 1):
            nz = noise_of(seed + item, NOISE_SCALE)
            for key, dim, sc in scores[3 * item:3 * item + 3]:
                m = min(m, float(gaps_of(sc + nz[key], dim).min()))
                if m < TIE_MARGIN:
                    return m
        return m
    seed = next((s_ for s_ in range(seed0, seed0 + SEEDS) if min_gap(s_) >= TIE_MARGIN), None)
    if seed is None:
        print("refused: no noise seed in [%d, %d) without a near-tie; nothing written" % (seed0, seed0 + SEEDS))
        return 1
    res, gap = run(seed, NOISE_SCALE)
    print("noise_seed %d at %gx noise: smallest hard-gate gap %.3e" % (seed, NOISE_SCALE, gap))
    if gap < TIE_MARGIN:
        print("refused: a gate choice lies within TIE_MARGIN of a tie; nothing written")
        return 1
    res["gate_min_gap"] = np.array(gap, np.float64)
    res["noise_seed"], res["noise_scale"] = np.array(seed), np.array(NOISE_SCALE, np.float64)
    res["weight_seed"] = np.array(int(g["weight_seed"]))
    res["source"] = np.array("golden_ft_ce")
    path = os.path.join(HERE, "golden_item_embedding.npz")
    np.savez_compressed(path, **res)
    print("item_embedding ->", path, os.path.getsize(path) // 1024, "KiB")
    return 0


def cli_case():
    """Build the reference's parser without parsing: its get_parser() ends in parse_args(), which is replaced for the
    call by a function that hands the parser itself back."""
    sys.path.insert(0, REF)
    import importlib
    orig = argparse.ArgumentParser.parse_args
    argparse.ArgumentParser.parse_args = lambda self, *a, **k: self
    try:
        ref = importlib.import_module("finetune")
        assert os.path.dirname(os.path.abspath(ref.__file__)) == os.path.abspath(REF), ref.__file__
        parser = ref.get_parser()
    finally:
        argparse.ArgumentParser.parse_args = orig
    opts = []
    for a in parser._actions:
        if not a.option_strings or a.dest == "help":
            continue
        flag = isinstance(a, argparse._StoreTrueAction)
        opts.append({"option": a.option_strings[0], "dest": a.dest, "flag": flag,
                     "type": None if flag or a.type is None else a.type.__name__, "default": a.default,
                     "required": bool(a.required)})
    path = os.path.join(HERE, "finetune_cli.json")
    json.dump({"options": opts}, open(path, "w"), indent=1)
    print("cli ->", path, len(opts), "options")
    return 0


if __name__ == "__main__":
    _stub_imports()
    torch.set_num_threads(16)
    what = sys.argv[1:] or ["item_embedding", "cli"]
    rc = 0
    if "cli" in what:
        rc |= cli_case()
    if "item_embedding" in what:
        rc |= item_embedding_case()
    sys.exit(rc)
