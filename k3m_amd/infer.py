"""Item-embedding inference: K3MEngine.embed.

The eval-mode forward up to c_final over the forward-only kernel forms (no GELU pre-activation, xhat / rstd,
attention probabilities / LSE, gate ys / idx): the op bodies are the training step's (BertLayerOp / ConnectionOp
fwd_steps with save=False, K3MEngine._fusion_fwd / _struct_fwd with save=False), nothing is kept for a backward and
no ctx is returned.

Stream dedup (the merge rule).  Without dropout the two copies of a stream that the wide buffers carry (the title in
passes t.v and t.pv, the PV in passes pv.v and t.pv, the image in passes t.v and pv.v) are identical until the first
op whose inputs differ between them: a co-attention block (the partners differ) or, for the image stream, a layer
with dynamic attention (its gate reads the title for one copy and the PV for the other).  Until then a stream is ONE
buffer; the first co-attention blocks read its rows for both of their roles and write the wide buffers as the
training step does.  infer_plan(cfg) is that rule as a pure function of the config.
"""
import collections

import torch

from . import debug
from . import _lib as L
from . import engine as E
from . import ops
from .params import dynamic_attention

MERGED, SPLIT = "merged", "split"

PlanEntry = collections.namedtuple("PlanEntry", "kind index text image")


def infer_plan(cfg, dedup=True):
    """[PlanEntry(kind, index, text, image)] per schedule entry of embed(): the layout ("merged": one buffer for
    both copies, "split": the wide buffer) of the text streams and of the image stream that the entry READS.  An entry
    runs on what it reads, except a co-attention block, which reads either layout and always writes the wide
    buffers.  image is None without the image modality, where no stream is duplicated (nothing to merge: "split").
    dedup=False (K3M_INFER_DEDUP=0): wide from the start."""
    sch = E.schedule(cfg)
    if not getattr(cfg, "use_image", True):
        return [PlanEntry(k, i, SPLIT, None) for k, i in sch if k != "v"]
    dyn = dynamic_attention(cfg)
    tm = vm = bool(dedup)
    plan = []
    for kind, i in sch:
        if kind == "v" and dyn:   # the copies' partners (title, PV) differ: the layer's inputs differ
            vm = False
        plan.append(PlanEntry(kind, i, MERGED if tm else SPLIT, MERGED if vm else SPLIT))
        if kind == "c":   # each copy met another partner
            tm = vm = False
    return plan


def sequences(eng, batch, noise=None, seed=None):
    """The eval-mode, forward-only encoder and fusion up to the fused sequences: (seq_tp [B T + B P, H] fp32, the
    title rows then the PV rows; seq_v [B R, Hv] fp32, None without the image modality; rng, the call's draw
    state).  The part embed() and predict_masked() (k3m_amd/predict.py) share."""
    if not eng.use_image:
        return _sequences_text(eng, batch, noise, seed)
    c, fp, dev = eng.cfg, eng.fp, eng.device
    if debug.ON:
        debug.check_batch(batch, c)
    fp.refresh_shadow()
    H, Hv, ED = eng.H, eng.Hv, eng.enc_dtype
    ids, tt, mt = batch["input_ids"], batch["segment_ids"], batch["input_mask"]
    pids, ptt, mp = batch["input_ids_pv"], batch["segment_ids_pv"], batch["input_mask_pv"]
    feat, loc, mv = batch["image_feat"], batch["image_loc"], batch["image_mask"]
    B, T = ids.shape
    P, R = pids.shape[1], feat.shape[1]
    BT, BP, BR = B * T, B * P, B * R
    rng = E.Rng(eng.base_seed * 1000003 + (seed if seed is not None else eng.step_count))
    f32 = dict(dtype=torch.float32, device=dev)
    plan = infer_plan(c, eng.infer_dedup)
    # both streams start as one buffer; the plan says where a stream's copies diverge
    tm = vm = bool(eng.infer_dedup)

    mask_t, mask_p, mask_v = E._ext_mask(mt), E._ext_mask(mp), E._ext_mask(mv)
    wide_masks = {}

    def twice(name, m):   # the stacked key mask of a wide segment, built when the stream first runs wide
        if name not in wide_masks:
            wide_masks[name] = torch.cat([m, m]).contiguous()
        return wide_masks[name]

    # ---- embeddings: the fp32 individual candidates; the encoder copies are written in the encoder dtype
    emb = (fp.p["embeddings.word_embeddings.weight"], fp.p["embeddings.position_embeddings.weight"],
           fp.p["embeddings.token_type_embeddings.weight"], eng.emb_ln.g, eng.emb_ln.b)
    ind_t = torch.empty((BT, H), **f32)
    ind_pv = torch.empty((BP, H), **f32)
    if tm:
        XT = torch.empty((BT + BP, H), dtype=ED, device=dev)
        ops.embed_fwd(ids, tt, *emb, ind_t, XT[0:BT], None, None, None, 0.0, rng.seed, 0)
        ops.embed_fwd(pids, ptt, *emb, ind_pv, XT[BT:], None, None, None, 0.0, rng.seed, 0)
    else:
        XT = torch.empty((2 * BT + 2 * BP, H), dtype=ED, device=dev)
        ops.embed_fwd(ids, tt, *emb, ind_t, XT[0:BT], XT[BT:2 * BT], None, None, 0.0, rng.seed, 0)
        ops.embed_fwd(pids, ptt, *emb, ind_pv, XT[2 * BT:2 * BT + BP], XT[2 * BT + BP:], None, None, 0.0, rng.seed, 0)
    feat2 = feat.reshape(BR, feat.shape[2])
    loc2 = loc.reshape(BR, loc.shape[2])
    img = eng.vemb_img.fwd(feat2)
    lce = eng.vemb_loc.fwd(loc2)
    ind_v = torch.empty((BR, Hv), **f32)
    ops.ln_fwd(img, lce, eng.vemb_ln.g, eng.vemb_ln.b, ind_v, None, None)
    del img, lce
    XV = torch.empty((BR if vm else 2 * BR, Hv), dtype=ED, device=dev)
    ops.convert(ind_v, XV[0:BR])   # computed and converted once when merged
    if not vm:
        ops.convert(ind_v, XV[BR:])

    if eng.dyn_attn:   # 0/1 masks of the image streams' text partners: the title (pass 1), the PV (pass 2)
        mt01, mp01 = mt.to(torch.float32).contiguous(), mp.to(torch.float32).contiguous()

    def tparts():   # (title of pass t.v, title of pass t.pv, PV of pass pv.v, PV of pass t.pv)
        if tm:
            return XT[0:BT], XT[0:BT], XT[BT:], XT[BT:]
        return XT[0:BT], XT[BT:2 * BT], XT[2 * BT:2 * BT + BP], XT[2 * BT + BP:]

    def vparts():   # (image of pass t.v, image of pass pv.v)
        return (XV, XV) if vm else (XV[0:BR], XV[BR:])

    # ---- encoder
    for e in plan:
        kind, i = e.kind, e.index
        if kind == "t":
            segs = ([(0, B, T, mask_t), (BT, B, P, mask_p)] if tm else
                    [(0, 2 * B, T, twice("t", mask_t)), (2 * BT, 2 * B, P, twice("p", mask_p))])
            XT, _ = E._run(E._eval_view(eng.text[i]).fwd_steps(XT, segs, rng, save=False))
        elif kind == "v":
            if vm and e.image == SPLIT:   # the copies diverge in this layer: one buffer -> the wide one
                wide = torch.empty((2 * BR, Hv), dtype=ED, device=dev)
                ops.convert(XV, wide[0:BR])
                ops.convert(XV, wide[BR:])
                XV, vm = wide, False
            segs = [(0, B, R, mask_v)] if vm else [(0, 2 * B, R, twice("v", mask_v))]
            partner = None
            if eng.dyn_attn:
                t1, _, p2, _ = tparts()
                partner = [(t1, mt01), (p2, mp01)]
            XV, _ = E._run(E._eval_view(eng.image[i]).fwd_steps(XV, segs, rng, partner=partner, save=False))
        else:
            t1, t3, p2, p3 = tparts()
            v1, v2 = vparts()
            XT2 = torch.empty((2 * BT + 2 * BP, H), dtype=ED, device=dev)
            XV2 = torch.empty((2 * BR, Hv), dtype=ED, device=dev)
            ops_ = [E._eval_view(o) for o in (eng.co_tv[i], eng.co_pv[i], eng.co_tt[i])]
            args = [(v1, t1, B, R, T, mask_v, mask_t, rng, XV2[0:BR], XT2[0:BT]),
                    (v2, p2, B, R, P, mask_v, mask_p, rng, XV2[BR:], XT2[2 * BT:2 * BT + BP]),
                    (p3, t3, B, P, T, mask_p, mask_t, rng, XT2[2 * BT + BP:], XT2[BT:2 * BT])]
            gens = [o.fwd_steps(*a, save=False) for o, a in zip(ops_, args)]
            if E.GROUPED:
                E._lockstep(gens)
            else:
                for g in gens:
                    E._run(g)
            del t1, t3, p2, p3, v1, v2, args, gens
            XT, XV, tm, vm = XT2, XV2, False, False
    if ED != torch.float32:   # encoder -> fp32 fusion
        XT = ops.convert(XT, torch.empty(XT.shape, **f32))
        XV = ops.convert(XV, torch.empty(XV.shape, **f32))

    # ---- fusion (a stream that never split is both of its cross candidates), pooling, structure aggregator
    t1, t3, p2, p3 = tparts()
    v1, v2 = vparts()
    seq_tp = torch.empty((BT + BP, H), **f32)
    seq_v = torch.empty((BR, Hv), **f32)
    streams = {"v": (ind_v, v1, v2, seq_v, Hv), "t": (ind_t, t1, t3, seq_tp[0:BT], H),
               "pv": (ind_pv, p2, p3, seq_tp[BT:], H)}
    eng._fusion_fwd(streams, noise, rng, save=False)
    return seq_tp, seq_v, rng


def embed(eng, batch, noise=None, seed=None, groups=1, keep=None):
    """K3MEngine.embed; see there.  keep: _struct_fwd's (triples)."""
    if not eng.use_image:
        return _embed_text(eng, batch, noise, seed, groups, keep)
    dev, H, Hv = eng.device, eng.H, eng.Hv
    seq_tp, seq_v, rng = sequences(eng, batch, noise, seed)
    B, T = batch["input_ids"].shape
    P, R = batch["input_ids_pv"].shape[1], batch["image_feat"].shape[1]
    BT = B * T
    f32 = dict(dtype=torch.float32, device=dev)
    mean_v = torch.empty((B, Hv), **f32)
    pooled_t = torch.empty((B, H), **f32)
    pooled_pv = torch.empty((B, H), **f32)
    L.call("k3m_seq_mean", seq_v.data_ptr(), B, R, 1, Hv, 1.0, mean_v.data_ptr(), 0, L.F32, L.stream())
    L.call("k3m_seq_mean", seq_tp.data_ptr(), B, T, 1, H, 1.0, pooled_t.data_ptr(), 0, L.F32, L.stream())
    L.call("k3m_seq_mean", seq_tp[BT:].data_ptr(), B, P, 1, H, 1.0, pooled_pv.data_ptr(), 0, L.F32, L.stream())
    pooled_v = eng.map_b2i.fwd(mean_v)
    c_init = torch.empty((B, H), **f32)
    L.call("k3m_mean3", pooled_v.data_ptr(), pooled_t.data_ptr(), pooled_pv.data_ptr(), c_init.data_ptr(),
           c_init.numel(), L.F32, L.stream())
    c_final, _ = eng._struct_fwd({"B": B, "T": T, "P": P}, batch, seq_tp, c_init, rng, None, None, groups, save=False,
                                 keep=keep)
    return {"c_initial": c_init, "c_final": c_final, "pooled_t": pooled_t, "pooled_pv": pooled_pv,
            "pooled_v": pooled_v}


def triples(eng, batch, noise=None, seed=None, groups=1):
    """K3MEngine.triples; see there.  embed() with the structure aggregator's gathered rows kept: p and v are
    views of the thirds of X [B NPV, 3 H] = [c_init | p | v]."""
    keep = {}
    out = embed(eng, batch, noise=noise, seed=seed, groups=groups, keep=keep)
    H = eng.H
    X = keep["X"]
    B = out["c_final"].shape[0]
    X3 = X.view(B, X.shape[0] // B, 3 * H)
    return {"c_final": out["c_final"], "p": X3[:, :, H:2 * H], "v": X3[:, :, 2 * H:], "nvalid": keep["nvalid"]}


def _sequences_text(eng, batch, noise, seed):
    """sequences() of the model without the image modality (k3m_amd/engine_text.py's layout: one [title | PV] buffer,
    no duplicated stream, so nothing merges)."""
    from . import engine_text
    c, fp, dev = eng.cfg, eng.fp, eng.device
    if debug.ON:
        debug.check_batch(batch, c)
    fp.refresh_shadow()
    H, ED = eng.H, eng.enc_dtype
    ids, tt, mt = batch["input_ids"], batch["segment_ids"], batch["input_mask"]
    pids, ptt, mp = batch["input_ids_pv"], batch["segment_ids_pv"], batch["input_mask_pv"]
    B, T = ids.shape
    P = pids.shape[1]
    BT, BP = B * T, B * P
    Nt = BT + BP
    rng = E.Rng(eng.base_seed * 1000003 + (seed if seed is not None else eng.step_count))
    mask_t, mask_p = E._ext_mask(mt), E._ext_mask(mp)
    f32 = dict(dtype=torch.float32, device=dev)
    XT = torch.empty((Nt, H), dtype=ED, device=dev)
    ind = torch.empty((Nt, H), **f32)
    emb = (fp.p["embeddings.word_embeddings.weight"], fp.p["embeddings.position_embeddings.weight"],
           fp.p["embeddings.token_type_embeddings.weight"], eng.emb_ln.g, eng.emb_ln.b)
    ops.embed_fwd(ids, tt, *emb, ind[0:BT], XT[0:BT], None, None, None, 0.0, rng.seed, 0)
    ops.embed_fwd(pids, ptt, *emb, ind[BT:], XT[BT:], None, None, None, 0.0, rng.seed, 0)
    tsegs = [(0, B, T, mask_t), (BT, B, P, mask_p)]
    for kind, i in eng.schedule:
        if kind == "t":
            XT, _ = E._run(E._eval_view(eng.text[i]).fwd_steps(XT, tsegs, rng, save=False))
        else:   # stream 1 = PV, stream 2 = title
            XT2 = torch.empty_like(XT)
            gen = E._eval_view(eng.co_tt[i]).fwd_steps(XT[BT:], XT[0:BT], B, P, T, mask_p, mask_t, rng, XT2[BT:],
                                                       XT2[0:BT], save=False)
            if E.GROUPED:
                E._lockstep([gen])
            else:
                E._run(gen)
            del gen
            XT = XT2
    if ED != torch.float32:
        XT = ops.convert(XT, torch.empty((Nt, H), **f32))
    seq_tp = torch.empty((Nt, H), **f32)
    engine_text.gate_fwd(eng, ind, XT, seq_tp, noise, rng, BT, BP, save=False)
    return seq_tp, None, rng


def _embed_text(eng, batch, noise, seed, groups, keep=None):
    """embed() of the model without the image modality."""
    dev, H = eng.device, eng.H
    seq_tp, _, rng = _sequences_text(eng, batch, noise, seed)
    B, T = batch["input_ids"].shape
    P = batch["input_ids_pv"].shape[1]
    BT = B * T
    f32 = dict(dtype=torch.float32, device=dev)
    pooled_t = torch.empty((B, H), **f32)
    pooled_pv = torch.empty((B, H), **f32)
    L.call("k3m_seq_mean", seq_tp.data_ptr(), B, T, 1, H, 1.0, pooled_t.data_ptr(), 0, L.F32, L.stream())
    L.call("k3m_seq_mean", seq_tp[BT:].data_ptr(), B, P, 1, H, 1.0, pooled_pv.data_ptr(), 0, L.F32, L.stream())
    c_init = torch.empty((B, H), **f32)
    L.call("k3m_mean2", pooled_t.data_ptr(), pooled_pv.data_ptr(), c_init.data_ptr(), c_init.numel(), L.F32, L.stream())
    c_final, _ = eng._struct_fwd({"B": B, "T": T, "P": P}, batch, seq_tp, c_init, rng, None, None, groups, save=False,
                                 keep=keep)
    return {"c_initial": c_init, "c_final": c_final, "pooled_t": pooled_t, "pooled_pv": pooled_pv, "pooled_v": None}
