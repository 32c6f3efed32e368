"""The K3M step without the image modality (``cfg.use_image`` false): title + property-value knowledge only.

Reference: the ``use_image=False`` branches of BertForMultiModalPreTraining_tri_stru / K3MForItemAlignment
(vilbert_k3m/vilbert_k3m.py) — BertEncoder keeps ``layer`` and ``c_layer_pv_t`` (:1724-1743,
calculate_for_two_text :1510), the fusion gate chooses between the individual stream and the one cross stream
(pre_sampling_sequence :2331-2374 with ``sequence_c1 = None``), ``c_initial = (pooled_t + pooled_pv) / 2`` (:2725),
the NSP score uses ``pooled_t + pooled_pv`` (:1882-1883) and the image loss is a constant zero (:2815).  Only the
hard gate (if_pre_sampling 1) is defined upstream for this model; K3MEngine refuses the others.

A forward / backward pair of its own for the sections whose buffers differ from the tri-modal step's (embeddings,
encoder loop, fusion gate, pooling), over the op classes and drivers of k3m_amd/engine.py; the structure aggregator
+ LPM and the MLM head, forward and backward, are K3MEngine's own methods, shared by both steps.
Layout: ONE text buffer [B*T + B*P, 768] = [title | PV] — no duplicated streams (each stream has a single
partner) and no image work.  The title and PV rows are adjacent in every fusion buffer, so relu-cat, gate and
relu-split each run as one launch over both modalities; only the two scorer GEMMs (different weights) are per
modality, grouped into one launch under GROUP_GATE.
"""
import contextlib

import torch

from . import debug
from . import _lib as L
from . import engine as E
from . import ops


def gate_fwd(eng, ind, XT, seq_tp, noise, rng, BT, BP, save=True):
    """The two-candidate hard gate over [individual | cross] of the [title | PV] rows into seq_tp; returns what the
    backward keeps.  save=False: the forward-only kernel form (no ys / idx; the same draws)."""
    dev, H = eng.device, eng.H
    Nt = BT + BP
    f32 = dict(dtype=torch.float32, device=dev)
    cc = torch.empty((Nt, 2 * H), **f32)
    L.call("k3m_relu_cat2", ind.data_ptr(), XT.data_ptr(), cc.data_ptr(), Nt, H, L.F32, L.stream())
    cclo = eng._lo(cc)
    a = torch.empty((Nt, 2 * H), **f32)
    with (ops.grouped() if E.GROUP_GATE else contextlib.nullcontext()):
        eng.gate["t"].fwd(cclo[0:BT], out=a[0:BT], epi=L.EPI_BIAS_SIGMOID)
        eng.gate["pv"].fwd(cclo[BT:], out=a[BT:], epi=L.EPI_BIAS_SIGMOID)
    ys = torch.empty_like(a) if save else None
    idx = torch.empty((Nt * H,), dtype=torch.uint8, device=dev) if save else None
    nz, off_g = None, 0
    if noise is not None:
        nz = torch.cat([noise["t"].reshape(BT, 2 * H), noise["pv"].reshape(BP, 2 * H)]).to(**f32).contiguous()
    else:
        off_g = rng.take(Nt * 2 * H)
    L.call("k3m_gate2_fwd", a.data_ptr(), cc.data_ptr(), L.ptr(nz), L.ptr(ys), L.ptr(idx), seq_tp.data_ptr(),
           Nt, H, rng.seed, off_g, L.F32, L.stream())
    return (cc, a, ys, idx)


def forward(eng, batch, train=True, noise=None, ent_neg=None, val_neg=None, seed=None, groups=1):
    """K3MEngine.forward for use_image=False.  noise: optional {t: [B,T,2,H], pv: [B,P,2,H]}.  The image
    fields of ``batch`` (image_feat, image_loc, image_mask, image_label, image_target) are not read."""
    c, fp, dev = eng.cfg, eng.fp, eng.device
    if debug.ON:
        debug.check_batch(batch, c, ent_neg, val_neg)
    fp.refresh_shadow()
    H, ED = eng.H, eng.enc_dtype
    ids, tt, mt = batch["input_ids"], batch["segment_ids"], batch["input_mask"]
    pids, ptt, mp = batch["input_ids_pv"], batch["segment_ids_pv"], batch["input_mask_pv"]
    B, T = ids.shape
    P = pids.shape[1]
    BT, BP = B * T, B * P
    Nt = BT + BP
    rng = E.Rng(eng.base_seed * 1000003 + (seed if seed is not None else eng.step_count))
    ph = eng.p_h if train else 0.0
    ctx = {"B": B, "T": T, "P": P, "train": train, "seed": rng.seed}
    mask_t, mask_p = E._ext_mask(mt), E._ext_mask(mp)
    f32 = dict(dtype=torch.float32, device=dev)

    # ---- embeddings: the individual copies and the encoder input, one launch per stream
    XT = torch.empty((Nt, H), **f32)
    ind = torch.empty((Nt, H), **f32)
    xh = torch.empty((Nt, H), **f32)
    rs = torch.empty((Nt,), **f32)
    emb = (fp.p["embeddings.word_embeddings.weight"], fp.p["embeddings.position_embeddings.weight"],
           fp.p["embeddings.token_type_embeddings.weight"], eng.emb_ln.g, eng.emb_ln.b)
    off_t = rng.take(BT * H) if ph > 0 else 0
    ops.embed_fwd(ids, tt, *emb, ind[0:BT], XT[0:BT], None, xh[0:BT], rs[0:BT], ph, rng.seed, off_t)
    off_p = rng.take(BP * H) if ph > 0 else 0
    ops.embed_fwd(pids, ptt, *emb, ind[BT:], XT[BT:], None, xh[BT:], rs[BT:], ph, rng.seed, off_p)
    ctx["emb"] = (xh, rs, off_t, off_p)
    if ED != torch.float32:
        XT = ops.convert(XT, torch.empty((Nt, H), dtype=ED, device=dev))

    # ---- encoder: text layers over (B, T) and (B, P); co_tt[i] alone at each ('c', i)
    # (no such entry without co-attention: every stream once, text layers only)
    view = E._view(train)
    tsegs = [(0, B, T, mask_t), (BT, B, P, mask_p)]
    enc = []
    for kind, i in eng.schedule:
        if kind == "t" and i < eng.fixed_t:   # below the fixed_t_layer cut: forward-only, nothing kept
            XT, _ = E._run(view(eng.text[i]).fwd_steps(XT, tsegs, rng, save=not eng.frozen_nosave))
        elif kind == "t":
            XT, sv = E._run(view(eng.text[i]).fwd_steps(XT, tsegs, rng))
            enc.append((kind, i, sv))
        else:   # stream 1 = PV, stream 2 = title (BertConnectionLayer_two_text)
            op = view(eng.co_tt[i])
            XT2 = torch.empty_like(XT)
            gen = op.fwd_steps(XT[BT:], XT[0:BT], B, P, T, mask_p, mask_t, rng, XT2[BT:], XT2[0:BT])
            sv = E._lockstep([gen])[0] if E.GROUPED else E._run(gen)   # (a group of one is still a grouped launch)
            enc.append((kind, i, (sv, op)))
            XT = XT2
    ctx["enc"] = enc
    if ED != torch.float32:   # encoder -> fp32 fusion / heads
        XT = ops.convert(XT, torch.empty((Nt, H), **f32))

    # ---- two-candidate hard gate over [individual | cross]
    seq_tp = torch.empty((Nt, H), **f32)
    ctx["fus"] = gate_fwd(eng, ind, XT, seq_tp, noise, rng, BT, BP)
    ctx["seq_tp"] = seq_tp

    # ---- pooled outputs and c_initial (:2408-2409, :2725)
    pooled_t = torch.empty((B, H), **f32)
    pooled_pv = torch.empty((B, H), **f32)
    L.call("k3m_seq_mean", seq_tp.data_ptr(), B, T, 1, H, 1.0, pooled_t.data_ptr(), 0, L.F32, L.stream())
    L.call("k3m_seq_mean", seq_tp[BT:].data_ptr(), B, P, 1, H, 1.0, pooled_pv.data_ptr(), 0, L.F32, L.stream())
    c_init = torch.empty((B, H), **f32)
    L.call("k3m_mean2", pooled_t.data_ptr(), pooled_pv.data_ptr(), c_init.data_ptr(), c_init.numel(), L.F32, L.stream())

    # ---- structure aggregator + LPM
    c_final, lpm = eng._struct_fwd(ctx, batch, seq_tp, c_init, rng, ent_neg, val_neg, groups)
    if lpm is None:
        return {"c_initial": c_init, "c_final": c_final, "pooled_t": pooled_t, "pooled_pv": pooled_pv,
                "pooled_v": None}, ctx

    # ---- MLM head on the labelled rows; slot 2 of `losses` (the image loss) stays an exact zero (:2815)
    losses = torch.zeros((4,), **f32)
    labels, cnt = eng._mlm_labels(ctx, batch)
    hint = batch.get("_label_counts")
    if hint is not None:   # the region count of a loader's hint belongs to the unused image fields
        n_m = int(hint[0])
        eng._verify_hint((n_m, 0), cnt)
    else:
        n_m = int(cnt[0])   # host sync (labelled-row count)
    captured = eng._mlm_head(ctx, seq_tp, labels, n_m, losses)

    nsp = torch.empty((1,), **f32)
    L.call("k3m_nsp_loss", pooled_t.data_ptr(), pooled_pv.data_ptr(), None,
           fp.p["cls.seq_relationship.weight"].data_ptr(), fp.p["cls.seq_relationship.bias"].data_ptr(),
           batch["is_next"].contiguous().data_ptr(), batch["is_next_pv_v"].contiguous().data_ptr(),
           batch["is_next_pv_t"].contiguous().data_ptr(), B, H, nsp.data_ptr(), L.stream())
    out = {
        "masked_lm_loss": losses[0:1], "masked_lm_loss_pv": losses[1:2], "masked_img_loss": losses[2:3],
        "loss_lpm": lpm, "next_sentence_loss": nsp, "c_initial": c_init, "c_final": c_final,
        "pooled_t": pooled_t, "pooled_pv": pooled_pv, "pooled_v": None,
    }
    out["loss"] = losses[0:1] + losses[1:2] + losses[2:3] + lpm
    out.update(captured)
    return out, ctx


def backward(eng, ctx, w_mlm=1.0, w_lpm=1.0, grad_ready=None, w_mlm_pv=None):
    """K3MEngine._backward for use_image=False: no image gradient buffers or launches, and nothing accumulates
    into the never-grad score_cross1_*."""
    fp, dev = eng.fp, eng.device
    H = eng.H
    B, T, P = ctx["B"], ctx["T"], ctx["P"]
    BT, BP = B * T, B * P
    Nt = BT + BP
    batch = ctx["batch"]
    seq_tp = ctx["seq_tp"]
    dseq_tp = torch.zeros_like(seq_tp)
    f32 = dict(dtype=torch.float32, device=dev)

    # ---- MLM head, structure aggregator + LPM
    eng._mlm_bwd(ctx, dseq_tp, w_mlm, w_mlm_pv)
    dci = eng._struct_bwd(ctx, dseq_tp, w_lpm)

    # ---- pooled outputs: c_initial = (pooled_t + pooled_pv) / 2
    dpt = torch.empty((B, H), **f32)
    dppv = torch.empty((B, H), **f32)
    L.call("k3m_mean2_bwd", dci.data_ptr(), dpt.data_ptr(), dppv.data_ptr(), dci.numel(), 0, L.F32, L.stream())
    L.call("k3m_seq_mean_bwd", dpt.data_ptr(), B, T, 1, H, 1.0, dseq_tp.data_ptr(), L.F32, L.stream())
    L.call("k3m_seq_mean_bwd", dppv.data_ptr(), B, P, 1, H, 1.0, dseq_tp[BT:].data_ptr(), L.F32, L.stream())

    # ---- gate: elementwise part over both modalities, the two modalities' GEMMs grouped, relu-split
    cc, a, ys, idx = ctx["fus"]
    dc = torch.empty_like(cc)
    dpre = torch.empty_like(cc)
    L.call("k3m_gate2_bwd", dseq_tp.data_ptr(), a.data_ptr(), cc.data_ptr(), ys.data_ptr(), idx.data_ptr(),
           dc.data_ptr(), dpre.data_ptr(), Nt, H, L.F32, L.stream())
    ops.colsum(dpre[0:BT], eng.gate["t"].gb, accumulate=True)
    ops.colsum(dpre[BT:], eng.gate["pv"].gb, accumulate=True)
    dlo, clo = eng._lo(dpre), eng._lo(cc)
    with (ops.grouped() if E.GROUP_GATE else contextlib.nullcontext()):
        for m, (r0, r1) in (("t", (0, BT)), ("pv", (BT, Nt))):
            eng.gate[m].dgrad(dlo[r0:r1], dx=dc[r0:r1], beta=1.0)
            eng.gate[m].wgrad(dlo[r0:r1], clo[r0:r1], bias_done=True)
    d_ind = torch.empty((Nt, H), **f32)
    dXT = torch.empty((Nt, H), **f32)
    L.call("k3m_relu_split2_bwd", dc.data_ptr(), cc.data_ptr(), d_ind.data_ptr(), dXT.data_ptr(), Nt, H, 0, L.F32,
           L.stream())

    # ---- encoder, reversed
    if eng.enc_dtype != torch.float32:
        dXT = ops.convert(dXT, torch.empty(dXT.shape, dtype=eng.enc_dtype, device=dev))
    view = E._view(ctx["train"])
    for kind, i, sv in reversed(ctx["enc"]):
        if kind == "t":
            dXT = E._run(view(eng.text[i]).bwd_steps(dXT, sv))
        else:
            s, op = sv
            dXT2 = torch.empty_like(dXT)
            gen = op.bwd_steps(dXT[BT:], dXT[0:BT], s, dXT2[BT:], dXT2[0:BT])
            if E.GROUPED:
                E._lockstep([gen])
            else:
                E._run(gen)
            dXT = dXT2
        if grad_ready is not None:
            grad_ready(kind, i)

    # ---- embeddings
    ph = eng.p_h if ctx["train"] else 0.0
    if eng.fixed_t == 0:   # (below a cut dXT ends at the cut: the embeddings keep the individual candidate's gradient)
        ops.convert(dXT, d_ind, accumulate=True)
    xh, rs, off_t, off_p = ctx["emb"]
    gword = fp.g["embeddings.word_embeddings.weight"]
    gpos = fp.g["embeddings.position_embeddings.weight"]
    gtyp = fp.g["embeddings.token_type_embeddings.weight"]
    for r0, r1, off, ids, tt in ((0, BT, off_t, batch["input_ids"], batch["segment_ids"]),
                                 (BT, Nt, off_p, batch["input_ids_pv"], batch["segment_ids_pv"])):
        ds = torch.empty((r1 - r0, H), **f32)
        ops.ln_bwd(d_ind[r0:r1], xh[r0:r1], rs[r0:r1], eng.emb_ln.g, ds, ds, eng.emb_ln.gg, eng.emb_ln.gb, p_out=ph,
                   seed=ctx["seed"], off_out=off)
        ops.embed_bwd(ids.contiguous(), tt.contiguous(), ds, gword, gpos, gtyp)
    if grad_ready is not None:
        grad_ready("emb", 0)
