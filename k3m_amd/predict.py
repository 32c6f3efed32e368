"""Masked-token and masked-region prediction: K3MEngine.predict_masked.

The eval-mode, forward-only encoder and fusion of embed() (infer.sequences), then the two prediction heads on the
selected rows alone, each ending in ops.topk_logits (k3m_amd/csrc/topk_logits.hip): the decoder GEMM fused with a
running top-k, the log-sum-exp and the gold logit, so no [rows, vocabulary] logits exist.  Nothing is kept for a
backward and no ctx is returned.  masked_metrics() turns a result into accuracy@k and the gold NLL on the host.
"""
import json

import torch

from . import _lib as L
from . import infer
from . import ops

STREAMS = ("t", "pv", "v")


def _compact(flags, n, thresh, inner, outer, base, slot, idx, lab, src, cnt):
    """k3m_compact_labels_ex over flags (int64 [n rows]): appends the rows with flags >= thresh at cnt[0]."""
    L.call("k3m_compact_labels_ex", flags.data_ptr(), n, thresh, inner, outer, base, slot, idx.data_ptr(), L.ptr(lab),
           L.ptr(src), None, None, cnt.data_ptr(), L.stream())


def _positions(pos, n_items, length, name):
    if not isinstance(pos, torch.Tensor) or pos.dtype != torch.int64 or pos.dim() != 2 or pos.shape[1] != 2:
        raise ValueError("rows[%r]: an int64 [n, 2] tensor of (item, position) expected" % name)
    if pos.numel():
        p = pos.cpu()
        if int(p[:, 0].min()) < 0 or int(p[:, 0].max()) >= n_items or int(p[:, 1].min()) < 0 \
                or int(p[:, 1].max()) >= length:
            raise ValueError("rows[%r]: (item, position) outside [0, %d) x [0, %d)" % (name, n_items, length))
    return pos


def _head(eng, seq, rows, n, lin, ln, W, bias, k, gold):
    """One prediction head (BertLMPredictionHead / BertImgPredictionHead) on n gathered rows of seq, forward-only:
    transform GEMM with the bias+GELU epilogue, LN, fused decoder top-k.  Returns (scores, idx, lse, gold_score)."""
    dev = eng.device
    f32 = dict(dtype=torch.float32, device=dev)
    if n == 0:
        return (torch.empty((0, k), **f32), torch.empty((0, k), dtype=torch.int64, device=dev), torch.empty((0,), **f32),
                torch.empty((0,), **f32) if gold is not None else None)
    h = torch.empty((n, seq.shape[1]), **f32)
    ops.gather_rows(seq, rows, n, h)
    h1 = lin.fwd(h, epi=L.EPI_BIAS_GELU)   # aux None: the forward-only epilogue
    hl = torch.empty_like(h)
    ops.ln_fwd(h1, None, ln.g, ln.b, hl, None, None)
    return ops.topk_logits(hl, W, bias, k=k, gold=gold)


def _stream(pos, scores, idx, lse, gold, gold_score):
    out = {"pos": pos, "idx": idx, "logprob": scores - lse[:, None], "lse": lse}
    if gold is not None:
        out["gold"] = gold
        out["gold_logprob"] = gold_score - lse
    return out


def predict_masked(eng, batch, k=10, rows="labels", noise=None, seed=None, mask_id=103):
    """K3MEngine.predict_masked; see there."""
    if eng.task != "pretrain":
        raise ValueError("predict_masked: the %r engine has no prediction heads" % (eng.task,))
    if isinstance(k, bool) or not isinstance(k, int) or not 1 <= k <= ops.TOPK_LOGITS_MAX_K:
        raise ValueError("k = %r: an int in [1, %d]" % (k, ops.TOPK_LOGITS_MAX_K))
    explicit = isinstance(rows, dict)
    if not explicit and rows not in ("labels", "mask"):
        raise ValueError("rows = %r: 'labels', 'mask' or a dict of (item, position) tensors" % (rows,))
    if explicit and set(rows) - set(STREAMS):
        raise ValueError("rows: unknown stream(s) %s" % sorted(set(rows) - set(STREAMS)))
    dev, fp, c = eng.device, eng.fp, eng.cfg
    ids, pids = batch["input_ids"], batch["input_ids_pv"]
    B, T = ids.shape
    P = pids.shape[1]
    BT, BP = B * T, B * P
    regions = eng.use_image and eng.visual_target == 0
    R = batch["image_feat"].shape[1] if eng.use_image else 0
    R1 = R - 1
    i32 = dict(dtype=torch.int32, device=dev)
    i64 = dict(dtype=torch.int64, device=dev)

    # ---- row selection, in compaction order (title rows, then PV rows, row-major; then the regions)
    gold_m = gold_v = src_v = None
    if explicit:
        pt = _positions(rows.get("t", torch.empty((0, 2), dtype=torch.int64)), B, T, "t").to(dev)
        pp = _positions(rows.get("pv", torch.empty((0, 2), dtype=torch.int64)), B, P, "pv").to(dev)
        n_t, n_pv = pt.shape[0], pp.shape[0]
        idx_m = torch.cat([pt[:, 0] * T + pt[:, 1], BT + pp[:, 0] * P + pp[:, 1]]).to(torch.int32).contiguous()
        if "lm_label_ids" in batch and "lm_label_ids_pv" in batch:
            gold_m = torch.cat([batch["lm_label_ids"][pt[:, 0], pt[:, 1]],
                                batch["lm_label_ids_pv"][pp[:, 0], pp[:, 1]]]).to(torch.int64).contiguous()
        n_v = 0
        if regions and "v" in rows:
            pv_ = _positions(rows["v"], B, R1, "v").to(dev)
            n_v = pv_.shape[0]
            idx_v = (pv_[:, 0] * R + pv_[:, 1] + 1).to(torch.int32).contiguous()
            src_v = (pv_[:, 0] * R1 + pv_[:, 1]).contiguous()
    else:
        by_label = rows == "labels"
        if by_label:
            ft, fpv, thresh = batch["lm_label_ids"].contiguous(), batch["lm_label_ids_pv"].contiguous(), 0
        else:   # no label field is read
            ft, fpv, thresh = (ids == mask_id).to(torch.int64), (pids == mask_id).to(torch.int64), 1
        idx_m = torch.zeros((BT + BP,), **i32)
        lab_m = torch.zeros((BT + BP,), **i64) if by_label else None
        cnt = torch.zeros((3,), **i32)   # [0] title + PV rows, [1] regions, [2] title rows
        _compact(ft, BT, thresh, T, T, 0, 0, idx_m, lab_m, None, cnt)
        cnt[2:3].copy_(cnt[0:1])
        _compact(fpv, BP, thresh, P, P, BT, 1, idx_m, lab_m, None, cnt)
        with_v = regions and "image_label" in batch
        if with_v:
            idx_v = torch.zeros((B * R1,), **i32)
            src32 = torch.zeros((B * R1,), **i32)
            _compact(batch["image_label"].contiguous(), B * R1, 1, R1, R, 1, 2, idx_v, None, src32, cnt[1:2])
        n_m, n_v, n_t = [int(x) for x in cnt.tolist()]   # the host sync forward() makes for its labelled-row counts
        n_pv = n_m - n_t
        if by_label:
            gold_m = lab_m[:n_m]
        if with_v:
            src_v = src32[:n_v].to(torch.int64)
    n_m = n_t + n_pv

    # ---- encoder and fusion, as embed()
    seq_tp, seq_v, _ = infer.sequences(eng, batch, noise, seed)

    # ---- heads on the selected rows; the decoders are the fp32 master weights in either engine dtype
    E = fp.p["embeddings.word_embeddings.weight"]
    s, i, lse, gs = _head(eng, seq_tp, idx_m, n_m, eng.mlm_t, eng.mlm_ln, E, fp.p["cls.predictions.bias"], k, gold_m)
    rows_m = idx_m[:n_m].to(torch.int64)
    pos_t = torch.stack([rows_m[:n_t] // T, rows_m[:n_t] % T], 1)
    pos_pv = torch.stack([(rows_m[n_t:] - BT) // P, (rows_m[n_t:] - BT) % P], 1)

    def part(a, lo, hi):
        return None if a is None else a[lo:hi]
    out = {"t": _stream(pos_t, s[:n_t], i[:n_t], lse[:n_t], part(gold_m, 0, n_t), part(gs, 0, n_t)),
           "pv": _stream(pos_pv, s[n_t:], i[n_t:], lse[n_t:], part(gold_m, n_t, n_m), part(gs, n_t, n_m))}
    if regions and (src_v is not None):
        Cv = c.v_target_size
        if "image_target" in batch:
            tgt = batch["image_target"].reshape(B * R1, Cv)
            gold_v = tgt[src_v].argmax(1).contiguous() if n_v else torch.empty((0,), **i64)
        s, i, lse, gs = _head(eng, seq_v, idx_v, n_v, eng.img_t, eng.img_ln, fp.p["cls.imagePredictions.decoder.weight"],
                              fp.p["cls.imagePredictions.decoder.bias"], k, gold_v)
        pos_v = torch.stack([src_v // R1, src_v % R1], 1)
        out["v"] = _stream(pos_v, s, i, lse, gold_v, gs)
    return out


def masked_metrics(result, ks=(1, 5, 10)):
    """{stream: {"n": rows with a gold, "nll": mean -gold_logprob, "acc@k": share of those rows whose gold is among
    the first k predictions, for every k of ks}} over the streams of a predict_masked result that carry a gold (rows
    whose gold is -1 are not counted).  Computed on the host.  A k larger than the result's is an error."""
    out = {}
    for name in STREAMS:
        r = result.get(name)
        if r is None or "gold" not in r:
            continue
        idx, gold, glp = r["idx"].cpu(), r["gold"].cpu(), r["gold_logprob"].cpu().double()
        if ks and max(ks) > idx.shape[1]:
            raise ValueError("accuracy@%d from a top-%d result" % (max(ks), idx.shape[1]))
        keep = gold >= 0
        n = int(keep.sum())
        idx, gold, glp = idx[keep], gold[keep], glp[keep]
        m = {"n": n, "nll": float(-glp.sum() / n) if n else float("nan")}
        for kk in ks:
            hit = (idx[:, :kk] == gold[:, None]).any(1)
            m["acc@%d" % kk] = float(hit.double().sum() / n) if n else float("nan")
        out[name] = m
    return out


STREAM_NAMES = {"t": "title", "pv": "pv", "v": "region"}


def eval_ks(k):
    """The accuracy@k columns of a top-k evaluation: 1, 5 and k itself, those not above k."""
    return tuple(sorted({kk for kk in (1, 5, k) if kk <= k}))


class MaskedEval(object):
    """Accuracy@k and gold NLL of predict_masked results summed over the batches of a validation set, and (path
    given) one JSON line per predicted position: item_id, stream, position, gold, topk as [[id, logprob], ...]."""

    def __init__(self, k, path=""):
        self.k, self.ks = k, eval_ks(k)
        self.sums = {}
        self.out = open(path, "w") if path else None

    def add(self, result, item_ids):
        for name, m in masked_metrics(result, self.ks).items():
            s = self.sums.setdefault(name, {"n": 0, "nll": 0.0, **{"acc@%d" % kk: 0.0 for kk in self.ks}})
            if m["n"]:
                s["n"] += m["n"]
                for key in s:
                    if key != "n":
                        s[key] += m[key] * m["n"]
        if self.out is None:
            return
        for name in STREAMS:
            r = result.get(name)
            if r is None:
                continue
            pos, idx, lp = r["pos"].cpu().tolist(), r["idx"].cpu().tolist(), r["logprob"].cpu().tolist()
            gold = r["gold"].cpu().tolist() if "gold" in r else [None] * len(pos)
            for (item, p), ii, ll, g in zip(pos, idx, lp, gold):
                iid = item_ids[item]
                rec = {"item_id": iid.item() if hasattr(iid, "item") else iid, "stream": name, "position": p,
                       "gold": g, "topk": [[a, b] for a, b in zip(ii, ll)]}
                self.out.write(json.dumps(rec, ensure_ascii=False) + "\n")

    def summary(self):
        """{stream: {"n", "nll", "acc@k"...}}: the means over all rows added."""
        return {name: {key: (v if key == "n" else (v / s["n"] if s["n"] else float("nan"))) for key, v in s.items()}
                for name, s in self.sums.items()}

    def close(self):
        if self.out is not None:
            self.out.close()
            self.out = None
