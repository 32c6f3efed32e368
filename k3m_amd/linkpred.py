"""Link-prediction evaluation: what the LPM objective learned, as rankings.

The structure aggregator scores a triple (item i, property p_ij, value v_ij) by the TransE distance
|c_final_i + p_ij - v_ij|.  Two questions are asked of a pool of triples (a validation set):

* rank_values    which value does this item have for this property?  Every triple's query c_final_i + p_ij is
                 ranked against every value vector of the pool.
* rank_entities  which item does this (property, value) belong to?  v_ij - p_ij against every item's c_final.

Both are ops.lp_rank (k3m_amd/csrc/lprank.hip): the distance GEMM fused with a running top-k and the rank of the
gold candidate over all candidates; the [triples, candidates] matrix is never stored.  The vectors come from
K3MEngine.triples.  Metrics (mean rank, MRR, Hits@k) are computed on the host.
"""
import json

import numpy as np
import torch

from . import ops

_FNV_OFFSET = np.uint64(0xCBF29CE484222325)
_FNV_PRIME = np.uint64(0x100000001B3)
_NONNEG = np.uint64(0x7FFFFFFFFFFFFFFF)


def _host(t):
    return t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)


def _span_keys(batch, index_name):
    """int64 [B, NPV] (a CPU tensor): FNV-1a (64-bit, over the four little-endian bytes of every token id, folded to
    non-negative by clearing the sign bit) of the original token ids of the span index[i, j, 0] .. index[i, j, 1]
    (both ends included) of input_ids_pv; -1 past nvalid (the first j with index_p[i, j, 0] == 0)."""
    ids = _host(batch["input_ids_pv"]).astype(np.int64)
    lab = batch.get("lm_label_ids_pv")
    if lab is not None:   # a masked position holds [MASK] / a random id: its label is the original id
        lab = _host(lab).astype(np.int64)
        ids = np.where(lab != -1, lab, ids)
    index = _host(batch[index_name]).astype(np.int64)
    first = _host(batch["index_p"]).astype(np.int64)[:, :, 0]
    B, NPV = first.shape
    P = ids.shape[1]
    zero = first == 0
    nvalid = np.where(zero.any(1), zero.argmax(1), NPV)
    valid = np.arange(NPV)[None, :] < nvalid[:, None]
    lo, hi = index[:, :, 0], index[:, :, 1]
    h = np.full((B, NPV), _FNV_OFFSET, dtype=np.uint64)
    rows = np.arange(B)[:, None]
    span = int((hi - lo)[valid].max()) + 1 if valid.any() else 0
    for t in range(span):
        pos = lo + t
        live = valid & (pos <= hi) & (pos >= 0) & (pos < P)
        tok = ids[rows, np.clip(pos, 0, P - 1)].astype(np.uint64)
        for b in range(4):
            byte = (tok >> np.uint64(8 * b)) & np.uint64(0xFF)
            h = np.where(live, (h ^ byte) * _FNV_PRIME, h)   # uint64 arithmetic wraps: the hash's modulus
    keys = (h & _NONNEG).astype(np.int64)
    keys[~valid] = -1
    return torch.from_numpy(keys)


def value_keys(batch):
    """int64 [B, NPV]: one key per value span, equal for equal token sequences whatever the item and whether the
    loader masked them (lm_label_ids_pv, where present, restores a masked id).  The group ids of filtered value
    ranking: other occurrences of a triple's own value are neither listed nor counted.  See _span_keys."""
    return _span_keys(batch, "index_v")


def property_keys(batch):
    """int64 [B, NPV]: value_keys' hash over the property spans (index_p)."""
    return _span_keys(batch, "index_p")


class TriplePool(object):
    """The triples of a set of items, on the device: c_final [items, H]; p, v [triples, H] of the valid triples;
    item_row [triples] (the row of c_final a triple belongs to), triple_index [triples] (its j within the item),
    value_key / property_key [triples]; item_ids (host list, one per item)."""

    def __init__(self):
        self._parts = {name: [] for name in ("c_final", "p", "v", "item_row", "triple_index", "value_key",
                                             "property_key")}
        self.item_ids = []
        self._cat = None

    def add(self, triples_result, keys, item_ids):
        """One batch: a K3MEngine.triples result, keys = (value_keys(batch), property_keys(batch)), and the items'
        ids (any JSON-serialisable values, one per item)."""
        cf, p, v, nvalid = (triples_result[name] for name in ("c_final", "p", "v", "nvalid"))
        B, NPV = p.shape[0], p.shape[1]
        if len(item_ids) != B:
            raise ValueError("%d item ids for a batch of %d items" % (len(item_ids), B))
        vk, pk = (k.to(cf.device) for k in keys)
        if vk.shape != (B, NPV) or pk.shape != (B, NPV):
            raise ValueError("keys: two int64 [%d, %d] tensors expected" % (B, NPV))
        valid = torch.arange(NPV, device=cf.device)[None, :] < nvalid.to(torch.int64)[:, None]
        item, j = valid.nonzero(as_tuple=True)
        base = len(self.item_ids)
        parts = {"c_final": cf.float(), "p": p[item, j].float(), "v": v[item, j].float(), "item_row": item + base,
                 "triple_index": j, "value_key": vk[item, j], "property_key": pk[item, j]}
        for name, t in parts.items():
            self._parts[name].append(t.contiguous())
        self.item_ids.extend(i.item() if hasattr(i, "item") else i for i in item_ids)
        self._cat = None

    def tensors(self):
        """{c_final, p, v, item_row, triple_index, value_key, property_key}: the batches joined (once per add)."""
        if self._cat is None:
            if not self.item_ids:
                raise ValueError("an empty pool")
            self._cat = {name: torch.cat(parts).contiguous() for name, parts in self._parts.items()}
        return self._cat

    @property
    def n_items(self):
        return len(self.item_ids)

    @property
    def n_triples(self):
        return sum(int(t.shape[0]) for t in self._parts["item_row"])


def _ranked(q, c, gold, k, farthest, gid=None):
    d2, idx, gold_d2, rank = ops.lp_rank(q.contiguous(), c.contiguous(), gold=gold.contiguous(), k=k, q_gid=gid,
                                         c_gid=gid, farthest=farthest)
    return {"rank": rank, "gold_dist": gold_d2.sqrt(), "idx": idx, "dist": d2.sqrt()}


def _empty(pool, k):
    dev = pool._parts["c_final"][0].device if pool._parts["c_final"] else torch.device("cpu")
    return {"rank": torch.empty((0,), dtype=torch.int64, device=dev), "gold_dist": torch.empty((0,), device=dev),
            "idx": torch.empty((0, k), dtype=torch.int64, device=dev), "dist": torch.empty((0, k), device=dev)}


def rank_values(pool, k, farthest=False, filtered=True):
    """Value ranking over a TriplePool: for every triple the query c_final_i + p_ij against every value vector v of
    the pool; the gold is the triple's own v.  filtered=True: the value keys are the group ids, so other triples that
    carry the same value (the same token sequence) are neither listed nor counted; False is the raw ranking.
    Returns {rank [n] int64, gold_dist [n], idx [n, k] (rows of the pool's triples; -1 padding), dist [n, k]}:
    Euclidean distances (the square roots are taken here, not in the op), nearest first (farthest=True: farthest
    first, for a model trained with the reference's loss sign)."""
    if pool.n_triples == 0:
        return _empty(pool, k)
    t = pool.tensors()
    q = t["c_final"][t["item_row"]] + t["p"]
    gold = torch.arange(pool.n_triples, dtype=torch.int64, device=q.device)
    return _ranked(q, t["v"], gold, k, farthest, t["value_key"] if filtered else None)


def rank_entities(pool, k, farthest=False):
    """Entity ranking over a TriplePool: for every triple the query v_ij - p_ij against every item's c_final; the
    gold is the triple's item.  Returns rank_values' fields, idx holding rows of the pool's items.  The ranking is
    raw: the filtered setting would exempt, per query, every item that carries the same (property, value), and one
    group id per candidate cannot express "items sharing this triple" (an item belongs to as many groups as it has
    triples)."""
    if pool.n_triples == 0:
        return _empty(pool, k)
    t = pool.tensors()
    return _ranked(t["v"] - t["p"], t["c_final"], t["item_row"], k, farthest)


def link_metrics(rank, ks=(1, 3, 10)):
    """{"n", "mr", "mrr", "hits@k"..., "skipped"} of a rank vector, on the host: mean rank, mean reciprocal rank and
    the share of ranks <= k.  Rows with rank 0 (no gold) are left out and counted in "skipped"; n == 0 gives zeros."""
    r = _host(rank).astype(np.int64).reshape(-1)
    keep = r > 0
    n = int(keep.sum())
    r = r[keep].astype(np.float64)
    out = {"n": n, "mr": float(r.mean()) if n else 0.0, "mrr": float((1.0 / r).mean()) if n else 0.0}
    for kk in ks:
        out["hits@%d" % kk] = float((r <= kk).mean()) if n else 0.0
    out["skipped"] = int((~keep).sum())
    return out


def eval_ks(k):
    """The Hits@k columns of a top-k evaluation: 1, 3 and k itself, those not above k."""
    return tuple(sorted({kk for kk in (1, 3, k) if kk <= k}))


TASKS = ("value", "entity")


class LinkEval(object):
    """Link-prediction metrics over the batches of a validation set (the MaskedEval of this task): add() pools the
    triples of a batch, close() ranks the pool (both tasks) and, with a path, writes one JSON line per triple:
    item_id, triple (its index within the item), value_rank, value_topk as [[item_id, triple], ...] and entity_rank.
    summary(): {"value" / "entity": link_metrics + "gold_dist" (mean distance of the gold) and "top1_dist" (mean
    distance of the rank-1 neighbour)}."""

    def __init__(self, k, path="", farthest=False, filtered=True):
        self.k, self.ks = k, eval_ks(k)
        self.farthest, self.filtered = farthest, filtered
        self.pool = TriplePool()
        self.path = path
        self._summary = None

    def add(self, trainer, batch, item_ids, **kw):
        self.pool.add(trainer.triples(batch, **kw), (value_keys(batch), property_keys(batch)), item_ids)

    def _stats(self, res):
        m = link_metrics(res["rank"], self.ks)
        n = int(res["rank"].shape[0])
        m["gold_dist"] = float(res["gold_dist"].double().mean()) if n else 0.0
        m["top1_dist"] = float(res["dist"][:, 0].double().mean()) if n else 0.0
        return m

    def close(self):
        if self._summary is not None:
            return
        val = rank_values(self.pool, self.k, farthest=self.farthest, filtered=self.filtered)
        ent = rank_entities(self.pool, self.k, farthest=self.farthest)
        self._summary = {"value": self._stats(val), "entity": self._stats(ent)}
        if not self.path:
            return
        with open(self.path, "w") as f:
            if self.pool.n_triples == 0:
                return
            ids = self.pool.item_ids
            t = self.pool.tensors()
            item, tri = t["item_row"].cpu().tolist(), t["triple_index"].cpu().tolist()
            vr, er, vi = val["rank"].cpu().tolist(), ent["rank"].cpu().tolist(), val["idx"].cpu().tolist()
            for n in range(len(item)):
                rec = {"item_id": ids[item[n]], "triple": tri[n], "value_rank": vr[n],
                       "value_topk": [[ids[item[r]], tri[r]] for r in vi[n] if r >= 0], "entity_rank": er[n]}
                f.write(json.dumps(rec, ensure_ascii=False) + "\n")

    def summary(self):
        self.close()
        return self._summary
