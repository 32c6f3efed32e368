"""Top-k item retrieval over item embeddings: the consumer of K3MEngine.embed / item_embedding.

    index = build_index(model, item_batches)             # embed a catalogue once (forward-only path)
    scores, rows, ids = index.search(queries, k=10)      # the k most similar items of every query, on the GPU
    rank_metrics(ids, truth)                             # Rank@1/5/10, the paper's downstream metric

The search is ops.topk_sim (k3m_amd/csrc/topk.hip): the similarity GEMM fused with a running top-k, run block by
block over the stored embeddings with ``accumulate``, so the [queries, catalogue] score matrix never exists.
"""
import os

import numpy as np
import torch

from . import ops

METRICS = ("cosine", "inner")
BLOCK_ROWS = 1 << 18   # rows per stored block (768 MB of fp32 at H = 768)


class ItemIndex(object):
    """A catalogue of item embeddings on the device, kept in blocks of at most ``block_rows`` rows.  Row r of the
    index (the order of the add() calls) belongs to item ``ids[r]``."""

    def __init__(self, metric="cosine", device=None, block_rows=BLOCK_ROWS):
        if metric not in METRICS:
            raise ValueError("metric %r: one of %s" % (metric, METRICS))
        if int(block_rows) < 1:
            raise ValueError("block_rows must be positive")
        self.metric = metric
        self.device = torch.device(device) if device is not None else torch.device("cuda")
        self.block_rows = int(block_rows)
        self.ids = []
        self.blocks = []   # fp32 [n_b, H] device tensors, every one but the last with block_rows rows
        self.hidden = None

    def __len__(self):
        return len(self.ids)

    def add(self, item_ids, embeddings):
        """Append items: ``item_ids`` a list of n ids (int or str), ``embeddings`` an fp32 [n, H] tensor."""
        item_ids = list(item_ids)
        if not isinstance(embeddings, torch.Tensor) or embeddings.dim() != 2:
            raise ValueError("embeddings: a 2-D tensor [n, H] expected")
        if embeddings.dtype != torch.float32:
            raise ValueError("embeddings: dtype %s, float32 expected" % embeddings.dtype)
        if embeddings.shape[0] != len(item_ids):
            raise ValueError("%d item ids for %d embedding rows" % (len(item_ids), embeddings.shape[0]))
        H = embeddings.shape[1]
        if self.hidden is not None and H != self.hidden:
            raise ValueError("embeddings have %d columns, the index has %d" % (H, self.hidden))
        if H % 4 != 0 or not 4 <= H <= 4096:
            raise ValueError("H = %d: a multiple of 4 in [4, 4096]" % H)
        self.hidden = H
        e = embeddings.detach().to(self.device)
        pos = 0
        while pos < e.shape[0]:
            if self.blocks and self.blocks[-1].shape[0] < self.block_rows:
                take = min(self.block_rows - self.blocks[-1].shape[0], e.shape[0] - pos)
                self.blocks[-1] = torch.cat([self.blocks[-1], e[pos:pos + take]]).contiguous()
            else:
                take = min(self.block_rows, e.shape[0] - pos)
                self.blocks.append(e[pos:pos + take].clone().contiguous())
            pos += take
        self.ids.extend(item_ids)

    def embeddings(self):
        """All stored rows as one fp32 [len, H] device tensor (a copy)."""
        if not self.blocks:
            return torch.empty((0, self.hidden or 0), dtype=torch.float32, device=self.device)
        return torch.cat(self.blocks)

    def search(self, queries, k, query_ids=None):
        """(scores [Nq, k] fp32, rows [Nq, k] int64, ids): the k most similar stored items of every query row, best
        first (equal scores: lower row first).  ids[i][j] is the item id of rows[i, j], or None for a slot past the
        number of eligible items (row -1, score -inf).  query_ids: a list of Nq item ids; a query never retrieves
        the stored item with its own id (catalogue-against-itself search)."""
        q = queries.detach().to(self.device).contiguous()
        q_rows = None
        if query_ids is not None:
            query_ids = list(query_ids)
            if len(query_ids) != q.shape[0]:
                raise ValueError("%d query ids for %d queries" % (len(query_ids), q.shape[0]))
            row_of = {}
            for r, i in enumerate(self.ids):
                row_of.setdefault(i, r)
            q_rows = torch.tensor([row_of.get(i, -1) for i in query_ids], dtype=torch.int64, device=self.device)
        out, base = None, 0
        for blk in self.blocks:
            out = ops.topk_sim(q, blk, k, metric=self.metric, c_base=base, q_ids=q_rows, out=out,
                               accumulate=out is not None)
            base += blk.shape[0]
        if out is None:   # an empty index: the padding
            empty = torch.empty((0, q.shape[1]), dtype=torch.float32, device=self.device)
            out = ops.topk_sim(q, empty, k, metric=self.metric)
        scores, rows = out
        ids = [[self.ids[r] if r >= 0 else None for r in row] for row in rows.cpu().tolist()]
        return scores, rows, ids

    # ---- a directory of .npy files: meta.npy (metric as a string), ids.npy, block_<b>.npy
    def save(self, path):
        os.makedirs(path, exist_ok=True)
        ids = np.asarray(self.ids) if self.ids else np.zeros((0,), np.int64)
        if ids.ndim != 1 or ids.dtype.kind not in "iuU":
            raise ValueError("item ids must be all ints or all strings to be saved")
        np.save(os.path.join(path, "meta.npy"), np.asarray([self.metric, str(len(self.blocks)), str(self.block_rows)]),
                allow_pickle=False)
        np.save(os.path.join(path, "ids.npy"), ids, allow_pickle=False)
        for b, blk in enumerate(self.blocks):
            np.save(os.path.join(path, "block_%d.npy" % b), blk.cpu().numpy(), allow_pickle=False)

    @classmethod
    def load(cls, path, device=None):
        meta = np.load(os.path.join(path, "meta.npy"), allow_pickle=False)
        index = cls(metric=str(meta[0]), device=device, block_rows=int(meta[2]))
        ids = np.load(os.path.join(path, "ids.npy"), allow_pickle=False).tolist()
        n = 0
        for b in range(int(meta[1])):
            blk = np.load(os.path.join(path, "block_%d.npy" % b), allow_pickle=False)
            index.add(ids[n:n + blk.shape[0]], torch.from_numpy(blk))
            n += blk.shape[0]
        if n != len(ids):
            raise ValueError("%s: %d ids for %d embedding rows" % (path, len(ids), n))
        return index


_EMBED_ARGS = ("input_ids", "image_feat", "image_loc", "token_type_ids", "attention_mask", "image_attention_mask",
               "input_ids_pv", "token_type_ids_pv", "attention_mask_pv", "index_p", "index_v")


def build_index(model, item_batches, metric="cosine", seed=0):
    """An ItemIndex of c_final of every item of ``item_batches`` through ``model.item_embedding`` (K3MForItemAlignment:
    the forward-only path).  A batch is a dict with item_embedding's argument names plus "item_ids"; batch b draws
    the hard gate with seed + b (as write_predictions does), so the index is reproducible from the call."""
    index = ItemIndex(metric=metric, device=model.engine.device)
    for b, batch in enumerate(item_batches):
        kw = {k: batch[k] for k in _EMBED_ARGS if batch.get(k) is not None}
        _, c_final = model.item_embedding(noise=batch.get("noise"), seed=int(seed) + b, **kw)
        index.add(batch["item_ids"], c_final)
    return index


def retrieve_pairs(model, batches, path, k=10, metric="cosine", noise=None, seed=0, ks=(1, 5, 10)):
    """The driver's --do_retrieve: embed both items of every pair of ``batches`` (pair dicts as write_predictions
    takes them, through model.predict: batch b draws the hard gate with seed + b), index the item-2 side (an item id
    met again keeps its first embedding), search it with the item-1 side and write one JSON line per pair to ``path``:
    {"src_item_id", "tgt_item_ids": the k retrieved ids (null: an empty slot), "scores"}.  Returns (lines written,
    rank_metrics over the pairs with label 1, the pair's item 2 being the truth)."""
    import json
    from .finetune import _pair_args
    eng = model.engine
    index = ItemIndex(metric=metric, device=eng.device)
    seen = set()
    src_ids, tgt_ids, labels, queries = [], [], [], []
    for bi, pair in enumerate(batches):
        e1, e2, _, _ = model.predict(**_pair_args(pair, eng.use_image), noise=noise[bi] if noise is not None else None,
                                     seed=int(seed) + bi, embeddings=True)
        ids2 = list(pair["item_ids_2"])
        new = [r for r, i in enumerate(ids2) if i not in seen and i not in ids2[:r]]
        if new:
            index.add([ids2[r] for r in new], e2[torch.tensor(new, device=e2.device)].contiguous())
            seen.update(ids2)
        queries.append(e1.clone())
        src_ids.extend(pair["item_ids_1"])
        tgt_ids.extend(ids2)
        labels.extend(pair["labels"].detach().float().cpu().reshape(-1).tolist())
    if not queries:
        open(path, "w", encoding="utf-8").close()
        return 0, rank_metrics([], [], ks)
    scores, _, ids = index.search(torch.cat(queries), k)
    scores = scores.cpu().tolist()
    with open(path, "w", encoding="utf-8") as w:
        for s, got, sc in zip(src_ids, ids, scores):
            w.write(json.dumps({"src_item_id": s, "tgt_item_ids": got,
                                "scores": [x if x != float("-inf") else None for x in sc]}) + "\n")
    pos = [i for i, y in enumerate(labels) if y == 1.0]
    return len(src_ids), rank_metrics([ids[i] for i in pos], [tgt_ids[i] for i in pos], ks)


def rank_metrics(ids, truth, ks=(1, 5, 10)):
    """{"rank@k": share of the queries whose true match is among their first k retrieved ids}.  ids: one list of
    retrieved item ids per query (None = an empty slot); truth[i]: the matching item id of query i, or a set / list /
    tuple of them (any one counts).  No queries: every share is 0.0."""
    ids, truth = list(ids), list(truth)
    if len(ids) != len(truth):
        raise ValueError("%d result lists for %d truths" % (len(ids), len(truth)))
    hits = {int(k): 0 for k in ks}
    for got, want in zip(ids, truth):
        want = set(want) if isinstance(want, (set, frozenset, list, tuple)) else {want}
        want.discard(None)
        first = next((r for r, i in enumerate(got) if i is not None and i in want), None)
        for k in hits:
            if first is not None and first < k:
                hits[k] += 1
    n = len(ids)
    return {"rank@%d" % k: (hits[k] / n if n else 0.0) for k in hits}
