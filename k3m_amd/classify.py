"""Item classification: the first downstream task of the K3M paper's result table, c_final -> category.

The encoder is the engine's "encoder up to c_final" task on single items (groups = 1); the head is the reference's
ClassificationHead (vilbert_k3m.py:2164-2183) over ONE item's embedding, with ``num_labels`` outputs:

    x = dropout_p(e);  u = classifier.dense(x);  h = dropout_p(tanh(u));  z = classifier.out_proj(h)
    loss = F.cross_entropy(z, labels, weight=class_weight, ignore_index=-1, label_smoothing=cfg.label_smoothing)

The two Linears run on the project's GEMM (Lin.fwd / dgrad / wgrad); dropout, tanh and the cross entropy are the
kernels of k3m_amd/csrc/classify.hip.  One stated deviation from torch: when no labelled row carries weight
(S = sum of w[label] == 0) the loss is 0 and every gradient is zero, where torch returns NaN.  Inference
(``predict``) is engine.embed, the dense Linear, tanh and ops.topk_logits: the [B, C] logits are never stored.

Optimizer and schedule are the item-alignment ones (torch.optim.AdamW's update, k3m_adamw_torch; WarmupLinearSchedule).
"""
import json
import os
import warnings

import torch

from . import _lib as L
from . import debug, ops
from .engine import K3MEngine, Lin
from .finetune import HEAD_OFFSET
from .trainer import Trainer

ENGINE_FIELDS = ("input_ids", "segment_ids", "input_mask", "input_ids_pv", "segment_ids_pv", "input_mask_pv",
                 "index_p", "index_v")
IMAGE_FIELDS = ("image_feat", "image_loc", "image_mask")
LABELS_FILE = "labels.json"


def _elementwise(name, *lead, B, H, p, seed, off, out):
    L.call(name, *[t.data_ptr() for t in lead], B, H, p, seed, off, out.data_ptr(), L.stream())
    return out


class K3MForItemClassification(object):
    """The classification model on one GPU.  ``forward`` returns (logits [B, C], loss); ``backward()`` accumulates
    the gradients of that loss into ``engine.fp.grad``; ``predict`` is the forward-only top-k."""

    def __init__(self, cfg, device=None, seed=1234, dtype="fp32", engine=None, class_weight=None):
        if getattr(cfg, "task", None) != "item_classification":
            raise ValueError("config must come from k3m_amd.config.classify_config (task 'item_classification')")
        self.cfg = cfg
        self.C = int(cfg.num_labels)
        self.eps = float(getattr(cfg, "label_smoothing", 0.0))
        self.engine = engine if engine is not None else K3MEngine(cfg, device, seed=seed, dtype=dtype)
        fp = self.engine.fp
        self.cls_dense = Lin(fp, "classifier.dense")
        self.cls_out = Lin(fp, "classifier.out_proj")
        self.p_h = cfg.hidden_dropout_prob
        self.class_weight = None
        self.set_class_weight(class_weight)
        self.pred = None   # int32 [B]: the argmax of the last forward's logits
        self._ctx = None

    def set_class_weight(self, w):
        """float32 [C] weights of the cross entropy (None: all ones)."""
        if w is None:
            self.class_weight = None
            return
        w = torch.as_tensor(w)
        if w.dtype != torch.float32 or tuple(w.shape) != (self.C,):
            raise ValueError("class_weight: a float32 [%d] tensor expected, got %s %s"
                             % (self.C, w.dtype, tuple(w.shape)))
        if bool((w < 0).any()) or not bool(torch.isfinite(w).all()):
            raise ValueError("class_weight: weights must be finite and >= 0")
        self.class_weight = w.to(self.engine.device).contiguous()

    def __call__(self, *args, **kw):
        return self.forward(*args, **kw)

    def _split(self, batch, need_labels):
        """(the engine's batch, labels int64 [B] on the device or None)"""
        eng = self.engine
        names = ENGINE_FIELDS + (IMAGE_FIELDS if eng.use_image else ())
        missing = [k for k in names if batch.get(k) is None]
        if need_labels and batch.get("labels") is None:
            missing.append("labels")
        if missing:
            raise TypeError("missing batch fields: %s" % missing)
        eb = {k: batch[k].to(eng.device).contiguous() for k in names}
        labels = batch.get("labels")
        if labels is not None:
            B = eb["input_ids"].shape[0]
            if labels.dtype != torch.int64 or tuple(labels.shape) != (B,):
                raise ValueError("labels: an int64 [%d] tensor expected, got %s %s"
                                 % (B, labels.dtype, tuple(labels.shape)))
            labels = labels.to(eng.device).contiguous()
            if debug.ON:
                debug.check_range(labels, 0, self.C, "labels", ignore=-1)
        return eb, labels

    def forward(self, batch, train=True, noise=None, seed=None):
        """batch: the engine's fields plus ``labels`` (int64 [B], -1 = unlabelled).  noise: optional {v,t,pv}
        gumbel-noise dict (explicit randomness for parity); seed: the step's draw otherwise.  The returned logits
        are a copy made before dz overwrites the one [B, C] buffer."""
        eb, labels = self._split(batch, True)
        out, ctx = self.engine.forward(eb, train=train, noise=noise, seed=seed, groups=1)
        p = self.p_h if train else 0.0
        logits, loss, ctx["head"] = self._head_forward(out["c_final"], labels, p, ctx["seed"])
        self._ctx = ctx
        return logits, loss

    def _head_forward(self, cf, labels, p, sd):
        """The head and the loss over c_final [B, H]; returns (logits copy, loss, what _head_backward needs)."""
        dev = cf.device
        B, H = cf.shape
        C = self.C
        x = cf if p == 0.0 else _elementwise("k3m_cls_drop_fwd", cf, B=B, H=H, p=p, seed=sd, off=HEAD_OFFSET,
                                             out=torch.empty_like(cf))
        u = self.cls_dense.fwd(x)
        h = _elementwise("k3m_cls_tanh_drop_fwd", u, B=B, H=H, p=p, seed=sd, off=HEAD_OFFSET + B * H,
                         out=torch.empty_like(u))
        z = self.cls_out.fwd(h)
        logits = z.clone()
        loss = torch.zeros((1,), dtype=torch.float32, device=dev)
        rows = torch.empty((B,), dtype=torch.float32, device=dev)
        lse = torch.empty((B,), dtype=torch.float32, device=dev)
        pred = torch.empty((B,), dtype=torch.int32, device=dev)
        denom = torch.empty((2,), dtype=torch.float32, device=dev)
        L.call("k3m_cls_ce_fwd_bwd", z.data_ptr(), C, labels.data_ptr(), L.ptr(self.class_weight), self.eps, B, C,
               rows.data_ptr(), lse.data_ptr(), loss.data_ptr(), pred.data_ptr(), denom.data_ptr(), L.stream())
        self.pred = pred
        return logits, loss, (x, u, h, z, B, H, p, sd)   # z holds dz

    def backward(self, grad_ready=None):
        """Gradients of the last forward's loss, ACCUMULATED into engine.fp.grad."""
        ctx, self._ctx = self._ctx, None
        if ctx is None:
            raise RuntimeError("backward() without a preceding forward()")
        ctx["d_c_final"] = self._head_backward(ctx["head"])
        self.engine.backward(ctx, grad_ready=grad_ready)

    def _head_backward(self, head):
        """Accumulates the classifier gradients; returns d loss / d c_final."""
        x, u, h, dz, B, H, p, sd = head
        self.cls_out.wgrad(dz, h)
        dh = self.cls_out.dgrad(dz)
        du = _elementwise("k3m_cls_tanh_drop_bwd", dh, u, B=B, H=H, p=p, seed=sd, off=HEAD_OFFSET + B * H, out=dh)
        self.cls_dense.wgrad(du, x)
        dx = self.cls_dense.dgrad(du)
        if p != 0.0:
            _elementwise("k3m_cls_drop_bwd", dx, B=B, H=H, p=p, seed=sd, off=HEAD_OFFSET, out=dx)
        return dx

    def predict(self, batch, k=1, noise=None, seed=None):
        """The k most probable categories of every item in eval mode: engine.embed, the dense Linear, tanh, then the
        out_proj decoder fused with a top-k and the log-sum-exp (ops.topk_logits).  Returns {ids [B, k] int64,
        logp [B, k] (logit - lse), lse [B]} and, when the batch has labels, gold_logp [B] (-inf for unlabelled
        rows).  k <= ops.TOPK_LOGITS_MAX_K; slots past C hold (-inf, -1).  No ctx is made and no gradient buffer is
        touched; a pending forward()'s ctx is left as it is."""
        eb, labels = self._split(batch, False)
        fp = self.engine.fp
        cf = self.engine.embed(eb, noise=noise, seed=seed)["c_final"]
        B, H = cf.shape
        u = self.cls_dense.fwd(cf)
        h = _elementwise("k3m_cls_tanh_drop_fwd", u, B=B, H=H, p=0.0, seed=0, off=0, out=u)
        scores, idx, lse, gs = ops.topk_logits(h, fp.p["classifier.out_proj.weight"], fp.p["classifier.out_proj.bias"],
                                               k=k, gold=labels)
        res = {"ids": idx, "logp": scores - lse[:, None], "lse": lse}
        if gs is not None:
            res["gold_logp"] = gs - lse
        return res


class ItemClassificationTrainer(Trainer):
    """The fine-tuning loop of the alignment task on the classification model: forward, backward, (DDP all-reduce),
    torch.optim.AdamW step, WarmupLinearSchedule step."""

    ADAMW = "k3m_adamw_torch"

    def __init__(self, cfg, device, lr=5e-5, warmup_steps=0, total_steps=10000, seed=42, ddp=None, beta1=0.9,
                 beta2=0.98, eps=1e-8, weight_decay=0.01, init=True, dtype="fp32", class_weight=None):
        super(ItemClassificationTrainer, self).__init__(cfg, device, lr=lr, warmup_steps=warmup_steps,
                                                        total_steps=total_steps, seed=seed, ddp=ddp, beta1=beta1,
                                                        beta2=beta2, eps=eps, weight_decay=weight_decay, init=init,
                                                        dtype=dtype)
        self.model = K3MForItemClassification(cfg, engine=self.engine, class_weight=class_weight)

    def step(self, batch, noise=None):
        """One optimisation step on a labelled item batch; returns {"logits", "loss", "pred"}."""
        eng = self.engine
        logits, loss = self.model.forward(batch, train=True, noise=noise, seed=self.global_step)
        pred = self.model.pred
        hook = self.ddp.grad_ready if self.ddp is not None else None
        if self.ddp is not None:
            self.ddp.begin(eng)
        self.model.backward(grad_ready=hook)
        if self.watch is not None:   # a label outside {-1, 0 .. C-1} gives a NaN loss: fail fast
            self.watch.push(self.global_step, loss)
        scale = 1.0
        if self.ddp is not None:
            self.ddp.finish()
            scale = 1.0 / self.ddp.world
        self.optimizer_step(grad_scale=scale)
        eng.step_count += 1
        return {"logits": logits, "loss": loss, "pred": pred}


def classification_metrics(ids, labels, ks=(1, 5)):
    """Host metrics of a top-k prediction: ids [N, k] (best first; -1 = no candidate), labels [N] (-1 = unlabelled,
    left out).  accuracy@k for every k of ``ks`` (the label among the first k ids), macro-F1 of the top-1 column
    over the classes that occur as a label or as a prediction (an absent precision or recall counts 0), the
    per-class support and the number of unlabelled rows left out."""
    import numpy as np
    ids = np.asarray(ids.cpu() if isinstance(ids, torch.Tensor) else ids).astype(np.int64)
    labels = np.asarray(labels.cpu() if isinstance(labels, torch.Tensor) else labels).astype(np.int64).reshape(-1)
    if ids.ndim != 2 or ids.shape[0] != labels.shape[0]:
        raise ValueError("ids [N, k] and labels [N] expected, got %s and %s" % (ids.shape, labels.shape))
    if any(k < 1 or k > ids.shape[1] for k in ks):
        raise ValueError("ks = %r: every k in [1, %d] (the width of ids)" % (tuple(ks), ids.shape[1]))
    keep = labels != -1
    y, top = labels[keep], ids[keep]
    n = int(keep.sum())
    out = {"n": n, "unlabelled": int((~keep).sum())}
    for k in ks:
        out["accuracy@%d" % k] = float((top[:, :k] == y[:, None]).any(1).mean()) if n else 0.0
    pred = top[:, 0] if n else np.zeros(0, np.int64)
    f1 = []
    for c in sorted(set(y.tolist()) | set(pred.tolist())):
        tp = int(((pred == c) & (y == c)).sum())
        fp_, fn = int(((pred == c) & (y != c)).sum()), int(((pred != c) & (y == c)).sum())
        f1.append(2.0 * tp / (2 * tp + fp_ + fn) if tp else 0.0)
    out["macro_f1"] = float(np.mean(f1)) if f1 else 0.0
    cls, cnt = np.unique(y, return_counts=True)
    out["support"] = {int(c): int(m) for c, m in zip(cls, cnt)}
    return out


def evaluate(model, batches, ks=(1, 5)):
    """The model over ``batches`` through predict() (nothing saved for a backward), the hard gate's draw seeded by
    the batch index; returns (classification_metrics, ids [N, max(ks)], labels [N])."""
    import numpy as np
    k = max(ks)
    ids, labels = [], []
    for bi, batch in enumerate(batches):
        r = model.predict(batch, k=k, seed=bi)
        ids.append(r["ids"].cpu().numpy())
        labels.append(batch["labels"].cpu().numpy())
    ids = np.concatenate(ids) if ids else np.zeros((0, k), np.int64)
    labels = np.concatenate(labels) if labels else np.zeros(0, np.int64)
    return classification_metrics(ids, labels, ks), ids, labels


def save_model(model, path, vocab):
    """The per-epoch ``K3M_item_classification-<p>_epoch-<e>.bin`` (state_dict()) and, beside it, ``labels.json``:
    the category of every output row."""
    from .checkpoint import model_state_dict
    torch.save(model_state_dict(model.engine.fp), path)
    vocab.save(os.path.join(os.path.dirname(os.path.abspath(path)), LABELS_FILE))


def load_encoder(model, state_dict):
    """Seed the model from a state dict of another head: ``classifier.*`` entries whose shape differs from this
    model's (a pretraining .bin has none, an alignment .bin a pair head) are left out, with a warning naming them;
    the rest goes through load_model_state_dict(strict=False).  Returns the names the file did not provide."""
    from .checkpoint import load_model_state_dict
    fp = model.engine.fp
    sd = {(k[7:] if k.startswith("module.") else k): v for k, v in state_dict.items()}
    skip = [k for k, v in sd.items()
            if k.startswith("classifier.") and k in fp.shapes and tuple(v.shape) != tuple(fp.shapes[k])]
    if skip:
        warnings.warn("load_encoder: left out %s (shape differs from this model's %d-way head)"
                      % (", ".join(sorted(skip)), model.C))
    return load_model_state_dict(fp, {k: v for k, v in sd.items() if k not in skip}, strict=False)


def write_predictions(model, batches, path, vocab, k=5, seed=0):
    """One .jsonl line per item: {"item_id", "pred": the k most probable categories (best first), "logp": their log
    probabilities}.  Batch b draws the hard gate's noise with seed + b."""
    n = 0
    with open(path, "w", encoding="utf-8") as w:
        for bi, batch in enumerate(batches):
            r = model.predict(batch, k=k, seed=int(seed) + bi)
            ids, logp = r["ids"].cpu().tolist(), r["logp"].cpu().tolist()
            for item_id, row, lp in zip(batch["item_ids"], ids, logp):
                keep = [j for j, c in enumerate(row) if c >= 0]
                w.write(json.dumps({"item_id": item_id, "pred": [vocab.names[row[j]] for j in keep],
                                    "logp": [lp[j] for j in keep]}, ensure_ascii=False) + "\n")
                n += 1
    return n
