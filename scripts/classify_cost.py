"""Cost of the item-classification training step at the alignment benchmark's shape
(scripts/bench_finetune.py: batch 32, title 50, PV 256, 30 PV slots, 36 regions, fp32) with C = 518 categories, and
the item-alignment step (32 pairs = 64 items) in the same process for the comparison.

* step time: a host clock around ``steps`` calls of Trainer.step that end in a device synchronise, after ``warmup``
  calls; items/s = batch * steps / time;
* the head's share: in a second timed window of the same length, HIP events around the model's _head_forward and
  _head_backward (dropout, the two Linears forward / dgrad / wgrad, tanh, the cross entropy); the share is the
  events' total over the window's device time (events from the window's first launch to its last).

Prints one JSON line.  Usage: python scripts/classify_cost.py [--steps 20] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

import torch

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "scripts"))


def timed(step, n):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        out = step()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--labels", type=int, default=518)
    ap.add_argument("--out", type=str, default="")
    a = ap.parse_args()
    from bench_finetune import pair_batch
    from k3m_amd.classify import ItemClassificationTrainer
    from k3m_amd.config import classify_config, finetune_config
    from k3m_amd.finetune import ItemAlignmentTrainer
    from k3m_amd.synthetic import synthetic_batch
    T, P, NPV, TRIPLES = 50, 256, 30, 30
    cfg_path = os.path.join(HERE, "configs", "bert_base_6layer_6conect.json")
    dev = torch.device("cuda", 0)
    B, C = a.batch, a.labels
    total = 10 * (2 * a.steps + a.warmup)

    tr = ItemClassificationTrainer(classify_config(cfg_path, C), dev, lr=5e-5, warmup_steps=a.warmup, total_steps=total,
                                   seed=42)
    batch = synthetic_batch(tr.engine.cfg, B, dev, seed=1234, T=T, P=P, n_triples=TRIPLES, npv=NPV)
    batch["labels"] = (torch.arange(B, device=dev) * 37) % C
    for _ in range(a.warmup):
        tr.step(batch)
    dt, out = timed(lambda: tr.step(batch), a.steps)

    # the head's share, in a window of its own
    model = tr.model
    spans = []

    def wrap(fn):
        def inner(*args):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            r = fn(*args)
            e1.record()
            spans.append((e0, e1))
            return r
        return inner

    hf, hb = model._head_forward, model._head_backward
    model._head_forward, model._head_backward = wrap(hf), wrap(hb)
    w0, w1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    w0.record()
    dt_ev, _ = timed(lambda: tr.step(batch), a.steps)
    w1.record()
    torch.cuda.synchronize()
    model._head_forward, model._head_backward = hf, hb
    head_ms = sum(e0.elapsed_time(e1) for e0, e1 in spans) / a.steps
    window_ms = w0.elapsed_time(w1) / a.steps
    del tr, model
    torch.cuda.empty_cache()

    al = ItemAlignmentTrainer(finetune_config(cfg_path, loss_type="ce"), dev, lr=5e-5, warmup_steps=a.warmup,
                              total_steps=total, seed=42)
    pair = pair_batch(al.engine.cfg, B, dev, 1234, T, P, NPV, TRIPLES)
    for _ in range(a.warmup):
        al.step(pair)
    dt_al, out_al = timed(lambda: al.step(pair), a.steps)

    res = {"metric": "item-classification fine-tune items/sec (bert_base_6layer_6conect, %d items/GPU, C=%d)" % (B, C),
           "value": round(B * a.steps / dt, 3), "unit": "items/s", "ms_per_step": round(1000 * dt / a.steps, 3),
           "steps": a.steps, "warmup": a.warmup, "dtype": "fp32", "loss": round(float(out["loss"]), 4),
           "config": {"workload": "K3MForItemClassification, T=%d P=%d NPV=%d R=37" % (T, P, NPV), "batch_items": B,
                      "num_labels": C},
           "head": {"ms_per_step": round(head_ms, 4), "window_ms_per_step": round(window_ms, 3),
                    "share": round(head_ms / window_ms, 5), "host_ms_per_step": round(1000 * dt_ev / a.steps, 3),
                    "what": "HIP events around _head_forward and _head_backward, a timed window of their own"},
           "alignment": {"value": round(B * a.steps / dt_al, 3), "unit": "pairs/s",
                         "items_per_s": round(2 * B * a.steps / dt_al, 3), "ms_per_step": round(1000 * dt_al / a.steps, 3),
                         "loss": round(float(out_al["loss"]), 4),
                         "what": "ItemAlignmentTrainer ce, %d pairs = %d items, the same process" % (B, 2 * B)}}
    line = json.dumps(res)
    print(line, flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
