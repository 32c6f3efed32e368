"""Cost of masked-position prediction.  One cell per process; HIP events around every call after
--warmup calls; median and range of --runs calls; one JSON line.

    python scripts/predict_cost.py kernel --n 10496 [--v 21128 --hidden 768 --k 10] --path fused|torch
    python scripts/predict_cost.py engine --dtype fp32|bf16 --path predict|forward [--batch 64]

kernel: ops.topk_logits (decoder GEMM + running top-k + log-sum-exp, topk_logits.hip) against the unfused
torch.topk(h @ E.T + b, k) plus torch.logsumexp on the same tensors.  FLOP = 2 n v h over the call's time against the
exact-f32 MFMA peak (157.3 TF/s); bytes = what each path has to move at least: the fused one reads h, E and b once
and writes the result, the torch one also writes the [n, v] logits and reads them back twice (selection, lse).
engine: K3MEngine.predict_masked at a synthetic batch (T 36, P 128, 36 boxes; rows = the labelled positions) against
forward(train=False) with capture_logits, the only route to logits before it; ms per call and the peak of
torch.cuda.max_memory_allocated over the timed calls."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

F32_MFMA_PEAK = 157.3e12


def timed(fn, runs, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    ms = []
    for _ in range(runs):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return {"median": statistics.median(ms), "min": min(ms), "max": max(ms)}


def kernel(a, dev):
    from k3m_amd import ops
    g = torch.Generator(device="cpu").manual_seed(0)
    h = torch.randn((a.n, a.hidden), generator=g).to(dev)
    E = (0.02 * torch.randn((a.v, a.hidden), generator=g)).to(dev)
    b = (0.02 * torch.randn((a.v,), generator=g)).to(dev)

    def torch_path():
        z = h @ E.T + b
        return torch.topk(z, a.k), torch.logsumexp(z, 1)
    fn = (lambda: ops.topk_logits(h, E, b, k=a.k, chunks=a.chunks)) if a.path == "fused" else torch_path
    ms = timed(fn, a.runs, a.warmup)
    flop = 2.0 * a.n * a.v * a.hidden
    least = 4.0 * (a.n + a.v) * a.hidden + 4.0 * a.v + a.n * (12.0 * a.k + 4.0)
    if a.path == "torch":
        least += 3 * 4.0 * a.n * a.v
    return {"cell": "kernel", "path": a.path, "n": a.n, "v": a.v, "hidden": a.hidden, "k": a.k, "ms": ms,
            "tflops": flop / (ms["median"] * 1e-3) / 1e12,
            "share_of_f32_mfma_peak": flop / (ms["median"] * 1e-3) / F32_MFMA_PEAK, "least_bytes": least}


def engine(a, dev):
    from k3m_amd.config import pretrain_config
    from k3m_amd.engine import K3MEngine
    from k3m_amd.synthetic import synthetic_batch
    from k3m_amd.weights import param_values
    cfg = pretrain_config(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "configs",
                                       "bert_base_6layer_6conect.json"))
    eng = K3MEngine(cfg, dev, dtype=a.dtype)
    eng.fp.load(param_values(cfg, 4321))
    batch = synthetic_batch(cfg, a.batch, dev, seed=3)
    rows = int((batch["lm_label_ids"] != -1).sum() + (batch["lm_label_ids_pv"] != -1).sum())
    base = torch.cuda.memory_allocated()
    if a.path == "predict":
        fn = lambda: eng.predict_masked(batch, k=a.k, seed=1)  # noqa: E731
    else:
        eng.capture_logits = True

        def fn():
            out, ctx = eng.forward(batch, train=False, seed=1)
            return out["mlm_logits"], out["img_logits"]
    ms = timed(fn, a.runs, a.warmup)
    return {"cell": "engine", "path": a.path, "dtype": a.dtype, "batch": a.batch, "k": a.k, "labelled_rows": rows,
            "ms": ms, "peak_allocated_gb": torch.cuda.max_memory_allocated() / 1e9, "resident_before_gb": base / 1e9}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("cell", choices=["kernel", "engine"])
    ap.add_argument("--path", required=True, choices=["fused", "torch", "predict", "forward"])
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--n", type=int, default=10496)
    ap.add_argument("--v", type=int, default=21128)
    ap.add_argument("--hidden", type=int, default=768)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--chunks", type=int, default=0)
    ap.add_argument("--dtype", default="fp32", choices=["fp32", "bf16"])
    ap.add_argument("--batch", type=int, default=64)
    a = ap.parse_args()
    if (a.cell == "kernel") != (a.path in ("fused", "torch")):
        raise SystemExit("kernel: --path fused|torch; engine: --path predict|forward")
    if not torch.cuda.is_available():
        raise SystemExit("predict_cost.py measures on the GPU; none found")
    dev = torch.device("cuda")
    print(json.dumps((kernel if a.cell == "kernel" else engine)(a, dev)), flush=True)


if __name__ == "__main__":
    main()
