"""Cost of link-prediction ranking.  One cell per process; HIP events around every call after --warmup
calls; median and range of --runs calls; one JSON line.

    python scripts/linkpred_cost.py kernel --nq 4096 [--nc 262144 --hidden 768 --k 10]
    python scripts/linkpred_cost.py engine --dtype fp32|bf16 [--batch 64 --batches 4]

kernel: ops.lp_rank (distance GEMM + running top-k + gold rank, lprank.hip) against the unfused torch path on the
same tensors in the same process: s = 2 q @ c.T - |c|^2, torch.topk(s, k), (s > s[i, gold[i]]).sum(1).  FLOP =
2 nq nc h over the call's time against the exact-f32 MFMA peak (157.3 TF/s); bytes = what each path has to move at
least: the fused one reads q and c once and writes the result, the torch one also writes the [nq, nc] scores and
reads them back twice (selection, count).
engine: LinkEval (K3MEngine.triples per batch, then both rankings over the pool) over synthetic batches (T 36, P 128,
36 boxes) against K3MEngine.embed alone on the same batches: what the ranking adds to the encoder's time."""
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
    c = torch.randn((a.nc, a.hidden), generator=g).to(dev)
    gold = torch.randint(0, a.nc, (a.nq,), generator=g).to(dev)
    q = (c[gold] + 0.9 * torch.randn((a.nq, a.hidden), generator=g).to(dev)).contiguous()
    rows = torch.arange(a.nq, device=dev)

    def torch_path():
        s = 2.0 * (q @ c.T) - (c * c).sum(1)
        return torch.topk(s, a.k), (s > s[rows, gold][:, None]).sum(1)
    fused = timed(lambda: ops.lp_rank(q, c, gold=gold, k=a.k, chunks=a.chunks), a.runs, a.warmup)
    unfused = timed(torch_path, a.runs, a.warmup)
    (ts, ti), tr = torch_path()
    d2, idx, gold_d2, rank = ops.lp_rank(q, c, gold=gold, k=a.k, chunks=a.chunks)
    flop = 2.0 * a.nq * a.nc * a.hidden
    least = 4.0 * (a.nq + a.nc) * a.hidden + a.nq * (12.0 * a.k + 8.0 + 12.0)
    return {"cell": "kernel", "nq": a.nq, "nc": a.nc, "hidden": a.hidden, "k": a.k, "lp_rank_ms": fused,
            "torch_ms": unfused, "torch_over_lp_rank": unfused["median"] / fused["median"],
            "lp_rank_tflops": flop / (fused["median"] * 1e-3) / 1e12,
            "lp_rank_share_of_f32_mfma_peak": flop / (fused["median"] * 1e-3) / F32_MFMA_PEAK,
            "torch_tflops": flop / (unfused["median"] * 1e-3) / 1e12,
            "lp_rank_least_bytes": least, "torch_least_bytes": least + 3 * 4.0 * a.nq * a.nc,
            "same_first_index": float((idx[:, 0] == ti[:, 0]).double().mean()),
            "same_rank": float((rank == tr + 1).double().mean())}


def engine(a, dev):
    from k3m_amd.config import pretrain_config
    from k3m_amd.engine import K3MEngine
    from k3m_amd.linkpred import LinkEval
    from k3m_amd.synthetic import synthetic_batch
    from k3m_amd.weights import param_values
    cfg = pretrain_config(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "configs",
                                       "bert_base_6layer_6conect.json"))
    eng = K3MEngine(cfg, dev, dtype=a.dtype)
    eng.fp.load(param_values(cfg, 4321))
    batches = [synthetic_batch(cfg, a.batch, dev, seed=3 + i) for i in range(a.batches)]
    stats = {}

    def embed_only():
        for b in batches:
            eng.embed(b, seed=1)

    def link_eval():
        ev = LinkEval(a.k)
        for i, b in enumerate(batches):
            ev.add(eng, b, list(range(i * a.batch, (i + 1) * a.batch)), seed=1)
        ev.close()
        stats.update(triples=ev.pool.n_triples, items=ev.pool.n_items)
    return {"cell": "engine", "dtype": a.dtype, "batch": a.batch, "batches": a.batches, "k": a.k,
            "link_eval_ms": timed(link_eval, a.runs, a.warmup), "embed_ms": timed(embed_only, a.runs, a.warmup), **stats}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("cell", choices=["kernel", "engine"])
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--nq", type=int, default=4096)
    ap.add_argument("--nc", type=int, default=262144)
    ap.add_argument("--hidden", type=int, default=768)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--chunks", type=int, default=0)
    ap.add_argument("--dtype", default="fp32", choices=["fp32", "bf16"])
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--batches", type=int, default=4)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("linkpred_cost.py measures on the GPU; none found")
    dev = torch.device("cuda")
    print(json.dumps((kernel if a.cell == "kernel" else engine)(a, dev)), flush=True)


if __name__ == "__main__":
    main()
