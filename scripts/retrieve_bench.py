"""Top-k retrieval: ops.topk_sim (fused similarity GEMM + running top-k, topk.hip) against the unfused torch path
torch.topk(Q @ C.T, k) on the same tensors, same process.  HIP events around every call, after
warm-up; the median of --runs calls.  Prints one JSON line per shape:

    python scripts/retrieve_bench.py [--runs 20] [--warmup 3] [--nc 262144] [--nq 4096 64]

FLOP = 2 Nq Nc H over the call's time against the exact-f32 MFMA peak (157.3 TF/s); bytes = what each path has to
move at least: the fused one reads Q and C once and writes the result, the torch one also writes the [Nq, Nc] score
matrix and reads it back for the selection."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from k3m_amd import ops  # noqa: E402

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
    return statistics.median(ms), min(ms), max(ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--nc", type=int, default=262144)
    ap.add_argument("--nq", type=int, nargs="+", default=[4096, 64])
    ap.add_argument("--hidden", type=int, default=768)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--metric", default="cosine", choices=["cosine", "inner"])
    ap.add_argument("--chunks", type=int, default=0)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("retrieve_bench.py measures on the GPU; none found")
    dev = torch.device("cuda")
    g = torch.Generator(device="cpu").manual_seed(0)
    c = torch.randn((a.nc, a.hidden), generator=g).to(dev)
    for nq in a.nq:
        q = torch.randn((nq, a.hidden), generator=g).to(dev)
        out = (torch.empty((nq, a.k), device=dev), torch.empty((nq, a.k), dtype=torch.int64, device=dev))
        fused = timed(lambda: ops.topk_sim(q, c, a.k, metric=a.metric, out=out, chunks=a.chunks), a.runs, a.warmup)
        unfused = timed(lambda: torch.topk(q @ c.T, a.k), a.runs, a.warmup)
        # same neighbours?  (inner product on both sides; torch's order among equal scores is unspecified)
        mine = ops.topk_sim(q, c, a.k, metric="inner", chunks=a.chunks)[1]
        theirs = torch.topk(q @ c.T, a.k).indices
        agree = float((mine == theirs).float().mean())
        flop = 2.0 * nq * a.nc * a.hidden
        in_bytes = 4.0 * (nq + a.nc) * a.hidden
        res_bytes = 12.0 * nq * a.k
        print(json.dumps({
            "nq": nq, "nc": a.nc, "hidden": a.hidden, "k": a.k, "metric": a.metric, "runs": a.runs,
            "topk_sim_ms": {"median": fused[0], "min": fused[1], "max": fused[2]},
            "torch_ms": {"median": unfused[0], "min": unfused[1], "max": unfused[2]},
            "speedup": unfused[0] / fused[0],
            "topk_sim_tflops": flop / (fused[0] * 1e-3) / 1e12,
            "topk_sim_share_of_f32_mfma_peak": flop / (fused[0] * 1e-3) / F32_MFMA_PEAK,
            "torch_tflops": flop / (unfused[0] * 1e-3) / 1e12,
            "topk_sim_min_bytes": in_bytes + res_bytes,
            "torch_min_bytes": in_bytes + 2 * 4.0 * nq * a.nc + res_bytes,
            "index_agreement_inner": agree}), flush=True)


if __name__ == "__main__":
    main()
