"""Cost table of the model without co-attention: ``Trainer.step`` with ``with_coattention`` off against
on, eager and as a captured hipGraph, at the config-2 shapes (synthetic bs 64 / T 36 / P 128 / 36 boxes + the global
region), both dtypes.  The two models live in ONE process and their timed runs ALTERNATE (on, off, on, off, ...), at
least three runs of ``--steps`` steps each after ``--warmup`` steps of both, each run timed on the host around a device
synchronisation.  Per cell: median and range of the runs (ms per step), the ratio off / on of the medians, the peak of
``torch.cuda.max_memory_allocated`` above what was resident before the run, and, with ``--count``, the kernels launched
in one profiled step (a separate step, after the timing).  ``eval`` rows time the evaluation forward
(``engine.forward(train=False)``, no backward).  One JSON line per cell.

usage:  python scripts/no_coattention_cost.py [--dtypes fp32 bf16] [--modes eager graph eval] [--count] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path.insert(0, REPO)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dtypes", nargs="+", default=["fp32", "bf16"])
    ap.add_argument("--modes", nargs="+", default=["eager", "graph", "eval"])
    ap.add_argument("--bs", type=int, default=64)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--count", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from k3m_amd.config import pretrain_config
    from k3m_amd.engine import label_counts
    from k3m_amd.synthetic import synthetic_batch
    from k3m_amd.trainer import Trainer
    assert torch.cuda.is_available(), "a measurement needs the GPU"
    dev = torch.device("cuda")
    cfg_path = os.path.join(REPO, "configs", "bert_base_6layer_6conect.json")
    lines = []

    def emit(row):
        line = json.dumps(row)
        print(line, flush=True)
        lines.append(line)
        if a.out:
            with open(a.out, "w") as f:
                f.write("\n".join(lines) + "\n")

    for dtype in a.dtypes:
        for mode in a.modes:
            trs, batches = {}, {}
            for flag in (True, False):
                cfg = pretrain_config(cfg_path, with_coattention=flag)
                tr = Trainer(cfg, dev, lr=1e-4, warmup_steps=0, total_steps=100000, seed=9, dtype=dtype)
                tr.graph = (mode == "graph")
                trs[flag] = tr
                batches[flag] = synthetic_batch(cfg, a.bs, dev, seed=21)
                batches[flag]["_label_counts"] = label_counts(batches[flag])

            def run(flag, n):
                tr, batch = trs[flag], batches[flag]
                for _ in range(n):
                    if mode == "eval":
                        tr.engine.forward(batch, train=False)
                    else:
                        tr.step(batch)

            for flag in (True, False):
                run(flag, a.warmup)
            torch.cuda.synchronize()
            ms = {True: [], False: []}
            peak = {}
            for _ in range(a.runs):
                for flag in (True, False):   # alternating: on, off, on, off, ...
                    torch.cuda.synchronize()
                    torch.cuda.reset_peak_memory_stats(dev)
                    base = torch.cuda.memory_allocated(dev)
                    t0 = time.perf_counter()
                    run(flag, a.steps)
                    torch.cuda.synchronize()
                    ms[flag].append(1e3 * (time.perf_counter() - t0) / a.steps)
                    peak[flag] = max(peak.get(flag, 0), int(torch.cuda.max_memory_allocated(dev) - base))
            med = {f: statistics.median(ms[f]) for f in ms}
            for flag in (True, False):
                tr = trs[flag]
                fp = tr.engine.fp
                row = {"dtype": dtype, "mode": mode, "with_coattention": flag, "bs": a.bs, "steps": a.steps,
                       "ms_median": med[flag], "ms_min": min(ms[flag]), "ms_max": max(ms[flag]), "ms_runs": ms[flag],
                       "ratio_to_with_coattention": med[flag] / med[True], "peak_above_resident_bytes": peak[flag],
                       "parameters": sum(fp.p[n].numel() for n, _ in fp.spec), "flat_elements": int(fp.data.numel())}
                if mode == "graph":
                    row["captures"], row["replays"] = tr._graphs.captures, tr._graphs.replays
                if a.count:
                    from torch.profiler import ProfilerActivity, profile
                    with profile(activities=[ProfilerActivity.CUDA]) as prof:
                        run(flag, 1)
                        torch.cuda.synchronize()
                    row["kernels_per_step"] = sum(e.count for e in prof.key_averages()
                                                  if "Memcpy" not in e.key and "Memset" not in e.key)
                emit(row)
            for tr in trs.values():
                tr.finish()
            del trs, batches
            torch.cuda.empty_cache()
    return 0


if __name__ == "__main__":
    sys.exit(main())
