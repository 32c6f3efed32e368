"""Cost table of frozen lower text layers: eager ``Trainer.step`` (no hipGraph) at the config-2
shapes (synthetic bs 64 / T 36 / P 128 / 36 boxes), 8 warm-up steps, three runs of 20 steps timed on the host around
a device synchronisation, a fresh process per cell, the whole table measured ``--passes`` times (default 2).  Cells:

    parent     a checkout of the parent commit (``--parent DIR``, built there; skipped when not given)
    ftl0       this tree, fixed_t_layer = 0   (must launch what the parent launches)
    ftl6       this tree, fixed_t_layer = 6
    ftl6save   this tree, fixed_t_layer = 6 with K3M_FROZEN_NOSAVE=0 (saving kernels, backward skipped)

Each cell reports the median and range of the three runs (ms per step), ``torch.cuda.max_memory_allocated`` and, with
``--count``, the kernels launched in one profiled step.  One JSON line per cell.

usage:  python scripts/fixed_t_layer_cost.py [--parent DIR] [--dtypes fp32 bf16] [--passes 2] [--out FILE]
        python scripts/fixed_t_layer_cost.py --cell ftl6 --dtype fp32        (one cell, in this process)
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
CELLS = {"parent": (0, None), "ftl0": (0, None), "ftl6": (6, None), "ftl6save": (6, "0")}


def run_cell(cell, dtype, bs, warmup, steps, runs, count):
    import torch
    sys.path.insert(0, os.getcwd())
    from k3m_amd.config import pretrain_config
    from k3m_amd.engine import label_counts
    from k3m_amd.synthetic import synthetic_batch
    from k3m_amd.trainer import Trainer
    fixed = CELLS[cell][0]
    dev = torch.device("cuda")
    cfg = pretrain_config(os.path.join(os.getcwd(), "configs", "bert_base_6layer_6conect.json"))
    cfg.fixed_t_layer = fixed   # (the parent's pretrain_config has no such argument; 0 is its default)
    tr = Trainer(cfg, dev, lr=1e-4, warmup_steps=0, total_steps=100000, seed=9, dtype=dtype)
    tr.graph = False
    batch = synthetic_batch(cfg, bs, dev, seed=21)
    batch["_label_counts"] = label_counts(batch)
    for _ in range(warmup):
        tr.step(batch)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats(dev)
    ms = []
    for _ in range(runs):
        t0 = time.perf_counter()
        for _ in range(steps):
            tr.step(batch)
        torch.cuda.synchronize()
        ms.append(1e3 * (time.perf_counter() - t0) / steps)
    res = {"cell": cell, "dtype": dtype, "fixed_t_layer": fixed, "nosave_env": os.environ.get("K3M_FROZEN_NOSAVE"),
           "ms_median": statistics.median(ms), "ms_min": min(ms), "ms_max": max(ms),
           "max_memory_allocated": int(torch.cuda.max_memory_allocated(dev))}
    if count:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            tr.step(batch)
            torch.cuda.synchronize()
        res["kernels_per_step"] = sum(e.count for e in prof.key_averages()
                                      if "Memcpy" not in e.key and "Memset" not in e.key)
    tr.finish()
    print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", default=None)
    ap.add_argument("--dtypes", nargs="+", default=["fp32", "bf16"])
    ap.add_argument("--passes", type=int, default=2)
    ap.add_argument("--bs", type=int, default=64)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--count", action="store_true")
    ap.add_argument("--out", default=None)
    ap.add_argument("--cell", default=None)
    ap.add_argument("--dtype", default="fp32")
    ap.add_argument("--cell-timeout", type=int, default=240)
    a = ap.parse_args()
    if a.cell:
        return run_cell(a.cell, a.dtype, a.bs, a.warmup, a.steps, a.runs, a.count)
    lines = []
    for p in range(a.passes):
        for dtype in a.dtypes:
            for cell, (_, nosave) in CELLS.items():
                if cell == "parent" and not a.parent:
                    continue
                env = dict(os.environ)
                env.pop("K3M_FROZEN_NOSAVE", None)
                if nosave is not None:
                    env["K3M_FROZEN_NOSAVE"] = nosave
                cmd = [sys.executable, os.path.abspath(__file__), "--cell", cell, "--dtype", dtype, "--bs", str(a.bs),
                       "--warmup", str(a.warmup), "--steps", str(a.steps), "--runs", str(a.runs)]
                if a.count:
                    cmd.append("--count")
                r = subprocess.run(cmd, cwd=a.parent if cell == "parent" else REPO, env=env, capture_output=True,
                                   text=True, timeout=a.cell_timeout)
                if r.returncode != 0:   # a failed cell ends the table: nothing more is started on the device
                    sys.stderr.write(r.stderr[-3000:])
                    return r.returncode
                row = json.loads(r.stdout.strip().splitlines()[-1])
                row["pass"] = p + 1
                line = json.dumps(row)
                print(line, flush=True)
                lines.append(line)
                if a.out:
                    with open(a.out, "w") as f:
                        f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
