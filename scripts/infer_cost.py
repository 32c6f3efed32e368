"""Cost table of item-embedding inference: one engine call at the config-2 shapes (synthetic bs 64 / T 36 /
P 128 / 36 boxes), 8 warm-up calls, three runs of 20 calls timed on the host around a device synchronisation, a fresh
process per cell, the whole table measured ``--passes`` times (default 2).  Rows:

    forward    forward(train=False) with the ctx dropped (the eval path before embed(); its launches are the parent's)
    embed0     embed() with K3M_INFER_DEDUP=0 (forward-only kernels, wide buffers from the start)
    embed      embed() with the stream dedup (the default)

Columns: fp32 / bf16, with and without co-attention.  Each cell reports the median and range of the three runs (ms per
call) and ``torch.cuda.max_memory_allocated``.  One JSON line per cell.

usage:  python scripts/infer_cost.py [--dtypes fp32 bf16] [--passes 2] [--out FILE]
        python scripts/infer_cost.py --cell embed --dtype fp32 [--noco]        (one cell, in this process)
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
CELLS = {"forward": None, "embed0": "0", "embed": "1"}


def run_cell(cell, dtype, noco, bs, warmup, steps, runs):
    import torch
    sys.path.insert(0, REPO)
    from k3m_amd.config import finetune_config
    from k3m_amd.engine import K3MEngine
    from k3m_amd.synthetic import synthetic_batch
    from k3m_amd.weights import param_values
    dev = torch.device("cuda")
    cfg = finetune_config(os.path.join(REPO, "configs", "bert_base_6layer_6conect.json"), loss_type="cosine",
                          with_coattention=not noco)
    eng = K3MEngine(cfg, dev, dtype=dtype)
    eng.fp.load(param_values(cfg, 4321))
    keep = ("input_ids", "segment_ids", "input_mask", "input_ids_pv", "segment_ids_pv", "input_mask_pv", "index_p",
            "index_v", "image_feat", "image_loc", "image_mask")
    batch = {k: v for k, v in synthetic_batch(cfg, bs, dev, seed=21).items() if k in keep}
    if cell == "forward":
        def call():
            out, ctx = eng.forward(batch, train=False, seed=1)
            del ctx
            return out
    else:
        assert eng.infer_dedup == (cell == "embed")

        def call():
            return eng.embed(batch, seed=1)
    for _ in range(warmup):
        call()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats(dev)
    ms = []
    for _ in range(runs):
        t0 = time.perf_counter()
        for _ in range(steps):
            call()
        torch.cuda.synchronize()
        ms.append(1e3 * (time.perf_counter() - t0) / steps)
    print(json.dumps({"cell": cell, "dtype": dtype, "coattention": not noco, "ms_median": statistics.median(ms),
                      "ms_min": min(ms), "ms_max": max(ms),
                      "max_memory_allocated": int(torch.cuda.max_memory_allocated(dev))}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dtypes", nargs="+", default=["fp32", "bf16"])
    ap.add_argument("--passes", type=int, default=2)
    ap.add_argument("--bs", type=int, default=64)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--cell", default=None)
    ap.add_argument("--dtype", default="fp32")
    ap.add_argument("--noco", action="store_true")
    ap.add_argument("--cell-timeout", type=int, default=240)
    a = ap.parse_args()
    if a.cell:
        return run_cell(a.cell, a.dtype, a.noco, a.bs, a.warmup, a.steps, a.runs)
    lines = []
    for p in range(a.passes):
        for noco in (False, True):
            for dtype in a.dtypes:
                for cell, dedup in CELLS.items():
                    env = dict(os.environ)
                    env.pop("K3M_INFER_DEDUP", None)
                    if dedup is not None:
                        env["K3M_INFER_DEDUP"] = dedup
                    cmd = [sys.executable, os.path.abspath(__file__), "--cell", cell, "--dtype", dtype, "--bs",
                           str(a.bs), "--warmup", str(a.warmup), "--steps", str(a.steps), "--runs", str(a.runs)]
                    if noco:
                        cmd.append("--noco")
                    r = subprocess.run(cmd, cwd=REPO, env=env, capture_output=True, text=True, timeout=a.cell_timeout)
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
