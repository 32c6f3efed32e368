"""bench.py's command line: the output dump's size cap and fixed sample (CPU), and a plain run's result line and
``--dump-outputs`` files from a real run at a small batch (GPU, a fresh child process)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_dump_outputs_caps_size_with_a_fixed_sample(tmp_path):
    import bench
    rng = np.random.RandomState(7)
    arrays = {"small": rng.rand(5).astype(np.float32), "big": rng.rand(300, 1000).astype(np.float32),
              "wide": rng.rand(200000).astype(np.float64)}
    limit = 600000
    bench.dump_outputs(str(tmp_path / "a"), arrays, limit=limit)
    bench.dump_outputs(str(tmp_path / "b"), arrays, limit=limit)
    got = {n: np.load(str(tmp_path / "a" / (n + ".npy"))) for n in arrays}
    assert sum(a.nbytes for a in got.values()) <= limit
    np.testing.assert_array_equal(got["small"], arrays["small"])   # under its share: whole
    share = limit // 3
    for n in ("big", "wide"):
        assert got[n].dtype == arrays[n].dtype and got[n].shape == (share // arrays[n].itemsize,)
        assert np.isin(got[n], arrays[n]).all()
        np.testing.assert_array_equal(got[n], np.load(str(tmp_path / "b" / (n + ".npy"))))   # the same sample again
    # everything fits: written whole, in the arrays' own shapes
    bench.dump_outputs(str(tmp_path / "c"), arrays)
    for n in arrays:
        np.testing.assert_array_equal(np.load(str(tmp_path / "c" / (n + ".npy"))), arrays[n])


@pytest.mark.gpu
def test_plain_run_line_and_dump(tmp_path):
    """Two runs with the same arguments (side by side, to keep the test short): the line of a plain run, the dumped
    outputs of the last timed step, and that the second run wrote the same bits (the dump runs in the deterministic
    mode; the weights move from the second step on, so 5 steps put 3 updates behind the dumped outputs)."""
    outs = [tmp_path / "dump_a", tmp_path / "dump_b"]
    procs = [subprocess.Popen([sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1", "--steps", "3",
                               "--warmup", "2", "--batch", "8", "--dump-outputs", str(o)], stdout=subprocess.PIPE,
                              stderr=subprocess.PIPE, text=True, cwd=REPO) for o in outs]
    done = [p.communicate(timeout=240) + (p.returncode,) for p in procs]
    lines = []
    for so, se, rc in done:
        line = [l for l in so.splitlines() if l.startswith("{")]
        assert rc == 0 and len(line) == 1, (rc, so[-2000:], se[-4000:])
        lines.append(json.loads(line[0]))
    res = lines[0]
    assert res["steps"] == 3 and res["unit"] == "samples/s" and res["higher_is_better"] is True
    assert res["dtype"] == "fp32" and res["metric"].startswith("pretrain samples/sec/GPU")
    assert res["ms_per_step"] > 0 and abs(res["value"] - 8 * 1000.0 / res["ms_per_step"]) <= 1e-4 * res["value"]
    assert res["deterministic"] is True
    # what takes runs of its own stays behind --full
    for k in ("roofline", "roofline_ffn1", "coattn", "gemm_all", "cpu_baseline", "parity", "host_issue_ms"):
        assert k not in res
    out = outs[0]
    got = {f[:-4]: np.load(str(out / f)) for f in sorted(os.listdir(str(out)))}
    assert {"loss", "masked_lm_loss", "masked_lm_loss_pv", "masked_img_loss", "loss_lpm", "next_sentence_loss",
            "pooled_t", "pooled_pv", "pooled_v", "c_initial", "c_final"} <= set(got)
    assert sum(a.nbytes for a in got.values()) <= 64 * 1000 * 1000
    for n, a in got.items():
        assert a.dtype in (np.float32, np.float64) and np.isfinite(a).all(), n
    assert got["pooled_t"].shape == (8, 768)
    assert abs(float(got["loss"][0]) - res["loss"]) <= 1e-4   # the line's is rounded to 4 decimals
    np.testing.assert_allclose(got["loss"][0], got["masked_lm_loss"][0] + got["masked_lm_loss_pv"][0]
                               + got["masked_img_loss"][0] + got["loss_lpm"][0], rtol=1e-5)
    assert sorted(os.listdir(str(outs[1]))) == sorted(os.listdir(str(out)))
    for n, a in got.items():
        b = np.load(str(outs[1] / (n + ".npy")))
        assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), n
    assert lines[1]["loss"] == res["loss"]
