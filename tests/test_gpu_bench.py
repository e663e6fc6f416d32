"""A plain ``bench.py --gpus 1 --steps N --warmup W`` run end to end on the MI355X: it exits 0 and prints one JSON line with
the contract's fields, runs none of the ``--full`` legs, and ``--dump-outputs`` writes the seven metrics and the depth map of
the last timed step.  ('fullsize': BASELINE configs[1], run with the heavy tests at the end, tests/conftest.py.)"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
def test_plain_bench_run_fullsize(tmp_path):
    out_dir = str(tmp_path / "dump")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                        "--dump-outputs", out_dir], capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    line = json.loads(r.stdout.strip().splitlines()[-1])
    assert (line["metric"], line["unit"], line["higher_is_better"], line["dtype"]) == ("frames/s", "frames/s", True, "f32")
    assert (line["n_gpus"], line["steps"], line["warmup"]) == (1, 3, 1)
    assert line["value"] > 0 and line["ms_per_step"] > 0
    assert abs(line["value"] - 4 * 3 / (3 * line["ms_per_step"] * 1e-3)) < 0.01 * line["value"]    # batch 1 x seq_len 4 frames
    assert line["ms_per_step_runs"]["runs"] == [line["ms_per_step"]]                                # one timed region
    for key in ("roofline", "roofline_hotpath", "roofline_front", "configs2", "cpu_baseline", "cpu_baseline_config1", "parity"):
        assert key not in line, key
    names = sorted(line["dumped_outputs"]["files"])
    assert names == sorted(["depth"] + [f"metric_{m}" for m in ("AbsRel", "SqRel", "RMSE", "RMSE_log", "Delta1", "Delta2", "Delta3")])
    depth = np.load(os.path.join(out_dir, "depth.npy"))
    assert depth.shape == (1, 384, 1280, 1) and np.isfinite(depth).all()
    absrel = float(np.load(os.path.join(out_dir, "metric_AbsRel.npy"))[0])             # (the line rounds it to 6 decimals)
    assert np.isfinite(absrel) and abs(absrel - line["AbsRel"]) <= 1e-6 * abs(absrel) + 1e-6
