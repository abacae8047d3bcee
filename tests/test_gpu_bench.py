"""bench.py as a command: a plain run (set-up, warmup, the timed steps, one JSON line) with --dump-outputs.

One short run in a child process (the bench owns its process: hardware queues, HIP runtime): the result line
carries the headline fields and none of what --full adds, --steps is the number of timed steps, and the
dumped arrays are what the last timed step handed out (float64 .npy, well under 64 MB, counts within the
workload's capacities, every value finite)."""
import json
import pathlib
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = pathlib.Path(__file__).resolve().parents[1]


def test_plain_bench_line_and_dumped_outputs(tmp_path):
    out = tmp_path / "dump"
    p = subprocess.run([sys.executable, str(ROOT / "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                        "--dump-outputs", str(out)], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = p.stdout.strip().splitlines()
    assert len(lines) == 1  # stdout is the one JSON line
    d = json.loads(lines[0])
    assert d["steps"] == 3 and d["warmup"] == 1 and d["n_gpus"] == 1
    assert d["unit"] == "frames/s" and d["higher_is_better"] is True and "fp16" in d["dtype"]
    assert d["ms_per_step"] > 0 and d["value"] == pytest.approx(1e3 / d["ms_per_step"], rel=1e-2)
    # only --full measures these
    assert not {"cpu_baseline", "ate", "fp16x3_run"} & set(d)
    assert not [k for k in d["stages_roofline"] if k.startswith("ba:")]

    files = {f.stem: np.load(f) for f in out.glob("*.npy")}
    assert {"sp_features", "sp_counts", "sg_indices0", "sg_indices1", "sg_mscores0", "sg_mscores1", "lines_left",
            "lines_right", "line_counts", "stereo_lines_right", "stereo_lines_valid", "ba_pose_q", "ba_pose_p",
            "ba_points", "ba_lines", "ba_chi2", "ba_iterations"} <= set(files)
    assert all(a.dtype == np.float64 and np.isfinite(a).all() for a in files.values())
    assert sum(a.nbytes for a in files.values()) <= 64 << 20
    K = 400  # the C3 workload's keypoint capacity
    assert files["sp_features"].shape == (2, K, 259)
    n = files["sp_counts"].astype(int)
    assert ((0 < n) & (n <= K)).all()
    for b in range(2):  # rows past the count are zeroed, the rows before it hold keypoints inside the image
        assert not files["sp_features"][b, n[b]:].any()
        assert (files["sp_features"][b, :n[b], 1] >= 0).all() and (files["sp_features"][b, :n[b], 1] < 752).all()
    assert files["sg_indices0"].shape == (2, K) and (files["sg_indices0"] >= -1).all() and (files["sg_indices0"] < K).all()
    assert files["ba_pose_q"].shape == (10, 4) and files["ba_pose_p"].shape == (10, 3)
    assert np.abs(np.linalg.norm(files["ba_pose_q"], axis=1) - 1).max() < 1e-9  # unit quaternions
    assert 0 < files["ba_chi2"][1] <= files["ba_chi2"][0]
