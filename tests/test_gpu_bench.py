"""A plain bench.py run on the GPU: exactly --steps timed steps, the headline fields and nothing the headline does not need,
and --dump-outputs writing the same arrays in two runs with the same arguments (seeded inputs, slice-order split-K sums)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FULL_ONLY = {"value_settled", "repeats", "host_post_ms_per_frame", "h2d_inclusive", "clocks_under_load", "roofline",
             "other_precisions", "configs2", "other_configs", "flip_rate", "cpu_baseline"}


def _bench(out_dir, steps=6):
    r = subprocess.run([sys.executable, "bench.py", "--gpus", "1", "--steps", str(steps), "--warmup", "2",
                        "--dump-outputs", str(out_dir)], capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout
    return json.loads(lines[0]), {f[:-len(".npy")]: np.load(os.path.join(out_dir, f)) for f in os.listdir(out_dir)}


def test_plain_bench_line_and_dumped_outputs(tmp_path, cuda):
    a, da = _bench(tmp_path / "a")
    b, db = _bench(tmp_path / "b")
    for line in (a, b):
        assert line["steps"] == 6 and line["warmup"] == 2 and line["unit"] == "frames/sec" and line["higher_is_better"] is True
        assert {"metric", "value", "dtype", "ms_per_step"} <= set(line) and not FULL_ONLY & set(line)
        assert abs(line["value"] - 6 / (line["ms_per_step"] * 6 / 1e3)) / line["value"] < 1e-3
        assert line["records_gathered"] == 6 and line["detections"] == 6 and line["poses"] == 6
    assert set(da) == set(db) and "records" in da and "cam_R" in da
    for k in da:
        assert da[k].dtype in (np.float32, np.float64) and len(da[k]) == 1, k
        np.testing.assert_array_equal(da[k], db[k], err_msg=k)
    assert np.isfinite(da["cam_R"]).all() and np.isfinite(da["keypoints"]).all()
