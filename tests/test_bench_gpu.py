"""bench.py on an MI355X: a plain run prints the headline line and nothing of --full, and --dump-outputs writes the last step's outputs."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
def test_plain_run_line_and_dumped_outputs(tmp_path):
    out = tmp_path / "dump"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "6", "--warmup", "3", "--surfels", "300000", "--loop", "30",
                        "--dump-outputs", str(out)], cwd=ROOT, capture_output=True, text=True, timeout=420)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = r.stdout.strip().splitlines()
    assert len(lines) == 1, lines
    d = json.loads(lines[0])
    assert d["steps"] == 6 and d["warmup"] == 3 and d["unit"] == "frames/s" and d["higher_is_better"] is True and d["dtype"] == "f32"
    assert d["metric"].startswith("frames/s") and d["ms_per_step"] > 0
    assert abs(d["value"] * d["ms_per_step"] - 1000.0) < 1.0
    assert d["roofline"] is None and d["cpu_baseline"] is None and "ms_per_frame_gpu" not in d and "value_sharded" not in d   # (measured with --full only)

    got = {f[:-4]: np.load(out / f) for f in os.listdir(out)}
    assert set(got) == {"pose", "ids_after", "surfel_count", "instance_table", "map_pc", "map_nr", "map_col", "map_tm", "map_label", "map_votes"}
    assert all(a.dtype in (np.float32, np.float64) for a in got.values())
    assert sum(a.nbytes for a in got.values()) <= 64 << 20
    n = int(got["surfel_count"][0])
    assert n == d["config"]["surfels_live"]
    s = min(n, 1 << 18)
    assert got["map_pc"].shape == (s, 4) and got["map_nr"].shape == (s, 4) and got["map_col"].shape == (s, 2) and got["map_tm"].shape == (s, 2)
    assert got["map_label"].shape == (s,) and got["map_votes"].shape == (min(s, 1 << 16), 48)
    assert got["ids_after"].shape == (480, 640) and got["instance_table"].shape == (96,)
    R = got["pose"][:3, :3].astype(np.float64)
    assert got["pose"].shape == (4, 4) and np.allclose(R @ R.T, np.eye(3), atol=1e-5) and np.array_equal(got["pose"][3], [0, 0, 0, 1])
    assert np.isfinite(got["map_pc"]).all() and (got["map_pc"][:, 3] > 0).any()
