"""C++ host layer: `ifx_replay --mask-lag K` applies the masks recorded for frame t at frame t + K through InstanceFusion::SnapshotSegmentation /
ProcessSegmentationDeferred.  K = 0 writes the files of a run without the flag, byte for byte; K = 3 runs and labels a non-empty set."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT, SMALL

REPLAY = os.path.join(ROOT, "instancefusion_amd", "ifx_replay")


@pytest.mark.gpu
def test_replay_mask_lag(small_stream, tmp_path):
    from instancefusion_amd import logio, synth

    st = small_stream
    n = 16                                                    # long enough for surfels to become stable (confidence > 2) and take labels
    # The first frame carries no depth: surfels of a map's FIRST frame start with the reference's -1 vote counters (init_unstable.vert), which keep a pixel out of
    # every mask box (instanceProjectMap != -1, IF/Core/InstanceFusionCuda.cu:915), so a log that starts on a full frame labels nothing in 16 frames; surfels
    # appended by later frames start at 0.  Then the 10-frame stream forth and back.
    src = [0] + [i if i < 10 else 18 - i for i in range(n)]
    klg = str(tmp_path / "s.klg")
    wr = logio.RawLogWriter(klg, depth="zlib", image="raw")
    for i in range(n + 1):
        wr.add(33333 * i, st["rgb"][src[i]], st["depth"][src[i]] if i > 0 else np.zeros_like(st["depth"][0]))
    wr.close()
    mdir = tmp_path / "masks"
    mdir.mkdir()
    for i in range(n):
        mk, cl = synth.canned_masks(st["obj"][src[i]], st["scene"])
        np.savez(mdir / f"{i:06d}.npz", masks=mk, class_ids=cl)
    common = ["--width", str(SMALL["w"]), "--height", str(SMALL["h"]), "--fx", str(SMALL["fx"]), "--fy", str(SMALL["fy"]), "--cx", str(SMALL["cx"]),
              "--cy", str(SMALL["cy"]), "--max-surfels", "400000", "--masks", str(mdir), "--flann-every", "2", "--confidence", "2", "--no-close-loops"]
    outs = {}
    for tag, extra in (("plain", []), ("lag0", ["--mask-lag", "0"]), ("lag3", ["--mask-lag", "3"])):
        out = str(tmp_path / tag)
        r = subprocess.run([REPLAY, klg] + common + extra + ["--out", out, "--labels", out + ".labels"], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr
        assert f"{n} frames" in r.stdout and " 0 segmentation calls" not in r.stdout, r.stdout
        outs[tag] = out
    assert open(outs["plain"] + ".freiburg").read() == open(outs["lag0"] + ".freiburg").read()
    for suffix in (".ply", "_Instance.ply", ".labels"):
        assert open(outs["plain"] + suffix, "rb").read() == open(outs["lag0"] + suffix, "rb").read(), suffix
    assert (np.fromfile(outs["plain"] + ".labels", np.int32) >= 0).sum() > 0
    lab3 = np.fromfile(outs["lag3"] + ".labels", np.int32)
    assert lab3.size > 0 and (lab3 >= 0).sum() > 0
