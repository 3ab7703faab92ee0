"""The C++ host's deferred segmentation on the spatially sharded map: `ifx_replay --shard-ranks -1 --mask-lag 4` (InstanceFusion::SnapshotSegmentation /
ProcessSegmentationDeferred on a sharded host: ifx_owner_segmentation_snapshot / ifx_owner_process_segmentation_deferred, every exchange a RCCL collective
enqueued by libifx.so) against the unsharded `ifx_replay --mask-lag 4`: identical trajectory file, PLY models and labels."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT, SMALL

REPLAY = os.path.join(ROOT, "instancefusion_amd", "ifx_replay")


@pytest.mark.gpu
def test_cpp_replay_sharded_world_of_one_mask_lag_equals_unsharded(small_stream, tmp_path):
    """test_cpp_replay_sharded_world_of_one_equals_unsharded's log and masks, the masks of frame t arriving at frame t + 4 on both sides."""
    from instancefusion_amd import logio, synth

    st = small_stream
    n = 16                                                    # long enough for surfels to become stable (confidence > 2) and take labels
    src = [i if i < 10 else 18 - i for i in range(n + 1)]
    klg = str(tmp_path / "s.klg")
    wr = logio.RawLogWriter(klg, depth="zlib", image="raw")
    for i in range(n + 1):
        wr.add(33333 * i, st["rgb"][src[i]], st["depth"][src[i]])
    wr.close()
    mdir = tmp_path / "masks"
    mdir.mkdir()
    for i in range(n):
        mk, cl = synth.canned_masks(st["obj"][src[i]], st["scene"])
        np.savez(mdir / f"{i:06d}.npz", masks=mk, class_ids=cl)
    common = ["--width", str(SMALL["w"]), "--height", str(SMALL["h"]), "--fx", str(SMALL["fx"]), "--fy", str(SMALL["fy"]), "--cx", str(SMALL["cx"]),
              "--cy", str(SMALL["cy"]), "--max-surfels", "400000", "--masks", str(mdir), "--flann-every", "2", "--confidence", "2", "--no-close-loops", "--mask-lag", "4"]
    outs = {}
    for tag, extra in (("one", []), ("shard", ["--shard-ranks", "-1"])):
        out = str(tmp_path / tag)
        r = subprocess.run([REPLAY, klg] + common + extra + ["--out", out, "--labels", out + ".labels"], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr
        assert f"{n} frames" in r.stdout and " 0 segmentation calls" not in r.stdout
        outs[tag] = out
    assert open(outs["one"] + ".freiburg").read() == open(outs["shard"] + ".freiburg").read()
    for suffix in (".ply", "_Instance.ply"):
        assert open(outs["one"] + suffix, "rb").read() == open(outs["shard"] + suffix, "rb").read(), suffix
    lab = np.fromfile(outs["one"] + ".labels", np.int32)
    assert lab.size > 0 and np.array_equal(lab, np.fromfile(outs["shard"] + ".labels", np.int32))
