"""What a tracker run enqueues, pinned: the launch counts of the tracker's kernels (option kernel_timing, ifx_kernel_ms) over three synthetic frames, under every
setting that changes the run's form -- the prologue chain and where it ends, the list and the fused iterations, the persistent level kernel in front of and behind
two-launch iterations, no pyramid, fast odometry, ICP only, photometric only, and the model-to-model tracker of the loop-closure detection (the CHECK_SKIP kernels).

The counts are compared with tests/golden/tracker_launch_counts.json, which this file records when run as a program (`python tests/test_gpu_tracker_launches.py
--record`, the package to record from first on PYTHONPATH).  Counts do not pin grids: the bit-for-bit comparisons between the forms (tests/test_gpu_parity.py,
tests/test_gpu_rgb_fused_step.py, tests/test_gpu_rgb_candidates.py) are what notices a changed grid."""
import json
import os
import sys

import pytest

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "tracker_launch_counts.json")
SIZES = {"160x120": dict(w=160, h=120, fx=132.0, fy=132.0, cx=80.0, cy=60.0), "320x240": dict(w=320, h=240, fx=264.0, fy=264.0, cx=160.0, cy=120.0)}   # (tests/test_gpu_rgb_fused_step.py)
NAMES = ["track_gn_begin", "icp_residual@L0", "icp_residual@L1", "icp_residual@L2", "rgb_step_solve@L0", "rgb_step_solve@L1", "rgb_step_solve@L2", "gn_level", "gn_level_solo",
         "track_end", "so3_fused"]
FRAMES = 3
# gn_prologue_blocks = 50: the launches of a list run have 8 / 24 / 85 blocks at levels 2 / 1 / 0 of 160x120 and 29 / 94 / 338 of 320x240 (ICP blocks + list blocks), so
# the chain ends after level 1 of the small size and after level 2 of the large one -- before the finest level in both: rgb_step_solve@L0 counts every iteration
SETTINGS = {
    "defaults": {},
    "gn_prologue=0": dict(gn_prologue=0),
    "rgb_cand=0": dict(rgb_cand=0),
    "rgb_fuse=0": dict(rgb_fuse=0),
    "rgb_fuse=5": dict(rgb_fuse=5),
    "gn_persist=4": dict(gn_persist=4),
    "gn_persist=5,blocks=1<<20": dict(gn_persist=5, gn_persist_blocks=1 << 20),
    "gn_prologue_blocks=50": dict(gn_prologue_blocks=50),
    "pyramid=0": dict(pyramid=0),
    "fast_odom=1": dict(fast_odom=1),
    "icp_weight_x1000=100000": dict(icp_weight_x1000=100000),
    "icp_weight_x1000=0": dict(icp_weight_x1000=0),
    "loop_closure": "loop_closure",
}


def _streams():
    from instancefusion_amd import synth

    return {name: synth.make_stream(FRAMES, K["w"], K["h"], K["fx"], K["fy"], K["cx"], K["cy"], noise=True) for name, K in SIZES.items()}


def _counts(ifx, st, size, setting):
    opts = SETTINGS[setting]
    lc = opts == "loop_closure"
    g = ifx.ElasticFusion(max_surfels=400000, **SIZES[size], **(dict(time_delta=1) if lc else {}))   # (time_delta = 1: the detection is due from the second frame on)
    if lc:
        g.set_loop_closure(True)
    else:
        for k, v in opts.items():
            g.set_option(k, v)
    g.set_option("kernel_timing", 1)
    for i in range(FRAMES):
        g.processFrame(st[size]["rgb"][i], st[size]["depth"][i])
    out = {name: g.kernel_ms(name)[1] for name in NAMES}
    g.close()
    return out


@pytest.fixture(scope="module")
def ifx():
    import instancefusion_amd as m

    m.lib()
    return m


@pytest.fixture(scope="module")
def streams():
    return _streams()


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


@pytest.mark.parametrize("size", list(SIZES))
@pytest.mark.parametrize("setting", list(SETTINGS))
def test_tracker_launch_counts(ifx, streams, golden, size, setting):
    got = _counts(ifx, streams, size, setting)
    print(f"{size} {setting}: {got}")
    assert got == golden[size][setting]


def test_recorded_counts_show_the_forms(golden):
    """The recorded table itself: each setting must have reached the form it is there for."""
    for size in SIZES:
        t = golden[size]
        d = t["defaults"]
        assert set(t) == set(SETTINGS) and all(set(t[s]) == set(NAMES) for s in t)
        assert d["rgb_step_solve@L0"] == FRAMES - 1 and d["rgb_step_solve@L1"] == 0 and d["rgb_step_solve@L2"] == 0   # the chain reaches the finest level, every iteration but the run's last is fused
        assert d["icp_residual@L0"] == 10 * (FRAMES - 1) and d["gn_level"] == 0 and d["track_end"] == 0
        assert t["rgb_fuse=0"]["rgb_step_solve@L0"] == 10 * (FRAMES - 1) and t["rgb_fuse=5"]["rgb_step_solve@L1"] == 5 * (FRAMES - 1)
        assert t["gn_persist=4"]["gn_level"] == FRAMES - 1 and t["gn_persist=4"]["icp_residual@L2"] == 0
        assert t["gn_persist=5,blocks=1<<20"]["gn_level"] == 2 * (FRAMES - 1) and t["gn_persist=5,blocks=1<<20"]["gn_level_solo"] == 2 * (FRAMES - 1)
        assert t["gn_prologue_blocks=50"]["rgb_step_solve@L0"] == 10 * (FRAMES - 1)                                 # the chain ended before the finest level
        assert t["pyramid=0"]["icp_residual@L1"] == 0 and t["fast_odom=1"]["icp_residual@L0"] == 3 * (FRAMES - 1)
        assert t["loop_closure"]["icp_residual@L0"] > d["icp_residual@L0"]                                          # the model-to-model run's launches (CHECK_SKIP)


if __name__ == "__main__":
    if sys.argv[1:] != ["--record"]:
        sys.exit("usage: python tests/test_gpu_tracker_launches.py --record   (writes tests/golden/tracker_launch_counts.json)")
    sys.path.append(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))   # (behind PYTHONPATH: the package named there is the one recorded)
    import torch  # noqa: F401  (first, as tests/conftest.py does: the library binds to the HIP runtime torch ships)

    import instancefusion_amd as pkg

    pkg.lib()
    print("recording from", os.path.dirname(pkg.__file__))
    st = _streams()
    table = {size: {setting: _counts(pkg, st, size, setting) for setting in SETTINGS} for size in SIZES}
    with open(GOLDEN, "w") as f:
        json.dump(table, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(table))
