"""`reloc` and `frameToFrameRGB` through the C++ host layer: ifx_replay --reloc ends a replay at the first lost frame, as IF/main.cpp:137-142 does, and a translation
unit that constructs ElasticFusion with frameToFrameRGB = true builds and runs frames."""
import os
import subprocess

import pytest

import reloc_reference as rr
from conftest import ROOT

HOST = os.path.join(ROOT, "instancefusion_amd", "host")
REPLAY = os.path.join(ROOT, "instancefusion_amd", "ifx_replay")
LIBDIR = os.path.join(ROOT, "instancefusion_amd")


def _build(tmp_path):
    exe = str(tmp_path / "host_f2f_frame")
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-pthread", "-I", os.path.join(ROOT, "include"), "-I", HOST,
                    os.path.join(ROOT, "tests", "cpp", "host_f2f_frame.cpp"), "-L", LIBDIR, "-lifx", "-lz", f"-Wl,-rpath,{LIBDIR}", "-o", exe], check=True)
    return exe


def test_frame_to_frame_rgb_unit_builds(tmp_path):
    _build(tmp_path)


@pytest.mark.gpu
@pytest.mark.parametrize("reloc", [0, 1])
def test_host_class_runs_frames_with_frame_to_frame_rgb(tmp_path, reloc):
    r = subprocess.run([_build(tmp_path), "160", "120", str(reloc)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert r.stdout.startswith("frames 4 surfels ") and int(r.stdout.split()[3]) > 10000 and " lost 0 fused 1" in r.stdout, r.stdout


@pytest.mark.gpu
def test_replay_ends_at_the_first_lost_frame(tmp_path):
    """A log of the scenario's frames 0-17: with --reloc the map is lost at frame 16 (eleven frames in a row failed the gate), the program prints the reference's
    line and exits with status 1; without it every frame is fused whatever the tracker produced and it exits 0."""
    from instancefusion_amd import logio

    st = rr.scenario_stream()
    klg = str(tmp_path / "scenario.klg")
    wr = logio.RawLogWriter(klg)
    for i in range(18):
        wr.add(33333 * i, st["rgb"][i], st["depth"][i])
    wr.close()
    K = rr.SCENARIO
    common = [REPLAY, klg, "--width", str(K["w"]), "--height", str(K["h"]), "--fx", str(K["fx"]), "--fy", str(K["fy"]), "--cx", str(K["cx"]), "--cy", str(K["cy"]),
              "--max-surfels", "262144", "--out", str(tmp_path / "M")]
    r = subprocess.run(common + ["--reloc"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 1 and "Elastic fusion lost!" in r.stdout, (r.returncode, r.stdout, r.stderr)
    r = subprocess.run(common, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "Elastic fusion lost!" not in r.stdout and "17 frames" in r.stdout   # (the replay loop stops in front of the log's last record, as IF/main.cpp does), (r.returncode, r.stdout, r.stderr)
