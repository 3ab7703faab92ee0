"""C++ hosts and the free-viewpoint render of a spatially sharded map: a small program (tests/cpp/sharded_view_check.cpp) compiles against ifx_host.hpp with plain
g++ -- no HIP header -- and drives ElasticFusionInterface::RenderMapToBuffer / RenderMapIDToBuffer on a sharded host (ifx_owner_render_view); ifx_replay
--shard-ranks -1 --view-ppm writes the bytes of the unsharded replay."""
import os
import subprocess

import pytest

from conftest import ROOT, SMALL

HOST = os.path.join(ROOT, "instancefusion_amd", "host")
LIBDIR = os.path.join(ROOT, "instancefusion_amd")
REPLAY = os.path.join(LIBDIR, "ifx_replay")


def _build(tmp_path):
    exe = str(tmp_path / "sharded_view_check")
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-pthread", "-I", os.path.join(ROOT, "include"), "-I", HOST,
                    os.path.join(ROOT, "tests", "cpp", "sharded_view_check.cpp"), "-L", LIBDIR, "-lifx", "-lz", "-ldl", f"-Wl,-rpath,{LIBDIR}", "-o", exe], check=True)
    return exe


def test_sharded_render_compiles_and_refuses_without_gpu(tmp_path):
    """without a GPU Init fails and RenderMapToBuffer throws with its buffers untouched (the program checks them); with one, the empty map at a world of one is the
    clear colour with alpha 0 and ids -1, at two collectives and 24 B / pixel -- one and 8 B / pixel for the ids alone"""
    import torch

    r = subprocess.run([_build(tmp_path)], capture_output=True, text=True, check=True, cwd=str(tmp_path))
    lines = r.stdout.splitlines()
    if not torch.cuda.is_available():
        assert lines[0].startswith("refused: ifx_render_view: "), r.stdout      # (no handle: the host is not sharded, nor anything else)
        return
    px = 37 * 29
    assert lines == ["created", f"empty {px} of {px}", f"collectives 2 bytes {24 * px}", f"ids only: collectives 1 bytes {8 * px}"], r.stdout


@pytest.mark.gpu
def test_replay_view_ppm_sharded_equals_unsharded(small_stream, tmp_path):
    """ifx_replay --view-ppm over the same .klg, unsharded and as a world of one on the sharded path (--shard-ranks -1): the same bytes, from the default camera with the
    colours and from a given one with the instance colours"""
    from instancefusion_amd import logio

    st = small_stream
    klg = str(tmp_path / "s.klg")
    wr = logio.RawLogWriter(klg, depth="zlib", image="jpeg", jpeg_quality=95)
    for i in range(8):
        wr.add(33333 * i, st["rgb"][i], st["depth"][i])
    wr.close()
    common = ["--width", str(SMALL["w"]), "--height", str(SMALL["h"]), "--fx", str(SMALL["fx"]), "--fy", str(SMALL["fy"]), "--cx", str(SMALL["cx"]),
              "--cy", str(SMALL["cy"]), "--max-surfels", "400000", "--confidence", "2", "--no-close-loops"]
    views = {"gui": ["--view-size", "160x120"],
             "posed": ["--view-size", "200x90", "--view-instances", "--view-pose", "0.8660254 0 0.5 -0.4 0 1 0 0.05 -0.5 0 0.8660254 -0.6 0 0 0 1"]}
    for name, extra in views.items():
        out = {}
        for kind, shard in (("one", []), ("sharded", ["--shard-ranks", "-1"])):
            prefix = str(tmp_path / f"{kind}_{name}")
            r = subprocess.run([REPLAY, klg] + common + shard + ["--out", prefix, "--view-ppm", prefix + ".ppm"] + extra, capture_output=True, text=True, timeout=300)
            assert r.returncode == 0, r.stderr
            out[kind] = open(prefix + ".ppm", "rb").read()
        w, h = (int(v) for v in extra[1].split("x"))
        head = f"P6\n{w} {h}\n255\n".encode()
        assert out["one"].startswith(head) and len(out["one"]) == len(head) + w * h * 3
        assert out["sharded"] == out["one"], name
        assert len(set(out["one"][len(head):])) > 8, name      # the map is in view: more than the GUI's white
