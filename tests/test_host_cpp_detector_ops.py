"""C++ host layer: ElasticFusion::RoiAlignForward / Nms compile against ifx_host.hpp with plain g++ -- no HIP header.  Without a GPU the map cannot be created and the
helper says so; with one, one call of each operator through the C++ class gives the statement's values (tests/detector_ops_numpy.py): every ROIAlign bit, the
kept indices, -1 behind them, the count."""
import os
import subprocess

import numpy as np

from conftest import ROOT

HOST = os.path.join(ROOT, "instancefusion_amd", "host")
LIBDIR = os.path.join(ROOT, "instancefusion_amd")


def test_detector_ops_compile_refuse_without_gpu_and_equal_the_statement(tmp_path):
    import torch

    import detector_ops_numpy as dn

    exe = str(tmp_path / "detector_ops_check")
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-pthread", "-I", os.path.join(ROOT, "include"), "-I", HOST,
                    os.path.join(ROOT, "tests", "cpp", "detector_ops_check.cpp"), "-L", LIBDIR, "-lifx", "-lz", "-ldl", f"-Wl,-rpath,{LIBDIR}", "-o", exe], check=True)
    rng = np.random.default_rng(21)
    B, Cn, H, W, n, ph, pw, ratio, nb = 2, 70, 11, 13, 6, 7, 7, 2, 150
    scale, thr = np.float32(0.25), np.float32(0.5)
    inp = rng.standard_normal((B, Cn, H, W)).astype(np.float32)
    x0, y0 = rng.uniform(-8, 40, n), rng.uniform(-8, 30, n)
    rois = np.stack([rng.integers(0, B, n).astype(np.float64), x0, y0, x0 + rng.uniform(0, 40, n), y0 + rng.uniform(0, 30, n)], axis=1).astype(np.float32)
    c = rng.uniform(0, 90, (nb, 2))
    boxes = np.concatenate([c, c + rng.uniform(4, 40, (nb, 2))], axis=1).astype(np.float32)
    scores = rng.random(nb).astype(np.float32)
    fin, fout = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(fin, "wb") as f:
        f.write(np.asarray([B, Cn, H, W, n, ph, pw, ratio, nb], np.int32).tobytes())
        f.write(np.asarray([scale, thr], np.float32).tobytes())
        for a in (inp, rois, boxes, scores):
            f.write(a.tobytes())
    r = subprocess.run([exe, fin, fout], capture_output=True, text=True, check=True, cwd=str(tmp_path))
    lines = r.stdout.splitlines()
    if not torch.cuda.is_available():
        assert lines[0].startswith("refused: ifx_create") and "no HIP device" in lines[0], r.stdout
        return
    ref = dn.roi_align_forward(inp, rois, scale, ph, pw, ratio)
    keep = dn.nms(boxes, scores, thr)
    assert 0 < keep.size < nb
    assert lines[0] == f"wrote {ref.size} {keep.size}", r.stdout
    assert lines[1].startswith("refused n: ifx_nms:") and "8192" in lines[1], r.stdout
    raw = open(fout, "rb").read()
    assert len(raw) == ref.size * 4 + nb * 8 + 4
    got = np.frombuffer(raw, np.float32, ref.size).reshape(ref.shape)
    got_keep = np.frombuffer(raw, np.int64, nb, ref.size * 4)
    got_count = int(np.frombuffer(raw, np.int32, 1, ref.size * 4 + nb * 8)[0])
    assert np.array_equal(got.view(np.uint32), ref.view(np.uint32))
    assert got_count == keep.size and np.array_equal(got_keep[:got_count], keep) and (got_keep[got_count:] == -1).all()
