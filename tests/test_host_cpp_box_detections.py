"""C++ host layer: ElasticFusion::BoxDetections compiles against ifx_host.hpp with plain g++ -- no HIP header.  Without a GPU the map cannot be created and the
helper says so; with one, one call through the C++ class gives the bytes of the Python call and of the statement (tests/box_detections_numpy.py): boxes, scores,
labels, indices, the padding behind the count, the count, the stats; one refused call reports the library's message."""
import os
import subprocess

import numpy as np

import box_detections_cases as bc
from conftest import ROOT

HOST = os.path.join(ROOT, "instancefusion_amd", "host")
LIBDIR = os.path.join(ROOT, "instancefusion_amd")


def test_box_detections_compile_refuse_without_gpu_and_equal_the_python_call(tmp_path):
    import torch

    import box_detections_numpy as bd

    exe = str(tmp_path / "box_detections_check")
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-pthread", "-I", os.path.join(ROOT, "include"), "-I", HOST,
                    os.path.join(ROOT, "tests", "cpp", "box_detections_check.cpp"), "-L", LIBDIR, "-lifx", "-lz", "-ldl", f"-Wl,-rpath,{LIBDIR}", "-o", exe], check=True)
    R, Cn, M, rows = 400, 81, 60, 80
    st, nms, weights = np.float32(0.05), np.float32(0.5), np.asarray(bc.WEIGHTS, np.float32)
    logits, reg, prop, img = bc.head(60, R, Cn, scale=2.5)
    fin, fout = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(fin, "wb") as f:
        f.write(np.asarray([R, Cn, Cn, M, rows, img[0], img[1]], np.int32).tobytes())
        f.write(np.asarray([st, nms], np.float32).tobytes())
        f.write(weights.tobytes())
        for a in (logits, reg, prop):
            f.write(a.tobytes())
    r = subprocess.run([exe, fin, fout], capture_output=True, text=True, check=True, cwd=str(tmp_path))
    lines = r.stdout.splitlines()
    if not torch.cuda.is_available():
        assert lines[0].startswith("refused: ifx_create") and "no HIP device" in lines[0], r.stdout
        return
    import instancefusion_amd as ifx

    ref = bd.box_detections(logits, reg, prop, img, st, nms, M, tuple(weights))
    pb, ps, pl, pi, c, stats = bd.padded(ref, rows)
    assert c == M and stats[1] > M
    assert lines[0] == f"wrote {c}", r.stdout
    assert lines[1].startswith("refused max_out: ifx_box_detections:") and "8192" in lines[1], r.stdout
    raw = open(fout, "rb").read()
    assert len(raw) == rows * 36 + 12
    got_boxes = np.frombuffer(raw, np.uint32, rows * 4).reshape(rows, 4)
    got_scores = np.frombuffer(raw, np.uint32, rows, rows * 16)
    got_labels = np.frombuffer(raw, np.int64, rows, rows * 20)
    got_index = np.frombuffer(raw, np.int64, rows, rows * 28)
    got_tail = np.frombuffer(raw, np.int32, 3, rows * 36)
    assert got_tail.tolist() == [c, int(stats[0]), int(stats[1])]
    assert np.array_equal(got_boxes, pb.view(np.uint32)) and np.array_equal(got_scores, ps.view(np.uint32))
    assert np.array_equal(got_labels, pl) and np.array_equal(got_index, pi)
    ef = ifx.ElasticFusion(w=160, h=120, fx=132.0, fy=132.0, cx=80.0, cy=60.0, max_surfels=100000)       # the same bytes as the Python call
    d = [torch.from_numpy(a).cuda() for a in (logits, reg, prop)]
    b, s, l, i, n, k = ef.box_detections(*d, img, float(st), float(nms), M, tuple(weights), max_out=rows, padded=True)
    assert int(n.item()) == c and k.tolist() == got_tail[1:].tolist() and np.array_equal(b.cpu().numpy().view(np.uint32), got_boxes)
    assert np.array_equal(s.cpu().numpy().view(np.uint32), got_scores) and np.array_equal(l.cpu().numpy(), got_labels) and np.array_equal(i.cpu().numpy(), got_index)
    ef.close()
