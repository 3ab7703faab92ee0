"""C++ host layer: ElasticFusion::RpnProposalsFpn compiles against ifx_host.hpp with plain g++ -- no HIP header.  Without a GPU the map cannot be created and the
helper says so; with one, one call through the C++ class on a three-level input gives the bytes of the Python call and of the statement (tests/rpn_fpn_numpy.py):
boxes, logits, levels, indices, the padding behind the count, the count, the levels' counts; nine levels are refused."""
import os
import subprocess

import numpy as np

import rpn_fpn_cases as fc
from conftest import ROOT

HOST = os.path.join(ROOT, "instancefusion_amd", "host")
LIBDIR = os.path.join(ROOT, "instancefusion_amd")


def test_rpn_fpn_compile_refuse_without_gpu_and_equal_the_python_call(tmp_path):
    import torch

    import rpn_fpn_numpy as rf

    exe = str(tmp_path / "rpn_fpn_check")
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-pthread", "-I", os.path.join(ROOT, "include"), "-I", HOST,
                    os.path.join(ROOT, "tests", "cpp", "rpn_fpn_check.cpp"), "-L", LIBDIR, "-lifx", "-lz", "-ldl", f"-Wl,-rpath,{LIBDIR}", "-o", exe], check=True)
    shapes, pre, post, Fn = [(3, 56, 52), (3, 28, 26), (3, 7, 7)], 1000, 300, 800        # level 0 selects (8736 anchors), the others sort only
    thr, min_size = np.float32(0.5), np.float32(2.0)
    levels, img = fc.pyramid(60, shapes)
    fin, fout = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(fin, "wb") as f:
        f.write(np.asarray([len(shapes), pre, post, Fn, img[0], img[1]], np.int32).tobytes())
        f.write(np.asarray([thr, min_size], np.float32).tobytes())
        f.write(np.asarray(shapes, np.int32).tobytes())
        for lv in levels:
            for a in lv:
                f.write(a.tobytes())
    r = subprocess.run([exe, fin, fout], capture_output=True, text=True, check=True, cwd=str(tmp_path))
    lines = r.stdout.splitlines()
    if not torch.cuda.is_available():
        assert lines[0].startswith("refused: ifx_create") and "no HIP device" in lines[0], r.stdout
        return
    import instancefusion_amd as ifx

    ref = rf.rpn_proposals_fpn(levels, img, pre, post, thr, min_size, Fn)
    pb, pl, pv, pi, c, lc = rf.padded(ref, Fn)
    assert 0 < c < Fn and (lc > 0).all()
    assert lines[0] == f"wrote {c}", r.stdout
    assert lines[1].startswith("refused levels: ifx_rpn_proposals_fpn:") and "1 .. 8" in lines[1], r.stdout
    raw = open(fout, "rb").read()
    assert len(raw) == Fn * 32 + 4 + 4 * len(shapes)
    got_boxes = np.frombuffer(raw, np.uint32, Fn * 4).reshape(Fn, 4)
    got_logits = np.frombuffer(raw, np.uint32, Fn, Fn * 16)
    got_level = np.frombuffer(raw, np.int32, Fn, Fn * 20)
    got_index = np.frombuffer(raw, np.int64, Fn, Fn * 24)
    got_count = int(np.frombuffer(raw, np.int32, 1, Fn * 32)[0])
    got_lc = np.frombuffer(raw, np.int32, len(shapes), Fn * 32 + 4)
    assert got_count == c and np.array_equal(got_level, pv) and np.array_equal(got_index, pi) and np.array_equal(got_lc, lc)
    assert np.array_equal(got_boxes, pb.view(np.uint32)) and np.array_equal(got_logits, pl.view(np.uint32))
    ef = ifx.ElasticFusion(w=160, h=120, fx=132.0, fy=132.0, cx=80.0, cy=60.0, max_surfels=100000)       # the same bytes as the Python call
    d = [[torch.from_numpy(a).cuda() for a in lv] for lv in levels]
    b, s, v, i, n, k = ef.rpn_proposals_fpn([x[0] for x in d], [x[1] for x in d], [x[2] for x in d], img, pre, post, float(thr), float(min_size), Fn, padded=True)
    assert int(n.item()) == got_count and np.array_equal(b.cpu().numpy().view(np.uint32), got_boxes) and np.array_equal(i.cpu().numpy(), got_index)
    assert np.array_equal(v.cpu().numpy(), got_level) and np.array_equal(k.cpu().numpy(), got_lc)
    assert torch.equal(s, torch.sigmoid(torch.from_numpy(got_logits.view(np.float32).copy()).cuda()))
    ef.close()
