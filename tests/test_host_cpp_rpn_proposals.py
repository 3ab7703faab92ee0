"""C++ host layer: ElasticFusion::RpnProposals / BoxDecode compile against ifx_host.hpp with plain g++ -- no HIP header.  Without a GPU the map cannot be created and
the helper says so; with one, one call of each through the C++ class gives the bytes of the Python calls and of the statement (tests/rpn_proposals_numpy.py):
boxes, logits, indices, the padding behind the count, the count, every decoded box."""
import os
import subprocess

import numpy as np

import rpn_proposals_cases as rc
from conftest import ROOT

HOST = os.path.join(ROOT, "instancefusion_amd", "host")
LIBDIR = os.path.join(ROOT, "instancefusion_amd")


def test_rpn_proposals_compile_refuse_without_gpu_and_equal_the_python_calls(tmp_path):
    import torch

    import rpn_proposals_numpy as rp

    exe = str(tmp_path / "rpn_proposals_check")
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-pthread", "-I", os.path.join(ROOT, "include"), "-I", HOST,
                    os.path.join(ROOT, "tests", "cpp", "rpn_proposals_check.cpp"), "-L", LIBDIR, "-lifx", "-lz", "-ldl", f"-Wl,-rpath,{LIBDIR}", "-o", exe], check=True)
    A, H, W, pre, post, rows, k = 15, 30, 40, 1500, 2000, 37, 81
    thr, min_size, weights = np.float32(0.5), np.float32(2.0), np.asarray([10, 10, 5, 5], np.float32)
    obj, reg, anc, img = rc.level(50, A, H, W)
    rng = np.random.default_rng(51)
    c0 = rng.uniform(0, 400, (rows, 2))
    boxes = np.concatenate([c0, c0 + rng.uniform(2, 200, (rows, 2))], axis=1).astype(np.float32)
    codes = (rng.standard_normal((rows, k, 4)) * 0.7 * weights).reshape(rows, 4 * k).astype(np.float32)
    fin, fout = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(fin, "wb") as f:
        f.write(np.asarray([A, H, W, pre, post, img[0], img[1], rows, k], np.int32).tobytes())
        f.write(np.asarray([thr, min_size], np.float32).tobytes())
        f.write(weights.tobytes())
        for a in (obj, reg, anc, codes, boxes):
            f.write(a.tobytes())
    r = subprocess.run([exe, fin, fout], capture_output=True, text=True, check=True, cwd=str(tmp_path))
    lines = r.stdout.splitlines()
    if not torch.cuda.is_available():
        assert lines[0].startswith("refused: ifx_create") and "no HIP device" in lines[0], r.stdout
        return
    import instancefusion_amd as ifx

    ref = rp.rpn_proposals(obj, reg, anc, img, pre, post, thr, min_size)
    pb, pl, pi, c = rp.padded(ref, post)
    assert 0 < c < post
    assert lines[0] == f"wrote {c}", r.stdout
    assert lines[1].startswith("refused pre: ifx_rpn_proposals:") and "8192" in lines[1], r.stdout
    raw = open(fout, "rb").read()
    assert len(raw) == post * 28 + 4 + codes.size * 4
    got_boxes = np.frombuffer(raw, np.uint32, post * 4).reshape(post, 4)
    got_logits = np.frombuffer(raw, np.uint32, post, post * 16)
    got_index = np.frombuffer(raw, np.int64, post, post * 20)
    got_count = int(np.frombuffer(raw, np.int32, 1, post * 28)[0])
    got_dec = np.frombuffer(raw, np.uint32, codes.size, post * 28 + 4).reshape(codes.shape)
    assert got_count == c and np.array_equal(got_index, pi) and np.array_equal(got_boxes, pb.view(np.uint32)) and np.array_equal(got_logits, pl.view(np.uint32))
    assert np.array_equal(got_dec, rp.box_decode(codes, boxes, weights).view(np.uint32))
    ef = ifx.ElasticFusion(w=160, h=120, fx=132.0, fy=132.0, cx=80.0, cy=60.0, max_surfels=100000)       # the same bytes as the Python calls
    d = [torch.from_numpy(a).cuda() for a in (obj, reg, anc, codes, boxes)]
    b, s, i, n = ef.rpn_proposals(d[0], d[1], d[2], img, pre, post, float(thr), float(min_size), padded=True)
    dec = ef.box_decode(d[3], d[4], tuple(weights))
    assert int(n.item()) == got_count and np.array_equal(b.cpu().numpy().view(np.uint32), got_boxes) and np.array_equal(i.cpu().numpy(), got_index)
    assert torch.equal(s, torch.sigmoid(torch.from_numpy(got_logits.view(np.float32).copy()).cuda()))
    assert np.array_equal(dec.cpu().numpy().view(np.uint32), got_dec)
    ef.close()
