"""C++ host layer: ElasticFusion::MaskHeadSelect and InstanceFusion::ProcessSegmentationDetections compile against ifx_host.hpp with plain g++ -- no HIP header.
Without a GPU the map cannot be created and the call refuses loudly; with one, MaskHeadSelect through the C++ class gives the bytes of the Python call and of the
statement (tests/mask_head_numpy.py), ProcessSegmentationDetections returns the kept count the Python call returns, and one refused call reports the library's
message."""
import os
import subprocess

import numpy as np

import mask_head_cases as mc
from conftest import ROOT

HOST = os.path.join(ROOT, "instancefusion_amd", "host")
LIBDIR = os.path.join(ROOT, "instancefusion_amd")


def test_mask_head_compiles_refuses_without_gpu_and_equals_the_python_call(tmp_path):
    import torch

    import mask_head_numpy as mh

    exe = str(tmp_path / "mask_head_check")
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-pthread", "-I", os.path.join(ROOT, "include"), "-I", HOST,
                    os.path.join(ROOT, "tests", "cpp", "mask_head_check.cpp"), "-L", LIBDIR, "-lifx", "-lz", "-ldl", f"-Wl,-rpath,{LIBDIR}", "-o", exe], check=True)
    R, Cn, M = 40, 5, 14
    c = mc.head(70, R, Cn, M)
    c["out_size"] = (160, 120)
    c["class_map"] = (50 + 3 * np.arange(Cn)).astype(np.int32)
    fin, fout = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(fin, "wb") as f:
        f.write(np.asarray([R, Cn, M, *c["in_size"], *c["out_size"], 1, 1], np.int32).tobytes())
        f.write(np.asarray([c["score_thresh"]], np.float32).tobytes())
        for k in ("logits", "boxes", "scores", "labels", "class_map"):
            f.write(c[k].tobytes())
    r = subprocess.run([exe, fin, fout], capture_output=True, text=True, check=True, cwd=str(tmp_path))
    lines = r.stdout.splitlines()
    if not torch.cuda.is_available():
        assert lines[0].startswith("refused: InstanceFusion::ProcessSegmentationDetections") and "no CPU fallback" in lines[0], r.stdout
        return
    import instancefusion_amd as ifx

    pm, pb, pc, pr, k = mh.padded(mh.mask_head_select(**c), R)
    assert 3 < k[0] < R
    assert lines[0] == f"wrote {k[0]}", r.stdout
    assert lines[1] == f"detections kept {k[0]}", r.stdout
    assert lines[2].startswith("refused 65: ifx_process_segmentation_detections:") and "64" in lines[2], r.stdout
    raw = open(fout, "rb").read()
    assert len(raw) == R * M * M * 4 + R * 16 + R * 8 + 4
    got_m = np.frombuffer(raw, np.uint32, R * M * M).reshape(R, M, M)
    got_b = np.frombuffer(raw, np.uint32, R * 4, R * M * M * 4).reshape(R, 4)
    got_c = np.frombuffer(raw, np.int32, R, R * M * M * 4 + R * 16)
    got_r = np.frombuffer(raw, np.int32, R, R * M * M * 4 + R * 20)
    got_k = np.frombuffer(raw, np.int32, 1, R * M * M * 4 + R * 24)
    assert np.array_equal(got_m, pm.view(np.uint32)) and np.array_equal(got_b, pb.view(np.uint32))
    assert np.array_equal(got_c, pc) and np.array_equal(got_r, pr) and got_k[0] == k[0]
    ef = ifx.ElasticFusion(w=160, h=120, fx=132.0, fy=132.0, cx=80.0, cy=60.0, max_surfels=100000)       # the same bytes and the same count as the Python calls
    d = {n: torch.from_numpy(c[n]).cuda() for n in ("logits", "boxes", "scores", "labels", "class_map")}
    m, b, cl, rw, kk = ef.mask_head_select(d["logits"], d["boxes"], d["scores"], d["labels"], c["in_size"], c["out_size"], c["score_thresh"], True,
                                           class_map=d["class_map"], padded=True)
    assert int(kk.item()) == k[0] and np.array_equal(m.cpu().numpy().view(np.uint32), got_m) and np.array_equal(b.cpu().numpy().view(np.uint32), got_b)
    assert np.array_equal(cl.cpu().numpy(), got_c) and np.array_equal(rw.cpu().numpy(), got_r)
    kept = ifx.InstanceFusion(ef).process_segmentation_detections(d["logits"], d["boxes"], d["scores"], d["labels"], c["in_size"], 100, c["score_thresh"],
                                                                  class_map=d["class_map"])
    assert kept == k[0]
    ef.close()
