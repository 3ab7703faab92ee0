"""C++ host layer: InstanceFusion::DetectorInputSize / DetectorInput compile against ifx_host.hpp with plain g++ -- no HIP header.  The size call works anywhere;
without a GPU DetectorInput refuses loudly (as test_host_cpp_seg_rois.py); with one, the C++ method writes the bytes the Python call writes for the same two
frames, which are the statement's (tests/detector_input_numpy.py)."""
import os
import subprocess

import numpy as np

from conftest import ROOT

HOST = os.path.join(ROOT, "instancefusion_amd", "host")
LIBDIR = os.path.join(ROOT, "instancefusion_amd")
W, H = 160, 120
K = dict(fx=132.0, fy=132.0, cx=80.0, cy=60.0)


def test_detector_input_compiles_refuses_without_gpu_and_equals_python(tmp_path):
    import torch

    import detector_input_numpy as dn
    from instancefusion_amd import synth

    exe = str(tmp_path / "detector_input_check")
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-pthread", "-I", os.path.join(ROOT, "include"), "-I", HOST,
                    os.path.join(ROOT, "tests", "cpp", "detector_input_check.cpp"), "-L", LIBDIR, "-lifx", "-lz", "-ldl", f"-Wl,-rpath,{LIBDIR}", "-o", exe], check=True)
    st = synth.make_stream(2, W, H, noise=True, **K)
    frames, out = str(tmp_path / "frames.bin"), str(tmp_path / "out.bin")
    with open(frames, "wb") as f:
        for i in range(2):
            f.write(st["rgb"][i].tobytes()); f.write(st["depth"][i].tobytes())
    r = subprocess.run([exe, frames, out], capture_output=True, text=True, check=True, cwd=str(tmp_path))
    lines = r.stdout.splitlines()
    assert lines[0] == "size 133 100 160 128", r.stdout
    if not torch.cuda.is_available():
        assert lines[1].startswith("refused: InstanceFusion::DetectorInput") and "no CPU fallback" in lines[1], r.stdout
        return
    assert lines[1] == f"wrote {3 * 128 * 160}", r.stdout
    assert lines[2].startswith("refused std: ifx_detector_input:") and "std" in lines[2], r.stdout
    got = np.fromfile(out, np.float32).reshape(1, 3, 128, 160)
    import instancefusion_amd as ifx

    e = ifx.ElasticFusion(w=W, h=H, max_surfels=200000, **K)
    inst = ifx.InstanceFusion(e)
    for i in range(2):
        e.processFrame(st["rgb"][i], st["depth"][i])
    t, (oh, ow) = inst.detector_input(min_size=100, size_divisible=32, to_bgr255=True, swap_rb=True)
    torch.cuda.synchronize()
    py = t.cpu().numpy()
    e.close()
    ref, size = dn.detector_input(st["rgb"][1], min_size=100, size_divisible=32, to_bgr255=True, swap_rb=True)
    assert (oh, ow) == size == (100, 133)
    assert np.array_equal(py.view(np.uint32), ref.view(np.uint32))
    assert np.array_equal(got.view(np.uint32), py.view(np.uint32))
