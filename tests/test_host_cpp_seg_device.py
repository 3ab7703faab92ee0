"""C++ host layer: InstanceFusion::ProcessSegmentationDevice (masks already on the device) compiles against ifx_host.hpp with plain g++ -- no HIP header -- and
refuses loudly where there is no GPU (as test_host_cpp.py's class-surface check)."""
import os
import subprocess

from conftest import ROOT

HOST = os.path.join(ROOT, "instancefusion_amd", "host")
LIBDIR = os.path.join(ROOT, "instancefusion_amd")


def test_process_segmentation_device_compiles_and_refuses_without_gpu(tmp_path):
    import torch

    exe = str(tmp_path / "seg_device_check")
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-pthread", "-I", os.path.join(ROOT, "include"), "-I", HOST,
                    os.path.join(ROOT, "tests", "cpp", "seg_device_check.cpp"), "-L", LIBDIR, "-lifx", "-lz", f"-Wl,-rpath,{LIBDIR}", "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, check=True, cwd=str(tmp_path))
    if torch.cuda.is_available():
        lines = r.stdout.splitlines()
        assert lines[0] == "created", r.stdout
        assert lines[1].startswith("refused 257: ifx_process_segmentation_device:") and "256" in lines[1], r.stdout
    else:
        assert r.stdout.startswith("refused: InstanceFusion::ProcessSegmentationDevice") and "no CPU fallback" in r.stdout, r.stdout
