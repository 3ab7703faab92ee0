"""C++ host layer: InstanceFusion::ProcessSegmentationRois / ProcessSegmentationDeferredRois (the mask head's ROI masks and boxes) compile against ifx_host.hpp
with plain g++ -- no HIP header -- and refuse loudly where there is no GPU (as test_host_cpp_seg_device.py)."""
import os
import subprocess

from conftest import ROOT

HOST = os.path.join(ROOT, "instancefusion_amd", "host")
LIBDIR = os.path.join(ROOT, "instancefusion_amd")


def test_process_segmentation_rois_compiles_and_refuses_without_gpu(tmp_path):
    import torch

    exe = str(tmp_path / "seg_rois_check")
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-pthread", "-I", os.path.join(ROOT, "include"), "-I", HOST,
                    os.path.join(ROOT, "tests", "cpp", "seg_rois_check.cpp"), "-L", LIBDIR, "-lifx", "-lz", f"-Wl,-rpath,{LIBDIR}", "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, check=True, cwd=str(tmp_path))
    lines = r.stdout.splitlines()
    if torch.cuda.is_available():
        assert lines[0] == "created", r.stdout
        assert lines[1].startswith("refused 65: ifx_process_segmentation_rois:") and "64" in lines[1], r.stdout
        assert lines[2].startswith("refused 257: ifx_process_segmentation_rois:") and "256" in lines[2], r.stdout
    else:
        assert lines[0].startswith("refused: InstanceFusion::ProcessSegmentationRois") and "no CPU fallback" in lines[0], r.stdout
        assert lines[1].startswith("refused deferred: InstanceFusion::ProcessSegmentationDeferredRois") and "no CPU fallback" in lines[1], r.stdout
