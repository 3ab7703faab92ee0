"""C++ host layer: the default detector's methods (InstanceFusion::ProcessSegmentationUnmolded / ProcessSegmentationDeferredUnmolded / MoldedInputSize /
DetectorInputMolded, ElasticFusion::UnmoldDetections) compile against ifx_host.hpp with plain g++ -- no HIP header --, give the ctypes layer's sizes, and
refuse loudly where there is no GPU (as test_host_cpp_seg_rois.py)."""
import os
import subprocess

from conftest import ROOT

HOST = os.path.join(ROOT, "instancefusion_amd", "host")
LIBDIR = os.path.join(ROOT, "instancefusion_amd")


def test_unmolded_methods_compile_match_ctypes_and_refuse_without_gpu(tmp_path):
    import torch

    import instancefusion_amd as ifx

    exe = str(tmp_path / "seg_unmolded_check")
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-pthread", "-I", os.path.join(ROOT, "include"), "-I", HOST,
                    os.path.join(ROOT, "tests", "cpp", "seg_unmolded_check.cpp"), "-L", LIBDIR, "-lifx", "-lz", f"-Wl,-rpath,{LIBDIR}", "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, check=True, cwd=str(tmp_path))
    lines = r.stdout.splitlines()
    assert lines[0] == "size " + " ".join(str(v) for v in ifx.molded_input_size(640, 480, 800, 1024)) == "size 1024 768 1024 1024 128 0 896 1024", r.stdout
    assert lines[1].startswith("refused size: ifx_molded_input_size"), r.stdout
    if torch.cuda.is_available():
        assert lines[2] == "created 0", r.stdout
        assert lines[3].startswith("refused 65: ifx_process_segmentation_unmolded:") and "64" in lines[3], r.stdout
        assert lines[4].startswith("refused 257: ifx_process_segmentation_unmolded:") and "256" in lines[4], r.stdout
        assert lines[5].startswith("refused window: ifx_unmold_detections: ifx_unmold_detections:") and "window" in lines[5], r.stdout
        assert lines[6].startswith("refused input: ifx_detector_input_molded: ifx_detector_input_molded: NULL"), r.stdout
    else:
        assert lines[2].startswith("refused: InstanceFusion::ProcessSegmentationUnmolded") and "no CPU fallback" in lines[2], r.stdout
        assert lines[3].startswith("refused deferred: InstanceFusion::ProcessSegmentationDeferredUnmolded") and "no CPU fallback" in lines[3], r.stdout
        assert lines[4].startswith("refused input: InstanceFusion::DetectorInputMolded") and "no CPU fallback" in lines[4], r.stdout
