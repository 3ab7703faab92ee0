"""C++ host layer: InstanceFusion::setCompareMapType / getCompareMapType / maskCompareMap / segmentationMatches compile against ifx_host.hpp with plain g++ -- no
HIP header -- refuse loudly where there is no GPU, and on one reproduce the X scene of tests/test_gpu_compare_map.py: under the box rule both masks match
instance 3, under the mask rule "\\" matches 2 and "/" matches 3."""
import os
import subprocess

import pytest

from conftest import ROOT

HOST = os.path.join(ROOT, "instancefusion_amd", "host")
LIBDIR = os.path.join(ROOT, "instancefusion_amd")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("compare_map") / "compare_map_check")
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-pthread", "-I", os.path.join(ROOT, "include"), "-I", HOST,
                    os.path.join(ROOT, "tests", "cpp", "compare_map_check.cpp"), "-L", LIBDIR, "-lifx", "-lz", f"-Wl,-rpath,{LIBDIR}", "-o", out], check=True)
    return out


def test_compare_map_type_compiles_and_refuses_without_gpu(exe, tmp_path):
    import torch

    if torch.cuda.is_available():
        return                                              # (the GPU test below runs it)
    r = subprocess.run([exe, "2"], capture_output=True, text=True, check=True, cwd=str(tmp_path))
    assert r.stdout.startswith("refused: ") and "no CPU fallback" in r.stdout, r.stdout


@pytest.mark.gpu
@pytest.mark.parametrize("rule, best", [(1, "3 3"), (2, "2 3")])
def test_cpp_reproduces_the_x_scene(exe, tmp_path, rule, best):
    r = subprocess.run([exe, str(rule)], capture_output=True, text=True, cwd=str(tmp_path))
    assert r.returncode == 0, (r.stdout, r.stderr[-2000:])
    assert r.stdout.splitlines() == [f"type {rule}", f"best {best}", f"target {best}", "stage 2 3"], r.stdout
