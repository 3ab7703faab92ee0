"""Grid arithmetic of the kNN search (instancefusion_amd/csrc/ifx_knn_grid.h): a stand-alone host program under AddressSanitizer + UBSan, no GPU.
knn_grid_side is monotone, within [2, 256], has side^3 <= max(8, 8 * count) and is 256 from 2^21 points on, for count in {0, 1, 2, 9, 10, 11, 4096, 2^21 - 1, 2^21,
INT_MAX} and a sweep; the row loop of the vote kernels yields exactly the new cells of a shell row, each once, and the shell walk visits every cell of a grid once."""
import os
import subprocess

from conftest import ROOT


def test_grid_side_and_shell_rows(tmp_path):
    exe = str(tmp_path / "knn_grid_check")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(ROOT, "instancefusion_amd", "csrc"), os.path.join(ROOT, "tests", "cpp", "knn_grid_check.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    assert r.stdout.strip().endswith(" 0 bad")
