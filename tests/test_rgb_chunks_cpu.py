"""Chunk arithmetic of the fused photometric step (instancefusion_amd/csrc/ifx_rgb_chunks.h): a stand-alone host program under AddressSanitizer + UBSan, no GPU.
Every index of [0, n) is covered exactly once and none is >= n, for n in {0, 1, 255, 256, 257, capacity - 1, capacity} and counts above the capacity."""
import os
import subprocess

from conftest import ROOT


def test_chunks_cover_the_list_exactly_once(tmp_path):
    exe = str(tmp_path / "rgb_chunks_check")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(ROOT, "instancefusion_amd", "csrc"), os.path.join(ROOT, "tests", "cpp", "rgb_chunks_check.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    assert r.stdout.strip().endswith(" 0 bad")
