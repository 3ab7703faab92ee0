"""Own-records form of the fused photometric step (instancefusion_amd/csrc/ifx_rgb_own.h, option rgb_own): a stand-alone host program under AddressSanitizer +
UBSan, no GPU.  The static shares cover [0, n) exactly once for every n in 0 .. 3 * G * 256 + 3, G in {1, 2, 3, 32, 33, 64, 1024}, and for counts above the
capacity; a model of the take-over protocol -- a block that stops waiting hands its share to the last arriver -- is run through every interleaving of two and
three blocks (tests/cpp/rgb_own_check.cpp)."""
import os
import subprocess

from conftest import ROOT


def test_shares_cover_the_list_and_no_interleaving_loses_a_share(tmp_path):
    exe = str(tmp_path / "rgb_own_check")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(ROOT, "instancefusion_amd", "csrc"), os.path.join(ROOT, "tests", "cpp", "rgb_own_check.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(r.stdout[-1500:])
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    assert r.stdout.strip().endswith(" 0 bad")
    assert r.stdout.count("0 with a share lost") == 4
