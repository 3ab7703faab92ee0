"""Owner lookup and lattice test of the view-list walk (instancefusion_amd/csrc/ifx_walk_owner.h, k_raster_view): a stand-alone host program under
AddressSanitizer + UBSan, no GPU (tests/cpp/walk_owner_check.cpp).  For area vectors of 64 lanes the table + max-scan + carry lookup is compared, for every
candidate g in [0, total), with a literal transcription of the two readlane loops it replaced and with the definition #{ j : incl[j] <= g }: all zero; a single
non-zero lane at 0 or 63; all ones; one area of 1, 63, 64, 65, 4096 and 512 x 512 alone and among ones; the largest mark (63 boxes of 512 x 512 in front); sums on 64
and 128 and one off them; empty runs across step boundaries; 6000 seeded random vectors.  The mark's first-candidate half is compared with excl[] at every candidate.
The unsigned lattice test is compared with % for every x in [0, 65535] and step in [1, 64]."""
import os
import subprocess

import pytest

from conftest import ROOT


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("walk_owner") / "walk_owner_check")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(ROOT, "instancefusion_amd", "csrc"), os.path.join(ROOT, "tests", "cpp", "walk_owner_check.cpp"), "-o", out], check=True)
    return out


def test_lookup_matches_the_two_loops_and_lattice_test_matches_modulo(exe):
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(r.stdout[-1500:])
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    last = r.stdout.strip().splitlines()[-1].split()
    assert last[-2:] == ["0", "bad"]
    assert int(last[0]) > 6000 and int(last[4]) == 64 * 65536


def test_the_cases_tell_a_wrong_carry(exe):
    """The check has teeth: with the first lane's owner (not the last lane's) carried out of a step, the program fails, and the cases with a box that reaches over
    a step boundary say so; 'all zero', 'all ones' and a single area of at most 64 cannot (no box crosses a boundary)."""
    r = subprocess.run([exe, "carry"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 1, (r.stdout[-2000:], r.stderr[-2000:])
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("wrong carry caught by:")][0]
    for name in ("one area among ones", "sum on a step boundary", "empty run across a boundary", "random"):
        assert "[" + name + "]" in line, line
    assert "[all zero]" not in line and "[all ones]" not in line
