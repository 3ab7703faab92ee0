"""C++ host layer: InstanceFusion::checkLoopClosure / mergeInstances / findDuplicateInstances / resolveMergePairs compile against ifx_host.hpp with plain g++ -- no
HIP header -- and refuse loudly where there is no GPU; on one, checkLoopClosure on a table with a chain leaves the votes, colours and table that the Python call
leaves on the same map, and column 4 reset; `ifx_replay --merge-duplicates` runs a short log to its end."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT, SMALL

HOST = os.path.join(ROOT, "instancefusion_amd", "host")
LIBDIR = os.path.join(ROOT, "instancefusion_amd")
REPLAY = os.path.join(LIBDIR, "ifx_replay")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("instance_merge") / "instance_merge_check")
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-pthread", "-I", os.path.join(ROOT, "include"), "-I", HOST,
                    os.path.join(ROOT, "tests", "cpp", "instance_merge_check.cpp"), "-L", LIBDIR, "-lifx", "-lz", f"-Wl,-rpath,{LIBDIR}", "-o", out], check=True)
    return out


def test_merge_wrappers_compile_and_refuse_without_gpu(exe, tmp_path):
    import torch

    if torch.cuda.is_available():
        return                                              # (the GPU test below runs it)
    r = subprocess.run([exe, str(tmp_path / "m.bin")], capture_output=True, text=True, check=True, cwd=str(tmp_path))
    assert r.stdout.startswith("refused: ") and "no CPU fallback" in r.stdout, r.stdout


def test_replay_knows_the_switch():
    r = subprocess.run([REPLAY, "--help"], capture_output=True, text=True)
    assert r.returncode == 0 and "--merge-duplicates" in r.stderr
    r = subprocess.run([REPLAY, "x.klg", "--merge-duplicates", "--shard-ranks", "-1"], capture_output=True, text=True)
    assert r.returncode == 2 and "sharded" in r.stderr


@pytest.mark.gpu
def test_check_loop_closure_equals_the_python_call(exe, tmp_path):
    import instancefusion_amd as ifx
    import instance_merge_numpy as im
    from test_gpu_instance_merge import NI, Sheet, cls_of, raw

    path = str(tmp_path / "m.bin")
    r = subprocess.run([exe, path], capture_output=True, text=True, cwd=str(tmp_path))
    assert r.returncode == 0, (r.stdout, r.stderr[-2000:])
    lines = r.stdout.splitlines()
    blob = np.fromfile(path, np.uint32)
    n = int(blob[0])
    assert lines[0] == f"n {n} {n}" and lines[1] == "column4 reset" and lines[2].startswith("duplicates"), r.stdout
    sizes = [n * 48, n * 2, n * 2, n * 48, n * 2, NI]
    v0, c0, t0, v1, c1, table1 = np.split(blob[1:], np.cumsum(sizes)[:-1])
    v0, c0, t0, v1, c1 = v0.reshape(n, 48), c0.reshape(n, 2), t0.reshape(n, 2), v1.reshape(n, 48), c1.reshape(n, 2)
    assert (v0 != v1).any(axis=1).sum() > n // 2            # the merge did something
    ifx.lib()
    s = Sheet(ifx, [cls_of(i) for i in range(8)])
    base = s.g.download()
    idx = np.arange(n) % base["pc"].shape[0]
    m = {k: base[k][idx].copy() for k in base}
    m["votes"], m["col"], m["tm"] = v0.view(np.float32), c0.view(np.float32), t0.view(np.float32)
    s.g.upload(m)
    table = s.inst.getLoopClosureInstanceTable()
    table[5, 4], table[3, 4], table[6, 4] = 3, 1, 0
    done = s.inst.check_loop_closure(table)
    assert done.tolist() == [[3, 1], [5, 1], [6, 0]] and np.array_equal(table[:, 4], np.arange(NI))
    after = raw(s.g)
    assert np.array_equal(im.bits(after["votes"]), v1) and np.array_equal(im.bits(after["col"]), c1)
    assert np.array_equal(s.inst.getInstanceTable(), table1.view(np.int32))
    e_votes, _, e_col, e_table = im.merge(v0.view(np.float32), t0.view(np.float32), c0.view(np.float32)[:, 1], [cls_of(i) if i < 8 else -1 for i in range(NI)], s.inst_colour, done)
    assert np.array_equal(im.bits(e_votes), v1) and np.array_equal(im.bits(e_col), c1[:, 1]) and np.array_equal(e_table, table1.view(np.int32))
    s.close()


@pytest.mark.gpu
def test_replay_with_merge_duplicates_runs_to_the_end(small_stream, tmp_path):
    from instancefusion_amd import logio, synth

    st, n = small_stream, 10
    klg = str(tmp_path / "s.klg")
    wr = logio.RawLogWriter(klg, depth="zlib", image="raw")
    for i in range(n + 1):
        wr.add(33333 * i, st["rgb"][min(i, 9)], st["depth"][min(i, 9)])
    wr.close()
    mdir = tmp_path / "masks"
    mdir.mkdir()
    for i in range(n):
        mk, cl = synth.canned_masks(st["obj"][min(i, 9)], st["scene"])
        np.savez(mdir / f"{i:06d}.npz", masks=mk, class_ids=cl)
    args = ["--width", str(SMALL["w"]), "--height", str(SMALL["h"]), "--fx", str(SMALL["fx"]), "--fy", str(SMALL["fy"]), "--cx", str(SMALL["cx"]), "--cy", str(SMALL["cy"]),
            "--max-surfels", "400000", "--masks", str(mdir), "--confidence", "2", "--out", str(tmp_path / "C"), "--merge-duplicates"]
    r = subprocess.run([REPLAY, klg] + args, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    assert f"{n} frames" in r.stdout and "duplicate instances merged" in r.stderr
