"""C++ host layer: ElasticFusion::FpnRoiAlign compiles against ifx_host.hpp with plain g++ -- no HIP header.  Without a GPU the map cannot be created and the helper
says so; with one, one call through the C++ class gives the statement's values (tests/fpn_pooler_numpy.py): every pooled bit and every level, and scales that are
no ladder come back as the library's refusal."""
import os
import subprocess

import numpy as np

from conftest import ROOT

HOST = os.path.join(ROOT, "instancefusion_amd", "host")
LIBDIR = os.path.join(ROOT, "instancefusion_amd")


def test_fpn_pooler_compiles_refuses_without_gpu_and_equals_the_statement(tmp_path):
    import torch

    import fpn_pooler_numpy as fp

    exe = str(tmp_path / "fpn_pooler_check")
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-pthread", "-I", os.path.join(ROOT, "include"), "-I", HOST,
                    os.path.join(ROOT, "tests", "cpp", "fpn_pooler_check.cpp"), "-L", LIBDIR, "-lifx", "-lz", "-ldl", f"-Wl,-rpath,{LIBDIR}", "-o", exe], check=True)
    rng = np.random.default_rng(23)
    B, Cn, n, ph, pw, ratio = 2, 70, 12, 7, 7, 2
    scales = [0.25, 0.125, 0.0625]
    sizes = [(24, 32), (12, 16), (6, 8)]
    feats = [rng.standard_normal((B, Cn, h, w)).astype(np.float32) for h, w in sizes]
    side = 2.0 ** rng.uniform(3, 10, n)
    x0, y0 = rng.uniform(-8, 100, n), rng.uniform(-8, 70, n)
    rois = np.stack([rng.integers(0, B, n).astype(np.float64), x0, y0, x0 + side, y0 + side * rng.uniform(0.7, 1.4, n)], axis=1).astype(np.float32)
    rois[3, 1:] = (30, 10, 10, 40)                          # a negative area: no level
    fin, fout = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(fin, "wb") as f:
        f.write(np.asarray([len(scales), B, Cn, n, ph, pw, ratio], np.int32).tobytes())
        for (h, w), s in zip(sizes, scales):
            f.write(np.asarray([h, w], np.int32).tobytes() + np.asarray([s], np.float32).tobytes())
        for a in feats + [rois]:
            f.write(a.tobytes())
    r = subprocess.run([exe, fin, fout], capture_output=True, text=True, check=True, cwd=str(tmp_path))
    lines = r.stdout.splitlines()
    if not torch.cuda.is_available():
        assert lines[0].startswith("refused: ifx_create") and "no HIP device" in lines[0], r.stdout
        return
    ref, lev = fp.fpn_roi_align(feats, rois, scales, ph, pw, ratio)
    assert set(lev.tolist()) == {-1, 0, 1, 2}
    assert lines[0] == f"wrote {ref.size}", r.stdout
    assert lines[1].startswith("refused scales: ifx_fpn_roi_align:") and "scales" in lines[1], r.stdout
    raw = open(fout, "rb").read()
    assert len(raw) == ref.size * 4 + n * 4
    got = np.frombuffer(raw, np.float32, ref.size).reshape(ref.shape)
    got_lev = np.frombuffer(raw, np.int32, n, ref.size * 4)
    assert np.array_equal(got_lev, lev)
    assert np.array_equal(got.view(np.uint32), ref.view(np.uint32))
