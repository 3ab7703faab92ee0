"""C++ hosts and the device forms of the sharded segmentation call: a small program (tests/cpp/owner_seg_device_check.cpp) compiles against ifx_host.hpp with plain
g++ -- no HIP header --, and at a world of one (n_ranks = -1, root = 0) drives the ROI form through begin, the exchange list and resume; its labels equal the
Python run's."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT, SMALL

HOST = os.path.join(ROOT, "instancefusion_amd", "host")
LIBDIR = os.path.join(ROOT, "instancefusion_amd")


def _build(tmp_path):
    exe = str(tmp_path / "owner_seg_device_check")
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-pthread", "-I", os.path.join(ROOT, "include"), "-I", HOST,
                    os.path.join(ROOT, "tests", "cpp", "owner_seg_device_check.cpp"), "-L", LIBDIR, "-lifx", "-lz", "-ldl", f"-Wl,-rpath,{LIBDIR}", "-o", exe], check=True)
    return exe


def test_owner_forms_compile_and_refuse_without_gpu(tmp_path):
    import torch

    r = subprocess.run([_build(tmp_path)], capture_output=True, text=True, check=True, cwd=str(tmp_path))
    assert r.stdout.splitlines()[0] == ("created" if torch.cuda.is_available() else "refused: no handle without a GPU"), r.stdout


@pytest.mark.gpu
def test_rois_form_from_cpp_equals_python(small_stream, tmp_path):
    import torch

    import instancefusion_amd as ifx
    import owner_seg_record_numpy as rec
    from instancefusion_amd import sharded
    from test_gpu_seg_rois import _roi_case

    ifx.lib()
    st = small_stream
    NF, AT = 6, 4
    W, H = SMALL["w"], SMALL["h"]
    d_rgb = torch.from_numpy(st["rgb"][:NF].copy()).cuda()
    d_dep = torch.from_numpy(st["depth"][:NF].view(np.int16).copy()).cuda()
    one = ifx.ElasticFusion(**SMALL, max_surfels=400000)
    for i in range(AT):
        one.enqueue_frame_device(d_rgb[i].data_ptr(), d_dep[i].data_ptr(), i)
    m = one.download()
    m["pc"][:, 3] = 20.0                      # every surfel stable: the id image is populated and the masks find surfels to vote for
    pose, tick = one.getCurrPose(), one.tick
    one.close()
    rois, boxes, cls, _ = _roi_case(st, NF - 1, np.random.default_rng(8))
    n, M = rois.shape[0], rois.shape[-1]
    # the Python run: the same calls in the same order
    ef = ifx.ElasticFusion(**SMALL, max_surfels=400000, n_ranks=-1, rank=0)
    for i in range(NF):
        if i == AT:
            ef.upload(m); ef.set_pose(pose, tick)
            sharded.emulate_owner_predict([ef])
        sharded.emulate_owner_ranks([ef], d_rgb[i].data_ptr(), d_dep[i].data_ptr())
    sharded.emulate_owner_segmentation_rois([ef], 0, st["rgb"][NF - 1], st["depth"][NF - 1], torch.from_numpy(rois).cuda(), torch.from_numpy(boxes).cuda(), cls, 100,
                                            superpixels=True, max_n=16)
    want = ifx.InstanceFusion(ef).labels()
    ef.close()
    assert (want >= 0).sum() > 30             # (a sanity floor of the scenario, not a parity figure)
    # the C++ run
    src, out = str(tmp_path / "in.bin"), str(tmp_path / "labels.bin")
    with open(src, "wb") as f:
        f.write(np.asarray([NF, W, H, n, M, AT, m["pc"].shape[0], tick], np.int32).tobytes())
        f.write(np.asarray([SMALL["fx"], SMALL["fy"], SMALL["cx"], SMALL["cy"]], np.float32).tobytes())
        f.write(np.ascontiguousarray(pose, np.float32).tobytes())
        for k in ("pc", "nr", "col", "tm", "ic", "votes"):
            f.write(np.ascontiguousarray(m[k], np.float32).tobytes())
        for i in range(NF):
            f.write(np.ascontiguousarray(st["rgb"][i], np.uint8).tobytes())
            f.write(np.ascontiguousarray(st["depth"][i], np.uint16).tobytes())
        f.write(np.ascontiguousarray(rois, np.float32).tobytes())
        f.write(np.ascontiguousarray(boxes, np.float32).tobytes())
        f.write(np.ascontiguousarray(cls, np.int32).tobytes())
    r = subprocess.run([_build(tmp_path), src, out], capture_output=True, text=True, cwd=str(tmp_path), timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.splitlines()
    assert lines[0] == f"record {4 * rec.record_words(2, 16, M, W * H)} op {4 | 0 << 8}", r.stdout
    assert lines[1] == "exchanges 3" and lines[2] == f"labels {want.shape[0]}", r.stdout       # the record, the boxes, the model depth
    assert np.array_equal(np.fromfile(out, np.int32), want)
