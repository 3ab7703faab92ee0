"""C++ host layer: ElasticFusion::KerasProposals, PyramidRoiAlign and KerasDetections compile against ifx_host.hpp with plain g++ -- no HIP header.  Without a GPU
the map cannot be created and the helper says so; with one, the three calls through the C++ class and ifx_pyramid_level_thresholds give the bytes of the numpy
statement (tests/keras_layers_numpy.py): the helper prints a checksum of every output buffer, the padding behind the counts included, and one refused call reports
the library's message."""
import os
import subprocess

import numpy as np
import pytest

import keras_layers_gpu as kg
import keras_layers_numpy as kl
from conftest import ROOT

HOST = os.path.join(ROOT, "instancefusion_amd", "host")
LIBDIR = os.path.join(ROOT, "instancefusion_amd")
F = np.float32


def _fnv(a):
    h = 1469598103934665603
    for b in np.ascontiguousarray(a).tobytes():
        h = ((h ^ b) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
    return f"{h:016x}"


def _build(tmp_path):
    exe = str(tmp_path / "keras_layers_check")
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-pthread", "-I", os.path.join(ROOT, "include"), "-I", HOST,
                    os.path.join(ROOT, "tests", "cpp", "keras_layers_check.cpp"), "-L", LIBDIR, "-lifx", "-lz", "-ldl", f"-Wl,-rpath,{LIBDIR}", "-o", exe], check=True)
    return exe


def _inputs(tmp_path):
    n, pre, count, image, R, Cn, M, Cf, pool, nb = 3000, 1000, 120, (512, 512), 300, 9, 40, 4, 7, 50
    probs, bbox, anc = kg.proposal_case(70, n, image=512)
    rng = np.random.default_rng(71)
    side = np.exp(rng.uniform(np.log(0.03), np.log(0.6), (R, 2)))
    p = rng.uniform(0, 1, (R, 2)) * (1 - side)
    rois = np.concatenate([p, p + side], axis=1).astype(F)
    cprobs = (rng.random((R, Cn)) * 0.02).astype(F)
    cprobs[np.arange(R), rng.integers(0, Cn, R)] += F(0.8)
    deltas = (rng.standard_normal((R, Cn, 4)) * 0.5).astype(F)
    maps = [rng.standard_normal((1, s, s, Cf)).astype(F) for s in (16, 8, 4, 2)]
    bside = np.exp(rng.uniform(np.log(0.03), np.log(0.95), (nb, 2)))
    bp = rng.uniform(0, 1, (nb, 2)) * (1 - bside)
    boxes = np.concatenate([bp, bp + bside], axis=1).astype(F)
    window = (8, 16, 500, 480)
    thr = (0.7, 0.6, 0.3)
    fin = str(tmp_path / "in.bin")
    with open(fin, "wb") as f:
        f.write(np.asarray([n, pre, count, image[0], image[1], R, Cn, M, Cf, pool, nb, 1], np.int32).tobytes())
        f.write(np.asarray(thr, F).tobytes())
        f.write(np.asarray(window, F).tobytes())
        for a in (probs, bbox, anc, rois, cprobs, deltas, *maps, boxes):
            f.write(np.ascontiguousarray(a, F).tobytes())
    return fin, dict(n=n, pre=pre, count=count, image=image, M=M, pool=pool, window=window, thr=thr, probs=probs, bbox=bbox, anc=anc, rois=rois, cprobs=cprobs,
                     deltas=deltas, maps=maps, boxes=boxes)


def test_compiles_and_refuses_without_a_gpu(tmp_path):
    import torch

    exe = _build(tmp_path)
    if torch.cuda.is_available():
        return
    fin, _ = _inputs(tmp_path)
    r = subprocess.run([exe, fin], capture_output=True, text=True, check=True, cwd=str(tmp_path))
    assert r.stdout.startswith("refused: ifx_create") and "no HIP device" in r.stdout, r.stdout


@pytest.mark.gpu
def test_three_members_equal_the_statement(tmp_path):
    exe = _build(tmp_path)
    fin, c = _inputs(tmp_path)
    r = subprocess.run([exe, fin], capture_output=True, text=True, check=True, cwd=str(tmp_path), timeout=120)
    lines = r.stdout.splitlines()
    assert len(lines) == 5, r.stdout
    pb, pi, pc = kl.proposals_padded(kl.keras_proposals(c["probs"], c["bbox"], c["anc"], c["image"], c["pre"], c["count"], c["thr"][0]), c["count"])
    assert 0 < pc <= c["count"] and not np.isnan(pb).any()
    assert lines[0] == f"proposals {_fnv(pb)} index {_fnv(pi)} count {pc}", r.stdout
    pooled, lv = kl.pyramid_roi_align(c["maps"], c["boxes"][None], c["image"], (c["pool"], c["pool"]))
    assert len(set(lv[0].tolist())) >= 3
    assert lines[1] == f"pooled {_fnv(pooled)} levels {_fnv(lv.astype(np.int32))}", r.stdout
    pd, pn, px, dc = kl.detections_padded(kl.keras_detections(c["rois"], c["cprobs"], c["deltas"], c["window"], c["image"], c["thr"][1], c["thr"][2], c["M"]), c["M"])
    assert 0 < dc <= c["M"]
    assert lines[2] == f"detections {_fnv(pd)} norm {_fnv(pn)} index {_fnv(px)} count {dc}", r.stdout
    T = kl.level_thresholds(*c["image"]).view(np.uint32)
    assert lines[3] == "thresholds " + " ".join(f"{int(v):08x}" for v in T), r.stdout
    assert lines[4].startswith("refused count: ifx_keras_proposals:") and "8192" in lines[4], r.stdout
