"""What the kNN colour smoothing costs on dense maps: python tools/knn_grid_cost.py [calls] [synthetic surfels]   (IFX_LIB = another build of the library to compare with)

Two maps: the one ten frames of the 320x240 stream build (a pipeline map), and synth.make_map with 1 M surfels.  Per map: the HIP-event average of knn_vote and of the
other launches of a call (ifx_kernel_ms), and the host clock around whole calls (each ends in a stream synchronise).  One line of JSON per map; a checksum of the
colours after the calls, so that two builds can be seen to compute the same."""
import json
import os
import sys
import time
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch  # noqa: F401  (first, so that libifx.so binds to the HIP runtime torch ships)

import instancefusion_amd as ifx
from instancefusion_amd import synth

calls = int(sys.argv[1]) if len(sys.argv) > 1 else 20
n_synth = int(sys.argv[2]) if len(sys.argv) > 2 else 1_000_000
W, H = 320, 240
K = dict(fx=264.0, fy=264.0, cx=160.0, cy=120.0)
KERNELS = ("knn_vote", "knn_bounds", "knn_grid", "knn_count", "knn_scatter")


def labelled(m):
    """labels for a third of the surfels (ids 0 .. 5), planted through the vote store, so that the vote has something to write"""
    n = m["pc"].shape[0]
    rng = np.random.RandomState(2)
    lab = rng.randint(0, 6, n)
    votes = np.zeros((n, 48), np.float32)
    pick = np.nonzero(rng.rand(n) < 0.33)[0]
    votes[pick, lab[pick] // 2] = np.where(lab[pick] % 2 == 0, np.float32(7 << 16), np.float32(7))
    m["votes"] = votes
    return m


def measure(what, g, st):
    inst = ifx.InstanceFusion(g)
    inst.ProcessSegmentation(st["rgb"][0], st["depth"][0], np.zeros((1, H, W), np.uint8), np.array([1], np.int32), 0)   # the label scan
    for _ in range(3):
        inst.flannKnnVoteSurfelMap()
    g.set_option("kernel_timing", 1); g.kernel_ms("__reset__")
    t0 = time.perf_counter()
    for _ in range(calls):
        inst.flannKnnVoteSurfelMap()
    wall = (time.perf_counter() - t0) / calls * 1e3
    ms = {k: round(g.kernel_ms(k)[0], 5) for k in KERNELS}
    g.set_option("kernel_timing", 0)
    col = g.download(("col",))["col"]
    print(json.dumps(dict(map=what, surfels=int(g.count), calls=calls, lib=os.path.relpath(ifx.LIB_PATH, ROOT), kernel_ms=ms, call_wall_ms=round(wall, 4),
                          colours_crc=zlib.crc32(col.tobytes()), recoloured=int((col[:, 1] != 7434609).sum()))), flush=True)


st = synth.make_stream(10, W, H, noise=True, **K)
g = ifx.ElasticFusion(w=W, h=H, max_surfels=400000, **K)
for i in range(10):
    g.processFrame(st["rgb"][i], st["depth"][i])
g.upload(labelled(g.download()))
measure("pipeline_320x240", g, st)
g.close()

m = labelled(synth.make_map(n_synth, st["scene"], st["poses_world"][0], 10))
g = ifx.ElasticFusion(w=W, h=H, max_surfels=n_synth + 100, **K)
g.processFrame(st["rgb"][0], np.zeros_like(st["depth"][0]))
g.upload(m)
measure("synthetic", g, st)
g.close()
