"""What option "id_rule" = 1 costs on the bench workload (640x480 stream into a 5 M-surfel synthetic map, as tools/ktimes.py): frames/s over a 20-frame
window and the per-kernel HIP-event times (option kernel_timing) of the launches that draw the id image, for id_rule 0 and 1.

    python tools/id_rule_cost.py [surfels] [frames]"""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: F401,E402  (first: libifx.so binds to the HIP runtime torch ships)

import instancefusion_amd as ifx  # noqa: E402
from instancefusion_amd import synth  # noqa: E402

n = int(sys.argv[1]) if len(sys.argv) > 1 else 5_000_000
frames = int(sys.argv[2]) if len(sys.argv) > 2 else 20
W, H = 640, 480
K = dict(fx=528.0, fy=528.0, cx=320.0, cy=240.0)
st = synth.make_stream(40, W, H, noise=True, loop_len=90, **K)
m = synth.make_map(n, st["scene"], st["poses_world"][0], 1000)
NAMES = ("raster_view", "clean_raster_view", "splat_resolve", "raster_finish", "raster_quad", "raster_view_ids", "ids_raster_quad", "ids_resolve")


def run(rule):
    ef = ifx.ElasticFusion(w=W, h=H, max_surfels=n + 1_500_000, **K)
    ef.processFrame(st["rgb"][0], st["depth"][0]); ef.upload(m); ef.set_pose(st["poses"][0], 1000); ef.combined_predict(st["poses"][0], 1000, 1000)
    ef.set_option("id_rule", rule)
    for i in range(1, 11):
        ef.processFrame(st["rgb"][i], st["depth"][i])
    ef.sync()
    t0 = time.perf_counter()
    for i in range(11, 11 + frames):
        ef.processFrame(st["rgb"][i % 40], st["depth"][i % 40])
    ef.sync()
    fps = frames / (time.perf_counter() - t0)
    ef.set_option("kernel_timing", 1); ef.kernel_ms("__reset__")
    for i in range(11 + frames, 11 + 2 * frames):
        ef.processFrame(st["rgb"][i % 40], st["depth"][i % 40])
    ef.sync()
    k = {nm: ef.kernel_ms(nm) for nm in NAMES}
    ef.set_option("kernel_timing", 0)
    t0 = time.perf_counter()
    ids = ef.image("ids_after")      # the on-demand completion of the lazy lattice (a segmentation call's first step)
    ens_ms = (time.perf_counter() - t0) * 1e3
    ef.close()
    return fps, k, ens_ms, int((ids > 0).sum())


for rule in (0, 1, 0, 1):
    fps, k, ens_ms, drawn = run(rule)
    print(f"id_rule {rule}: {fps:.1f} frames/s over {frames} frames ({n} surfels, {W}x{H}); whole id image on demand + download {ens_ms:.2f} ms, {drawn} pixels drawn")
    for nm, (avg, cnt) in k.items():
        if cnt:
            print(f"    {nm:20s} {avg * 1e3:8.1f} us x {cnt}")
