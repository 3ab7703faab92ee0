"""What the mask rule of the compare map (option compare_map 2: mask IoU over 3 x 3-dilated pixel sets, the reference's compareMapType 2) costs next to the box
rule, on the bench workload (640x480 frame, 5 M-surfel synthetic map): the frame's canned masks, and R = 100 masks (80 rectangles of a 10 x 8 grid and 20 repeats
that the overlap clean empties, so that the table does not overflow).  Per mask set the two rules take turns in one process; per call the stream time (the call's
HIP-event span, option stage_timing) and the host-return time (entry to return, behind the call's own synchronisation), once with the superpixel stages (flags 2,
as the bench calls it) and once without (flags 0: the rule's own difference is easier to read where the superpixels do not dominate the call).  Calls that met an eviction are left out
(told by the table's occupancy dropping).  Then the new kernels' own times (option kernel_timing).  A library without the option (the parent commit's, for the
A/B of rule 1) reports rule 1 alone.  One line of JSON at the end.

    python tools/compare_map_cost.py [surfels] [calls per point]"""
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402,F401  (first: libifx.so binds to the HIP runtime torch ships)
import numpy as np  # noqa: E402

import instancefusion_amd as ifx  # noqa: E402
from instancefusion_amd import synth  # noqa: E402

n = int(sys.argv[1]) if len(sys.argv) > 1 else 5_000_000
calls = int(sys.argv[2]) if len(sys.argv) > 2 else 30
W, H = 640, 480
K = dict(fx=528.0, fy=528.0, cx=320.0, cy=240.0)
st = synth.make_stream(40, W, H, noise=True, loop_len=90, **K)
m = synth.make_map(n, st["scene"], st["poses_world"][0], 1000)


def grid_masks():
    out = np.zeros((100, H, W), np.uint8)
    for k in range(100):
        c = k % 80
        x0, y0 = (c % 10) * 64 + 4, (c // 10) * 60 + 4
        out[k, y0:y0 + 52, x0:x0 + 56] = 255
    return out, (1 + np.arange(100) % 80).astype(np.int32)


def run(masks, cls, label, result):
    ef = ifx.ElasticFusion(w=W, h=H, max_surfels=n + 1_500_000, **K)
    ef.processFrame(st["rgb"][0], st["depth"][0]); ef.upload(m); ef.set_pose(st["poses"][0], 1000); ef.combined_predict(st["poses"][0], 1000, 1000)
    for i in range(1, 11):
        ef.processFrame(st["rgb"][i], st["depth"][i])
    ef.sync()
    inst = ifx.InstanceFusion(ef)
    L = ef.L
    rules = [1]
    try:
        ef.set_option("compare_map", 2)
        ef.set_option("compare_map", 1)
        rules.append(2)
    except ifx.IfxError:
        pass
    nm = masks.shape[0]
    h_masks, h_cls = np.ascontiguousarray(masks), np.ascontiguousarray(cls.astype(np.int32))
    frame = [500]

    def call(rule, flags=2):
        if len(rules) > 1:
            ef.set_option("compare_map", rule)
        frame[0] += 3
        t0 = time.perf_counter()
        r = L.ifx_process_segmentation(ef.handle, None, None, h_masks.ctypes.data_as(C.c_void_p), h_cls.ctypes.data_as(C.c_void_p), nm, frame[0], flags)
        dt = (time.perf_counter() - t0) * 1e6
        assert r == 0, L.ifx_last_error(ef.handle)
        return dt

    for r in rules * 4:   # warm-up: allocations, first launches, the registrations
        call(r); call(r, 0)
    ef.set_option("stage_timing", 1)
    print(f"compare_map_cost [{label}]: {W}x{H}, {n} surfels, {nm} masks, host entry on the resident frame; {calls} calls per point, the rules taking turns")
    for flags, fl in ((2, "superpixels"), (0, "plain")):
        wall, span, ev = {r: [] for r in rules}, {r: [] for r in rules}, {r: [] for r in rules}
        used = int((inst.getInstanceTable() >= 0).sum())
        for k in range(calls):
            for r in (rules if k % 2 == 0 else rules[::-1]):
                ef.stage_ms(reset=True)
                dt = call(r, flags)
                s = ef.stage_ms()["instance"] * 1e3
                now = int((inst.getInstanceTable() >= 0).sum())
                if now >= used:
                    wall[r].append(dt); span[r].append(s)
                else:
                    ev[r].append(s)
                used = now
        for r in rules:
            if ev[r]:   # (a call whose table overflowed: the eviction, the host-driven tail and a full label scan)
                print(f"  {fl:11s} rule {r} stream, the {len(ev[r])} calls that met an eviction: median {np.median(ev[r]):7.1f} us")
                result[f"{label}_{fl}_rule{r}_evicting_stream_us"] = [round(float(np.median(ev[r])), 1), len(ev[r])]
            for name, a in (("stream", np.asarray(span[r])), ("host return", np.asarray(wall[r]))):
                if len(a) == 0:
                    print(f"  {fl:11s} rule {r} {name:11s}: every call met an eviction")
                    continue
                print(f"  {fl:11s} rule {r} {name:11s} ({len(a)} calls without eviction): median {np.median(a):7.1f} us  p10 {np.percentile(a, 10):7.1f}  "
                      f"p90 {np.percentile(a, 90):7.1f}  min {a.min():7.1f}  max {a.max():7.1f}")
                result[f"{label}_{fl}_rule{r}_{name.replace(' ', '_')}_us"] = [round(float(np.median(a)), 1), round(float(np.percentile(a, 10)), 1), round(float(np.percentile(a, 90)), 1)]
    ef.set_option("stage_timing", 0)
    ef.set_option("kernel_timing", 1)
    names = ("project_bbox_inst", "project_bbox_pres", "project_bbox_mask", "cmp_count", "seg_compare", "seg_compare_iou")
    for r in rules:
        ef.kernel_ms("__reset__")
        for _ in range(10):
            call(r)
        ef.sync()
        ks = {k_: ef.kernel_ms(k_) for k_ in names}
        print(f"  rule {r} kernels (HIP events, option kernel_timing): " + "  ".join(f"{k_} {avg * 1e3:.1f} us x {c}" for k_, (avg, c) in ks.items() if c))
        for k_, (avg, c) in ks.items():
            if c:
                result[f"{label}_rule{r}_{k_}_us"] = round(avg * 1e3, 1)
    ef.set_option("kernel_timing", 0)
    if len(rules) > 1:
        best, target = inst.segmentation_matches()
        print(f"  rule 2, last call: {int((best > 0).sum())} of {nm} masks matched, {int((target >= 0).sum())} voted")
    ef.close()


res = {"surfels": n, "calls": calls, "lib": os.path.basename(os.path.dirname(os.path.dirname(ifx.LIB_PATH)))}
bm, bc = synth.canned_masks(st["obj"][10], st["scene"])
run(bm, bc, "bench", res)
gm, gc = grid_masks()
run(gm, gc, "R100", res)
print(json.dumps(res))
