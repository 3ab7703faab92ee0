"""What a segmentation call costs when the masks are already on the GPU (ifx_process_segmentation_device) against the host entry, on the bench workload
(640x480 frame, 5 M-surfel synthetic map, the frame's 8 canned masks): wall time per call -- from entry to the return behind the call's own synchronisation --
for the host entry on the bridge's uint8 masks (host-u8), and the device entry on shuffled uint8 masks (device-u8) and on shuffled float32 probabilities
(device-f32), the three in a random order in each round; then the per-kernel HIP-event times (option kernel_timing) of the mask ingestion of each form.  The C entry points are
called directly (ctypes), so no Python wrapper work is in the figures.

    python tools/seg_device_cost.py [surfels] [calls per form]"""
import ctypes as C
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402  (first: libifx.so binds to the HIP runtime torch ships)
import numpy as np  # noqa: E402

import instancefusion_amd as ifx  # noqa: E402
from instancefusion_amd import synth  # noqa: E402

n = int(sys.argv[1]) if len(sys.argv) > 1 else 5_000_000
calls = int(sys.argv[2]) if len(sys.argv) > 2 else 40
W, H = 640, 480
K = dict(fx=528.0, fy=528.0, cx=320.0, cy=240.0)
st = synth.make_stream(40, W, H, noise=True, loop_len=90, **K)
m = synth.make_map(n, st["scene"], st["poses_world"][0], 1000)

ef = ifx.ElasticFusion(w=W, h=H, max_surfels=n + 1_500_000, **K)
ef.processFrame(st["rgb"][0], st["depth"][0]); ef.upload(m); ef.set_pose(st["poses"][0], 1000); ef.combined_predict(st["poses"][0], 1000, 1000)
for i in range(1, 11):
    ef.processFrame(st["rgb"][i], st["depth"][i])
ef.sync()
L = ef.L
fi = 10
masks, cls = synth.canned_masks(st["obj"][fi], st["scene"])
nm = masks.shape[0]
rng = np.random.default_rng(7)
perm = rng.permutation(nm)
d_u8 = torch.from_numpy(masks[perm]).cuda()
prob = np.where(masks[perm] > 0, rng.uniform(0.5001, 1.0, masks.shape), rng.uniform(0.0, 0.5, masks.shape)).astype(np.float32)
d_f32 = torch.from_numpy(prob).cuda()
d_cls = torch.from_numpy(cls[perm].astype(np.int32)).cuda()
h_masks, h_cls = np.ascontiguousarray(masks), np.ascontiguousarray(cls.astype(np.int32))
torch.cuda.synchronize()
frame = [500]


def call(form):
    frame[0] += 3
    if form == "host-u8":
        return L.ifx_process_segmentation(ef.handle, None, None, h_masks.ctypes.data_as(C.c_void_p), h_cls.ctypes.data_as(C.c_void_p), nm, frame[0], 2)
    t = d_u8 if form == "device-u8" else d_f32
    fmt = ifx.MASK_U8 if form == "device-u8" else ifx.MASK_F32
    return L.ifx_process_segmentation_device(ef.handle, C.c_void_p(t.data_ptr()), fmt, 0.5, C.c_void_p(d_cls.data_ptr()), nm, frame[0], 2, None)


FORMS = ("host-u8", "device-u8", "device-f32")
for f in FORMS * 5:   # warm-up: allocations, first launches
    assert call(f) == 0, L.ifx_last_error(ef.handle)
ef.sync(); torch.cuda.synchronize()
# Repeated calls on one frame keep registering a few instances until the table is full and the call evicts its twenty weakest (the host-driven tail and a full
# label scan: ~2.5 ms instead of ~0.6).  Which form meets an eviction is a matter of position: the forms go in a random order each round, and the figures are
# given for the calls without an eviction (told by the table's occupancy dropping) and for all calls.
inst = ifx.InstanceFusion(ef)
wall = {f: [] for f in FORMS}
evict = {f: [] for f in FORMS}
used = int((inst.getInstanceTable() >= 0).sum())
order_rng = np.random.default_rng(1)
for k in range(calls):
    for j in order_rng.permutation(len(FORMS)):
        f = FORMS[j]
        t0 = time.perf_counter()
        r = call(f)
        wall[f].append((time.perf_counter() - t0) * 1e6)
        assert r == 0, L.ifx_last_error(ef.handle)
        now = int((inst.getInstanceTable() >= 0).sum())
        evict[f].append(now < used)
        used = now
print(f"seg_device_cost: {W}x{H}, {n} surfels, {nm} masks ({nm * W * H / 1e6:.2f} MB as uint8, {nm * W * H * 4 / 1e6:.2f} MB as float32), superpixels on; "
      f"{calls} calls per form, in a random order each round")
for f in FORMS:
    a, e = np.asarray(wall[f]), np.asarray(evict[f])
    q = a[~e]
    print(f"  {f:11s} wall per call without eviction ({len(q)} calls): median {np.median(q):7.1f} us  mean {q.mean():7.1f}  p10 {np.percentile(q, 10):7.1f}  "
          f"p90 {np.percentile(q, 90):7.1f}  min {q.min():7.1f};  with eviction ({int(e.sum())} calls): median {np.median(a[e]) if e.any() else float('nan'):7.1f} us")
ef.set_option("kernel_timing", 1)
NAMES = ("mask_clean_overlap", "mask_area", "mask_order", "mask_gather", "project_bbox_mask", "seg_compare")
for f in FORMS:
    ef.kernel_ms("__reset__")
    for _ in range(10):
        assert call(f) == 0
    ef.sync()
    ks = {nm_: ef.kernel_ms(nm_) for nm_ in NAMES}
    print(f"  {f:11s} kernels (HIP events, option kernel_timing): " + "  ".join(f"{k_} {avg * 1e3:.1f} us x {c}" for k_, (avg, c) in ks.items() if c))
ef.set_option("kernel_timing", 0)
ef.close()
