"""What a segmentation call costs when it is fed the mask head's own output (ifx_process_segmentation_rois: n x 28 x 28 probabilities and n boxes, pasted on the
GPU) on the bench workload (640x480 frame, 5 M-surfel synthetic map, the frame's 8 canned masks as ROIs: tight boxes, 28 x 28 area averages): wall time per call --
from entry to the return behind the call's own synchronisation -- for the ROI entry (rois), for the device entry on the same masks pasted beforehand as float32
(device-f32), and for what the ROI entry replaces: the same paste done in PyTorch on the GPU, one interpolate per mask as maskrcnn-benchmark's Masker does it
(the box arithmetic on the host, which holds the boxes here too), followed by the device entry (torch-paste + device-f32).  The three go in a random order in
each round.  Then the per-kernel HIP-event times (option kernel_timing) of the ingestion.  The C entry points are called directly (ctypes).

    python tools/seg_roi_cost.py [surfels] [calls per form]"""
import ctypes as C
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: E402  (first: libifx.so binds to the HIP runtime torch ships)
import numpy as np  # noqa: E402

import instancefusion_amd as ifx  # noqa: E402
import roi_paste_numpy as rp  # noqa: E402
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
M = 28
rois, boxes = rp.rois_from_masks(masks[perm], M)
pasted = np.stack([rp.paste_roi(r, b, W, H, 0.5) for r, b in zip(rois, boxes)])
iou = [float(((p != 0) & (q != 0)).sum() / max(((p != 0) | (q != 0)).sum(), 1)) for p, q in zip(pasted, masks[perm])]
d_rois, d_boxes = torch.from_numpy(rois).cuda(), torch.from_numpy(boxes).cuda()
d_f32 = torch.from_numpy((pasted != 0).astype(np.float32)).cuda()
d_cls = torch.from_numpy(cls[perm].astype(np.int32)).cuda()
recs = [rp.roi_record(b, M, 1 << 30, 1 << 30) for b in boxes]   # (unclipped: b0, b1 and, through the clip's upper ends, the size of the resize)
torch.cuda.synchronize()
frame = [500]
P = lambda t: C.c_void_p(t.data_ptr())


def torch_paste():
    """The Masker's paste in PyTorch on the GPU: pad, one bilinear resize per mask to its expanded box, threshold, copy the part inside the image."""
    out = torch.zeros((nm, H, W), dtype=torch.float32, device="cuda")
    padded = torch.nn.functional.pad(d_rois, (1, 1, 1, 1))
    for i, (b, rec) in enumerate(zip(boxes, recs)):
        if rec is None:
            continue
        b0, b1 = rec[0], rec[1]
        w, h = rec[3] - b0, rec[5] - b1
        big = torch.nn.functional.interpolate(padded[i][None, None], size=(h, w), mode="bilinear", align_corners=False)[0, 0] > 0.5
        x0, x1, y0, y1 = max(b0, 0), min(b0 + w, W), max(b1, 0), min(b1 + h, H)
        if x1 > x0 and y1 > y0:
            out[i, y0:y1, x0:x1] = big[y0 - b1:y1 - b1, x0 - b0:x1 - b0]
    return out


def call(form):
    frame[0] += 3
    if form == "rois":
        return L.ifx_process_segmentation_rois(ef.handle, P(d_rois), M, P(d_boxes), 0.5, P(d_cls), nm, frame[0], 2, None)
    t = torch_paste() if form == "torch-paste + device-f32" else d_f32
    return L.ifx_process_segmentation_device(ef.handle, P(t), ifx.MASK_F32, 0.5, P(d_cls), nm, frame[0], 2, None)


FORMS = ("rois", "device-f32", "torch-paste + device-f32")
differ = int(((torch_paste() > 0.5) != (d_f32 > 0.5)).sum())
for f in FORMS * 5:   # warm-up: allocations, first launches
    assert call(f) == 0, L.ifx_last_error(ef.handle)
ef.sync(); torch.cuda.synchronize()
# (evictions: as tools/seg_device_cost.py -- the forms go in a random order each round, the calls that met an eviction are reported apart)
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
print(f"seg_roi_cost: {W}x{H}, {n} surfels, {nm} ROIs of {M}x{M} ({nm * (M * M + 4) * 4 / 1e3:.1f} KB; pasted: {nm * W * H * 4 / 1e6:.2f} MB as float32), superpixels on; "
      f"{calls} calls per form, in a random order each round")
print(f"  paste against the canned masks: IoU {min(iou):.3f} .. {max(iou):.3f}; PyTorch's GPU paste differs from the statement on {differ} pixels")
for f in FORMS:
    a, e = np.asarray(wall[f]), np.asarray(evict[f])
    q = a[~e]
    print(f"  {f:24s} wall per call without eviction ({len(q)} calls): median {np.median(q):7.1f} us  mean {q.mean():7.1f}  p10 {np.percentile(q, 10):7.1f}  "
          f"p90 {np.percentile(q, 90):7.1f}  min {q.min():7.1f};  with eviction ({int(e.sum())} calls): median {np.median(a[e]) if e.any() else float('nan'):7.1f} us")
ef.set_option("kernel_timing", 1)
NAMES = ("roi_area", "mask_area", "mask_order", "roi_gather", "mask_gather", "project_bbox_mask", "seg_compare")
for f in FORMS[:2]:
    ef.kernel_ms("__reset__")
    for _ in range(10):
        assert call(f) == 0
    ef.sync()
    ks = {nm_: ef.kernel_ms(nm_) for nm_ in NAMES}
    print(f"  {f:24s} kernels (HIP events, option kernel_timing): " + "  ".join(f"{k_} {avg * 1e3:.1f} us x {c}" for k_, (avg, c) in ks.items() if c))
ef.set_option("kernel_timing", 0)
ef.close()
