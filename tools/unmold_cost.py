"""What the default detector's output and input cost on the GPU (ifx_unmold_detections, ifx_process_segmentation_unmolded, ifx_detector_input_molded) beside the
routes they replace, on the same handle and the same build.  Workload: R = 100 detections, M = 28, C = 81 at 640 x 480 behind the window of (800, 1024); the boxes
are those of the synthetic stream's mask silhouettes, jittered to fill the 100 rows; the map is the stream's after six frames.
  stage      ElasticFusion.unmold_detections(padded=True): select, memset, paste -- HIP events on the stream
  full       InstanceFusion.process_segmentation_unmolded: the stage, the 4-byte read, ifx_process_segmentation_device on the kept masks
  today      the same masks made on the host beforehand (not timed: the reference's CPU loop), then their n x P byte upload from pinned memory and
             InstanceFusion.process_segmentation_device -- what a user of the default detector does without this entry
  input      InstanceFusion.detector_input_molded(800, 1024) next to InstanceFusion.detector_input(min_size=800, max_size=1333, size_divisible=32)
`warm` warm-up calls, then `calls` timed ones: per call the HIP-event time on the stream and the host time until the call returns; medians.

    python tools/unmold_cost.py [calls] [warm]"""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: E402  (first: libifx.so binds to the HIP runtime torch ships)
import numpy as np  # noqa: E402

import instancefusion_amd as ifx  # noqa: E402
import unmold_numpy as un  # noqa: E402
from instancefusion_amd import synth  # noqa: E402

calls = int(sys.argv[1]) if len(sys.argv) > 1 else 200
warm = int(sys.argv[2]) if len(sys.argv) > 2 else 50
W, H, R, M, Cn = 640, 480, 100, 28, 81
K = dict(w=W, h=H, fx=528.0, fy=528.0, cx=320.0, cy=240.0)


def timed(fn, reps):
    dev, host = [], []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        t0 = time.perf_counter()
        fn()
        t1 = time.perf_counter()
        b.record()
        b.synchronize()
        dev.append(a.elapsed_time(b) * 1e3); host.append((t1 - t0) * 1e6)
    return float(np.median(dev)), float(np.median(host))


st = synth.make_stream(6, W, H, K["fx"], K["fy"], K["cx"], K["cy"], noise=True)
ef = ifx.ElasticFusion(**K, max_surfels=1 << 20)
inst = ifx.InstanceFusion(ef)
for i in range(6):
    pose = ef.processFrame(st["rgb"][i], st["depth"][i])
    if i == 3:                                                 # every surfel stable, as the segmentation tests prepare their maps
        m = ef.download(); m["pc"][:, 3] = 20.0
        ef.upload(m); ef.set_pose(pose, ef.tick)
size = ifx.molded_input_size(W, H, 800, 1024)
window = size[4:]
scale = un.box_scale(window, W, H)
rng = np.random.default_rng(1)
canned, _ = synth.canned_masks(st["obj"][5], st["scene"])
rows = []
while len(rows) < R:
    ys, xs = np.nonzero(canned[len(rows) % len(canned)])
    j = rng.integers(-6, 7, 4) if len(rows) >= len(canned) else np.zeros(4, np.int64)
    y1, x1 = int(np.clip(ys.min() + j[0], 0, H - 2)), int(np.clip(xs.min() + j[1], 0, W - 2))
    y2, x2 = int(np.clip(ys.max() + 1 + j[2], y1 + 1, H)), int(np.clip(xs.max() + 1 + j[3], x1 + 1, W))
    rows.append([(y1 + 0.25) / scale + window[0], (x1 + 0.25) / scale + window[1], (y2 + 0.25) / scale + window[0], (x2 + 0.25) / scale + window[1],
                 1 + len(rows) % (Cn - 1), rng.uniform(0.7, 1.0)])
det = np.array(rows, np.float32)
y, x = np.mgrid[0:M, 0:M] / (M - 1.0)
masks = rng.random((R, M, M, Cn)).astype(np.float32)
for r in range(R):
    masks[r, :, :, int(det[r, 4])] = 1.0 / (1.0 + np.exp((np.hypot(x - 0.5, y - 0.5) - rng.uniform(0.3, 0.5)) * 12.0))
d_det, d_masks = torch.from_numpy(det).cuda(), torch.from_numpy(masks).cuda()
w_m, w_c, w_b, _, _, kept = un.unmold_detections(det, masks, window, W, H)
g = ef.unmold_detections(d_det, d_masks, window, (W, H), padded=True)
torch.cuda.synchronize()
print(f"unmold_cost: {torch.cuda.get_device_name(0)}, {warm} warm-up and {calls} timed calls, medians")
print(f"  R = {R}, M = {M}, C = {Cn}, {W} x {H}, window {tuple(window)}; kept {int(g[5].item())} (statement {kept}); masks equal to the statement's: "
      f"{bool(np.array_equal(g[0].cpu().numpy(), w_m))}; box area {int(((w_b[:, 2] - w_b[:, 0]) * (w_b[:, 3] - w_b[:, 1])).sum())} of {R * W * H} pixels, "
      f"{int(w_m.sum())} inside")
host_masks = torch.from_numpy(w_m[:kept] * np.uint8(255)).pin_memory()
host_cls = w_c[:kept].copy()
frame = [100]


def stage():
    ef.unmold_detections(d_det, d_masks, window, (W, H), padded=True)


def full():
    frame[0] += 3
    inst.process_segmentation_unmolded(d_det, d_masks, window, frame[0])


def today():
    frame[0] += 3
    inst.process_segmentation_device(host_masks.to("cuda", non_blocking=True), host_cls, frame[0])


def device_only():
    frame[0] += 3
    inst.process_segmentation_device(resident, host_cls, frame[0])


resident = host_masks.cuda()
out_m = out_d = None


def molded():
    global out_m
    out_m = inst.detector_input_molded(min_dim=800, max_dim=1024, out=out_m)[0]


def benchmark_form():
    global out_d
    out_d = inst.detector_input(min_size=800, max_size=1333, size_divisible=32, out=out_d)[0]


for name, fn in (("stage: unmold_detections, padded", stage), ("full: process_segmentation_unmolded", full), ("today: upload of n x P bytes + process_segmentation_device", today),
                 ("      process_segmentation_device on resident masks", device_only), ("input: detector_input_molded (800, 1024)", molded),
                 ("       detector_input (800, 1333, 32)", benchmark_form)):
    timed(fn, warm)
    dev, host = timed(fn, calls)
    print(f"    {name:60s}: stream {dev:9.1f} us;  the call returns after {host:9.1f} us")
ef.set_option("kernel_timing", 1)
ef.kernel_ms("__reset__")
for _ in range(calls):
    stage(); molded()
ef.sync(); torch.cuda.synchronize()
print("    kernels (HIP events around every launch, average per launch):")
for n in ("unmold_select", "unmold_paste", "detector_input_molded"):
    avg, k = ef.kernel_ms(n)
    print(f"      {n:24s} {avg * 1e3:8.1f} us x {k:4d}")
ef.set_option("kernel_timing", 0)
ef.close()
