"""What multi-level ROI pooling costs on the GPU (ifx_fpn_roi_align, one launch) beside the reference's formulation on the same inputs and the same build:
LevelMapper in stock tensor operations, then per level a nonzero, a gather, ElasticFusion.roi_align_forward and an index_put into a zero-filled result
(maskrcnn_benchmark/modeling/poolers.py:31-42 and :104-121).  Workloads: the pyramid of an 800 x 1344 image (200 x 336, 100 x 168, 50 x 84, 25 x 42; 256 channels),
1000 ROIs at 7 x 7 and sampling ratio 2 (the box head) and 100 ROIs at 14 x 14 and ratio 2 (the mask head).  Per figure: HIP-event time of the whole call on its
stream and the host time until the call returns; the two paths are run alternately, `rounds` rounds of `calls` calls each, and the median of every round and the
median of those medians are printed.  The results of the two paths are compared first.

    python tools/fpn_pooler_cost.py [calls] [rounds]"""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402  (first: libifx.so binds to the HIP runtime torch ships)
import numpy as np  # noqa: E402

import instancefusion_amd as ifx  # noqa: E402

calls = int(sys.argv[1]) if len(sys.argv) > 1 else 30
rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 5
ef = ifx.ElasticFusion(w=640, h=480, fx=528.0, fy=528.0, cx=320.0, cy=240.0, max_surfels=100000)
rng = np.random.default_rng(1)
SCALES = [0.25, 0.125, 0.0625, 0.03125]


def timed(fn, reps):
    """HIP-event time of fn() on the current stream and the host time until it returns: medians in us"""
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


def reference_loop(x, rois, res, ratio, out):
    """LevelMapper and the loop of Pooler.forward, the pooling by this library's ROIAlign"""
    s = torch.sqrt((rois[:, 3] - rois[:, 1] + 1) * (rois[:, 4] - rois[:, 2] + 1))
    lv = torch.floor(4 + torch.log2(s / 224 + 1e-6))
    levels = torch.clamp(lv, min=2, max=5).to(torch.int64) - 2
    out.zero_()
    for level, (feat, scale) in enumerate(zip(x, SCALES)):
        idx = torch.nonzero(levels == level).squeeze(1)                  # the host waits here for the count
        out[idx] = ef.roi_align_forward(feat, rois[idx], scale, res, res, ratio)
    return out, levels


print(f"fpn_pooler_cost: {torch.cuda.get_device_name(0)}, {rounds} alternating rounds of {calls} calls, medians")
x = [torch.randn(1, 256, 800 >> k, 1344 >> k, device="cuda") for k in (2, 3, 4, 5)]
for (n, res) in ((1000, 7), (100, 14)):
    side = 2.0 ** rng.uniform(4.0, 10.0, n)                                # 16 .. 1024 px: every level
    w, h = side * rng.uniform(0.7, 1.4, n), side / rng.uniform(0.7, 1.4, n)
    cx, cy = rng.uniform(0, 1344, n), rng.uniform(0, 800, n)
    rois = torch.from_numpy(np.stack([np.zeros(n), cx - w / 2, cy - h / 2, cx + w / 2, cy + h / 2], axis=1).astype(np.float32)).cuda()
    out = torch.empty(n, 256, res, res, device="cuda")
    ref_out = torch.empty_like(out)
    lev = torch.empty(n, dtype=torch.int32, device="cuda")
    one = lambda: ef.fpn_roi_align(x, rois, SCALES, res, res, 2, out=out, levels_out=lev)
    loop = lambda: reference_loop(x, rois, res, 2, ref_out)
    one()
    _, ref_lev = loop()
    torch.cuda.synchronize()
    per_level = torch.bincount(lev.long(), minlength=4).tolist()
    differ = int((lev.long() != ref_lev).sum())
    same = bool(torch.equal(out[lev.long() == ref_lev], ref_out[lev.long() == ref_lev]))
    print(f"  {n} ROIs x 256 x {res} x {res}, ratio 2: ROIs per level {per_level}; {out.numel() * 4 / 1e6:.1f} MB written; levels that differ from torch's LevelMapper "
          f"on the device: {differ}; pooled rows of equal level bit-equal: {same}")
    for _ in range(3):
        one(); loop()
    torch.cuda.synchronize()
    res_one, res_loop = [], []
    for _ in range(rounds):
        res_one.append(timed(one, calls))
        res_loop.append(timed(loop, calls))
    for name, r, syncs in (("ifx_fpn_roi_align (one launch)", res_one, 0), ("per-level loop (poolers.py)  ", res_loop, 4)):
        dev, host = [v[0] for v in r], [v[1] for v in r]
        print(f"    {name}: stream {np.median(dev):8.1f} us {[round(v, 1) for v in dev]};  the call returns after {np.median(host):8.1f} us {[round(v, 1) for v in host]};  "
              f"host synchronisations per call: {syncs}")
    ef.set_option("kernel_timing", 1)
    ef.kernel_ms("__reset__")
    for _ in range(calls):
        one()
    ef.sync(); torch.cuda.synchronize()
    avg, cnt = ef.kernel_ms("fpn_roi_align")
    print(f"    kernel fpn_roi_align (HIP events around the launch): {avg * 1e3:.1f} us x {cnt}")
    ef.kernel_ms("__reset__")
    for _ in range(calls):
        loop()
    ef.sync(); torch.cuda.synchronize()
    avg, cnt = ef.kernel_ms("roi_align")
    print(f"    kernel roi_align in the loop: {avg * 1e3:.1f} us x {cnt} (one launch per level: {avg * 1e3 * len(SCALES):.1f} us per call)")
    ef.set_option("kernel_timing", 0)
ef.close()
