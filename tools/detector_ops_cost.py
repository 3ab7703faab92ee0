"""What the detector's two operators cost on the GPU (ifx_roi_align_forward, ifx_nms) at the detector's own sizes: HIP-event time of the whole call on its stream,
the kernels' own times (option kernel_timing), the host time of the enqueue.  ROIAlign: 1000 ROIs x 256 channels x 7 x 7 at sampling ratio 2 on a 200 x 336 map
(the box head at stride 4) and 100 x 256 x 14 x 14 (the mask head).  NMS: n = 1000 and 6000 (the RPN with and without FPN), and 1000 boxes in 80 groups in one
call against the box head's loop of 80 ungrouped calls.  For orientation only, a plain-PyTorch formulation written here is timed beside each (gathers and
elementwise kernels for ROIAlign; the IoU matrix on the device, downloaded and reduced on the host, for NMS -- what the reference does with its mask words).  The
results of the two paths are compared first.

    python tools/detector_ops_cost.py [calls]"""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402  (first: libifx.so binds to the HIP runtime torch ships)
import numpy as np  # noqa: E402

import instancefusion_amd as ifx  # noqa: E402

calls = int(sys.argv[1]) if len(sys.argv) > 1 else 50
ef = ifx.ElasticFusion(w=640, h=480, fx=528.0, fy=528.0, cx=320.0, cy=240.0, max_surfels=100000)
rng = np.random.default_rng(1)


def timed(fn, reps):
    """HIP-event time of fn() on the current stream and the host time until it returns: medians in us"""
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
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


def kernel_times(fn, names, reps):
    ef.set_option("kernel_timing", 1)
    ef.kernel_ms("__reset__")
    for _ in range(reps):
        fn()
    ef.sync(); torch.cuda.synchronize()
    out = []
    for k in names:
        avg, n = ef.kernel_ms(k)
        out.append(f"{k} {avg * 1e3:.1f} us x {n}")
    ef.set_option("kernel_timing", 0)
    return ", ".join(out)


def torch_roi_align(inp, rois, scale, ph, pw, ratio):
    """ROIAlign at a fixed sampling ratio in stock tensor operations (not held to the rule's operation order)"""
    B, Cn, H, W = inp.shape
    n = rois.shape[0]
    bidx = rois[:, 0].long()
    sw, sh, ew, eh = (rois[:, i] * scale for i in (1, 2, 3, 4))
    bw, bh = (ew - sw).clamp(min=1) / pw, (eh - sh).clamp(min=1) / ph

    def axis(start, bin_size, pooled, size):
        p = torch.arange(pooled, device=inp.device, dtype=torch.float32).repeat_interleave(ratio)[None, :]
        i = torch.arange(ratio, device=inp.device, dtype=torch.float32).repeat(pooled)[None, :]
        y = (start[:, None] + p * bin_size[:, None]) + ((i + 0.5) * bin_size[:, None]) / ratio
        valid = (y >= -1) & (y <= size)
        y = y.clamp(min=0)
        lo = y.long().clamp(max=size - 1)
        hi = (lo + 1).clamp(max=size - 1)
        y = torch.where(lo >= size - 1, lo.float(), y)
        l = y - lo.float()
        return lo, hi, l, 1 - l, valid

    yl, yh, ly, hy, vy = axis(sh, bh, ph, H)
    xl, xh, lx, hx, vx = axis(sw, bw, pw, W)
    bb = bidx[:, None, None]
    Y, X = (lambda a: a[:, :, None]), (lambda a: a[:, None, :])
    val = ((Y(hy) * X(hx))[..., None] * inp[bb, :, Y(yl), X(xl)] + (Y(hy) * X(lx))[..., None] * inp[bb, :, Y(yl), X(xh)]
           + (Y(ly) * X(hx))[..., None] * inp[bb, :, Y(yh), X(xl)] + (Y(ly) * X(lx))[..., None] * inp[bb, :, Y(yh), X(xh)])
    val = val * (Y(vy) & X(vx))[..., None]                           # [n, ph * r, pw * r, C]
    return val.view(n, ph, ratio, pw, ratio, Cn).sum(dim=(2, 4)).permute(0, 3, 1, 2) / (ratio * ratio)


def torch_nms(boxes, scores, thr):
    """the IoU matrix on the device, the greedy pass on the host"""
    order = torch.sort(scores, descending=True, stable=True).indices
    b = boxes[order]
    area = (b[:, 2] - b[:, 0] + 1) * (b[:, 3] - b[:, 1] + 1)
    w = (torch.minimum(b[:, None, 2], b[None, :, 2]) - torch.maximum(b[:, None, 0], b[None, :, 0]) + 1).clamp(min=0)
    h = (torch.minimum(b[:, None, 3], b[None, :, 3]) - torch.maximum(b[:, None, 1], b[None, :, 1]) + 1).clamp(min=0)
    inter = w * h
    over = (inter / (area[:, None] + area[None, :] - inter) > thr).cpu().numpy()
    n = over.shape[0]
    removed = np.zeros(n, bool)
    kept = []
    for i in range(n):
        if not removed[i]:
            kept.append(i)
            removed[i + 1:] |= over[i, i + 1:]
    return torch.sort(order[torch.as_tensor(kept, device=boxes.device)]).values


def boxes_for(n, extent):
    c = rng.uniform(0, extent, (n, 2))
    return torch.from_numpy(np.concatenate([c, c + rng.uniform(8, 120, (n, 2))], axis=1).astype(np.float32)).cuda()


print(f"detector_ops_cost: {torch.cuda.get_device_name(0)}, {calls} calls per figure, medians")
inp = torch.randn(1, 256, 200, 336, device="cuda")
for (n, ph, pw) in ((1000, 7, 7), (100, 14, 14)):
    x0, y0 = rng.uniform(0, 1100, n), rng.uniform(0, 650, n)
    rois = torch.from_numpy(np.stack([np.zeros(n), x0, y0, x0 + rng.uniform(16, 400, n), y0 + rng.uniform(16, 300, n)], axis=1).astype(np.float32)).cuda()
    out = ef.roi_align_forward(inp, rois, 0.25, ph, pw, 2)
    ref = torch_roi_align(inp, rois, 0.25, ph, pw, 2)
    print(f"  roi_align {n} x 256 x {ph} x {pw}, ratio 2, map 200 x 336: {out.numel() * 4 / 1e6:.1f} MB written; largest difference from the PyTorch formulation "
          f"{float((out - ref).abs().max()):.2e}")
    fn = lambda: ef.roi_align_forward(inp, rois, 0.25, ph, pw, 2, out=out)
    dev, host = timed(fn, calls)
    print(f"    ifx_roi_align_forward: {dev:9.1f} us on the stream, the call returns after {host:7.1f} us;  kernel (HIP events): {kernel_times(fn, ['roi_align'], calls)}")
    dev, host = timed(lambda: torch_roi_align(inp, rois, 0.25, ph, pw, 2), max(calls // 5, 5))
    print(f"    plain PyTorch:         {dev:9.1f} us on the stream")
for n in (1000, 6000):
    boxes, scores = boxes_for(n, 1200.0), torch.from_numpy(rng.random(n).astype(np.float32)).cuda()
    keep = ef.nms(boxes, scores, 0.7)
    print(f"  nms n = {n}, threshold 0.7: {keep.numel()} kept; equal to the PyTorch formulation: {bool(torch.equal(keep, torch_nms(boxes, scores, 0.7)))}")
    fn = lambda: ef.nms(boxes, scores, 0.7, padded=True)
    dev, host = timed(fn, calls)
    print(f"    ifx_nms (padded, no read-back): {dev:9.1f} us on the stream, the call returns after {host:7.1f} us;  kernels: {kernel_times(fn, ['nms_sort', 'nms_mask', 'nms_reduce'], calls)}")
    dev, host = timed(lambda: ef.nms(boxes, scores, 0.7), calls)
    print(f"    ifx_nms with the count read:    {host:9.1f} us until the call returns")
    dev, host = timed(lambda: torch_nms(boxes, scores, 0.7), max(calls // 10, 3))
    print(f"    plain PyTorch + host loop:      {host:9.1f} us until the call returns")
n, G = 1000, 80
boxes, scores = boxes_for(n, 1200.0), torch.from_numpy(rng.random(n).astype(np.float32)).cuda()
groups = torch.from_numpy(rng.integers(0, G, n).astype(np.int32)).cuda()
idx = [torch.nonzero(groups == g).reshape(-1) for g in range(G)]
per = [(boxes[i].contiguous(), scores[i].contiguous()) for i in idx]


def loop():
    return torch.sort(torch.cat([i[ef.nms(b, s, 0.5)] for i, (b, s) in zip(idx, per)])).values


one = ef.nms(boxes, scores, 0.5, groups=groups)
print(f"  nms 1000 boxes in 80 groups, threshold 0.5: {one.numel()} kept; equal to 80 ungrouped calls: {bool(torch.equal(one, loop()))}")
dev, host = timed(lambda: ef.nms(boxes, scores, 0.5, groups=groups), calls)
print(f"    one grouped call, count read:   {host:9.1f} us until the call returns ({dev:.1f} us on the stream)")
dev, host = timed(loop, max(calls // 5, 5))
print(f"    80 ungrouped calls, counts read:{host:9.1f} us until the loop returns")
ef.close()
