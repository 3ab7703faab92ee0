"""What the box head's post-processing costs on the GPU: the stage in the stock-PyTorch formulation of INTEGRATION.md §5 (PostProcessor.forward with the per-class
loop of filter_results replaced by one grouped ElasticFusion.nms: softmax, BoxCoder.decode over [R, 4 C], four clamps, nonzero, two gathers, the suppression, and the
reference's kthvalue on the host for the limit) against the one call ElasticFusion.box_detections, on the same inputs: R = 1000 proposals x C = 81 classes, the
released parameters (0.05 / 0.5 / 100, weights (10, 10, 5, 5)), logits scaled so that a few thousand candidates pass the threshold.  Per call and alternating between
the two: HIP-event time on the stream and wall time until the result (its count included) is on the host's side of the call; after warm-up, medians.  The one
call's kernels by HIP events (option kernel_timing) follow.  The restatement uses torch's softmax and exp and is not held to the rule's bits: the two results are
compared by count, labels and rows.

    python tools/box_detections_cost.py [calls]"""
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: E402  (first: libifx.so binds to the HIP runtime torch ships)
import numpy as np  # noqa: E402

import box_detections_cases as bc  # noqa: E402
import instancefusion_amd as ifx  # noqa: E402

calls = int(sys.argv[1]) if len(sys.argv) > 1 else 50
ef = ifx.ElasticFusion(w=640, h=480, fx=528.0, fy=528.0, cx=320.0, cy=240.0, max_surfels=100000)
CLIP = math.log(1000.0 / 16)
WX, WY, WW, WH = bc.WEIGHTS


def as_the_snippet(logits, reg, b, image, score_thresh, nms, M):
    """inference.py:43-146 for one image with INTEGRATION.md's grouped suppression; box_coder.py:52-95, bounding_box.py:214-219"""
    prob = torch.nn.functional.softmax(logits, -1)
    num_classes = prob.shape[1]
    widths, heights = b[:, 2] - b[:, 0] + 1, b[:, 3] - b[:, 1] + 1
    ctr_x, ctr_y = b[:, 0] + 0.5 * widths, b[:, 1] + 0.5 * heights
    dx, dy, dw, dh = reg[:, 0::4] / WX, reg[:, 1::4] / WY, reg[:, 2::4] / WW, reg[:, 3::4] / WH
    dw, dh = torch.clamp(dw, max=CLIP), torch.clamp(dh, max=CLIP)
    pcx, pcy = dx * widths[:, None] + ctr_x[:, None], dy * heights[:, None] + ctr_y[:, None]
    pw, ph = torch.exp(dw) * widths[:, None], torch.exp(dh) * heights[:, None]
    boxes = torch.zeros_like(reg)
    boxes[:, 0::4] = pcx - 0.5 * pw
    boxes[:, 1::4] = pcy - 0.5 * ph
    boxes[:, 2::4] = pcx + 0.5 * pw - 1
    boxes[:, 3::4] = pcy + 0.5 * ph - 1
    boxes = boxes.reshape(-1, 4)
    boxes[:, 0].clamp_(min=0, max=image[0] - 1)
    boxes[:, 1].clamp_(min=0, max=image[1] - 1)
    boxes[:, 2].clamp_(min=0, max=image[0] - 1)
    boxes[:, 3].clamp_(min=0, max=image[1] - 1)
    inds = (prob[:, 1:].t() > score_thresh).nonzero()                          # [K,2]: (class - 1, proposal), class-major as the loop concatenates
    cls, rows = inds[:, 0] + 1, inds[:, 1]
    boxes_k = boxes.view(-1, num_classes, 4)[rows, cls]
    scores_k = prob[rows, cls]
    keep = ef.nms(boxes_k, scores_k, nms, groups=cls.int())
    boxes_k, scores_k, cls, rows = boxes_k[keep], scores_k[keep], cls[keep], rows[keep]
    n = int(scores_k.shape[0])
    if n > M > 0:
        t, _ = torch.kthvalue(scores_k.cpu(), n - M + 1)
        keep = torch.nonzero(scores_k >= t.item()).squeeze(1)
        boxes_k, scores_k, cls, rows = boxes_k[keep], scores_k[keep], cls[keep], rows[keep]
    return boxes_k, scores_k, cls, rows


def one_call(logits, reg, b, image, score_thresh, nms, M):
    return ef.box_detections(logits, reg, b, image, score_thresh, nms, M)


def timed_pair(fns, args, reps):
    """the functions alternating, call by call: per function the medians of the HIP-event time and of the wall time until it returns (us)"""
    for _ in range(5):
        for fn in fns:
            fn(*args)
    torch.cuda.synchronize()
    dev, wall = [[] for _ in fns], [[] for _ in fns]
    for _ in range(reps):
        for k, fn in enumerate(fns):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            t0 = time.perf_counter()
            fn(*args)
            t1 = time.perf_counter()
            b.record()
            b.synchronize()
            dev[k].append(a.elapsed_time(b) * 1e3); wall[k].append((t1 - t0) * 1e6)
    return [(float(np.median(d)), float(np.median(w))) for d, w in zip(dev, wall)]


print(f"box_detections_cost: {torch.cuda.get_device_name(0)}, {calls} calls per figure, alternating, medians")
KERNELS = ["bd_softmax", "bd_count", "bd_compact", "bd_sort_decode", "bd_mask", "bd_reduce"]
for R, Cn, scale in ((1000, 81, 2.5), (1000, 81, 6.0)):
    logits, reg, prop, image = bc.head(1, R, Cn, scale=scale)
    args = (torch.from_numpy(logits).cuda(), torch.from_numpy(reg).cuda(), torch.from_numpy(prop).cuda(), image, 0.05, 0.5, 100)
    rb, rs, rl, rr = as_the_snippet(*args)
    ob, os_, ol, oi = one_call(*args)
    stats = ef.box_detections(*args, padded=True)[5].tolist()
    same = rb.shape == ob.shape and torch.equal(rl, ol) and torch.equal(rr, oi)
    print(f"  R = {R}, C = {Cn}, logits x {scale}: K = {stats[0]} candidates, D = {stats[1]} kept, {ob.shape[0]} detections (the restatement: {rb.shape[0]}"
          + (f", same labels and rows; largest coordinate difference {float((rb - ob).abs().max()):.2e}, largest score difference {float((rs - os_).abs().max()):.2e})"
             if same else "; labels or rows differ: torch's last bits moved a score or an IoU across a threshold)"))
    (d_ref, w_ref), (d_one, w_one) = timed_pair((as_the_snippet, one_call), args, calls)
    print(f"    the stock-PyTorch formulation: {d_ref:9.1f} us on the stream, {w_ref:9.1f} us until the call returns (nonzero, the count, kthvalue on the host)")
    print(f"    ifx_box_detections:            {d_one:9.1f} us on the stream, {w_one:9.1f} us until the call returns (the count's read)")
    fn = lambda: ef.box_detections(*args, padded=True)
    (d_pad, w_pad), = timed_pair((lambda *a: fn(),), (), calls)
    print(f"    ifx_box_detections, padded:    {d_pad:9.1f} us on the stream, {w_pad:9.1f} us until the call returns (no synchronisation)")
    ef.set_option("kernel_timing", 1)
    ef.kernel_ms("__reset__")
    for _ in range(calls):
        fn()
    ef.sync(); torch.cuda.synchronize()
    parts = []
    for k in KERNELS:
        avg, n = ef.kernel_ms(k)
        if n:
            parts.append(f"{k} {avg * 1e3:.1f} us ({n} timed)")
    ef.set_option("kernel_timing", 0)
    print("    kernels (HIP events, each launch alone): " + ", ".join(parts))
ef.close()
