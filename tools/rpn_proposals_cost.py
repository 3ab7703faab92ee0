"""What the RPN's proposal stage costs on the GPU: the stage as the reference writes it (RPNPostProcessor.forward_for_single_feature_map, restated here in stock
PyTorch on the same device with ElasticFusion.nms in the place of _C.nms: sigmoid, topk, gathers, BoxCoder.decode, four clamps, the boolean index of
remove_small_boxes, the suppression, keep[:post]) against the one call ElasticFusion.rpn_proposals, at the reference's own level (38 x 50 x 15 anchors, 6000 / 200 /
0.7) and at an FPN level 0 (200 x 336 x 3, 1000 / 1000 / 0.7).  Per call and alternating between the two: HIP-event time on the stream and wall time until the
result (its count included) is on the host's side of the call; after warm-up, medians.  The one call's kernels by HIP events (option kernel_timing) follow.
The restatement uses torch.exp and is not held to the rule's bits: the two results are compared by count and by the largest coordinate difference.

    python tools/rpn_proposals_cost.py [calls]"""
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: E402  (first: libifx.so binds to the HIP runtime torch ships)
import numpy as np  # noqa: E402

import instancefusion_amd as ifx  # noqa: E402
import rpn_proposals_cases as rc  # noqa: E402

calls = int(sys.argv[1]) if len(sys.argv) > 1 else 50
ef = ifx.ElasticFusion(w=640, h=480, fx=528.0, fy=528.0, cx=320.0, cy=240.0, max_surfels=100000)
CLIP = math.log(1000.0 / 16)


def as_the_reference(obj, reg, anchors, image, pre, post, thr, min_size):
    """inference.py:74-121 for N = 1, box_coder.py:52-95, bounding_box.py:214-219, boxlist_ops.py:9-48, operator for operator"""
    A, H, W = obj.shape
    o = obj.view(1, A, 1, H, W).permute(0, 3, 4, 1, 2).reshape(1, -1).sigmoid()
    r = reg.view(1, A, 4, H, W).permute(0, 3, 4, 1, 2).reshape(1, -1, 4)
    o, top = o.topk(min(pre, A * H * W), dim=1, sorted=True)
    batch = torch.arange(1, device=obj.device)[:, None]
    r = r[batch, top].view(-1, 4)
    b = anchors.reshape(1, -1, 4)[batch, top].view(-1, 4)
    widths, heights = b[:, 2] - b[:, 0] + 1, b[:, 3] - b[:, 1] + 1
    ctr_x, ctr_y = b[:, 0] + 0.5 * widths, b[:, 1] + 0.5 * heights
    dx, dy, dw, dh = r[:, 0::4] / 1.0, r[:, 1::4] / 1.0, r[:, 2::4] / 1.0, r[:, 3::4] / 1.0
    dw, dh = torch.clamp(dw, max=CLIP), torch.clamp(dh, max=CLIP)
    pcx, pcy = dx * widths[:, None] + ctr_x[:, None], dy * heights[:, None] + ctr_y[:, None]
    pw, ph = torch.exp(dw) * widths[:, None], torch.exp(dh) * heights[:, None]
    boxes = torch.zeros_like(r)
    boxes[:, 0::4] = pcx - 0.5 * pw
    boxes[:, 1::4] = pcy - 0.5 * ph
    boxes[:, 2::4] = pcx + 0.5 * pw - 1
    boxes[:, 3::4] = pcy + 0.5 * ph - 1
    score = o[0]
    boxes[:, 0].clamp_(min=0, max=image[0] - 1)
    boxes[:, 1].clamp_(min=0, max=image[1] - 1)
    boxes[:, 2].clamp_(min=0, max=image[0] - 1)
    boxes[:, 3].clamp_(min=0, max=image[1] - 1)
    ws, hs = boxes[:, 2] - boxes[:, 0] + 1, boxes[:, 3] - boxes[:, 1] + 1
    keep = ((ws >= min_size) & (hs >= min_size)).nonzero().squeeze(1)
    boxes, score = boxes[keep], score[keep]
    keep = ef.nms(boxes, score, thr)[:post]
    return boxes[keep], score[keep]


def one_call(obj, reg, anchors, image, pre, post, thr, min_size):
    return ef.rpn_proposals(obj, reg, anchors, image, pre, post, thr, min_size)[:2]


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


print(f"rpn_proposals_cost: {torch.cuda.get_device_name(0)}, {calls} calls per figure, alternating, medians")
KERNELS = ["rpn_hist", "rpn_count", "rpn_compact", "rpn_sort_decode", "rpn_mask", "rpn_reduce"]
for (A, H, W), pre, post in (((15, 38, 50), 6000, 200), ((3, 200, 336), 1000, 1000)):
    obj, reg, anc, image = rc.level(1, A, H, W, spread=0.2)
    args = (torch.from_numpy(obj).cuda(), torch.from_numpy(reg).cuda(), torch.from_numpy(anc).cuda(), image, pre, post, 0.7, 0)
    rb, rs = as_the_reference(*args)
    ob, os_ = one_call(*args)
    same = rb.shape == ob.shape
    print(f"  {H} x {W} x {A} = {A * H * W} anchors, pre {pre}, post {post}, threshold 0.7: {ob.shape[0]} proposals (the restatement: {rb.shape[0]}"
          + (f"; largest coordinate difference {float((rb - ob).abs().max()):.2e})" if same else "; the counts differ: torch.exp's last bit moved an IoU across the threshold)"))
    (d_ref, w_ref), (d_one, w_one) = timed_pair((as_the_reference, one_call), args, calls)
    print(f"    as the reference writes it: {d_ref:9.1f} us on the stream, {w_ref:9.1f} us until the call returns (two synchronisations)")
    print(f"    ifx_rpn_proposals:          {d_one:9.1f} us on the stream, {w_one:9.1f} us until the call returns (the count's read)")
    fn = lambda: ef.rpn_proposals(*args, padded=True)
    (d_pad, w_pad), = timed_pair((lambda *a: fn(),), (), calls)
    print(f"    ifx_rpn_proposals, padded:  {d_pad:9.1f} us on the stream, {w_pad:9.1f} us until the call returns (no synchronisation)")
    ef.set_option("kernel_timing", 1)
    ef.kernel_ms("__reset__")
    for _ in range(calls):
        fn()
    ef.sync(); torch.cuda.synchronize()
    parts = []
    for k in KERNELS:
        avg, n = ef.kernel_ms(k)
        if n:
            parts.append(f"{k} {avg * 1e3:.1f} us x {n // calls}")
    ef.set_option("kernel_timing", 0)
    print("    kernels (HIP events, each launch alone): " + ", ".join(parts))
ef.close()
