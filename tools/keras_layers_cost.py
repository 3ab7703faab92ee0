"""What the Keras detector's three layers cost on the GPU at the reference's configuration, each against a plain torch-op composition of the same rule -- the
baseline a user who runs the network under PyTorch has today (no torchvision: the suppression is the usual loop over the kept boxes, one IoU row and one 4-byte
read per kept box):

  proposals    65 472 anchors -> 6000 -> 1000                    ElasticFusion.keras_proposals
  ROI align    1000 boxes x 256 channels x 7 x 7, 100 x 256 x 14 x 14, maps of 256^2 .. 32^2 (NHWC)    ElasticFusion.pyramid_roi_align
  detections   1000 ROIs x 81 classes                            ElasticFusion.keras_detections

Per call and alternating between the two: HIP-event time on the stream and wall time until the call returns; after warm-up, medians.  The library's launches per
call are counted by its kernel timing; the composition's by torch's profiler where it is available.  The compositions use torch's exp and are not held to the
rule's bits: the results are compared by count and rows.  Writes the figures to profiles/keras_layers_cost.txt (or the path given).

    python tools/keras_layers_cost.py [calls] [output file]"""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: E402  (first: libifx.so binds to the HIP runtime torch ships)
import numpy as np  # noqa: E402

import instancefusion_amd as ifx  # noqa: E402
import keras_layers_gpu as kg  # noqa: E402

calls = int(sys.argv[1]) if len(sys.argv) > 1 else 30
OUT = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "keras_layers_cost.txt")
ef = ifx.ElasticFusion(w=640, h=480, fx=528.0, fy=528.0, cx=320.0, cy=240.0, max_surfels=100000)
IMG = (1024, 1024)
STD = torch.tensor([0.1, 0.1, 0.2, 0.2], device="cuda")
lines = []


def say(s):
    print(s)
    lines.append(s)


def decode(boxes, deltas):
    h, w = boxes[:, 2] - boxes[:, 0], boxes[:, 3] - boxes[:, 1]
    cy, cx = boxes[:, 0] + 0.5 * h + deltas[:, 0] * h, boxes[:, 1] + 0.5 * w + deltas[:, 1] * w
    h, w = h * torch.exp(deltas[:, 2]), w * torch.exp(deltas[:, 3])
    y1, x1 = cy - 0.5 * h, cx - 0.5 * w
    return torch.stack([y1, x1, y1 + h, x1 + w], dim=1)


def loop_nms(boxes, thr, limit):
    """boxes in descending score: the kept positions.  The plain-torch loop: per kept box one IoU row over the rest and a boolean index (a host read of its size)"""
    area = (boxes[:, 2] - boxes[:, 0]) * (boxes[:, 3] - boxes[:, 1])
    order = torch.arange(boxes.shape[0], device=boxes.device)
    keep = []
    while order.numel() > 0 and len(keep) < limit:
        i = order[0]
        keep.append(i)
        rest = order[1:]
        ih = (torch.minimum(boxes[i, 2], boxes[rest, 2]) - torch.maximum(boxes[i, 0], boxes[rest, 0])).clamp(min=0)
        iw = (torch.minimum(boxes[i, 3], boxes[rest, 3]) - torch.maximum(boxes[i, 1], boxes[rest, 1])).clamp(min=0)
        inter = ih * iw
        iou = torch.where((area[i] <= 0) | (area[rest] <= 0), torch.zeros_like(inter), inter / (area[i] + area[rest] - inter))
        order = rest[~(iou > thr)]
    return torch.stack(keep) if keep else torch.zeros(0, dtype=torch.int64, device=boxes.device)


def proposals_torch(probs, bbox, anchors):
    scores, ix = torch.topk(probs[:, 1], 6000, sorted=True)
    b = decode(anchors[ix], bbox[ix] * STD)
    b = torch.stack([b[:, 0].clamp(0, IMG[0]), b[:, 1].clamp(0, IMG[1]), b[:, 2].clamp(0, IMG[0]), b[:, 3].clamp(0, IMG[1])], dim=1) / 1024.0
    keep = loop_nms(b, 0.7, 1000)
    out = torch.zeros((1000, 4), device="cuda")
    out[:keep.numel()] = b[keep]
    return out, ix[keep]


def roi_align_torch(maps, boxes, pool):
    """PyramidROIAlign on NHWC maps of one image: the level expression, per level a nonzero, four gathers and the blend, a scatter back into box order"""
    y1, x1, y2, x2 = boxes.unbind(1)
    lvl = torch.log2(torch.sqrt((y2 - y1) * (x2 - x1)) / (224.0 / 1024.0))
    lvl = (4 + torch.round(lvl).int()).clamp(2, 5)
    out = torch.zeros((boxes.shape[0], pool, pool, maps[0].shape[-1]), device="cuda")
    t = torch.arange(pool, device="cuda", dtype=torch.float32) / (pool - 1)
    for l, m in enumerate(maps):
        ix = (lvl == l + 2).nonzero()[:, 0]
        if ix.numel() == 0:
            continue
        H, W = m.shape[1] - 1, m.shape[2] - 1
        ys = (y1[ix, None] + (y2 - y1)[ix, None] * t[None]) * H
        xs = (x1[ix, None] + (x2 - x1)[ix, None] * t[None]) * W
        ok = ((ys >= 0) & (ys <= H))[:, :, None] & ((xs >= 0) & (xs <= W))[:, None, :]
        ys, xs = ys.clamp(0, H), xs.clamp(0, W)
        y0, x0 = ys.floor().long(), xs.floor().long()
        yb, xb = ys.ceil().long(), xs.ceil().long()
        ly, lx = (ys - y0)[:, :, None, None], (xs - x0)[:, None, :, None]
        f = m[0]
        top = f[y0[:, :, None], x0[:, None, :]] + (f[y0[:, :, None], xb[:, None, :]] - f[y0[:, :, None], x0[:, None, :]]) * lx
        bot = f[yb[:, :, None], x0[:, None, :]] + (f[yb[:, :, None], xb[:, None, :]] - f[yb[:, :, None], x0[:, None, :]]) * lx
        out[ix] = (top + (bot - top) * ly) * ok[..., None]
    return out


def detections_torch(rois, probs, deltas):
    R = probs.shape[0]
    cls = probs.argmax(1)
    score = probs[torch.arange(R, device="cuda"), cls]
    b = decode(rois, deltas[torch.arange(R, device="cuda"), cls] * STD) * 1024.0
    b = torch.round(b.clamp(0, 1024))
    keep = ((cls > 0) & (score >= 0.7)).nonzero()[:, 0]
    order = keep[torch.argsort(score[keep], descending=True, stable=True)]
    shifted = b[order] + (cls[order].float() * 4096.0)[:, None]             # the class-offset trick: one suppression for all classes
    kept = order[loop_nms(shifted, 0.3, 100)]
    det = torch.zeros((100, 6), device="cuda")
    det[:kept.numel()] = torch.cat([b[kept], cls[kept].float()[:, None], score[kept][:, None]], dim=1)
    return det, kept


def timed_pair(fns, reps):
    for _ in range(3):
        for fn in fns:
            fn()
    torch.cuda.synchronize()
    dev, wall = [[] for _ in fns], [[] for _ in fns]
    for _ in range(reps):
        for k, fn in enumerate(fns):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            t0 = time.perf_counter()
            fn()
            t1 = time.perf_counter()
            b.record()
            b.synchronize()
            dev[k].append(a.elapsed_time(b) * 1e3); wall[k].append((t1 - t0) * 1e6)
    return [(float(np.median(d)), float(np.median(w))) for d, w in zip(dev, wall)]


def launches_of(fn):
    """device kernels and memsets / copies of one call by torch's profiler; None where it is not available"""
    try:
        from torch.profiler import ProfilerActivity, profile

        fn(); torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            fn(); torch.cuda.synchronize()
        return sum(1 for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA)
    except Exception:
        return None


def own_launches(fn, names):
    ef.set_option("kernel_timing", 1)
    ef.kernel_ms("__reset__")
    fn()
    ef.sync(); torch.cuda.synchronize()
    got = [(k, *ef.kernel_ms(k)) for k in names]
    ef.set_option("kernel_timing", 0)
    return sum(n for _, _, n in got), ", ".join(f"{k} {avg * 1e3:.1f} us" + (f" x {n}" if n > 1 else "") for k, avg, n in got if n)


def report(title, base, own, names, note):
    (d_ref, w_ref), (d_one, w_one) = timed_pair((base, own), calls)
    nb, (no, parts) = launches_of(base), own_launches(own, names)
    say(f"  {title}")
    say(f"    torch-op composition: {d_ref:10.1f} us on the stream, {w_ref:10.1f} us until the call returns, " + (f"{nb} device operations" if nb is not None else "launches not counted"))
    say(f"    the library's call:   {d_one:10.1f} us on the stream, {w_one:10.1f} us until the call returns, {no} launches ({note})")
    say(f"    kernels (HIP events, each launch alone): {parts}")


say(f"keras_layers_cost: {torch.cuda.get_device_name(0)}, {calls} calls per figure, alternating, medians")
probs, bbox, anc = (kg.cuda(a) for a in kg.proposal_case(1, 65472))
ref_p = proposals_torch(probs, bbox, anc)
own_p = ef.keras_proposals(probs, bbox, anc, IMG, padded=True)
say(f"  proposals: the library keeps {int(own_p[2].item())}, the composition {ref_p[1].numel()}; same anchors: {torch.equal(own_p[1][:ref_p[1].numel()], ref_p[1])}")
report("proposals, 65 472 -> 6000 -> 1000", lambda: proposals_torch(probs, bbox, anc), lambda: ef.keras_proposals(probs, bbox, anc, IMG, padded=True),
       ["kp_hist", "kp_count", "kp_compact", "kp_sort_decode", "kp_mask", "kp_reduce"], "and one memset; padded form, no read")
rng = np.random.default_rng(2)
maps = [kg.cuda(rng.standard_normal((1, s, s, 256)).astype(np.float32)) for s in (256, 128, 64, 32)]
for n, pool in ((1000, 7), (100, 14)):
    side = np.exp(rng.uniform(np.log(0.02), np.log(0.9), (n, 2)))
    p0 = rng.uniform(0, 1, (n, 2)) * (1 - side)
    boxes = kg.cuda(np.concatenate([p0, p0 + side], axis=1).astype(np.float32))
    a, b = roi_align_torch(maps, boxes, pool), ef.pyramid_roi_align(maps, boxes, IMG, (pool, pool))
    say(f"  ROI align {n} x 256 x {pool} x {pool}: largest difference to the composition {float((a - b).abs().max()):.2e}")
    report(f"ROI align, {n} boxes x 256 channels x {pool} x {pool}", lambda: roi_align_torch(maps, boxes, pool), lambda: ef.pyramid_roi_align(maps, boxes, IMG, (pool, pool)),
           ["pyramid_roi_align"], "enqueue only")
rois = kg.cuda(np.concatenate([p0, p0 + side], axis=1).astype(np.float32)).repeat(10, 1)[:1000].contiguous()
cp = rng.random((1000, 81)).astype(np.float32) * 0.002
cp[np.arange(1000), rng.integers(0, 81, 1000)] += 0.85
cprobs, deltas = kg.cuda(cp), kg.cuda((rng.standard_normal((1000, 81, 4)) * 0.5).astype(np.float32))
ref_d = detections_torch(rois, cprobs, deltas)
own_d = ef.keras_detections(rois, cprobs, deltas, (0, 0, 1024, 1024), IMG, padded=True)
say(f"  detections: the library keeps {int(own_d[3].item())}, the composition {ref_d[1].numel()}; same rows: {torch.equal(own_d[2][:ref_d[1].numel()], ref_d[1])}")
report("detections, 1000 x 81", lambda: detections_torch(rois, cprobs, deltas), lambda: ef.keras_detections(rois, cprobs, deltas, (0, 0, 1024, 1024), IMG, padded=True),
       ["kd_rows", "kd_sort", "kd_mask", "kd_reduce"], "padded form, no read")
ef.close()
os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
with open(OUT, "w") as f:
    f.write("\n".join(lines) + "\n")
