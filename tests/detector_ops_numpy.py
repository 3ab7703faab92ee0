"""The two detector operators in numpy, as include/ifx_c_api.h states them (ifx_roi_align_forward, ifx_nms; k_roi_align / k_nms_* in csrc/ifx_detector.hip).

roi_align_forward: maskrcnn-benchmark's RoIAlignForward (csrc/cuda/ROIAlign_cuda.cu:65-122 with bilinear_interpolate :16-62) in the operation order of
csrc/cpu/ROIAlign_cpu.cpp -- every operation rounded to f32, none fused.  nms: csrc/cuda/nms.cu (IoU strictly greater than the threshold), with an optional group
per box.  Both are held against the reference's CPU operators by tests/test_detector_ops_cpu.py through tests/golden/detector_ops_ref.npz."""
import numpy as np

F = np.float32


def _axis(start, bin_size, pooled, grid, size):
    """the samples of one axis: [pooled, grid] arrays low, high (int), l, h (f32 weights of high / low), valid"""
    p = np.arange(pooled, dtype=F)[:, None]
    i = np.arange(grid, dtype=F)[None, :]
    y = (start + p * bin_size) + ((i + F(0.5)) * bin_size) / F(grid)
    assert y.dtype == F
    with np.errstate(invalid="ignore"):
        valid = ~((y < F(-1.0)) | (y > F(size)))
    y = np.where(valid, y, F(0))
    y = np.where(y <= 0, F(0), y)
    lo = y.astype(np.int32)
    top = lo >= size - 1
    hi = np.where(top, size - 1, lo + 1)
    lo = np.where(top, size - 1, lo)
    y = np.where(top, lo.astype(F), y)
    l = y - lo.astype(F)
    h = F(1) - l
    return lo, hi, l.astype(F), h.astype(F), valid


def roi_align_forward(inp, rois, spatial_scale, pooled_h, pooled_w, sampling_ratio):
    """inp [B,C,H,W] f32, rois [n,5] f32 (batch index, x0, y0, x1, y1) -> [n,C,pooled_h,pooled_w] f32"""
    inp = np.ascontiguousarray(inp, F)
    rois = np.ascontiguousarray(rois, F).reshape(-1, 5)
    B, C, H, W = inp.shape
    scale = F(spatial_scale)
    out = np.zeros((rois.shape[0], C, pooled_h, pooled_w), F)
    for r in range(rois.shape[0]):
        b = rois[r, 0]
        if not (b > -1 and b < B):          # (int)b outside 0 .. B-1: zeros
            continue
        b = int(b)
        sw, sh, ew, eh = rois[r, 1] * scale, rois[r, 2] * scale, rois[r, 3] * scale, rois[r, 4] * scale
        rw, rh = np.maximum(ew - sw, F(1)), np.maximum(eh - sh, F(1))
        bh, bw = rh / F(pooled_h), rw / F(pooled_w)
        gh = sampling_ratio if sampling_ratio > 0 else int(np.ceil(rh / F(pooled_h)))
        gw = sampling_ratio if sampling_ratio > 0 else int(np.ceil(rw / F(pooled_w)))
        yl, yh, ly, hy, vy = _axis(sh, bh, pooled_h, gh, H)
        xl, xh, lx, hx, vx = _axis(sw, bw, pooled_w, gw, W)
        Y = lambda a: a[:, :, None, None]
        X = lambda a: a[None, None, :, :]
        w1, w2, w3, w4 = Y(hy) * X(hx), Y(hy) * X(lx), Y(ly) * X(hx), Y(ly) * X(lx)
        img = inp[b]
        v1, v2, v3, v4 = img[:, Y(yl), X(xl)], img[:, Y(yl), X(xh)], img[:, Y(yh), X(xl)], img[:, Y(yh), X(xh)]
        val = ((w1 * v1 + w2 * v2) + w3 * v3) + w4 * v4          # [C, ph, gh, pw, gw]
        val = np.where(Y(vy) & X(vx), val, F(0))
        assert val.dtype == F
        acc = np.zeros((C, pooled_h, pooled_w), F)
        for iy in range(gh):
            for ix in range(gw):
                acc = acc + val[:, :, iy, :, ix]
        out[r] = acc / F(gh * gw)
    return out


def nms_order(scores):
    """descending score, equal scores by ascending index, NaN behind every number"""
    s = np.asarray(scores, F).reshape(-1)
    nan = np.isnan(s)
    return np.lexsort((np.arange(s.size), np.where(nan, F(0), -s), nan))


def iou_row(a, b):
    """f32 IoU of box a [4] against boxes b [m,4], nms.cu:15-24 (max / min as fmaxf / fminf)"""
    a = np.asarray(a, F)
    b = np.asarray(b, F).reshape(-1, 4)
    one = F(1)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        w = np.fmax(np.fmin(a[2], b[:, 2]) - np.fmax(a[0], b[:, 0]) + one, F(0))
        h = np.fmax(np.fmin(a[3], b[:, 3]) - np.fmax(a[1], b[:, 1]) + one, F(0))
        inter = w * h
        sa = (a[2] - a[0] + one) * (a[3] - a[1] + one)
        sb = (b[:, 2] - b[:, 0] + one) * (b[:, 3] - b[:, 1] + one)
        r = inter / (sa + sb - inter)
    assert r.dtype == F
    return r


def nms(boxes, scores, threshold, groups=None):
    """the kept indices, ascending (int64).  groups: a box suppresses only boxes of its own group."""
    boxes = np.ascontiguousarray(boxes, F).reshape(-1, 4)
    n = boxes.shape[0]
    order = nms_order(scores)
    assert order.size == n
    sb = boxes[order]
    sg = None if groups is None else np.asarray(groups, np.int32).reshape(-1)[order]
    removed = np.zeros(n, bool)
    thr = F(threshold)
    kept = []
    for i in range(n):
        if removed[i]:
            continue
        kept.append(i)
        if i + 1 < n:
            with np.errstate(invalid="ignore"):
                over = iou_row(sb[i], sb[i + 1:]) > thr
            if sg is not None:
                over &= sg[i + 1:] == sg[i]
            removed[i + 1:] |= over
    return np.sort(order[np.asarray(kept, np.int64)]).astype(np.int64)


def pairs_at_threshold(boxes, threshold):
    """how many pairs have an IoU exactly equal to the threshold: where nms_cpu.cpp (>=) and nms.cu (>) part"""
    boxes = np.ascontiguousarray(boxes, F).reshape(-1, 4)
    return int(sum(int((iou_row(boxes[i], boxes[i + 1:]) == F(threshold)).sum()) for i in range(boxes.shape[0] - 1)))
