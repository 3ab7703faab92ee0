"""The RPN's proposal stage of one level of one image and the box decoding in it, in numpy, as include/ifx_c_api.h states them (ifx_rpn_proposals, ifx_box_decode;
k_rpn_* / k_box_decode in csrc/ifx_detector.hip).

maskrcnn-benchmark's RPNPostProcessor.forward_for_single_feature_map (modeling/rpn/inference.py:74-121): order by logit, BoxCoder.decode (modeling/box_coder.py:
52-95) with the exponential EXP spelt out in f64, clip_to_image (structures/bounding_box.py:214-219), remove_small_boxes and boxlist_nms (structures/boxlist_ops.py)
-- every f32 operation rounded to f32, none fused.  Suppression is detector_ops_numpy's.  Held against the reference's own Python by
tests/test_rpn_proposals_cpu.py through tests/golden/rpn_proposals_ref.npz."""
import math

import numpy as np

from detector_ops_numpy import iou_row, nms_order

F = np.float32
D = np.float64
XFORM_CLIP = F(math.log(1000.0 / 16))
LOG2E, LN2_HI, LN2_LO = D(1.4426950408889634), D(6.93147180369123816490e-01), D(1.90821492927058770002e-10)
COEFF = [D(1.0) / D(math.factorial(i)) for i in range(14)]


def EXP(x):
    """f32 -> f32: 2^k * (the Taylor sum to r^13 of the reduced argument), in f64 operations in this order, then one rounding to f32"""
    x = np.asarray(x, F)
    nan = np.isnan(x)
    v = np.clip(np.where(nan, F(0), x).astype(D), D(-104.0), D(90.0))
    k = np.rint(v * LOG2E)
    r = (v - k * LN2_HI) - k * LN2_LO
    p = np.full(v.shape, COEFF[13], D)
    for i in range(12, -1, -1):
        p = p * r + COEFF[i]
    with np.errstate(over="ignore", under="ignore"):
        out = np.ldexp(p, k.astype(np.int32)).astype(F)
    return np.where(nan, x, out)


def decode_parts(codes, boxes, weights=(1, 1, 1, 1), xform_clip=None):
    """codes [n,4k], boxes [n,4] -> pcx, pcy, pw, ph [n,k] (f32)"""
    codes = np.ascontiguousarray(codes, F)
    boxes = np.ascontiguousarray(boxes, F).reshape(-1, 4)
    if codes.ndim != 2:
        codes = codes.reshape(boxes.shape[0], -1)
    wx, wy, ww, wh = (F(v) for v in weights)
    clip = XFORM_CLIP if xform_clip is None or not xform_clip > 0 else F(xform_clip)
    half, one = F(0.5), F(1)
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        w = (boxes[:, 2] - boxes[:, 0] + one)[:, None]
        h = (boxes[:, 3] - boxes[:, 1] + one)[:, None]
        cx = boxes[:, 0][:, None] + half * w
        cy = boxes[:, 1][:, None] + half * h
        dx, dy, dw, dh = codes[:, 0::4] / wx, codes[:, 1::4] / wy, codes[:, 2::4] / ww, codes[:, 3::4] / wh
        dw = np.where(dw > clip, clip, dw)                # min with the clip; a NaN stays
        dh = np.where(dh > clip, clip, dh)
        pcx, pcy = dx * w + cx, dy * h + cy
        pw, ph = EXP(dw) * w, EXP(dh) * h
    for a in (pcx, pcy, pw, ph):
        assert a.dtype == F
    return pcx, pcy, pw, ph


def box_decode(codes, boxes, weights=(1, 1, 1, 1), clip_to=None, xform_clip=None):
    """BoxCoder.decode: codes [n,4k] against boxes [n,4] -> [n,4k]; clip_to (width, height): clip_to_image on top"""
    pcx, pcy, pw, ph = decode_parts(codes, boxes, weights, xform_clip)
    half, one = F(0.5), F(1)
    out = np.zeros((pcx.shape[0], 4 * pcx.shape[1]), F)
    with np.errstate(invalid="ignore", over="ignore"):
        out[:, 0::4] = pcx - half * pw
        out[:, 1::4] = pcy - half * ph
        out[:, 2::4] = pcx + half * pw - one
        out[:, 3::4] = pcy + half * ph - one
    if clip_to is not None:
        for c, hi in ((0, clip_to[0]), (1, clip_to[1]), (2, clip_to[0]), (3, clip_to[1])):
            v = out[:, c::4]
            with np.errstate(invalid="ignore"):
                out[:, c::4] = np.where(v < 0, F(0), np.where(v > F(hi - 1), F(hi - 1), v))      # a NaN stays
    return out


def flatten(objectness, regression):
    """permute_and_flatten: [A,H,W], [4A,H,W] -> logits [H W A], codes [H W A, 4], row i = (y W + x) A + a"""
    objectness = np.asarray(objectness, F)
    A, H, W = objectness.shape
    regression = np.asarray(regression, F).reshape(A, 4, H, W)
    return np.ascontiguousarray(objectness.transpose(1, 2, 0)).reshape(-1), np.ascontiguousarray(regression.transpose(2, 3, 0, 1)).reshape(-1, 4)


def candidates(objectness, regression, anchors, image_size, pre_nms_top_n, min_size=0, weights=(1, 1, 1, 1)):
    """the survivors in front of the suppression, in the candidates' order: (boxes [s,4], logits [s], index [s] int64)"""
    logits, codes = flatten(objectness, regression)
    anchors = np.ascontiguousarray(anchors, F).reshape(-1, 4)
    n = logits.size
    assert anchors.shape[0] == n
    top = nms_order(logits)[:min(int(pre_nms_top_n), n)]
    boxes = box_decode(codes[top], anchors[top], weights, clip_to=image_size)
    with np.errstate(invalid="ignore"):
        keep = (boxes[:, 2] - boxes[:, 0] + F(1) >= F(min_size)) & (boxes[:, 3] - boxes[:, 1] + F(1) >= F(min_size))
    return boxes[keep], logits[top][keep], top[keep].astype(np.int64)


def suppress(boxes, threshold, limit):
    """ifx_nms's rule on boxes already in their order: the positions of the first `limit` kept"""
    n = boxes.shape[0]
    removed = np.zeros(n, bool)
    kept = []
    for i in range(n):
        if removed[i]:
            continue
        kept.append(i)
        if len(kept) == limit:
            break
        if i + 1 < n:
            with np.errstate(invalid="ignore"):
                removed[i + 1:] |= iou_row(boxes[i], boxes[i + 1:]) > F(threshold)
    return np.asarray(kept, np.int64)


def rpn_proposals(objectness, regression, anchors, image_size, pre_nms_top_n, post_nms_top_n, nms_thresh, min_size=0, weights=(1, 1, 1, 1)):
    """-> (boxes [c,4] f32, logits [c] f32, index [c] int64): the proposals, best first"""
    boxes, logits, index = candidates(objectness, regression, anchors, image_size, pre_nms_top_n, min_size, weights)
    keep = suppress(boxes, nms_thresh, int(post_nms_top_n))
    return boxes[keep], logits[keep], index[keep]


def padded(result, post_nms_top_n):
    """the device's uncut form: zeros and -1 behind the count"""
    boxes, logits, index = result
    c = boxes.shape[0]
    pb, pl, pi = np.zeros((post_nms_top_n, 4), F), np.zeros(post_nms_top_n, F), np.full(post_nms_top_n, -1, np.int64)
    pb[:c], pl[:c], pi[:c] = boxes, logits, index
    return pb, pl, pi, c


def near_threshold(boxes, threshold, eps=1e-5):
    """how many pairs of the (ordered) survivors have an IoU within eps of the threshold"""
    t = 0
    for i in range(boxes.shape[0] - 1):
        with np.errstate(invalid="ignore"):
            t += int((np.abs(iou_row(boxes[i], boxes[i + 1:]).astype(D) - D(F(threshold))) <= eps).sum())
    return t


def exp_sweep():
    """the fixed arguments EXP is held to exp on: a dense sweep of its whole clamped range, and the clip value"""
    return np.concatenate([np.linspace(-104.0, 90.0, 1940001).astype(F), np.asarray([XFORM_CLIP], F)])


def coordinate_ulp(codes, boxes, weights=(1, 1, 1, 1)):
    """per decoded box [n,k]: one f32 ulp of the largest magnitude among pcx, pcy, pw, ph -- the unit of the bound the golden comparison uses"""
    parts = np.stack([np.abs(p) for p in decode_parts(codes, boxes, weights)])
    return np.spacing(np.nanmax(parts, axis=0).astype(F))
