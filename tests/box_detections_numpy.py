"""The box head's post-processing of one image in numpy, as include/ifx_c_api.h states it (ifx_box_detections; k_bd_* in csrc/ifx_detector.hip).

maskrcnn-benchmark's PostProcessor (modeling/roi_heads/box_head/inference.py:43-146): softmax with the sum in f64 in ascending class order, the threshold, BoxCoder.decode
and clip_to_image per candidate (rpn_proposals_numpy.box_decode), the per-class suppression as one grouped ifx_nms (detector_ops_numpy.nms), the limit to
detections_per_img by the M-th largest kept score with every tie kept.  Held against the reference's own Python by tests/test_box_detections_cpu.py through
tests/golden/box_detections_ref.npz."""
import numpy as np

from detector_ops_numpy import iou_row, nms, nms_order
from rpn_proposals_numpy import EXP, box_decode

F = np.float32
D = np.float64
CAP = 8192


def softmax_parts(logits):
    """logits [R,C] -> (d [R,C] f32 = x - max, e [R,C] f32 = EXP(d), bad [R]: a NaN in the row or a maximum that is not finite)"""
    x = np.ascontiguousarray(logits, F)
    assert x.ndim == 2
    with np.errstate(invalid="ignore"):
        nan = np.isnan(x).any(axis=1)
        m = np.where(nan, F(0), np.max(np.where(np.isnan(x), F(0), x), axis=1, initial=-np.inf)).astype(F)
        bad = nan | ~np.isfinite(m)
        d = x - np.where(bad, F(0), m)[:, None]
    d = np.where(bad[:, None], F(0), d).astype(F)
    return d, EXP(d), bad


def softmax(logits):
    """F.softmax(logits, -1) by the rule: p = f32(f64(e) / s), s the f64 sum of e with j ascending; a bad row is all NaN"""
    d, e, bad = softmax_parts(logits)
    s = np.zeros(e.shape[0], D)
    for j in range(e.shape[1]):
        s = s + e[:, j].astype(D)
    with np.errstate(invalid="ignore", divide="ignore"):
        p = (e.astype(D) / s[:, None]).astype(F)
    p[bad] = np.nan
    return p


def candidates(logits, regression, proposals, image_size, score_thresh, weights=(10, 10, 5, 5), xform_clip=None):
    """class-major, row ascending within a class: (boxes [K,4], scores [K], labels [K] int64, index [K] int64)"""
    p = softmax(logits)
    R, C = p.shape
    regression = np.ascontiguousarray(regression, F)
    creg = regression.shape[-1] // 4 if regression.ndim == 2 else regression.size // max(4 * R, 1)
    regression = regression.reshape(R, 4 * creg)
    assert creg in (1, C)
    with np.errstate(invalid="ignore"):
        hit = p[:, 1:] > F(score_thresh)                                  # [R, C-1]; a NaN compares false
    j, r = np.nonzero(hit.T)                                              # class-major
    labels = (j + 1).astype(np.int64)
    index = r.astype(np.int64)
    dec = box_decode(regression, np.ascontiguousarray(proposals, F).reshape(R, 4), weights, clip_to=image_size, xform_clip=xform_clip).reshape(R, creg, 4)
    boxes = dec[index, labels if creg == C else 0]
    return boxes.reshape(-1, 4), p[index, labels], labels, index


def limit_threshold(kept_scores, M):
    """the M-th largest of the kept scores when there are more than M > 0 of them, else None"""
    if M <= 0 or kept_scores.size <= M:
        return None
    return kept_scores[nms_order(kept_scores)[M - 1]]


def box_detections(logits, regression, proposals, image_size, score_thresh=0.05, nms_thresh=0.5, detections_per_img=100, weights=(10, 10, 5, 5), xform_clip=None):
    """-> (boxes [c,4] f32, scores [c] f32, labels [c] int64, index [c] int64, K, D); K > 8192: (empty ..., K, 0) and the count of the call is -1"""
    boxes, scores, labels, index = candidates(logits, regression, proposals, image_size, score_thresh, weights, xform_clip)
    K = int(scores.size)
    if K > CAP:
        return boxes[:0], scores[:0], labels[:0], index[:0], K, 0
    keep = nms(boxes, scores, nms_thresh, labels.astype(np.int32)) if K else np.zeros(0, np.int64)
    Dk = int(keep.size)
    t = limit_threshold(scores[keep], int(detections_per_img))
    if t is not None:
        keep = keep[scores[keep] >= t]
    return boxes[keep], scores[keep], labels[keep], index[keep], K, Dk


def padded(result, max_out):
    """the device's uncut form: (boxes [max_out,4], scores, labels, index, count, stats [2]); zeros and -1 behind the count, count -1 above the cap"""
    boxes, scores, labels, index, K, Dk = result
    c = boxes.shape[0]
    w = min(c, max_out)
    pb, ps = np.zeros((max_out, 4), F), np.zeros(max_out, F)
    pl, pi = np.full(max_out, -1, np.int64), np.full(max_out, -1, np.int64)
    pb[:w], ps[:w], pl[:w], pi[:w] = boxes[:w], scores[:w], labels[:w], index[:w]
    return pb, ps, pl, pi, (-1 if K > CAP else c), np.asarray([K, Dk], np.int32)


def softmax_true(logits):
    """f64: exp(d_j) / sum exp(d_i) from the f32 d_j -- what the statement's and torch's probabilities are measured against"""
    d, _, bad = softmax_parts(logits)
    ex = np.exp(d.astype(D))
    p = ex / ex.sum(axis=1, keepdims=True)
    p[bad] = np.nan
    return p


def ulp_distance(p32, true64):
    """|p32 - true| in units of the f32 spacing at |true|"""
    true64 = np.asarray(true64, D)
    unit = np.spacing(np.abs(true64).astype(F)).astype(D)
    return np.abs(np.asarray(p32, F).astype(D) - true64) / unit


def near(values, target, ulps=16):
    """how many f32 values lie within `ulps` spacings of target"""
    v = np.asarray(values, F).astype(D)
    return int((np.abs(v - D(F(target))) <= ulps * np.spacing(np.maximum(np.abs(v), abs(D(F(target)))).astype(F)).astype(D)).sum())


def close_scores(scores, ulps=16):
    """how many neighbouring pairs of the sorted scores lie within `ulps` spacings of each other"""
    s = np.sort(np.asarray(scores, F)).astype(D)
    if s.size < 2:
        return 0
    return int((np.diff(s) <= ulps * np.spacing(s[1:].astype(F)).astype(D)).sum())


def near_threshold(boxes, labels, threshold, eps=1e-5):
    """how many same-class pairs of candidates have an IoU within eps of the threshold"""
    t = 0
    for i in range(boxes.shape[0] - 1):
        with np.errstate(invalid="ignore"):
            iou = iou_row(boxes[i], boxes[i + 1:]).astype(D)
        t += int(((np.abs(iou - D(F(threshold))) <= eps) & (labels[i + 1:] == labels[i])).sum())
    return t
