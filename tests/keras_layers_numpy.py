"""The Keras Mask R-CNN's proposal, pyramid ROI and detection layers in numpy, as include/ifx_c_api.h states them (ifx_keras_proposals, ifx_pyramid_roi_align,
ifx_keras_detections; k_kp_* / k_pyramid_roi_align / k_kd_* in csrc/ifx_detector.hip).

deps/mask_rcnn/model.py: ProposalLayer.call (:227-311), PyramidROIAlign.call (:323-424), refine_detections_graph (:670-771) with apply_box_deltas_graph (:185-206)
and clip_boxes_graph (:209-224).  Every f32 operation is rounded to f32, none is fused; EXP is rpn_proposals_numpy's.  What is pinned to EXECUTED reference code
(tests/test_keras_layers_cpu.py through tests/golden/keras_layers_ref.npz): the decode against utils.apply_box_deltas, the suppression against
utils.non_max_suppression, the level rule against the reference's own expression.  TensorFlow is not available and its kernels are not in the reference tree:
tf.image.non_max_suppression's corner ordering and area test, tf.image.crop_and_resize's sampling, tf.nn.top_k's tie rule and tf.round are stated here from
TensorFlow's documented behaviour and its CPU kernels' published source (non_max_suppression_op.cc, crop_and_resize_op.cc), not executed."""
import math

import numpy as np

from detector_ops_numpy import nms_order
from rpn_proposals_numpy import EXP

F = np.float32
STD_DEV = (0.1, 0.1, 0.2, 0.2)         # RPN_BBOX_STD_DEV and BBOX_STD_DEV, deps/mask_rcnn/config.py


def decode(boxes, deltas):
    """apply_box_deltas_graph, model.py:185-206, operation for operation: boxes [n,4] y1, x1, y2, x2; deltas [n,4] dy, dx, log(dh), log(dw) -> [n,4] f32"""
    b = np.ascontiguousarray(boxes, F).reshape(-1, 4)
    d = np.ascontiguousarray(deltas, F).reshape(-1, 4)
    half = F(0.5)
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        h = b[:, 2] - b[:, 0]                       # :194
        w = b[:, 3] - b[:, 1]
        cy = b[:, 0] + half * h
        cx = b[:, 1] + half * w
        cy = cy + d[:, 0] * h                       # :199 center_y += deltas[:, 0] * height
        cx = cx + d[:, 1] * w
        h = h * EXP(d[:, 2])                        # :201 height *= tf.exp(deltas[:, 2])
        w = w * EXP(d[:, 3])
        y1 = cy - half * h                          # :204
        x1 = cx - half * w
        y2 = y1 + h
        x2 = x1 + w
    out = np.stack([y1, x1, y2, x2], axis=1)
    assert out.dtype == F
    return out


def clip(v, lo, hi):
    """clip_boxes_graph's tf.maximum(tf.minimum(v, hi), lo), model.py:217-220; a NaN stays a NaN"""
    v = np.asarray(v, F)
    with np.errstate(invalid="ignore"):
        v = np.where(v > F(hi), F(hi), v)
        return np.where(v < F(lo), F(lo), v).astype(F)


def clip_boxes(boxes, window):
    wy1, wx1, wy2, wx2 = (F(v) for v in window)
    return np.stack([clip(boxes[:, 0], wy1, wy2), clip(boxes[:, 1], wx1, wx2), clip(boxes[:, 2], wy1, wy2), clip(boxes[:, 3], wx1, wx2)], axis=1)


def tf_iou_row(a, b):
    """tf.image.non_max_suppression's IoU (non_max_suppression_op.cc, IOU): box a [4] against boxes b [m,4], corners ordered first, an area <= 0 gives 0"""
    a = np.asarray(a, F)
    b = np.asarray(b, F).reshape(-1, 4)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        aymin, aymax, axmin, axmax = np.fmin(a[0], a[2]), np.fmax(a[0], a[2]), np.fmin(a[1], a[3]), np.fmax(a[1], a[3])
        bymin, bymax, bxmin, bxmax = np.fmin(b[:, 0], b[:, 2]), np.fmax(b[:, 0], b[:, 2]), np.fmin(b[:, 1], b[:, 3]), np.fmax(b[:, 1], b[:, 3])
        area_a = (aymax - aymin) * (axmax - axmin)
        area_b = (bymax - bymin) * (bxmax - bxmin)
        ih = np.fmax(np.fmin(aymax, bymax) - np.fmax(aymin, bymin), F(0))
        iw = np.fmax(np.fmin(axmax, bxmax) - np.fmax(axmin, bxmin), F(0))
        inter = ih * iw
        iou = inter / (area_a + area_b - inter)
        iou = np.where((area_a <= 0) | (area_b <= 0), F(0), iou)
    assert iou.dtype == F
    return iou


def tf_nms(boxes, threshold, limit):
    """boxes [n,4] ALREADY in descending score: the kept positions, in order, at most `limit` (iou > threshold suppresses, strictly; a NaN compares false)"""
    boxes = np.ascontiguousarray(boxes, F).reshape(-1, 4)
    n = boxes.shape[0]
    removed = np.zeros(n, bool)
    thr = F(threshold)
    kept = []
    for i in range(n):
        if removed[i]:
            continue
        kept.append(i)
        if len(kept) >= limit:
            break
        if i + 1 < n:
            with np.errstate(invalid="ignore"):
                removed[i + 1:] |= tf_iou_row(boxes[i], boxes[i + 1:]) > thr
    return np.asarray(kept, np.int64)


def keras_proposals(probs, bbox, anchors, image_shape, pre_nms_limit=6000, proposal_count=1000, nms_threshold=0.7, std_dev=STD_DEV):
    """ProposalLayer.call for one image: probs [n,2], bbox [n,4], anchors [n,4] pixels -> (proposals [c,4] normalised, index [c] int64)"""
    probs = np.ascontiguousarray(probs, F).reshape(-1, 2)
    bbox = np.ascontiguousarray(bbox, F).reshape(-1, 4)
    anchors = np.ascontiguousarray(anchors, F).reshape(-1, 4)
    ih, iw = F(image_shape[0]), F(image_shape[1])
    scores = probs[:, 1]                                                    # :254
    with np.errstate(invalid="ignore", over="ignore"):
        deltas = bbox * np.asarray(std_dev, F)[None, :]                     # :257
    K = min(int(pre_nms_limit), anchors.shape[0])                           # :263
    ix = nms_order(scores)[:K]                                              # :264 tf.nn.top_k: equal scores by ascending index
    boxes = decode(anchors[ix], deltas[ix])                                 # :276
    boxes = clip_boxes(boxes, (0, 0, ih, iw))                               # :282-287
    with np.errstate(invalid="ignore"):
        boxes = boxes / np.asarray([ih, iw, ih, iw], F)[None, :]            # :294
    assert boxes.dtype == F
    kept = tf_nms(boxes, nms_threshold, int(proposal_count))                # :298
    return boxes[kept], ix[kept].astype(np.int64)


def proposals_padded(result, proposal_count):
    """(proposals [P,4] with zero rows, index [P] with -1, count) as ifx_keras_proposals writes them"""
    boxes, index = result
    c = boxes.shape[0]
    pb = np.zeros((proposal_count, 4), F)
    pi = np.full(proposal_count, -1, np.int64)
    pb[:c] = boxes
    pi[:c] = index
    return pb, pi, c


def level_thresholds(image_h, image_w):
    """T0, T1, T2 of ifx_pyramid_level_thresholds: f64, rounded once to f32"""
    c = 224.0 / math.sqrt(float(image_h) * float(image_w))
    r2 = math.sqrt(2.0)
    return np.asarray([c * (r2 / 4.0), c * (r2 / 2.0), c * r2], np.float64).astype(F)


def levels(boxes, image_h, image_w):
    """boxes [..., 4] normalised -> int32 levels 2 .. 5: model.py:357-367 with round / clamp written as compares"""
    b = np.asarray(boxes, F)
    T = level_thresholds(image_h, image_w)
    with np.errstate(invalid="ignore", over="ignore"):
        s = np.sqrt((b[..., 2] - b[..., 0]) * (b[..., 3] - b[..., 1]))
        assert s.dtype == F
        return (2 + (s > T[0]).astype(np.int32) + (s >= T[1]).astype(np.int32) + (s > T[2]).astype(np.int32)).astype(np.int32)


def crop_axis(a1, a2, pool, size):
    """one axis of crop_and_resize_op.cc's bilinear sampling: (lo [pool] int, hi [pool] int, lerp [pool] f32, inside [pool] bool)"""
    a1, a2 = F(a1), F(a2)
    sm1 = F(size - 1)
    with np.errstate(invalid="ignore", over="ignore"):
        if pool > 1:
            scale = ((a2 - a1) * sm1) / F(pool - 1)
            pos = a1 * sm1 + np.arange(pool).astype(F) * scale
        else:
            pos = np.asarray([(F(0.5) * (a1 + a2)) * sm1], F)
        assert pos.dtype == F
        inside = (pos >= 0) & (pos <= sm1)              # a NaN is outside
        safe = np.where(inside, pos, F(0))
        top = np.floor(safe)
        lerp = safe - top
    return top.astype(np.int64), np.ceil(safe).astype(np.int64), lerp.astype(F), inside


def pyramid_roi_align(features, boxes, image_shape, pool_shape):
    """features: four arrays [B,H_l,W_l,C] (P2 .. P5); boxes [B,n,4] normalised -> (out [B,n,ph,pw,C] f32, levels [B,n] int32)"""
    features = [np.ascontiguousarray(f, F) for f in features]
    boxes = np.ascontiguousarray(boxes, F)
    B, n = boxes.shape[:2]
    ph, pw = int(pool_shape[0]), int(pool_shape[1])
    C = features[0].shape[3]
    lv = levels(boxes, image_shape[0], image_shape[1])
    out = np.zeros((B, n, ph, pw, C), F)
    for b in range(B):
        for r in range(n):
            f = features[lv[b, r] - 2][b]
            y1, x1, y2, x2 = boxes[b, r]
            ty, by, ly, iy = crop_axis(y1, y2, ph, f.shape[0])
            lx_, rx, lx, ix = crop_axis(x1, x2, pw, f.shape[1])
            tl, tr = f[ty[:, None], lx_[None, :]], f[ty[:, None], rx[None, :]]
            bl, br = f[by[:, None], lx_[None, :]], f[by[:, None], rx[None, :]]
            with np.errstate(invalid="ignore", over="ignore"):
                top = tl + (tr - tl) * lx[None, :, None]
                bot = bl + (br - bl) * lx[None, :, None]
                v = top + (bot - top) * ly[:, None, None]
            assert v.dtype == F
            out[b, r] = np.where((iy[:, None] & ix[None, :])[:, :, None], v, F(0))
    return out, lv


def first_max(probs):
    """best = 0; probs[j] > probs[best]: best = j -- class 0 when probs[0] is a NaN, else the lowest index of the largest number"""
    p = np.asarray(probs, F)
    nan = np.isnan(p)
    return np.where(nan[:, 0], 0, np.argmax(np.where(nan, -np.inf, p), axis=1)).astype(np.int32)


def keras_detections(rois, probs, deltas, window, image_shape, min_confidence=0.7, nms_threshold=0.3, max_instances=100, std_dev=STD_DEV):
    """refine_detections_graph for one image: rois [R,4], probs [R,C], deltas [R,C,4] -> (detections [c,6], boxes_norm [c,4], index [c] int64)"""
    rois = np.ascontiguousarray(rois, F).reshape(-1, 4)
    probs = np.ascontiguousarray(probs, F)
    R = probs.shape[0]
    deltas = np.ascontiguousarray(deltas, F).reshape(R, -1, 4)
    ih, iw = F(image_shape[0]), F(image_shape[1])
    rows = np.arange(R)
    class_ids = first_max(probs)                                            # :686
    class_scores = probs[rows, class_ids]                                   # :689
    with np.errstate(invalid="ignore", over="ignore"):
        specific = deltas[rows, class_ids] * np.asarray(std_dev, F)[None, :]    # :691-695
        refined = decode(rois, specific) * np.asarray([ih, iw, ih, iw], F)[None, :]   # :694-699
    refined = clip_boxes(refined, window)                                   # :701
    assert refined.dtype == F
    ok = ~np.isnan(refined).any(axis=1)                                     # to_int32 of a NaN has no defined value: the row is dropped
    boxes = np.zeros((R, 4), F)
    boxes[ok] = np.rint(refined[ok]).astype(np.int32).astype(F)             # :703, and tf.to_float where the boxes are used
    keep = ok & (class_ids > 0)                                             # :708
    if F(min_confidence) != 0:                                              # :710 `if config.DETECTION_MIN_CONFIDENCE:`
        with np.errstate(invalid="ignore"):
            keep &= class_scores >= F(min_confidence)
    keep = np.nonzero(keep)[0]
    nms_keep = []
    for c in np.unique(class_ids[keep]):                                    # :721-745
        ixs = keep[class_ids[keep] == c]
        order = ixs[nms_order(class_scores[ixs])]
        nms_keep.append(order[tf_nms(boxes[order], nms_threshold, int(max_instances))])
    nms_keep = np.sort(np.concatenate(nms_keep)) if nms_keep else np.zeros(0, np.int64)     # :750-752 (a subset of keep)
    top = nms_keep[nms_order(class_scores[nms_keep])][:int(max_instances)]  # :754-758 tf.nn.top_k
    det = np.concatenate([boxes[top], class_ids[top].astype(F)[:, None], class_scores[top][:, None]], axis=1).astype(F)    # :762-766
    norm = (boxes[top] / np.asarray([ih, iw, ih, iw], F)[None, :]).astype(F)                # :1961-1963
    return det, norm, top.astype(np.int64)


def detections_padded(result, max_instances):
    """(detections [M,6], boxes_norm [M,4] with zero rows, index [M] with -1, count) as ifx_keras_detections writes them"""
    det, norm, index = result
    c = det.shape[0]
    pd, pn, pi = np.zeros((max_instances, 6), F), np.zeros((max_instances, 4), F), np.full(max_instances, -1, np.int64)
    pd[:c] = det
    pn[:c] = norm
    pi[:c] = index
    return pd, pn, pi, c
