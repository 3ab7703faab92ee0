"""The stretch between the mask head's last convolution and the ROI paste, in numpy, as include/ifx_c_api.h states it (ifx_mask_head_select; k_mh_select /
k_mh_sigmoid in csrc/ifx_detector.hip).

maskrcnn-benchmark's MaskPostProcessor.forward (modeling/roi_heads/mask_head/inference.py:27-61), BoxList.resize (structures/bounding_box.py:91-127) and
COCODemo.select_top_predictions (demo/predictor.py:224-243): which rows are kept, their order, the resized boxes, the class ids and the sigmoid of each kept row's own
channel -- every f32 operation rounded to f32, none fused, the exponential rpn_proposals_numpy's EXP.  Held against the reference's own Python by
tests/test_mask_head_cpu.py through tests/golden/mask_head_ref.npz."""
import os

import numpy as np

from detector_ops_numpy import nms_order
from rpn_proposals_numpy import EXP

F = np.float32
MAX_R, MAX_C, MAX_M = 1024, 1024, 64
PASTE_BAND = 2.0 ** -22       # the ROI paste's own tie band (roi_paste_numpy.BAND)


def sigmoid(x):
    """SIGMOID of the rule: e = EXP(-x), d = 1 + e, p = 1 / d, each rounded to f32; a NaN gives a NaN"""
    x = np.asarray(x, F)
    with np.errstate(over="ignore", invalid="ignore"):
        e = EXP(-x)
        d = F(1.0) + e
        p = F(1.0) / d
    assert p.dtype == F
    return p


def valid_rows(R, count):
    """the first min(max(count, 0), R) rows; None: all R"""
    return R if count is None else min(max(int(count), 0), R)


def kept_rows(scores, labels, C, score_thresh=0.7, sort_by_score=True, count=None):
    """The input rows the rule keeps, in its order (int32)."""
    s = np.asarray(scores, F).reshape(-1)
    lab = np.asarray(labels, np.int64).reshape(-1)
    t = F(score_thresh)
    assert not np.isnan(t), "a NaN score_thresh is refused"
    R = s.size
    with np.errstate(invalid="ignore"):
        keep = (np.full(R, True) if t == F(-np.inf) else s > t) & (lab >= 0) & (lab < C) & (np.arange(R) < valid_rows(R, count))
    rows = np.nonzero(keep)[0]
    if sort_by_score:
        rows = rows[nms_order(s[rows])]       # (rows ascend: equal scores by ascending row)
    return rows.astype(np.int32)


def ratios(in_size, out_size):
    return F(float(out_size[0]) / float(in_size[0])), F(float(out_size[1]) / float(in_size[1]))


def resize_boxes(boxes, in_size, out_size):
    b = np.asarray(boxes, F).reshape(-1, 4)
    rw, rh = ratios(in_size, out_size)
    with np.errstate(invalid="ignore", over="ignore"):
        out = b * np.array([rw, rh, rw, rh], F)
    assert out.dtype == F
    return out


def stage_outputs(own_logits, boxes, labels, rows, in_size, out_size, class_map=None):
    """The stage's outputs for the kept rows `rows`: own_logits [k,M,M] is each kept row's own channel, boxes [R,4] and labels [R] are the call's inputs"""
    own = np.asarray(own_logits, F)
    lab = np.asarray(labels, np.int64).reshape(-1)
    masks = sigmoid(own).reshape(len(rows), own.shape[-1], own.shape[-1])
    out_boxes = resize_boxes(np.asarray(boxes, F).reshape(-1, 4)[rows], in_size, out_size)
    cls = lab[rows] if class_map is None else np.asarray(class_map, np.int32).reshape(-1)[lab[rows]]
    return masks, out_boxes, cls.astype(np.int32), np.asarray(rows, np.int32)


def mask_head_select(logits, boxes, scores, labels, in_size, out_size, score_thresh=0.7, sort_by_score=True, count=None, class_map=None):
    """(roi_masks [k,M,M] f32, boxes [k,4] f32, class_ids [k] int32, rows [k] int32) of logits [R,C,M,M], boxes [R,4], scores [R], labels [R]"""
    x = np.asarray(logits, F)
    R, C, M = x.shape[0], x.shape[1], x.shape[3]
    assert x.shape == (R, C, M, M) and 1 <= M <= MAX_M and 1 <= C <= MAX_C and R <= MAX_R
    assert min(*in_size, *out_size) >= 1
    lab = np.asarray(labels, np.int64).reshape(-1)
    rows = kept_rows(scores, lab, C, score_thresh, sort_by_score, count)
    return stage_outputs(x[rows, lab[rows]], boxes, lab, rows, in_size, out_size, class_map)


def padded(result, R):
    """The device entry's R-row outputs: zeros in masks and boxes, -1 in class ids and rows behind kept; (masks, boxes, class_ids, rows, kept [1] int32)"""
    masks, boxes, cls, rows = result
    k, M = len(rows), masks.shape[-1]
    pm = np.zeros((R, M, M), F); pm[:k] = masks
    pb = np.zeros((R, 4), F); pb[:k] = boxes
    pc = np.full(R, -1, np.int32); pc[:k] = cls
    pr = np.full(R, -1, np.int32); pr[:k] = rows
    return pm, pb, pc, pr, np.asarray([k], np.int32)


# ---- the fixture of tools/make_golden_mask_head.py

def fixture_logits(q_label, labels, C):
    """The [R,C,M,M] logits of a fixture case from the stored bytes of each row's own channel: channel c of row r holds the bytes (q + 37 (c - label)) mod 256, so
    the label's channel is q itself and the others are there to be thrown away; logit = (byte - 128) / 16."""
    q = np.asarray(q_label, np.uint8)
    R, M = q.shape[0], q.shape[-1]
    lab = np.asarray(labels, np.int64).reshape(R)
    shift = (37 * (np.arange(C)[None, :] - lab[:, None])) % 256
    full = (q.astype(np.int64)[:, None] + shift[:, :, None, None]) % 256
    return ((full - 128).astype(F) / F(16.0)).astype(F)


def load_fixture():
    """The cases of tests/golden/mask_head_ref.npz: dicts of R, C, M, W, H, in_size, q (u8 [R,M,M]), logits (f32 [R,C,M,M]), boxes, scores, labels, and the
    reference's results: ref_rows (int32 [k], in its order), ref_boxes (f32 [k,4]), ref_masks (bool [k,H,W]); plus the measured sigmoid difference."""
    d = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "mask_head_ref.npz"))
    cases, qo, ro, ko, bo = [], 0, 0, 0, 0
    for i in range(len(d["r"])):
        R, C, M, W, H = (int(d[k][i]) for k in ("r", "c", "m", "w", "h"))
        k = int(d["kept"][i])
        q = d["q"][qo:qo + R * M * M].reshape(R, M, M); qo += R * M * M
        labels = d["labels"][ro:ro + R].astype(np.int64)
        nb = (W * H + 7) // 8
        ref_masks = np.stack([np.unpackbits(d["ref_bits"][bo + j * nb:bo + (j + 1) * nb])[:W * H].reshape(H, W).astype(bool) for j in range(k)]) if k else np.zeros((0, H, W), bool)
        cases.append(dict(R=R, C=C, M=M, W=W, H=H, in_size=(int(d["in_w"][i]), int(d["in_h"][i])), q=q, logits=fixture_logits(q, labels, C),
                          boxes=d["boxes"][ro:ro + R].astype(F), scores=d["scores"][ro:ro + R].astype(F), labels=labels,
                          ref_rows=d["ref_rows"][ko:ko + k].astype(np.int32), ref_boxes=d["ref_boxes"][ko:ko + k].astype(F), ref_masks=ref_masks))
        ro += R; ko += k; bo += k * nb
    assert qo == len(d["q"]) and ro == len(d["labels"]) and ko == len(d["ref_rows"]) and bo == len(d["ref_bits"])
    return cases, dict(sigmoid_max_abs=float(d["sigmoid_max_abs"]), sigmoid_max_ulp=float(d["sigmoid_max_ulp"]))
