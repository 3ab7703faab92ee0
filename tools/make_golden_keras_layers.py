#!/usr/bin/env python3
"""Writes tests/golden/keras_layers_ref.npz: inputs and recorded results of the reference's own utils.apply_box_deltas, utils.non_max_suppression and
utils.generate_pyramid_anchors (deps/mask_rcnn/utils.py:151-172, 114-148, 553-570), executed as they lie.  CPU only; needs the reference tree and numpy:

    python tools/make_golden_keras_layers.py <reference tree>

utils.py is loaded by path with the empty stand-in modules of tools/make_golden_unmold.py (tensorflow, skimage and scipy.misc are never touched by the three
functions).  The fixture holds arrays only.  It pins the numpy statement of the Keras layers (tests/keras_layers_numpy.py) where executed reference code exists:
the graph functions apply_box_deltas_graph and tf.image.non_max_suppression have these numpy twins in the reference tree; TensorFlow itself is not available.

Cases.  Decode: random boxes and deltas, plus zero deltas, large and small scale deltas, zero-sized and flipped boxes.  Suppression: float boxes with ordered
corners and scores without ties at thresholds 0.3 and 0.7 -- clusters of overlapping boxes, zero-area boxes (lines and points, some of them identical), and boxes
that only touch along an edge or at a corner.  Anchors: the reference's ratios and anchor stride on a 64 x 64 image (feature maps 16, 8, 4, 2, 1)."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "keras_layers_ref.npz")
F = np.float32


def decode_cases(rng):
    n = 320
    y1, x1 = rng.uniform(-50, 900, n), rng.uniform(-50, 900, n)
    boxes = np.stack([y1, x1, y1 + rng.uniform(1, 400, n), x1 + rng.uniform(1, 400, n)], axis=1).astype(F)
    deltas = (rng.standard_normal((n, 4)) * np.asarray([0.3, 0.3, 0.5, 0.5])).astype(F)
    deltas[:16] = 0
    deltas[16:32, 2:] = rng.uniform(2, 6, (16, 2))          # large scales
    deltas[32:48, 2:] = rng.uniform(-8, -2, (16, 2))        # small scales
    boxes[48:56, 2:] = boxes[48:56, :2]                     # zero-sized
    boxes[56:64] = boxes[56:64][:, [2, 3, 0, 1]]            # flipped
    return boxes, deltas


def nms_cases(rng):
    centres = rng.uniform(20, 200, (24, 2))
    boxes = []
    for c in centres:                                       # clusters of overlapping boxes
        for _ in range(6):
            cy, cx = c + rng.uniform(-6, 6, 2)
            hh, ww = rng.uniform(8, 40, 2)
            boxes.append([cy - hh / 2, cx - ww / 2, cy + hh / 2, cx + ww / 2])
    for k in range(8):                                      # zero area: lines and points, pairs of identical ones
        y, x = 10.0 + 5 * (k // 2), 300.0
        boxes.append([y, x, y, x + (20.0 if k % 4 < 2 else 0.0)])
    for k in range(6):                                      # a row of boxes that only touch along an edge, and a diagonal that touches at corners
        boxes.append([400.0, 10.0 + 16 * k, 416.0, 26.0 + 16 * k])
        boxes.append([450.0 + 8 * k, 10.0 + 8 * k, 458.0 + 8 * k, 18.0 + 8 * k])
    boxes = np.asarray(boxes, F)
    n = boxes.shape[0]
    scores = ((rng.permutation(n) + 1) / (n + 1)).astype(F)     # no ties
    assert np.unique(scores).size == n and (boxes[:, 2] >= boxes[:, 0]).all() and (boxes[:, 3] >= boxes[:, 1]).all()
    return boxes, scores


def main():
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    from make_golden_unmold import load_utils

    utils = load_utils(sys.argv[1])
    rng = np.random.default_rng(20260117)
    out = {}
    boxes, deltas = decode_cases(rng)
    with np.errstate(over="ignore", invalid="ignore"):
        out["decode_boxes"], out["decode_deltas"], out["decode_out"] = boxes, deltas, np.asarray(utils.apply_box_deltas(boxes.copy(), deltas.copy()))
    boxes, scores = nms_cases(rng)
    out["nms_boxes"], out["nms_scores"] = boxes, scores
    for thr in (0.3, 0.7):
        with np.errstate(invalid="ignore", divide="ignore"):
            out[f"nms_pick_{int(thr * 10)}"] = np.asarray(utils.non_max_suppression(boxes.copy(), scores.copy(), thr), np.int64)
    scales, ratios, strides = (32, 64, 128, 256, 512), (0.5, 1, 2), (4, 8, 16, 32, 64)      # RPN_ANCHOR_SCALES, RPN_ANCHOR_RATIOS, BACKBONE_STRIDES (config.py)
    shapes = np.asarray([[int(np.ceil(64 / s)), int(np.ceil(64 / s))] for s in strides])
    out["anchor_scales"], out["anchor_ratios"], out["anchor_strides"], out["anchor_shapes"] = np.asarray(scales), np.asarray(ratios, np.float64), np.asarray(strides), shapes
    out["anchors"] = np.asarray(utils.generate_pyramid_anchors(scales, ratios, shapes, strides, 1))
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    np.savez_compressed(OUT, **out)
    print(f"wrote {OUT}: {os.path.getsize(OUT)} bytes; decode {out['decode_out'].shape} {out['decode_out'].dtype}, picks "
          f"{out['nms_pick_3'].size} / {out['nms_pick_7'].size} of {boxes.shape[0]}, anchors {out['anchors'].shape} {out['anchors'].dtype}")


if __name__ == "__main__":
    main()
