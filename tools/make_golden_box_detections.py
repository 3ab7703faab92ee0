#!/usr/bin/env python3
"""Writes tests/golden/box_detections_ref.npz: what maskrcnn-benchmark's own Python gives for the box head's post-processing on small inputs.

    python tools/make_golden_box_detections.py /path/to/maskrcnn-benchmark-master

The reference is put on sys.path and runs on the CPU: PostProcessor.forward (maskrcnn_benchmark/modeling/roi_heads/box_head/inference.py:43-146).  Its extension
module maskrcnn_benchmark._C is an object whose `nms` is the reference's csrc/cpu/nms_cpu.cpp, compiled as a throw-away extension exactly as
tools/make_golden_detector_ops.py does: nothing compiled is kept and none of the reference's text is in this repository.  The file holds inputs and outputs only.
Cases: C = 2 / 3 / 81 classes, R from 1 to 300 rows (C = 81: at most 24, for the file's size), the weights (10, 10, 5, 5) and (1, 1, 1, 1), score_thresh 0.05 / 0.3,
nms 0.5 / 0.3, detections_per_img 100 / 5 / 0, one cls_agnostic case, images that clip some boxes, codes beyond the clip, logits scaled so that some cases keep more
than the limit and some fewer, proposals in clusters so that boxes of a class suppress each other.
The reference's order is not defined on ties and its softmax differs from the rule in the last bits, so a case is drawn again when, by the numpy statement
(tests/box_detections_numpy.py), a probability lies within 16 ulp of score_thresh, two candidate scores lie within 16 ulp of each other, or a same-class pair of
candidates has an IoU within 1e-5 of the threshold; the number of redraws is stored.  Before writing, the statement is held to every stored figure: equal count,
equal labels and proposal rows in equal order, every coordinate within 2 ulp of the largest magnitude among the box's pcx, pcy, pw, ph (the unit of
tools/make_golden_rpn_proposals.py), and every probability of the statement within 3 ulp of exp(d_j) / sum exp(d_i) evaluated in f64 from the f32 d_j -- one
rounding each from EXP, from the sum and from the conversion.  The worst distances of the statement and of torch's softmax to that value, and of the two to each
other, are stored."""
import os
import sys
import tempfile
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
OUT = os.path.join(ROOT, "tests", "golden", "box_detections_ref.npz")

CASES = 40
AGNOSTIC = 7


def det_case(rng, k):
    C = (2, 3, 81)[k % 3]
    R = int(rng.integers(1, 25 if C == 81 else 301))
    if k == 0:
        R = 1
    if k == 4:
        R = 300
    weights = ((10.0, 10.0, 5.0, 5.0), (1.0, 1.0, 1.0, 1.0))[(k // 3) % 2]
    score_thresh = (0.05, 0.3)[(k // 6) % 2]
    nms = (0.5, 0.3)[(k // 2) % 2]
    M = (100, 5, 0)[(k // 3) % 3]
    creg = 1 if k == AGNOSTIC else C
    image = (int(rng.integers(120, 400)), int(rng.integers(90, 300)))                                   # (width, height)
    clusters = int(rng.integers(R // 8 + 1, R // 2 + 2))
    ctr = rng.uniform(0, 1, (clusters, 2)) * np.asarray(image) * 1.1 - 0.05 * np.asarray(image)       # some clusters hang over the border
    size = rng.uniform(16, 120, (clusters, 2))
    which = rng.integers(0, clusters, R)
    c = ctr[which] + rng.normal(0, 4, (R, 2))
    s = size[which] * rng.uniform(0.85, 1.15, (R, 2))
    proposals = np.concatenate([c - s / 2, c + s / 2], axis=1).astype(np.float32)
    logits = (rng.standard_normal((R, C)) * (0.5, 1.5, 3.0)[(k // 9) % 3]).astype(np.float32)
    reg = rng.standard_normal((R, creg, 4)) * 0.25
    reg[..., 2:][rng.random((R, creg, 2)) < 0.05] = 7.0                                                # beyond the clip at either weight set
    reg = (reg * np.asarray(weights)).reshape(R, 4 * creg).astype(np.float32)
    return logits, reg, proposals, image, score_thresh, nms, M, weights


def main():
    import torch

    import box_detections_numpy as bd
    import rpn_proposals_numpy as rp
    from make_golden_detector_ops import load_reference

    if len(sys.argv) != 2:
        sys.exit(__doc__)
    rng = np.random.default_rng(20261019)
    data = {}
    with tempfile.TemporaryDirectory() as tmp:
        assert not os.path.abspath(tmp).startswith(ROOT + os.sep)
        ext = load_reference(os.path.join(sys.argv[1], "maskrcnn_benchmark"), tmp)
        sys.path.insert(0, sys.argv[1])
        stub = types.ModuleType("maskrcnn_benchmark._C")
        stub.nms = ext.nms
        sys.modules["maskrcnn_benchmark._C"] = stub
        from maskrcnn_benchmark.modeling.box_coder import BoxCoder
        from maskrcnn_benchmark.modeling.roi_heads.box_head.inference import PostProcessor
        from maskrcnn_benchmark.structures.bounding_box import BoxList

        worst_box, worst = 0.0, np.zeros(3)
        detections, redrawn, above, below, clipped, suppressed = 0, 0, 0, 0, 0, 0
        for k in range(CASES):
            while True:
                logits, reg, proposals, image, score_thresh, nms, M, weights = det_case(rng, k)
                p = bd.softmax(logits)
                cb, cs, cl, ci = bd.candidates(logits, reg, proposals, image, score_thresh, weights)
                tp = torch.nn.functional.softmax(torch.from_numpy(logits), -1).numpy().astype(np.float32)
                pos = {(j, tp[r, j].tobytes()): r for r in range(tp.shape[0]) for j in range(1, tp.shape[1]) if tp[r, j] > score_thresh}
                distinct = len(pos) == int((tp[:, 1:] > score_thresh).sum())                           # (within a class: the row of every detection)
                if distinct and bd.near(p, score_thresh) == 0 and bd.close_scores(cs) == 0 and bd.near_threshold(cb, cl, nms) == 0:
                    break
                redrawn += 1
            sel = PostProcessor(score_thresh, nms, M, BoxCoder(weights=weights), cls_agnostic_bbox_reg=reg.shape[1] == 4)
            with torch.no_grad():
                res = sel.forward((torch.from_numpy(logits), torch.from_numpy(reg)), [BoxList(torch.from_numpy(proposals.copy()), image, mode="xyxy")])[0]
            ref_boxes = res.bbox.numpy().astype(np.float32).reshape(-1, 4)
            ref_score, ref_label = res.get_field("scores").numpy().astype(np.float32), res.get_field("labels").numpy().astype(np.int64)
            ref_index = np.asarray([pos[(int(j), v.tobytes())] for j, v in zip(ref_label, ref_score)], np.int64)
            boxes, scores, labels, index, K, Dk = bd.box_detections(logits, reg, proposals, image, score_thresh, nms, M, weights)
            assert boxes.shape == ref_boxes.shape and np.array_equal(labels, ref_label) and np.array_equal(index, ref_index), (k, boxes.shape, ref_boxes.shape)
            if index.size:
                creg = reg.shape[1] // 4
                codes = reg.reshape(-1, creg, 4)[index, labels if creg > 1 else 0]
                unit = rp.coordinate_ulp(codes, proposals[index], weights)                               # [c, 1]
                err = float((np.abs(boxes.astype(np.float64) - ref_boxes) / unit).max())
                assert err <= 2.0, (k, err)
                worst_box = max(worst_box, err)
                raw = rp.box_decode(codes, proposals[index], weights)
                clipped += int((raw != boxes).any())
            true = bd.softmax_true(logits)
            d_stmt, d_torch = float(bd.ulp_distance(p, true).max()), float(bd.ulp_distance(tp, true).max())
            d_both = float((np.abs(p.astype(np.float64) - tp) / np.spacing(np.abs(true).astype(np.float32)).astype(np.float64)).max())
            assert d_stmt <= 3.0, (k, d_stmt)
            assert d_both <= d_stmt + d_torch
            worst = np.maximum(worst, [d_stmt, d_torch, d_both])
            if index.size:
                assert float(bd.ulp_distance(scores, true[index, labels]).max()) <= 3.0
            detections += index.size
            above += int(M > 0 and Dk > M)
            below += int(M > 0 and Dk < M)
            suppressed += int(Dk < K)
            data[f"det{k}_logits"], data[f"det{k}_regression"], data[f"det{k}_proposals"] = logits, reg, proposals
            data[f"det{k}_par"] = np.asarray([image[0], image[1], score_thresh, nms, M, K, Dk], np.float64)
            data[f"det{k}_weights"] = np.asarray(weights, np.float32)
            data[f"det{k}_boxes"], data[f"det{k}_scores"], data[f"det{k}_labels"], data[f"det{k}_index"] = ref_boxes, ref_score, ref_label, ref_index
    assert above >= 3 and below >= 3 and clipped >= 10 and suppressed >= 20, (above, below, clipped, suppressed)
    data["counts"] = np.asarray([CASES, redrawn, detections, above, below], np.int32)
    data["worst_box_ulp"] = np.asarray([worst_box], np.float64)
    data["worst_softmax_ulp"] = worst                                                                    # statement to f64, torch to f64, statement to torch
    print(f"{CASES} cases with {detections} detections ({redrawn} draws rejected; {above} cases above the limit, {below} below, {suppressed} with suppression, "
          f"{clipped} with clipped boxes): the statement has the reference's count, labels, rows and order; coordinates within {worst_box:.3f} of the unit (bound 2); "
          f"softmax: statement {worst[0]:.3f} ulp (bound 3), torch {worst[1]:.3f} ulp, statement to torch {worst[2]:.3f} ulp")
    np.savez_compressed(OUT, **data)
    print(f"{OUT}: {os.path.getsize(OUT)} bytes")
    assert os.path.getsize(OUT) < 600000


if __name__ == "__main__":
    main()
