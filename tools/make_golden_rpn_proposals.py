#!/usr/bin/env python3
"""Writes tests/golden/rpn_proposals_ref.npz: what maskrcnn-benchmark's own Python gives for the RPN's proposal stage and for BoxCoder.decode on small inputs.

    python tools/make_golden_rpn_proposals.py /path/to/maskrcnn-benchmark-master

The reference is put on sys.path and runs on the CPU: RPNPostProcessor.forward_for_single_feature_map (maskrcnn_benchmark/modeling/rpn/inference.py:74-121) and
BoxCoder.decode (modeling/box_coder.py:52-95).  Its extension module maskrcnn_benchmark._C is an object whose `nms` is the reference's csrc/cpu/nms_cpu.cpp, compiled
as a throw-away extension exactly as tools/make_golden_detector_ops.py does: nothing compiled is kept and none of the reference's text is in this repository.
The file holds inputs and outputs only.  Proposal cases: A = 1 / 3 / 15 anchors per cell, H and W from 1 to 14 (levels of at most 2940 anchors), image sizes that are
not multiples of the stride, the parameter sets (pre, post, threshold, min_size) = (100, 30, 0.7, 0), (n, 10, 0.5, 4), (50, 50, 0.7, 0), codes beyond the clip.
Decode cases: k = 1 / 2 / 81 boxes per row, the weights (1, 1, 1, 1) and (10, 10, 5, 5).
A proposal case is drawn again when two anchors have the same sigmoid value in f32 (the reference's topk and sort are not stable), when by the numpy statement a
pair of survivors has an IoU within 1e-5 of the threshold (nms_cpu.cpp has >=, the rule >, and the decoded boxes differ in their last bits) or when a clipped side of
a candidate lies within 1e-3 of min_size; the three counts (0) are stored.  Before writing, the statement (tests/rpn_proposals_numpy.py) is held to every stored
figure: equal counts, equal order, every coordinate within 2 ulp of the largest magnitude among the box's pcx, pcy, pw, ph -- EXP and torch.exp are each within
1 ulp of the true value and the products and sums add one rounding each; the largest difference seen, in that unit, is stored.  EXP itself is held to
float32(exp(float64(x))) on rpn_proposals_numpy.exp_sweep(): at most 1 ulp; the number of arguments that differ at all is stored."""
import os
import sys
import tempfile
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
OUT = os.path.join(ROOT, "tests", "golden", "rpn_proposals_ref.npz")

RPN_CASES = 42
DECODE_CASES = 20
STRIDE = 16


def make_anchors(rng, A, H, W):
    """[H W A, 4], row (y W + x) A + a: A boxes of different sizes and aspect ratios around the centre of every cell of stride 16"""
    sizes = rng.uniform(12, 90, A)
    ratios = rng.choice([0.5, 1.0, 2.0], A)
    w, h = sizes / np.sqrt(ratios), sizes * np.sqrt(ratios)
    base = np.stack([-(w - 1) / 2, -(h - 1) / 2, (w - 1) / 2, (h - 1) / 2], axis=1)              # [A, 4]
    ys, xs = np.mgrid[0:H, 0:W]
    ctr = np.stack([xs, ys, xs, ys], axis=-1).reshape(H * W, 1, 4) * STRIDE + (STRIDE - 1) / 2
    return (ctr + base[None]).reshape(-1, 4).astype(np.float32)


def rpn_case(rng, k):
    A = (1, 3, 15)[k % 3]
    hi = 9 if A == 15 else 15
    H, W = int(rng.integers(1, hi)), int(rng.integers(1, hi))
    if k == 41:
        A, H, W = 15, 14, 14
    if k == 3:
        H = W = 1
    n = A * H * W
    pre, post, thr, min_size = ((100, 30, 0.7, 0), (n, 10, 0.5, 4), (50, 50, 0.7, 0))[(k // 3) % 3]
    image = (W * STRIDE - int(rng.integers(1, STRIDE)), H * STRIDE - int(rng.integers(1, STRIDE)))       # (width, height): not multiples of the stride
    obj = rng.uniform(-4, 4, (A, H, W)).astype(np.float32)
    reg = (rng.standard_normal((4 * A, H, W)) * 0.6).astype(np.float32)
    r4 = reg.reshape(A, 4, H, W)
    big = rng.random((A, 2, H, W)) < 0.08
    r4[:, 2:][big] = rng.uniform(4.2, 9.0, int(big.sum())).astype(np.float32)                          # beyond the clip log(1000 / 16) = 4.135
    return obj, reg, make_anchors(rng, A, H, W), image, pre, post, thr, min_size


def main():
    import torch

    import rpn_proposals_numpy as rp
    from make_golden_detector_ops import load_reference

    if len(sys.argv) != 2:
        sys.exit(__doc__)
    rng = np.random.default_rng(20261018)
    data = {}
    with tempfile.TemporaryDirectory() as tmp:
        assert not os.path.abspath(tmp).startswith(ROOT + os.sep)
        ext = load_reference(os.path.join(sys.argv[1], "maskrcnn_benchmark"), tmp)
        sys.path.insert(0, sys.argv[1])
        stub = types.ModuleType("maskrcnn_benchmark._C")
        stub.nms = ext.nms
        sys.modules["maskrcnn_benchmark._C"] = stub
        from maskrcnn_benchmark.modeling.box_coder import BoxCoder
        from maskrcnn_benchmark.modeling.rpn.inference import RPNPostProcessor
        from maskrcnn_benchmark.structures.bounding_box import BoxList

        worst, proposals, redrawn = 0.0, 0, 0
        for k in range(RPN_CASES):
            while True:
                obj, reg, anchors, image, pre, post, thr, min_size = rpn_case(rng, k)
                logits, codes = rp.flatten(obj, reg)
                sig = torch.sigmoid(torch.from_numpy(logits)).numpy()
                ties = logits.size - np.unique(sig).size
                top = rp.nms_order(logits)[:min(pre, logits.size)]
                cb = rp.box_decode(codes[top], anchors[top], clip_to=image)
                sides = np.concatenate([cb[:, 2] - cb[:, 0] + 1, cb[:, 3] - cb[:, 1] + 1]).astype(np.float64)
                at_size = int((np.abs(sides - min_size) <= 1e-3).sum())
                sb, sl, si = rp.candidates(obj, reg, anchors, image, pre, min_size)
                at_thr = rp.near_threshold(sb, thr)
                if ties == 0 and at_size == 0 and at_thr == 0:
                    break
                redrawn += 1
            sel = RPNPostProcessor(pre, post, thr, min_size)
            with torch.no_grad():
                res = sel.forward_for_single_feature_map([BoxList(torch.from_numpy(anchors.copy()), image, mode="xyxy")], torch.from_numpy(obj)[None],
                                                         torch.from_numpy(reg)[None])[0]
            ref_boxes, ref_score = res.bbox.numpy().astype(np.float32), res.get_field("objectness").numpy().astype(np.float32)
            pos = {v.tobytes(): i for i, v in enumerate(sig)}
            ref_index = np.asarray([pos[v.tobytes()] for v in ref_score], np.int64)                 # (sigmoid values are distinct: the anchor of every proposal)
            boxes, lg, index = rp.rpn_proposals(obj, reg, anchors, image, pre, post, thr, min_size)
            assert boxes.shape == ref_boxes.shape and np.array_equal(index, ref_index), (k, boxes.shape, ref_boxes.shape)
            if index.size:
                unit = rp.coordinate_ulp(codes[index], anchors[index])                              # [c, 1]
                err = float((np.abs(boxes.astype(np.float64) - ref_boxes) / unit).max())
                assert err <= 2.0, (k, err)
                worst = max(worst, err)
            proposals += index.size
            data[f"rpn{k}_objectness"], data[f"rpn{k}_regression"], data[f"rpn{k}_anchors"] = obj, reg, anchors
            data[f"rpn{k}_par"] = np.asarray([image[0], image[1], pre, post, thr, min_size, ties, at_thr, at_size], np.float64)
            data[f"rpn{k}_boxes"], data[f"rpn{k}_score"], data[f"rpn{k}_index"] = ref_boxes, ref_score, ref_index
        worst_d = 0.0
        for k in range(DECODE_CASES):
            kk = (1, 2, 81)[k % 3]
            weights = ((1.0, 1.0, 1.0, 1.0), (10.0, 10.0, 5.0, 5.0))[(k // 3) % 2]
            n = int(rng.integers(1, 6 if kk == 81 else 40))
            c0 = rng.uniform(0, 500, (n, 2))
            boxes = np.concatenate([c0, c0 + rng.uniform(2, 300, (n, 2))], axis=1).astype(np.float32)
            codes = rng.standard_normal((n, kk, 4)) * 0.7
            codes[..., 2:][rng.random((n, kk, 2)) < 0.1] = 7.0                                        # beyond the clip at either weight set
            codes = (codes * np.asarray(weights)).reshape(n, 4 * kk).astype(np.float32)
            ref = BoxCoder(weights=weights).decode(torch.from_numpy(codes), torch.from_numpy(boxes)).numpy().astype(np.float32)
            mine = rp.box_decode(codes, boxes, weights)
            unit = np.repeat(rp.coordinate_ulp(codes, boxes, weights), 4, axis=1)
            err = float((np.abs(mine.astype(np.float64) - ref) / unit).max())
            assert mine.shape == ref.shape and err <= 2.0, (k, err)
            worst_d = max(worst_d, err)
            data[f"dec{k}_codes"], data[f"dec{k}_boxes"], data[f"dec{k}_out"] = codes, boxes, ref
            data[f"dec{k}_weights"] = np.asarray(weights, np.float32)
    x = rp.exp_sweep()
    with np.errstate(over="ignore", under="ignore"):
        mine, lib = rp.EXP(x), np.exp(x.astype(np.float64)).astype(np.float32)
    steps = np.abs(mine.view(np.int32).astype(np.int64) - lib.view(np.int32).astype(np.int64))
    assert steps.max() <= 1
    data["counts"] = np.asarray([RPN_CASES, DECODE_CASES], np.int32)
    data["worst_ulp"] = np.asarray([worst, worst_d], np.float64)
    data["exp_differs"] = np.asarray([int((steps != 0).sum()), x.size], np.int64)
    print(f"{RPN_CASES} proposal cases with {proposals} proposals ({redrawn} draws rejected), {DECODE_CASES} decode cases: the statement has the reference's counts and "
          f"order; largest difference {worst:.3f} / {worst_d:.3f} of the unit (bound 2); EXP differs from exp on {int((steps != 0).sum())} of {x.size} arguments")
    np.savez_compressed(OUT, **data)
    print(f"{OUT}: {os.path.getsize(OUT)} bytes")
    assert os.path.getsize(OUT) < 600000


if __name__ == "__main__":
    main()
