#!/usr/bin/env python3
"""Writes tests/golden/rpn_fpn_ref.npz: what maskrcnn-benchmark's own Python gives for the RPN's proposal stage over the levels of an FPN, on small pyramids.

    python tools/make_golden_rpn_fpn.py /path/to/maskrcnn-benchmark-master

The reference is put on sys.path and runs on the CPU: RPNPostProcessor(pre, post, thr, min_size, fpn_post_nms_top_n=F).eval().forward(anchors, objectness,
box_regression) for one image (maskrcnn_benchmark/modeling/rpn/inference.py:123-179: forward_for_single_feature_map per level, then select_over_all_levels).  Its
extension module maskrcnn_benchmark._C is an object whose `nms` is the reference's csrc/cpu/nms_cpu.cpp, compiled as a throw-away extension exactly as
tools/make_golden_rpn_proposals.py does: nothing compiled is kept and none of the reference's text is in this repository.  The file holds inputs and outputs only.
Cases: L = 2 / 3 / 5 / 8 levels, A = 1 / 3 anchors per cell, H and W halving (rounded up) from at most 14 x 14 down to 1 x 1, strides doubling from 4, an image
size that is no multiple of the stride, at most 3000 anchors per case; the parameter sets (pre, post, threshold, min_size) = (100, 30, 0.7, 0), (1000, 10, 0.5,
4), (50, 50, 0.7, 0); F below, at and above the number of proposals of all levels; in QUOTA_CASE one level reaches post_nms_top_n and another keeps fewer than
five; in EMPTY_CASE a level in the middle has H = 0 (the reference's own code cannot run a level without cells -- its permute_and_flatten refuses to
reshape a tensor of no elements -- so it is given the other levels; the stored inputs hold the empty one).
A case is drawn again when two anchors of the whole case have the same sigmoid value in f32 (the reference's topk is not stable), when by the numpy statement a
pair of survivors of a level has an IoU within 1e-5 of the threshold or when a clipped side of a candidate lies within 1e-3 of min_size; the three counts (0) are
stored.  Before writing, the statement (tests/rpn_fpn_numpy.py) is held to every stored figure of every case: equal count, equal level and anchor of every row
(recovered through the distinct sigmoid values), equal order, every coordinate within 2 ulp of the largest magnitude among the box's pcx, pcy, pw, ph (the bound
and the unit of the single-level fixture); the largest difference seen, in that unit, is stored."""
import os
import sys
import tempfile
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
OUT = os.path.join(ROOT, "tests", "golden", "rpn_fpn_ref.npz")

CASES = 24
QUOTA_CASE = 10
EMPTY_CASE = 13
PARAMS = ((100, 30, 0.7, 0), (1000, 10, 0.5, 4), (50, 50, 0.7, 0))


def make_anchors(rng, A, H, W, stride):
    """[H W A, 4], row (y W + x) A + a: A boxes of different sizes (in units of the stride) and aspect ratios around the centre of every cell"""
    sizes = rng.uniform(1.5, 6.0, A) * stride
    ratios = rng.choice([0.5, 1.0, 2.0], A)
    w, h = sizes / np.sqrt(ratios), sizes * np.sqrt(ratios)
    base = np.stack([-(w - 1) / 2, -(h - 1) / 2, (w - 1) / 2, (h - 1) / 2], axis=1)
    ys, xs = np.mgrid[0:H, 0:W]
    ctr = np.stack([xs, ys, xs, ys], axis=-1).reshape(H * W, 1, 4) * stride + (stride - 1) / 2
    return (ctr + base[None]).reshape(-1, 4).astype(np.float32)


def fpn_case(rng, k):
    """-> levels [(objectness, regression, anchors)], image (width, height), pre, post, thr, min_size"""
    L, A = (2, 3, 5, 8)[k % 4], (1, 3)[(k // 4) % 2]
    pre, post, thr, min_size = PARAMS[(k // 2) % 3]
    if k == QUOTA_CASE:
        L, A, (pre, post, thr, min_size) = 5, 3, PARAMS[1]
    H, W = int(rng.integers(9, 15)), int(rng.integers(9, 15))
    image = (W * 4 - int(rng.integers(1, 4)), H * 4 - int(rng.integers(1, 4)))                          # (width, height): no multiple of any stride
    levels = []
    for l in range(L):
        h, w = (0, W) if k == EMPTY_CASE and l == 1 else (H, W)
        obj = rng.uniform(-4, 4, (A, h, w)).astype(np.float32)
        reg = (rng.standard_normal((4 * A, h, w)) * 0.6).astype(np.float32)
        r4 = reg.reshape(A, 4, h, w)
        big = rng.random((A, 2, h, w)) < 0.08
        r4[:, 2:][big] = rng.uniform(4.2, 9.0, int(big.sum())).astype(np.float32)                       # beyond the clip log(1000 / 16) = 4.135
        levels.append((obj, reg, make_anchors(rng, A, h, w, 4 << l)))
        H, W = (H + 1) // 2, (W + 1) // 2
    assert sum(lv[0].size for lv in levels) <= 3000
    return levels, image, pre, post, thr, min_size


def main():
    import torch

    import rpn_fpn_numpy as rf
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
        from maskrcnn_benchmark.modeling.rpn.inference import RPNPostProcessor
        from maskrcnn_benchmark.structures.bounding_box import BoxList

        worst, proposals, redrawn, modes = 0.0, 0, 0, []
        for k in range(CASES):
            while True:
                levels, image, pre, post, thr, min_size = fpn_case(rng, k)
                flat = [rp.flatten(o, r) for o, r, _ in levels]
                sig = [torch.sigmoid(torch.from_numpy(lg)).numpy() for lg, _ in flat]
                ties = sum(s.size for s in sig) - np.unique(np.concatenate(sig)).size                   # over the whole case, not per level
                at_size = at_thr = 0
                for (o, r, a), (lg, codes) in zip(levels, flat):
                    if lg.size == 0:
                        continue
                    top = rp.nms_order(lg)[:min(pre, lg.size)]
                    cb = rp.box_decode(codes[top], a[top], clip_to=image)
                    sides = np.concatenate([cb[:, 2] - cb[:, 0] + 1, cb[:, 3] - cb[:, 1] + 1]).astype(np.float64)
                    at_size += int((np.abs(sides - min_size) <= 1e-3).sum())
                    at_thr += rp.near_threshold(rp.candidates(o, r, a, image, pre, min_size)[0], thr)
                mine = rf.rpn_proposals_fpn(levels, image, pre, post, thr, min_size, 8192)
                T = int(mine[4].sum())
                quota = k != QUOTA_CASE or (int(mine[4].max()) == post and 0 < int(mine[4].min()) < 5)
                if ties == 0 and at_size == 0 and at_thr == 0 and T >= 4 and quota:
                    break
                redrawn += 1
            mode = k % 3                                                                                # F below, at, above T
            Fn = (T // 2, T, T + 7)[mode]
            modes.append(mode)
            live = [i for i, lv in enumerate(levels) if lv[0].size]                                     # (the reference cannot run a level without cells)
            sel = RPNPostProcessor(pre, post, thr, min_size, fpn_post_nms_top_n=Fn).eval()
            with torch.no_grad():
                res = sel.forward([[BoxList(torch.from_numpy(levels[i][2].copy()), image, mode="xyxy") for i in live]],
                                  [torch.from_numpy(levels[i][0])[None] for i in live], [torch.from_numpy(levels[i][1])[None] for i in live])[0]
            ref_boxes, ref_score = res.bbox.numpy().astype(np.float32), res.get_field("objectness").numpy().astype(np.float32)
            pos = {v.tobytes(): (l, i) for l, s in enumerate(sig) for i, v in enumerate(s)}
            where = [pos[v.tobytes()] for v in ref_score]                                               # (sigmoid values are distinct: the level and anchor of every row)
            ref_level, ref_index = np.asarray([w[0] for w in where], np.int32), np.asarray([w[1] for w in where], np.int64)
            boxes, lg, level, index, level_counts = rf.rpn_proposals_fpn(levels, image, pre, post, thr, min_size, Fn)
            assert boxes.shape == ref_boxes.shape and boxes.shape[0] == min(Fn, T), (k, boxes.shape, ref_boxes.shape, Fn, T)
            assert np.array_equal(level, ref_level) and np.array_equal(index, ref_index), k
            for l in range(len(levels)):
                w = level == l
                if w.any():
                    unit = rp.coordinate_ulp(flat[l][1][index[w]], levels[l][2][index[w]])              # [c, 1]
                    err = float((np.abs(boxes[w].astype(np.float64) - ref_boxes[w]) / unit).max())
                    assert err <= 2.0, (k, l, err)
                    worst = max(worst, err)
            proposals += index.size
            for l, (o, r, a) in enumerate(levels):
                data[f"fpn{k}_l{l}_objectness"], data[f"fpn{k}_l{l}_regression"], data[f"fpn{k}_l{l}_anchors"] = o, r, a
            data[f"fpn{k}_par"] = np.asarray([image[0], image[1], pre, post, thr, min_size, Fn, len(levels), ties, at_thr, at_size], np.float64)
            data[f"fpn{k}_boxes"], data[f"fpn{k}_score"], data[f"fpn{k}_level"], data[f"fpn{k}_index"] = ref_boxes, ref_score, ref_level, ref_index
            data[f"fpn{k}_level_counts"] = level_counts
    assert set(modes) == {0, 1, 2}
    data["counts"] = np.asarray([CASES, QUOTA_CASE, EMPTY_CASE], np.int32)
    data["worst_ulp"] = np.asarray([worst], np.float64)
    data["redrawn"] = np.asarray([redrawn], np.int32)
    print(f"{CASES} cases with {proposals} proposals ({redrawn} draws rejected): the statement has the reference's counts, levels, anchors and order; largest "
          f"difference {worst:.3f} of the unit (bound 2)")
    np.savez_compressed(OUT, **data)
    print(f"{OUT}: {os.path.getsize(OUT)} bytes")
    assert os.path.getsize(OUT) < 600000


if __name__ == "__main__":
    main()
