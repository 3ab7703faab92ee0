#!/usr/bin/env python3
"""Writes tests/golden/fpn_pooler_ref.npz: what maskrcnn-benchmark's own FPN Pooler and LevelMapper give on small inputs.

    python tools/make_golden_fpn_pooler.py /path/to/maskrcnn-benchmark-master

The reference is put on sys.path and runs on the CPU: Pooler.forward and LevelMapper.__call__ (maskrcnn_benchmark/modeling/poolers.py:11-121) on BoxLists.  Its
extension module maskrcnn_benchmark._C is an object whose `roi_align_forward` is the reference's csrc/cpu/ROIAlign_cpu.cpp, compiled as a throw-away extension
exactly as tools/make_golden_detector_ops.py does: nothing compiled is kept and none of the reference's text is in this repository.  The file holds inputs and
outputs only.
Pooler cases: 1 to 4 levels (and one of 8), first scale 1 / 1/4 / 1/8 / 1/16, one or two images, 1 to 3 channels, square outputs 1 / 2 / 7 / 14, sampling ratios
0 .. 2, ROI sizes spread over every level and beyond both ends; in the cases with more than one level also an ROI with a NaN coordinate, one with infinite
ones (inf - inf) and one of negative area (no level: a row of zeros), and a box beyond the last edge.  Stored per case: the maps, the rois as convert_to_roi_format made them,
the scales, the result, and the levels LevelMapper gave (-1 where it gave no valid level).
LevelMapper sweeps (the reference's own arithmetic on the CPU, nothing else):
  sweep_v: every f32 v within 16 ulp of 2^-6 .. 2^3, through LevelMapper(k_min, k_max, canonical_scale=1, eps=0) on a stand-in box list whose area() is an f32 a
    with sqrt(a) == v (then s / 1 + 0 is v itself), once with the default canonical_level 4 (k_min -2, k_max 7) and once with 7 (k_min 0, k_max 10);
  edge_rois: real BoxLists through the default LevelMapper(2, 5): boxes whose sqrt(area) is exactly 56, 112, 224, 448, 896 and one f32 step either side,
    boxes whose v = sqrt(area) / 224 + 1e-6 lies within a few steps of 2^-2 .. 2^2, and areas of +inf, NaN, below 0, 0 and 1.
Before writing, the numpy statement (tests/fpn_pooler_numpy.py) is held against every stored figure -- every level and every output bit; any difference stops
the tool: the rule is what has to change then."""
import os
import sys
import tempfile
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
OUT = os.path.join(ROOT, "tests", "golden", "fpn_pooler_ref.npz")

F = np.float32
CASES = 26
POOLED = (7, 1, 2, 7, 14)


def step(x, k):
    """the f32 k steps above (below) x > 0"""
    return (np.asarray(x, F).view(np.uint32).astype(np.int64) + k).astype(np.uint32).view(F)


def box_of_area(a):
    """x0, y0, x1, y1 with (x1 - x0 + 1) * (y1 - y0 + 1) == a in f32 for 1 <= a < 2^24: a - 1 and (a - 1) + 1 are exact there"""
    a = np.asarray(a, F).reshape(-1)
    assert ((a >= 1) & (a < 2 ** 24)).all()
    z = np.zeros_like(a)
    return np.stack([z + F(1), z, a, z], axis=1).astype(F)


def area_with_root(v):
    """an f32 a with sqrt(a) == v (f32), for every entry of v"""
    v = np.asarray(v, F).reshape(-1)
    a = (v.astype(np.float64) ** 2).astype(F)
    for k in (0, -1, 1, -2, 2):
        c = step(a, k)
        hit = np.sqrt(c) == v
        a = np.where((np.sqrt(a) != v) & hit, c, a)
    assert (np.sqrt(a) == v).all()
    return a


def edge_rois():
    s = np.concatenate([step(F(x), np.arange(-1, 2)) for x in (56, 112, 224, 448, 896)])
    rois = [box_of_area(area_with_root(s)), np.asarray([[0, 0, 55, 55], [0, 0, 111, 111], [0, 0, 223, 223], [0, 0, 447, 447], [0, 0, 895, 895], [10, 20, 233, 243]], F)]
    for k in range(-2, 3):                                       # v at the edge itself: s = 224 * (2^k - 1e-6) and its neighbours
        s0 = F(224.0 * (2.0 ** k - 1e-6))
        rois.append(box_of_area(area_with_root(step(s0, np.arange(-6, 7)))))
    rois.append(np.asarray([[0, 0, np.inf, 10], [-np.inf, 0, np.inf, 10], [np.nan, 0, 10, 10], [np.inf, 0, np.inf, 10], [30, 10, 10, 40], [5, 5, 4, 4], [7, 7, 7, 7]], F))
    b = np.concatenate(rois)                                     # (the last rows: areas +inf, +inf, NaN, NaN, negative, 0, 1)
    return np.concatenate([np.zeros((b.shape[0], 1), F), b], axis=1)


def pooler_case(rng, k):
    levels = (4, 1, 2, 3, 4, 4, 8)[k % 7]
    k_min = 0 if levels == 8 else (2, 4, 3, 2, 0, 2)[k % 6]
    res = POOLED[k % 5]
    ratio = (2, 0, 1)[k % 3]
    B, C = 1 + k % 2, 1 + k % 3
    iw, ih = int(rng.integers(64, 161)), int(rng.integers(48, 129))
    if k_min == 0:
        iw, ih = iw // 4, ih // 4                                # (a map at scale 1: keep the file small)
    scales = [2.0 ** -(k_min + l) for l in range(levels)]
    feats = [rng.standard_normal((B, C, max(1, int(np.ceil(ih * s))), max(1, int(np.ceil(iw * s))))).astype(F) for s in scales]
    n = 8 if res == 14 else 14
    side = 2.0 ** rng.uniform(2.0, 11.0, n)                      # 4 .. 2048 px: below the first edge (112) and beyond the last (896)
    if ratio == 0:
        side = np.minimum(side, 600.0)                           # (an adaptive grid grows with the ROI)
    w, h = side * rng.uniform(0.6, 1.6, n), side / rng.uniform(0.6, 1.6, n)
    cx, cy = rng.uniform(-0.1 * iw, 1.1 * iw, n), rng.uniform(-0.1 * ih, 1.1 * ih, n)
    boxes = np.stack([cx - w / 2, cy - h / 2, cx + w / 2, cy + h / 2], axis=1).astype(F)
    boxes[0] = (0, 0, iw - 1, ih - 1)
    boxes[1] = boxes[1, [2, 3, 0, 1]]                            # reversed on both axes: a positive area, a malformed ROI
    boxes[2] = (5, 5, 5 - 1, 5 - 1)                              # area 0
    boxes[3] = (30, 10, 10, 40)                                  # a negative area: no level (one level: a malformed ROI)
    if levels > 1:
        boxes[4, 2] = np.nan
        boxes[5] = (np.inf, 0, np.inf, 10)                       # inf - inf: a NaN area
        boxes[6] = (-3000, -3000, 3000, 3000)                    # beyond the last edge of every ladder here
    img = np.sort(rng.integers(0, B, n))
    return feats, boxes, img, scales, res, ratio, (iw, ih)


class AreaList:
    """a stand-in box list for LevelMapper: only area() is asked"""
    def __init__(self, area):
        self.a = area

    def area(self):
        return self.a


def main():
    import torch

    import fpn_pooler_numpy as fp
    from make_golden_detector_ops import load_reference

    if len(sys.argv) != 2:
        sys.exit(__doc__)
    rng = np.random.default_rng(20261020)
    data = {}
    with tempfile.TemporaryDirectory() as tmp:
        assert not os.path.abspath(tmp).startswith(ROOT + os.sep)
        ext = load_reference(os.path.join(sys.argv[1], "maskrcnn_benchmark"), tmp)
        sys.path.insert(0, sys.argv[1])
        stub = types.ModuleType("maskrcnn_benchmark._C")
        stub.nms, stub.roi_align_forward = ext.nms, ext.roi_align_forward
        sys.modules["maskrcnn_benchmark._C"] = stub
        from maskrcnn_benchmark.modeling.poolers import LevelMapper, Pooler
        from maskrcnn_benchmark.structures.bounding_box import BoxList

        def mapped(mapper, lists, k_min, k_max):
            """LevelMapper's answer as int32, -1 where it is no level of k_min .. k_max (floor of a NaN, converted)"""
            lv = np.asarray(mapper(lists).to(torch.float64).numpy())
            return np.where((lv >= 0) & (lv <= k_max - k_min), lv, -1).astype(np.int32)

        # ---- the sweeps
        v = np.concatenate([step(F(2.0 ** k), np.arange(-16, 17)) for k in range(-6, 4)])
        area = torch.from_numpy(area_with_root(v))
        for lvl0, k_min, k_max in ((4, -2, 7), (7, 0, 10)):
            ref = mapped(LevelMapper(k_min, k_max, canonical_scale=1, canonical_level=lvl0, eps=0), [AreaList(area)], k_min, k_max)
            mine = fp.level_of_v(v, k_min, k_max, lvl0)
            assert np.array_equal(ref, mine), (lvl0, v[ref != mine], ref[ref != mine], mine[ref != mine])
            data[f"sweep_levels_l{lvl0}"] = ref
            data[f"sweep_par_l{lvl0}"] = np.asarray([lvl0, k_min, k_max], np.int32)
        data["sweep_v"] = v
        rois = edge_rois()
        ref = mapped(LevelMapper(2, 5), [BoxList(torch.from_numpy(rois[:, 1:].copy()), (1000, 1000), mode="xyxy")], 2, 5)
        mine = fp.levels(rois, 2, 5)
        assert np.array_equal(ref, mine), (rois[ref != mine], ref[ref != mine], mine[ref != mine])
        vv = fp.v_of_rois(rois)
        at_edge = sum(int(np.ptp(ref[(vv >= step(F(2.0 ** k), -8)) & (vv <= step(F(2.0 ** k), 8))]) > 0) for k in (-1, 0, 1))
        assert at_edge == 3, at_edge                             # the three inner edges are crossed inside their windows
        data["edge_rois"], data["edge_levels"] = rois, ref

        # ---- Pooler.forward
        outputs, per_level, none = 0, np.zeros(8, np.int64), 0
        for k in range(CASES):
            feats, boxes, img, scales, res, ratio, size = pooler_case(rng, k)
            lists = [BoxList(torch.from_numpy(boxes[img == i].copy()), size, mode="xyxy") for i in range(feats[0].shape[0])]
            pooler = Pooler(output_size=(res, res), scales=scales, sampling_ratio=ratio)
            with torch.no_grad():
                out = pooler([torch.from_numpy(f) for f in feats], lists).numpy()
                rois = pooler.convert_to_roi_format(lists).numpy().astype(F)
            k_min = int(round(-np.log2(scales[0])))
            k_max = k_min + len(scales) - 1
            assert (pooler.map_levels.k_min, pooler.map_levels.k_max) == (k_min, k_max)
            lev = mapped(pooler.map_levels, lists, k_min, k_max) if len(scales) > 1 else np.zeros(rois.shape[0], np.int32)
            assert np.isfinite(out).all()
            mine, mine_lev = fp.fpn_roi_align(feats, rois, scales, res, res, ratio)
            assert np.array_equal(mine_lev, lev), (k, lev, mine_lev)
            diff = int((mine.view(np.uint32) != out.view(np.uint32)).sum())
            assert mine.shape == out.shape and diff == 0, (k, diff, out.size)
            assert not out[lev < 0].any()
            outputs += out.size
            none += int((lev < 0).sum())
            per_level[:len(scales)] += np.bincount(lev[lev >= 0], minlength=len(scales))
            for l, f in enumerate(feats):
                data[f"pool{k}_feat{l}"] = f
            data[f"pool{k}_rois"], data[f"pool{k}_out"], data[f"pool{k}_levels"] = rois, out, lev
            data[f"pool{k}_scales"] = np.asarray(scales, F)
            data[f"pool{k}_par"] = np.asarray([res, ratio], np.int32)
    assert (per_level[:4] >= 20).all() and per_level[7] >= 1 and none >= 40, (per_level, none)
    data["counts"] = np.asarray([CASES, v.size, data["edge_rois"].shape[0]], np.int32)
    print(f"{CASES} Pooler cases with {outputs} outputs (ROIs per level {per_level.tolist()}, {none} of no level), {v.size} swept v at two canonical levels, "
          f"{data['edge_rois'].shape[0]} edge boxes: the statement equals every level and every bit")
    np.savez_compressed(OUT, **data)
    print(f"{OUT}: {os.path.getsize(OUT)} bytes")
    assert os.path.getsize(OUT) < 600000


if __name__ == "__main__":
    main()
