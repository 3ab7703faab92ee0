"""The detector operators' rules without a GPU: the numpy statement (tests/detector_ops_numpy.py) against the golden file made from maskrcnn-benchmark's own CPU
operators (tools/make_golden_detector_ops.py: csrc/cpu/ROIAlign_cpu.cpp and csrc/cpu/nms_cpu.cpp, compiled from their files) -- every ROIAlign output equal in its
bits, every keep list equal; grouped NMS against the per-group runs; and the directed cases that hold the statement to nms.cu where nms_cpu.cpp differs."""
import os

import numpy as np
import pytest

import detector_ops_numpy as dn
from conftest import ROOT

GOLDEN = os.path.join(ROOT, "tests", "golden", "detector_ops_ref.npz")


@pytest.fixture(scope="module")
def golden():
    return dict(np.load(GOLDEN))


def test_roi_align_statement_equals_the_reference_bit_for_bit(golden):
    n_roi = int(golden["counts"][0])
    assert n_roi == 40
    seen = set()
    outputs = 0
    for k in range(n_roi):
        inp, rois, ref = golden[f"roi{k}_input"], golden[f"roi{k}_rois"], golden[f"roi{k}_out"]
        scale, ph, pw, ratio = golden[f"roi{k}_par"]
        assert np.isfinite(inp).all() and np.isfinite(rois).all() and inp.shape[2] <= 17 and inp.shape[3] <= 13
        out = dn.roi_align_forward(inp, rois, np.float32(scale), int(ph), int(pw), int(ratio))
        assert out.shape == ref.shape and out.dtype == ref.dtype == np.float32
        assert np.array_equal(out.view(np.uint32), ref.view(np.uint32)), k
        seen.add((int(ph), int(pw), int(ratio), inp.shape[1]))
        outputs += ref.size
    assert outputs > 30000
    assert {s[:2] for s in seen} == {(1, 1), (2, 3), (7, 7), (14, 14)} and {s[2] for s in seen} == {0, 1, 2, 3} and {s[3] for s in seen} == {1, 3, 5}


def test_nms_statement_equals_the_reference(golden):
    n_nms = int(golden["counts"][1])
    assert n_nms == 60
    sizes = set()
    for k in range(n_nms):
        boxes, scores, ref = golden[f"nms{k}_boxes"], golden[f"nms{k}_scores"], golden[f"nms{k}_keep"]
        thr, ties = golden[f"nms{k}_par"]
        assert ties == 0 and dn.pairs_at_threshold(boxes, np.float32(thr)) == 0       # the one place where nms_cpu.cpp (>=) and nms.cu (>) part
        assert np.unique(scores).size == scores.size                                  # (the reference's sort is not stable)
        keep = dn.nms(boxes, scores, np.float32(thr))
        assert keep.dtype == np.int64 and np.array_equal(keep, ref), k
        sizes.add(boxes.shape[0])
    assert {1, 63, 64, 65, 128, 129, 300} <= sizes and max(sizes) <= 300


def _random_boxes(rng, n, extent=60.0):
    c = rng.uniform(0, extent, (n, 2))
    return np.concatenate([c, c + rng.uniform(4, 40, (n, 2))], axis=1).astype(np.float32)


def test_grouped_nms_is_the_per_group_runs():
    rng = np.random.default_rng(5)
    n = 400
    boxes = _random_boxes(rng, n)
    scores = rng.permutation(n).astype(np.float32)
    scores[::7] = scores[3]                                   # equal scores too
    groups = rng.integers(0, 9, n).astype(np.int32)
    got = dn.nms(boxes, scores, 0.4, groups)
    parts = []
    for g in range(9):
        idx = np.nonzero(groups == g)[0]
        parts.append(idx[dn.nms(boxes[idx], scores[idx], 0.4)])
    ref = np.sort(np.concatenate(parts))
    assert np.array_equal(got, ref)
    assert got.size > dn.nms(boxes, scores, 0.4).size         # groups do keep boxes apart
    assert np.array_equal(dn.nms(boxes, scores, 0.4, np.zeros(n, np.int32)), dn.nms(boxes, scores, 0.4))


def test_nms_directed_cases():
    # IoU exactly at the threshold is kept: 10 x 10 against 10 x 5 inside it, 50 / (100 + 50 - 50) = 0.5 (nms_cpu.cpp's >= would drop it)
    b = np.asarray([[0, 0, 9, 9], [0, 0, 9, 4]], np.float32)
    assert dn.iou_row(b[0], b[1:])[0] == np.float32(0.5) and dn.pairs_at_threshold(b, 0.5) == 1
    assert np.array_equal(dn.nms(b, np.asarray([2, 1], np.float32), 0.5), [0, 1])
    assert np.array_equal(dn.nms(b, np.asarray([2, 1], np.float32), np.nextafter(np.float32(0.5), np.float32(0))), [0])
    # equal scores go by index: the first of two identical boxes survives, whatever the order of a sort that is not stable
    same = np.tile(np.asarray([[3, 3, 20, 20]], np.float32), (5, 1))
    assert np.array_equal(dn.nms(same, np.full(5, 0.7, np.float32), 0.5), [0])
    assert np.array_equal(dn.nms(same, np.asarray([0.1, 0.9, 0.9, 0.1, 0.9], np.float32), 0.5), [1])
    assert np.array_equal(dn.nms_order(np.asarray([0.0, -0.0, 1.0, np.nan, -np.inf, 1.0], np.float32)), [2, 5, 0, 1, 4, 3])
    # the chain: A suppresses B, B overlaps C, A does not: C is kept (a suppressed box suppresses nothing)
    chain = np.asarray([[0, 0, 19, 9], [8, 0, 27, 9], [16, 0, 35, 9]], np.float32)
    assert dn.iou_row(chain[0], chain[1:])[0] > 0.4 and dn.iou_row(chain[1], chain[2:])[0] > 0.4 and dn.iou_row(chain[0], chain[2:])[0] < 0.4
    assert np.array_equal(dn.nms(chain, np.asarray([3, 2, 1], np.float32), 0.4), [0, 2])
    assert np.array_equal(dn.nms(chain, np.asarray([2, 3, 1], np.float32), 0.4), [1])
    # a NaN score is visited last, a box with a NaN coordinate neither suppresses nor is suppressed
    assert np.array_equal(dn.nms(same[:3], np.asarray([np.nan, 0.1, 0.2], np.float32), 0.5), [2])
    nanbox = same[:3].copy(); nanbox[1, 2] = np.nan
    assert np.array_equal(dn.nms(nanbox, np.asarray([3, 2, 1], np.float32), 0.5), [0, 1])
    assert dn.nms(np.zeros((0, 4), np.float32), np.zeros(0, np.float32), 0.5).size == 0


def test_roi_align_directed_cases():
    rng = np.random.default_rng(9)
    inp = rng.standard_normal((2, 3, 6, 5)).astype(np.float32)
    # a batch index out of range gives zeros; index 1 of 2 reads the second image
    rois = np.asarray([[2, 0, 0, 4, 4], [-1, 0, 0, 4, 4], [1, 0, 0, 4, 4], [0, 0, 0, 4, 4]], np.float32)
    out = dn.roi_align_forward(inp, rois, 1.0, 2, 2, 2)
    assert not out[0].any() and not out[1].any() and out[2].any()
    assert np.array_equal(out[2], dn.roi_align_forward(inp[1:], rois[3:], 1.0, 2, 2, 2)[0])
    # one sample per bin at a texel centre is that texel: ROI (0, 0, 4, 4) at ratio 1 and 2 x 2 bins samples (1, 1), (1, 3), (3, 1), (3, 3)
    one = dn.roi_align_forward(inp, rois[3:], 1.0, 2, 2, 1)[0]
    assert np.array_equal(one, inp[0][:, 1::2, 1::2][:, :2, :2])
    # wholly outside: every sample contributes +0
    far = dn.roi_align_forward(inp, np.asarray([[0, 40, 40, 50, 50]], np.float32), 1.0, 3, 3, 2)
    assert not far.any() and not np.signbit(far).any()
    # ratio 0: the grid is ceil(extent / pooled) per axis
    for ratio, roi in ((2, [0, 0, 0, 4, 4]), (2, [0, 0.5, 0.25, 3.5, 3.5]), (3, [0, 0, 0, 4.5, 5.5]), (1, [0, 3, 3, 1, 1])):    # (the last: reversed, 1 x 1)
        r = np.asarray([roi], np.float32)
        assert np.array_equal(dn.roi_align_forward(inp, r, 1.0, 2, 2, 0), dn.roi_align_forward(inp, r, 1.0, 2, 2, ratio)), roi
