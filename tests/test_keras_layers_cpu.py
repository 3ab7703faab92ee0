"""The Keras detector's three layers without a GPU: the numpy statement (tests/keras_layers_numpy.py) against what the reference tree can execute -- the fixture
recorded from utils.apply_box_deltas, utils.non_max_suppression and utils.generate_pyramid_anchors (tools/make_golden_keras_layers.py), and the level expression of
PyramidROIAlign.call evaluated in f32 numpy -- and the sampling against torch's grid_sample on the CPU.  TensorFlow is not available: what only its kernels define
(corner ordering and the area test of its suppression, crop_and_resize's extrapolation, top_k's ties) is stated, not executed; see the statement's docstring.
Also the host-only ifx_pyramid_level_thresholds through ctypes and its header's arithmetic in a stand-alone program under sanitizers."""
import os
import subprocess

import numpy as np
import pytest

import keras_layers_numpy as kl
from conftest import ROOT
from detector_ops_numpy import nms_order

F = np.float32
GOLDEN = os.path.join(ROOT, "tests", "golden", "keras_layers_ref.npz")


@pytest.fixture(scope="module")
def golden():
    return dict(np.load(GOLDEN))


def test_decode_against_apply_box_deltas(golden):
    """utils.apply_box_deltas on 320 rows (zero deltas, large and small scales, zero-sized and flipped boxes): within 4 ulp of the largest of |coordinate|, height
    and width -- one ulp between numpy's exp and EXP of the rule, carried through four roundings"""
    ref = golden["decode_out"]
    got = kl.decode(golden["decode_boxes"], golden["decode_deltas"])
    assert ref.dtype == F and got.shape == ref.shape == (320, 4)
    scale = np.maximum(np.abs(ref).max(axis=1), np.maximum(np.abs(ref[:, 2] - ref[:, 0]), np.abs(ref[:, 3] - ref[:, 1]))).astype(F)
    ulp = np.spacing(scale).astype(np.float64)
    err = np.abs(got.astype(np.float64) - ref.astype(np.float64)).max(axis=1) / ulp
    print("decode: worst error", float(err.max()), "ulp of the row's scale")
    assert (err <= 4.0).all(), float(err.max())
    exact = slice(0, 16)                                # zero deltas: EXP(0) == 1, nothing to round differently
    assert np.array_equal(got[exact].view(np.uint32), ref[exact].view(np.uint32))


@pytest.mark.parametrize("thr", [0.3, 0.7])
def test_suppression_picks_equal_the_reference(golden, thr):
    """utils.non_max_suppression on 164 float boxes with ordered corners and scores without ties: clusters, zero-area boxes, boxes that only touch"""
    boxes, scores = golden["nms_boxes"], golden["nms_scores"]
    order = nms_order(scores)
    picks = order[kl.tf_nms(boxes[order], thr, boxes.shape[0])]
    ref = golden[f"nms_pick_{int(thr * 10)}"]
    assert 0 < ref.size < boxes.shape[0]
    assert np.array_equal(picks, ref)
    zero = np.nonzero(((boxes[:, 2] - boxes[:, 0]) * (boxes[:, 3] - boxes[:, 1])) == 0)[0]
    assert zero.size == 8 and set(zero) <= set(picks)                       # zero-area boxes neither suppress nor are suppressed
    assert (boxes[-12:, 0] >= 400).all() and set(range(boxes.shape[0] - 12, boxes.shape[0])) <= set(picks)     # touching boxes have IoU 0
    limited = order[kl.tf_nms(boxes[order], thr, 10)]
    assert np.array_equal(limited, ref[:10])


def test_anchors_fixture_feeds_the_proposal_statement(golden):
    """utils.generate_pyramid_anchors for a 64 x 64 image, 3 (256 + 64 + 16 + 4 + 1) anchors; the statement runs on them and keeps the layer's invariants"""
    anchors = golden["anchors"]
    assert anchors.shape == (1023, 4) and np.isfinite(anchors).all()
    rng = np.random.default_rng(5)
    probs = rng.random((1023, 2)).astype(F)
    bbox = (rng.standard_normal((1023, 4)) * 0.5).astype(F)
    boxes, index = kl.keras_proposals(probs, bbox, anchors.astype(F), (64, 64), pre_nms_limit=600, proposal_count=100)
    assert 0 < boxes.shape[0] <= 100 and boxes.dtype == F and (boxes >= 0).all() and (boxes <= 1).all()
    assert np.unique(index).size == index.size and (np.diff(probs[index, 1]) <= 0).all()
    assert probs[index[0], 1] == probs[:, 1].max()
    # nothing suppressed at a threshold of 1: the 100 best
    b1, i1 = kl.keras_proposals(probs, bbox, anchors.astype(F), (64, 64), pre_nms_limit=600, proposal_count=100, nms_threshold=1.0)
    assert np.array_equal(i1, nms_order(probs[:, 1])[:100])


def _reference_levels(boxes, image_h, image_w):
    """model.py:357-367 in f32 numpy: log2_graph is tf.log(x) / tf.log(2.0); tf.round is np.rint (half to even)"""
    h = boxes[:, 2] - boxes[:, 0]
    w = boxes[:, 3] - boxes[:, 1]
    image_area = F(image_h * image_w)
    roi_level = np.log(np.sqrt(h * w) / (F(224.0) / np.sqrt(image_area))) / np.log(F(2.0))
    assert roi_level.dtype == F
    return np.minimum(5, np.maximum(2, 4 + np.rint(roi_level).astype(np.int32)))


@pytest.mark.parametrize("image", [(1024, 1024), (512, 640), (64, 64)])
def test_level_rule_equals_the_reference_expression(image):
    """20 000 random boxes; those within 1e-4 of a rounding boundary of log2 (where the reference's f32 logarithm, not the rule, decides) are left out"""
    ih, iw = image
    rng = np.random.default_rng(ih * 7 + iw)
    n = 20000
    side = np.exp(rng.uniform(np.log(0.01), np.log(1.0), (n, 2)))
    y1, x1 = rng.uniform(0, 1 - side[:, 0]), rng.uniform(0, 1 - side[:, 1])
    boxes = np.stack([y1, x1, y1 + side[:, 0], x1 + side[:, 1]], axis=1).astype(F)
    s = np.sqrt((boxes[:, 2] - boxes[:, 0]).astype(np.float64) * (boxes[:, 3] - boxes[:, 1]).astype(np.float64))
    l2 = np.log2(s / (224.0 / np.sqrt(float(ih * iw))))
    near = np.zeros(n, bool)
    for k in (3, 4, 5):
        near |= np.abs(l2 - (k - 4.5)) < 1e-4
    print("left out:", int(near.sum()), "of", n)
    assert near.mean() <= 0.01 and near.sum() <= 40          # the generator stays far below the 1 % the rule allows
    got = kl.levels(boxes, ih, iw)
    ref = _reference_levels(boxes, ih, iw)
    assert np.array_equal(got[~near], ref[~near])
    assert set(np.unique(got)) == ({2, 3, 4, 5} if ih > 64 else {2})


def test_level_rule_at_the_thresholds():
    """s exactly at T0, T1, T2 and one f32 step to either side: 2|2|3, 3|4|4, 4|4|5 -- half to even; zero and NaN: level 2"""
    T = kl.level_thresholds(1024, 1024)
    want = [(2, 2, 3), (3, 4, 4), (4, 4, 5)]
    for t, w in zip(T, want):
        for s, lv in zip((np.nextafter(t, F(0)), t, np.nextafter(t, F(9))), w):
            b = np.asarray([[0, 0, 1, 0]], F)
            b[0, 3] = _area_with_root(s)                                    # height 1: the product is the width, whose f32 square root is s
            assert kl.levels(b, 1024, 1024)[0] == lv, (s, lv)
    assert kl.levels(np.zeros((1, 4), F), 1024, 1024)[0] == 2
    assert kl.levels(np.asarray([[0, 0, np.nan, 1]], F), 1024, 1024)[0] == 2
    assert kl.levels(np.asarray([[0.5, 0.5, 0.2, 0.9]], F), 1024, 1024)[0] == 2     # a negative product: sqrt is NaN


def _area_with_root(s):
    """an f32 area whose correctly rounded f32 square root is exactly s"""
    a = F(np.float64(s) * np.float64(s))
    for cand in (a, np.nextafter(a, F(0)), np.nextafter(a, F(9))):
        if np.sqrt(F(cand)) == s:
            return F(cand)
    raise AssertionError(s)


def test_thresholds_entry_equals_the_statement():
    import instancefusion_amd as ifx

    for ih, iw in ((1024, 1024), (64, 64), (512, 640), (1, 1), (800, 1333), (46340, 46340)):
        got = ifx.pyramid_level_thresholds(ih, iw)
        assert np.array_equal(got.view(np.uint32), kl.level_thresholds(ih, iw).view(np.uint32)), (ih, iw)
    L = ifx.lib()
    o = np.zeros(3, F)
    assert L.ifx_pyramid_level_thresholds(0, 64, o.ctypes.data) == -1 and L.ifx_pyramid_level_thresholds(64, -1, o.ctypes.data) == -1
    assert L.ifx_pyramid_level_thresholds(64, 64, None) == -1
    with pytest.raises(ifx.IfxError):
        ifx.pyramid_level_thresholds(0, 0)


def test_thresholds_header_under_sanitizers(tmp_path):
    """tests/cpp/keras_levels_check.cpp over ifx_detector_prep.hpp with g++ -fsanitize=address,undefined (a program of its own: nothing sanitised is loaded into
    Python): the thresholds of a list of image sizes, as bit patterns, equal the statement's"""
    exe = str(tmp_path / "keras_levels_check")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "include"),
                    "-I", os.path.join(ROOT, "instancefusion_amd", "host"), os.path.join(ROOT, "tests", "cpp", "keras_levels_check.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    lines = r.stdout.splitlines()
    assert lines[-1] == "ok", r.stdout[-2000:]
    rows = [ln.split() for ln in lines if ln.startswith("thr ")]
    assert len(rows) >= 6
    for _, ih, iw, a, b, c in rows:
        want = kl.level_thresholds(int(ih), int(iw)).view(np.uint32)
        assert [int(a, 16), int(b, 16), int(c, 16)] == [int(v) for v in want], (ih, iw)


@pytest.mark.parametrize("pool", [(7, 7), (14, 14), (3, 5)])
def test_sampling_against_grid_sample(pool):
    """boxes wholly inside the map against torch.nn.functional.grid_sample(align_corners=True) on the CPU, per level; tolerance 2 (Hl + Wl) 2^-23 max|x|: the
    coordinate's rounding times the largest possible slope between neighbouring samples"""
    import torch

    rng = np.random.default_rng(pool[0] * 31 + pool[1])
    ih = iw = 512                                       # c = 0.4375: boxes inside the unit square reach all four levels (at 64 x 64 every one is level 2)
    C, n = 5, 120
    feats = [rng.standard_normal((1, s, s, C)).astype(F) for s in (16, 8, 4, 2)]
    side = np.exp(rng.uniform(np.log(0.03), np.log(0.95), (n, 2)))
    side[:20] = rng.uniform(0.7, 0.95, (20, 2))         # level 5
    y1, x1 = rng.uniform(0, 1 - side[:, 0]), rng.uniform(0, 1 - side[:, 1])
    boxes = np.stack([y1, x1, y1 + side[:, 0], x1 + side[:, 1]], axis=1).astype(F)
    boxes = np.clip(boxes, 0, 1)[None]
    out, lv = kl.pyramid_roi_align(feats, boxes, (ih, iw), pool)
    assert set(np.unique(lv)) == {2, 3, 4, 5}
    ph, pw = pool
    for r in range(n):
        f = feats[lv[0, r] - 2]
        y1, x1, y2, x2 = boxes[0, r].astype(np.float64)
        gy = 2.0 * (y1 + np.arange(ph) * (y2 - y1) / (ph - 1)) - 1.0
        gx = 2.0 * (x1 + np.arange(pw) * (x2 - x1) / (pw - 1)) - 1.0
        grid = np.stack(np.broadcast_arrays(gx[None, :], gy[:, None]), axis=-1)[None].astype(F)
        ref = torch.nn.functional.grid_sample(torch.from_numpy(f).permute(0, 3, 1, 2), torch.from_numpy(grid), mode="bilinear", padding_mode="zeros", align_corners=True)
        ref = ref[0].permute(1, 2, 0).numpy()
        tol = 2.0 * (f.shape[1] + f.shape[2]) * 2.0 ** -23 * float(np.abs(f).max())
        assert np.abs(out[0, r].astype(np.float64) - ref.astype(np.float64)).max() <= tol, (r, int(lv[0, r]))


def test_sampling_edges():
    """the zero row: every bin the top-left texel; outside: zeros; ending at 1.0: the last texel, floor == ceil; beyond 1.0: a zero band; flipped; NaN; 1 x 1"""
    rng = np.random.default_rng(3)
    feats = [rng.standard_normal((1, s, s, 2)).astype(F) for s in (16, 8, 4, 2)]
    boxes = np.asarray([[[0, 0, 0, 0], [1.5, 1.5, 1.8, 1.9], [0.5, 0.5, 1.0, 1.0], [0.5, 0.5, 1.25, 1.0], [0.9, 0.1, 0.1, 0.9], [np.nan, 0, 1, 1],
                         [0.25, 0.25, 0.75, 0.75]]], F)
    out, lv = kl.pyramid_roi_align(feats, boxes, (64, 64), (7, 7))
    assert (lv[0, :6] == 2).all() and (out[0, 0] == feats[0][0, 0, 0]).all()
    assert (out[0, 1] == 0).all() and (out[0, 5] == 0).all() and lv[0, 5] == 2
    f = feats[lv[0, 2] - 2][0]
    assert np.array_equal(out[0, 2][-1, -1], f[-1, -1])
    band = out[0, 3]
    assert (band[-1] == 0).all() and (band[0] != 0).any()
    straight, _ = kl.pyramid_roi_align(feats, np.asarray([[[0.1, 0.1, 0.9, 0.9]]], F), (64, 64), (7, 7))
    assert np.allclose(out[0, 4], straight[0, 0][::-1], atol=1e-5)
    one, _ = kl.pyramid_roi_align(feats, boxes[:, 6:], (64, 64), (1, 1))
    f = feats[lv[0, 6] - 2][0]
    s = f.shape[0] - 1
    assert one.shape == (1, 1, 1, 1, 2) and np.isfinite(one).all() and 0.5 * s == np.floor(0.5 * s) + 0.5     # the centre lies between four texels
    c = int(np.floor(0.5 * s))
    assert np.allclose(one[0, 0, 0, 0], f[c:c + 2, c:c + 2].mean(axis=(0, 1)), atol=1e-6)


def test_detection_statement_by_hand():
    """four rows on a 64 x 64 image, zero deltas: background, below the confidence, two overlapping boxes of one class"""
    rois = np.asarray([[0, 0, 0.5, 0.5], [0.1, 0.1, 0.6, 0.6], [0, 0, 0.5, 0.5], [0.03125, 0, 0.5, 0.5]], F)
    probs = np.asarray([[0.9, 0.05, 0.05], [0.3, 0.6, 0.1], [0.1, 0.1, 0.8], [0.05, 0.05, 0.9]], F)
    deltas = np.zeros((4, 3, 4), F)
    det, norm, index = kl.keras_detections(rois, probs, deltas, (0, 0, 64, 64), (64, 64), min_confidence=0.7, nms_threshold=0.3, max_instances=5)
    assert index.tolist() == [3] and det.tolist() == [[2.0, 0.0, 32.0, 32.0, 2.0, F(0.9)]]
    assert norm.tolist() == [[0.03125, 0.0, 0.5, 0.5]]
    det, _, index = kl.keras_detections(rois, probs, deltas, (0, 0, 64, 64), (64, 64), min_confidence=0.0, nms_threshold=0.3, max_instances=5)
    assert index.tolist() == [3, 1] and det[1].tolist() == [6.0, 6.0, 38.0, 38.0, 1.0, F(0.6)]
    det, _, index = kl.keras_detections(rois, probs, deltas, (8, 8, 24, 64), (64, 64), min_confidence=0.0, nms_threshold=1.0, max_instances=5)
    assert index.tolist() == [3, 2, 1] and det[0, :4].tolist() == [8.0, 8.0, 24.0, 32.0]
    # half to even: (2k + 1) / (2 H) times H is k + 0.5
    rois = np.asarray([[(2 * k + 1) / 128.0, 0, 0.75, 0.75] for k in range(4)], F)
    probs = np.tile(np.asarray([[0.1, 0.9]], F), (4, 1))
    det, _, index = kl.keras_detections(rois, probs, np.zeros((4, 2, 4), F), (0, 0, 64, 64), (64, 64), min_confidence=0.5, nms_threshold=1.0, max_instances=4)
    assert det[np.argsort(index), 0].tolist() == [0.0, 2.0, 2.0, 4.0]
