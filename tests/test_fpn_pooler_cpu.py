"""Multi-level ROI pooling without a GPU: the numpy statement (tests/fpn_pooler_numpy.py) against the golden file made from maskrcnn-benchmark's own Pooler.forward
and LevelMapper on the CPU (tools/make_golden_fpn_pooler.py) -- every level equal, every pooled output equal in its bits, on every Pooler case, every swept v and
every edge box; the thresholds the library's host side makes (ifx_fpn_level_thresholds) against the rule on the same sweeps; one level against plain ROIAlign."""
import ctypes as C
import os

import numpy as np
import pytest

import detector_ops_numpy as dn
import fpn_pooler_numpy as fp
from conftest import ROOT

GOLDEN = os.path.join(ROOT, "tests", "golden", "fpn_pooler_ref.npz")
F = np.float32


@pytest.fixture(scope="module")
def golden():
    return dict(np.load(GOLDEN))


def golden_case(golden, k):
    scales = golden[f"pool{k}_scales"]
    feats = [golden[f"pool{k}_feat{l}"] for l in range(scales.size)]
    res, ratio = (int(v) for v in golden[f"pool{k}_par"])
    return feats, golden[f"pool{k}_rois"], [float(s) for s in scales], res, ratio, golden[f"pool{k}_out"], golden[f"pool{k}_levels"]


def _step(x, k):
    return (np.asarray(x, F).view(np.uint32).astype(np.int64) + k).astype(np.uint32).view(F)


def test_statement_equals_the_reference_pooler_bit_for_bit(golden):
    cases = int(golden["counts"][0])
    assert cases == 26
    seen_levels, seen_res, seen_ratio, none, outputs = set(), set(), set(), 0, 0
    per_level = np.zeros(8, np.int64)
    for k in range(cases):
        feats, rois, scales, res, ratio, ref, ref_lev = golden_case(golden, k)
        out, lev = fp.fpn_roi_align(feats, rois, scales, res, res, ratio)
        assert lev.dtype == ref_lev.dtype == np.int32 and np.array_equal(lev, ref_lev), k
        assert out.shape == ref.shape and out.dtype == ref.dtype == F
        assert np.array_equal(out.view(np.uint32), ref.view(np.uint32)), k
        assert not ref[ref_lev < 0].any()
        seen_levels.add(len(scales)); seen_res.add(res); seen_ratio.add(ratio)
        none += int((ref_lev < 0).sum())
        per_level[:len(scales)] += np.bincount(ref_lev[ref_lev >= 0], minlength=len(scales))
        outputs += ref.size
    assert seen_levels == {1, 2, 3, 4, 8} and seen_res == {1, 2, 7, 14} and seen_ratio == {0, 1, 2}
    assert (per_level > 0).all() and none >= 40 and outputs > 25000


def test_level_rule_equals_the_reference_on_every_swept_v(golden):
    v = golden["sweep_v"]
    want = np.concatenate([_step(F(2.0 ** k), np.arange(-16, 17)) for k in range(-6, 4)])       # every f32 within 16 ulp of 2^-6 .. 2^3
    assert np.array_equal(v.view(np.uint32), want.view(np.uint32))
    for lvl0 in (4, 7):
        l0, k_min, k_max = (int(x) for x in golden[f"sweep_par_l{lvl0}"])
        ref = golden[f"sweep_levels_l{lvl0}"]
        assert l0 == lvl0 and ref.size == v.size == 330 and ref.min() == 0
        assert np.array_equal(fp.level_of_v(v, k_min, k_max, lvl0), ref)
    ref = golden["sweep_levels_l4"]
    # the two roundings show: a few v just below each power of two already have the upper level, which the exponent of v alone would not give
    exponent = np.clip(np.floor(np.log2(v.astype(np.float64))) + 4, -2, 7) + 2
    assert 10 <= int((exponent != ref).sum()) <= 50 and (ref >= exponent).all()


def test_level_rule_equals_the_reference_on_every_edge_box(golden):
    rois, ref = golden["edge_rois"], golden["edge_levels"]
    assert rois.shape == (int(golden["counts"][2]), 5) and ref.shape == (rois.shape[0],)
    assert np.array_equal(fp.levels(rois, 2, 5), ref)
    with np.errstate(invalid="ignore"):
        s = np.sqrt((rois[:, 3] - rois[:, 1] + F(1)) * (rois[:, 4] - rois[:, 2] + F(1)))
    for x in (56, 112, 224, 448, 896):                          # sqrt(area) exactly at the canonical sizes and one f32 step either side
        for k in (-1, 0, 1):
            assert (s == _step(F(x), k)).any(), (x, k)
    assert ref[-7:].tolist() == [3, 3, -1, -1, -1, 0, 0]        # areas +inf, +inf, NaN, NaN, negative, 0, 1
    assert set(ref.tolist()) == {-1, 0, 1, 2, 3}


def test_host_thresholds_reproduce_the_rule_on_the_sweeps(golden):
    import instancefusion_amd as ifx

    v = golden["sweep_v"]
    ladder = [2.0 ** -k for k in range(8)]                      # k_min 0, k_max 7: with canonical level 4 the edges 2^-3 .. 2^3, with 7 the edges 2^-6 .. 2^0
    for lvl0 in (4, 7):
        k_min, T = ifx.fpn_level_thresholds(ladder, lvl0)
        assert k_min == 0 and T.dtype == F and T.size == 7
        assert np.array_equal(T.view(np.uint32), fp.level_thresholds(0, 7, lvl0).view(np.uint32))
        got = fp.level_by_thresholds(v, T)
        assert np.array_equal(got, fp.level_of_v(v, 0, 7, lvl0))
        l0, ref_min, ref_max = (int(x) for x in golden[f"sweep_par_l{lvl0}"])
        assert np.array_equal(got, np.clip(golden[f"sweep_levels_l{lvl0}"] + ref_min, 0, 7))    # and the reference's own answer, clamped to this ladder
        assert set(got.tolist()) == set(range(8))
    # the released ladder on the edge boxes and on the golden ROIs
    k_min, T = ifx.fpn_level_thresholds([0.25, 0.125, 0.0625, 0.03125])
    assert k_min == 2 and T.size == 3
    assert np.array_equal(fp.level_by_thresholds(fp.v_of_rois(golden["edge_rois"]), T), golden["edge_levels"])
    for k in range(int(golden["counts"][0])):
        feats, rois, scales, res, ratio, ref, ref_lev = golden_case(golden, k)
        if len(scales) > 1:
            _, T = ifx.fpn_level_thresholds(scales)
            assert np.array_equal(fp.level_by_thresholds(fp.v_of_rois(rois), T), ref_lev), k
    # a negative eps can give a v below 0: no level by the rule (log2 is NaN), and by the thresholds
    v_neg = np.asarray([-1e-3, -0.0, 0.0, np.nan, np.inf], F)
    assert fp.level_of_v(v_neg, 2, 5).tolist() == fp.level_by_thresholds(v_neg, T).tolist() == [-1, 0, 0, -1, 3]


def test_host_thresholds_refuse_what_is_no_ladder():
    import instancefusion_amd as ifx

    L = ifx.lib()
    out = np.zeros(8, F)

    def call(scales, levels=None, p_out=out):
        sc = np.asarray(scales, F)
        return L.ifx_fpn_level_thresholds(sc.ctypes.data_as(C.c_void_p), len(scales) if levels is None else levels, 4,
                                          None if p_out is None else p_out.ctypes.data_as(C.c_void_p))

    assert call([0.25, 0.125]) == 2 and call([1.0]) == 0 and call([2.0 ** -k for k in range(119, 127)]) == 119
    for bad in ([0.3, 0.15], [0.25, 0.25], [0.25, 0.0625], [0.125, 0.25], [2.0, 1.0], [0.0], [-0.25], [np.nan], [np.inf], [2.0 ** -k for k in range(120, 128)],
                [2.0 ** -k for k in range(9)]):
        assert call(bad) == -1, bad
        assert fp.ladder(bad) is None
    assert call([0.25], levels=0) == -1 and call([0.25], p_out=None) == -1
    assert L.ifx_fpn_level_thresholds(None, 1, 4, out.ctypes.data_as(C.c_void_p)) == -1


def test_one_level_is_plain_roi_align(golden):
    rng = np.random.default_rng(5)
    feat = rng.standard_normal((2, 3, 9, 11)).astype(F)
    rois = np.asarray([[0, 2, 3, 30, 28], [1, -5, -5, 60, 50], [0, 30, 10, 10, 40], [1, 5, 5, 4, 4], [2, 0, 0, 9, 9]], F)   # a negative area and a batch index of 2 too
    out, lev = fp.fpn_roi_align([feat], rois, [0.25], 7, 7, 2)
    assert np.array_equal(out.view(np.uint32), dn.roi_align_forward(feat, rois, F(0.25), 7, 7, 2).view(np.uint32)) and not lev.any()
    assert out[2].any() and not out[4].any()
    multi, lev = fp.fpn_roi_align([feat, feat[:, :, :5, :6]], rois, [0.25, 0.125], 7, 7, 2)
    assert lev.tolist() == [0, 0, -1, 0, 0] and not multi[2].any() and np.array_equal(multi[:2], out[:2])
    seen = 0
    for k in range(int(golden["counts"][0])):
        feats, rois, scales, res, ratio, ref, ref_lev = golden_case(golden, k)
        if len(scales) == 1:
            assert np.array_equal(dn.roi_align_forward(feats[0], rois, F(scales[0]), res, res, ratio).view(np.uint32), ref.view(np.uint32)) and not ref_lev.any()
            seen += 1
    assert seen >= 3
