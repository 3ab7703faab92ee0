"""The mask head's select / sigmoid stage without a GPU: the numpy statement the kernels follow (tests/mask_head_numpy.py) against what maskrcnn-benchmark's own
MaskPostProcessor, BoxList.resize, Masker and select_top_predictions made of the same inputs (tests/golden/mask_head_ref.npz, written by
tools/make_golden_mask_head.py), the rule's edges (tests/mask_head_cases.py), and the three C-ABI entries in the header and the binding."""
import re

import numpy as np
import pytest

import mask_head_cases as mc
import mask_head_numpy as mh
import roi_paste_numpy as rp

F = np.float32
ENTRIES = ("ifx_mask_head_select", "ifx_process_segmentation_detections", "ifx_process_segmentation_deferred_detections")


@pytest.fixture(scope="module")
def fixture():
    return mh.load_fixture()


def test_fixture_covers_the_cases(fixture):
    cases, _ = fixture
    assert {c["M"] for c in cases} == {7, 14, 28} and {c["C"] for c in cases} == {2, 81} and {c["R"] for c in cases} == {1, 5, 40}
    assert {(c["W"], c["H"], c["in_size"]) for c in cases} == {(w, h, s) for (w, h) in ((160, 120), (320, 240)) for s in ((800, 600), (801, 607))}
    for c in cases:
        assert c["labels"].min() >= 0 and c["labels"].max() == c["C"] - 1 and not (c["q"] == 128).any()
        if c["R"] >= 5:
            assert c["scores"][0] == F(0.7) and 0 not in c["ref_rows"]                 # exactly at the threshold: out
            assert (c["labels"] == 0).any()
            kept = c["scores"][c["ref_rows"]]
            assert len(np.unique(kept)) < len(kept)                                    # exact ties among the kept scores
        if c["R"] == 40:
            assert (c["scores"] == np.nextafter(F(0.7), F(1))).any()
    assert sum(len(c["ref_rows"]) for c in cases) > 100


def test_statement_equals_the_reference(fixture):
    """Kept rows: the same set, and the same score at every place of the order (among equal scores torch's unstable sort permits any order; the rule's is by
    ascending row).  Resized boxes: bit-equal.  Pasted masks: equal pixel for pixel outside the tie band 2^-22 + the largest difference between SIGMOID and torch's
    CPU sigmoid that the tool measured on these samples; the band holds at most 1 of every 10^4 box pixels."""
    cases, meta = fixture
    band = mh.PASTE_BAND + meta["sigmoid_max_abs"]
    assert 0.0 <= meta["sigmoid_max_abs"] < 2.0 ** -20, meta                           # (a few ulp of a probability: the band stays a band)
    box_px = band_px = 0
    for c in cases:
        masks, boxes, cls, rows = mh.mask_head_select(c["logits"], c["boxes"], c["scores"], c["labels"], c["in_size"], (c["W"], c["H"]), 0.7, True)
        assert sorted(rows.tolist()) == sorted(c["ref_rows"].tolist())
        assert np.array_equal(c["scores"][rows], c["scores"][c["ref_rows"]])
        for s in np.unique(c["scores"][rows]):
            assert (np.diff(rows[c["scores"][rows] == s]) > 0).all()
        assert np.array_equal(cls, c["labels"][rows])
        at = {int(r): j for j, r in enumerate(c["ref_rows"])}
        for j, r in enumerate(rows):
            ref_j = at[int(r)]
            assert np.array_equal(boxes[j].view(np.uint32), c["ref_boxes"][ref_j].view(np.uint32)), (c["in_size"], boxes[j], c["ref_boxes"][ref_j])
            rect, v = rp.paste_values(masks[j], boxes[j], c["W"], c["H"])
            X0, X1, Y0, Y1 = rect
            tie = np.zeros((c["H"], c["W"]), bool)
            tie[Y0:Y1, X0:X1] = np.abs(v.astype(np.float64) - 0.5) <= band
            mine = rp.paste_roi(masks[j], boxes[j], c["W"], c["H"], 0.5) != 0
            box_px += (X1 - X0) * (Y1 - Y0)
            band_px += int(tie.sum())
            diff = (mine != c["ref_masks"][ref_j]) & ~tie
            assert not diff.any(), (c["R"], c["C"], c["M"], int(r), np.argwhere(diff)[:4])
    print(f"{box_px} box pixels, {band_px} within {band:.3e} of the threshold")
    assert box_px > 500000 and band_px * 10000 <= box_px, (band_px, box_px)


def test_sigmoid_measured_against_torch(fixture):
    """The figure in the fixture and in the header is what this machine's torch gives on the fixture's samples, give or take nothing."""
    import torch

    cases, meta = fixture
    worst = 0.0
    for c in cases:
        x = c["logits"][np.arange(c["R"]), c["labels"]]
        worst = max(worst, float(np.abs(mh.sigmoid(x).astype(np.float64) - torch.from_numpy(x).sigmoid().numpy().astype(np.float64)).max()))
    print(f"largest |SIGMOID - torch.sigmoid| on the fixture's samples: {worst:.6e}; the fixture says {meta['sigmoid_max_abs']:.6e} ({meta['sigmoid_max_ulp']:.3f} ulp)")
    assert worst <= meta["sigmoid_max_abs"]
    import instancefusion_amd as m
    assert f"differ by at most {meta['sigmoid_max_abs']:.6e} ({meta['sigmoid_max_ulp']:.3f} ulp of torch's value)" in open(m.HEADER_PATH).read()


def test_sigmoid_edges():
    x = np.asarray([200, -200, np.inf, -np.inf, 104, -104, 0, -0.0, 17, 1e-30], F)
    p = mh.sigmoid(x)
    assert p.tolist() == [1.0, 0.0, 1.0, 0.0, 1.0, 0.0, 0.5, 0.5, 1.0, 0.5]
    assert np.isnan(mh.sigmoid(np.asarray([np.nan], F))[0])
    xs = np.linspace(-30, 30, 4001).astype(F)
    true = 1.0 / (1.0 + np.exp(-xs.astype(np.float64)))
    # one rounding each from EXP, the sum and the division, each at most 2^-24 relative (the error of e reaches d scaled by e / (1 + e) < 1)
    assert (np.abs(mh.sigmoid(xs).astype(np.float64) - true) <= 3.0 * 2.0 ** -24 * true * (1 + 1e-6)).all()
    assert (np.diff(mh.sigmoid(xs)) >= 0).all()


def _independent(c):
    """The rule once more, row by row in plain Python."""
    R, C = c["logits"].shape[:2]
    n = R if c["count"] is None else min(max(c["count"], 0), R)
    t = F(c["score_thresh"])
    rows = [r for r in range(n) if 0 <= int(c["labels"][r]) < C and (t == F(-np.inf) or c["scores"][r] > t)]
    if c["sort_by_score"]:
        def key(r):
            s = c["scores"][r]
            return (1, 0.0, r) if np.isnan(s) else (0, -float(s), r)
        rows.sort(key=key)
    return rows


def test_edges_of_the_rule():
    cases = mc.edge_cases() + [("R = 1024, many equal scores", mc.many_equal_scores())] + [("R = 1", mc.head(3, 1, 1, 1)), ("R = 0", mc.head(3, 0, 3, 4))]
    seen_nan_kept = False
    for name, c in cases:
        masks, boxes, cls, rows = mh.mask_head_select(**c)
        R, C, M = c["logits"].shape[0], c["logits"].shape[1], c["logits"].shape[3]
        assert rows.tolist() == _independent(c), name
        assert masks.shape == (len(rows), M, M) and boxes.shape == (len(rows), 4) and cls.dtype == np.int32 and rows.dtype == np.int32, name
        lab = c["labels"][rows]
        assert ((lab >= 0) & (lab < C)).all(), name
        assert np.array_equal(cls, lab if c["class_map"] is None else c["class_map"][lab]), name
        seen_nan_kept |= bool(np.isnan(c["scores"][rows]).any())
        pm, pb, pc, pr, k = mh.padded((masks, boxes, cls, rows), R)
        assert k[0] == len(rows) and (pc[k[0]:] == -1).all() and (pr[k[0]:] == -1).all() and not pm[k[0]:].any() and not pb[k[0]:].any(), name
    assert seen_nan_kept                                        # only score_thresh == -inf lets a NaN score through
    by = dict(cases)
    assert len(mh.mask_head_select(**by["count 0"])[3]) == 0 and len(mh.mask_head_select(**by["count negative"])[3]) == 0
    assert np.array_equal(mh.mask_head_select(**by["count R"])[3], mh.mask_head_select(**by["count above R"])[3])
    assert len(mh.mask_head_select(**by["every row kept"])[3]) == 64 and len(mh.mask_head_select(**by["none kept"])[3]) == 0
    rows = mh.mask_head_select(**by["NaN, +-inf, score == thresh, +-0"])[3].tolist()
    assert rows[0] == 2 and 5 in rows and not {1, 3, 4, 6, 7, 8} & set(rows)
    rows = mh.mask_head_select(**by["the same, thresh -inf"])[3].tolist()
    assert rows[0] == 2 and rows[-3:] == [3, 1, 8] and rows.index(6) + 1 == rows.index(7)          # -0 == +0 by row; -inf, then the NaNs by row
    m = mh.mask_head_select(**by["logits +-200, +-inf, NaN, EXP's clamps"])[0]
    assert np.isnan(m).sum() == 1 and (m[~np.isnan(m)] >= 0).all() and (m[~np.isnan(m)] <= 1).all() and (m == 1).any() and (m == 0).any()
    c = by["out == in"]
    assert np.array_equal(mh.mask_head_select(**c)[1], c["boxes"][mh.mask_head_select(**c)[3]])
    with pytest.raises(AssertionError):
        mh.mask_head_select(**dict(by["plain"], score_thresh=float("nan")))


def test_header_declares_and_binding_covers_the_entries():
    import instancefusion_amd as m

    header = open(m.HEADER_PATH).read()
    bound = m.exported_symbols()
    for name in ENTRIES:
        decl = re.search(r"\bint\s+" + name + r"\s*\(([^;]*)\);", header)
        assert decl, name
        assert name in bound, name
        assert len(m._SIGS[name][1]) == decl.group(1).count(",") + 1, name
    for cite in ("inference.py:27-61", "predictor.py:224-243", "bounding_box.py:91-127", "mask_benchmark.py:54-82"):
        assert cite in header, cite
    assert callable(m.ElasticFusion.mask_head_select) and callable(m.mask_post_processor)
    for meth in ("process_segmentation_detections", "process_segmentation_deferred_detections"):
        assert callable(getattr(m.InstanceFusion, meth)), meth
