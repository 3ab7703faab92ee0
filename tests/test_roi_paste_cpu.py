"""The ROI paste without a GPU: the float32 statement the kernels follow (tests/roi_paste_numpy.py) against the masks maskrcnn-benchmark's own
paste_mask_in_image made of the same inputs (tests/golden/roi_paste_ref.npz, written by tools/make_golden_roi_paste.py), and the three C-ABI entries in the header
and the binding."""
import re

import numpy as np
import pytest

import roi_paste_numpy as rp

ENTRIES = ("ifx_process_segmentation_rois", "ifx_process_segmentation_deferred_rois", "ifx_paste_roi_masks")


@pytest.fixture(scope="module")
def fixture_cases():
    return rp.load_fixture()


def test_fixture_covers_the_cases(fixture_cases):
    c = fixture_cases
    assert {(k["W"], k["H"]) for k in c} == {(160, 120), (320, 240)}
    assert {k["M"] for k in c} == {7, 14, 28, 29, 56}
    assert {round(k["thr"], 2) for k in c} == {0.5, 0.25, 0.7}
    for M in (7, 14, 28, 29, 56):
        b = np.stack([k["box"] for k in c if k["M"] == M])
        w, h = b[:, 2] - b[:, 0], b[:, 3] - b[:, 1]
        assert (w < 1).any() and ((w >= 1) & (w <= 3)).any() and (w > 100).any()
    for W, H in ((160, 120), (320, 240)):
        b = np.stack([k["box"] for k in c if k["W"] == W])
        assert (b[:, 0] == 0).any() and (b[:, 1] == 0).any() and (b[:, 2] == W - 1).any() and (b[:, 3] == H - 1).any()
        assert ((b == (0, 0, W - 1, H - 1)).all(axis=1)).any()                      # the whole image
        assert (b % 1 == 0).all(axis=1).any() and (b % 1 == 0.5).all(axis=1).any()   # integer and half-integer corners
    assert all(k["ref"].any() for k in c if k["box"][2] - k["box"][0] > 100)


def test_statement_equals_the_reference_outside_the_tie_band(fixture_cases):
    """Every pixel whose interpolated value is farther than 2^-22 from the threshold equals the reference's; the band holds at most 1 of every 10^5 box pixels."""
    box_px = band_px = 0
    for k, c in enumerate(fixture_cases):
        mine, band = rp.paste_roi(c["roi"], c["box"], c["W"], c["H"], c["thr"], with_band=True)
        rect, _ = rp.paste_values(c["roi"], c["box"], c["W"], c["H"])
        assert rect is not None, k
        box_px += (rect[1] - rect[0]) * (rect[3] - rect[2])
        band_px += int(band.sum())
        diff = ((mine != 0) != c["ref"]) & ~band
        assert not diff.any(), (k, c["M"], c["box"], np.argwhere(diff)[:4])
    print(f"{box_px} box pixels, {band_px} within 2^-22 of the threshold")
    assert box_px > 1000000
    assert band_px * 100000 <= box_px, (band_px, box_px)


def test_empty_where_the_reference_raises():
    roi = np.full((7, 7), 0.9, np.float32)
    for box in ([np.nan, 0, 5, 5], [0, 0, np.inf, 5], [-50, -50, -40, -40], [200, 10, 220, 20], [0, 0, 3e7, 5], [-3e7, 0, 5, 5]):
        assert not rp.paste_roi(roi, box, 160, 120, 0.5).any(), box
    assert rp.paste_roi(roi, [10, 10, 20, 20], 160, 120, 0.5).any()
    assert not rp.paste_roi(roi, [20, 10, 10, 20], 160, 120, 0.5).any()       # x1 < x0: the expanded box holds no column
    nan = roi.copy(); nan[3, 3] = np.nan
    m = rp.paste_roi(nan, [10, 10, 20, 20], 160, 120, 0.5)
    assert m.any() and not m[15, 15]                                           # NaN compares false: outside


def test_order_is_stable_and_clean_keeps_the_last():
    roi = np.full((2, 4, 4), 0.9, np.float32)
    boxes = np.array([[10, 10, 20, 20], [14, 10, 24, 20]], np.float32)
    ori, clean, order, cls = rp.paste_rois(roi, boxes, [7, 8], 160, 120, 0.5)
    assert order.tolist() == [0, 1] and cls.tolist() == [7, 8]                 # equal areas keep their input order
    assert (ori[0] != 0).sum() == (ori[1] != 0).sum() > 0
    both = (ori[0] != 0) & (ori[1] != 0)
    assert both.any() and not clean[0][both].any() and np.array_equal(clean[1], ori[1])


def test_header_declares_and_binding_covers_the_entries():
    import instancefusion_amd as m

    header = open(m.HEADER_PATH).read()
    bound = m.exported_symbols()
    for name in ENTRIES:
        decl = re.search(r"\bint\s+" + name + r"\s*\(([^;]*)\);", header)
        assert decl, name
        assert name in bound, name
        assert len(m._SIGS[name][1]) == decl.group(1).count(",") + 1, name
    assert "inference.py:91-154" in header
    for meth in ("process_segmentation_rois", "process_segmentation_deferred_rois", "paste_roi_masks"):
        assert callable(getattr(m.InstanceFusion, meth)), meth
