"""CPU side of the adversarial superpixel cases (tests/slic_cases.py): the oracle's SLIC against labels of the reference's own gSLICr per-pixel functions
(tests/golden/slic_cases_ref.npz from tools/make_golden.py; live as well when oracle/_ref is built), the coverage those labels give -- asserted from the stored
labels, so that a later change of the generators cannot quietly empty the GPU tests -- and the oracle's merge against the numpy restatement of mergeSuperPixel on
labelings whose neighbour lists are capped and whose superpixels are emptied by the re-clustering."""
import ctypes as C
import os

import numpy as np
import pytest

import slic_cases as sc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF_SO = os.path.join(ROOT, "oracle", "_ref", "libref_slic.so")


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(os.path.join(ROOT, "tests", "golden", "slic_cases_ref.npz")))


def _oracle(orc, w, h):
    return orc.Oracle(w=w, h=h, max_surfels=1000, **sc.camera(w, h))


def test_golden_holds_every_case(gold):
    want = {sc.key(*c) for c in sc.golden_cases()}
    assert set(gold) == want and len(want) == 2 * 12 + 2 * 5
    for name, w, h in sc.golden_cases():
        a = gold[sc.key(name, w, h)]
        assert a.shape == (h, w) and a.dtype == np.int16 and a.min() >= 0 and a.max() < (w // 16) * (h // 16)


def test_oracle_slic_equals_golden(orc, gold):
    for (w, h) in sc.TINY_SIZES + sc.MID_SIZES:
        o = _oracle(orc, w, h)
        for name in sc.IMAGES:
            if sc.key(name, w, h) not in gold:
                continue
            seg, n = o.slic_segment(sc.image(name, w, h))
            assert n == (w // 16) * (h // 16)
            assert np.array_equal(seg, gold[sc.key(name, w, h)].astype(np.int32)), (name, w, h)
        o.close()


@pytest.mark.skipif(not os.path.exists(REF_SO), reason="oracle/_ref not built (needs /root/reference)")
def test_oracle_slic_equals_reference_build_live(orc, gold):
    ref = C.CDLL(REF_SO)
    ref.ref_slic_segment.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_float, C.c_int, C.c_void_p]
    for (w, h) in sc.TINY_SIZES + sc.MID_SIZES:
        o = _oracle(orc, w, h)
        for name in sc.IMAGES:
            rgb = sc.image(name, w, h)
            seg, n = o.slic_segment(rgb)
            rs = np.zeros((h, w), np.int32)
            assert ref.ref_slic_segment(rgb.ctypes.data, w, h, 16, 0.6, 5, rs.ctypes.data) == n
            assert np.array_equal(seg, rs), (name, w, h)
            if sc.key(name, w, h) in gold:      # the fixture is what this build writes: tools/make_golden.py regenerates it array for array
                assert np.array_equal(rs, gold[sc.key(name, w, h)].astype(np.int32)), (name, w, h)
        o.close()


def test_coverage_of_the_stored_labels(gold):
    """What the cases are for, measured on the stored labels alone (measured: 288 of 300 over the cap with up to 35 neighbours; 4 labels without a pixel;
    226 rows of the uniform image whose tie pixel at column 16 went to the left, i.e. the first, candidate)."""
    seg = gold["noise_bin_320x240"].astype(np.int32)
    nc = sc.neighbour_counts(seg, 300)
    assert (nc > 11).sum() >= 200, (nc > 11).sum()
    seg = gold["stripes1_328x248"].astype(np.int32)
    own = np.bincount(seg.ravel(), minlength=300)
    assert (own == 0).sum() >= 1, (own == 0).sum()
    # uniform image: the pixel at x = 16 is as far from the centre at 8 as from the one at 24; the first of the nine candidates in loop order is the left one, so the
    # label boundary lies ON column 16 (between 16 and 17) and not before it
    seg = gold["const_320x240"].astype(np.int32)
    on16 = (seg[:, 16] == seg[:, 15]) & (seg[:, 16] != seg[:, 17])
    assert on16.sum() >= 1, on16.sum()
    assert not (seg[:, 15] != seg[:, 16]).all()


MERGE_CASES = [(i, d) for i in ("noise_bin", "stripes1", "blobs") for d in ("tilt", "steps")]


@pytest.fixture(scope="module")
def merged(orc, gold):
    """The oracle's merge of the six cases at 320x240, computed once."""
    w, h = 320, 240
    o = _oracle(orc, w, h)
    out = {}
    for img, dep in MERGE_CASES:
        seg0 = gold[sc.key(img, w, h)].astype(np.int32)
        out[(img, dep)] = (seg0,) + o.merge_superpixels(sc.depth(dep, w, h), seg0)
    o.close()
    return out


@pytest.mark.parametrize("img,dep", MERGE_CASES)
def test_oracle_merge_against_the_restatement(merged, img, dep):
    """The comparisons and bounds of test_superpixel_merge_from_the_source, on labelings with capped (one-way) neighbour lists and emptied superpixels.  Measured: the
    two readings agree EXACTLY on all six cases -- re-clustered labels, region ids and the neighbour lists after connectSuperPixel's deletions differ nowhere."""
    from test_restatement_rest_numpy import _sp_merge_restated

    w, h, spn = 320, 240, 300
    seg0, seg_o, fin_o, info_o = merged[(img, dep)]
    K = sc.camera(w, h)
    cam = (np.float32(K["cx"]), np.float32(K["cy"]), np.float32(1.0 / K["fx"]), np.float32(1.0 / K["fy"]))
    seg_r, fin_r, info_r = _sp_merge_restated(sc.depth(dep, w, h), seg0, w, h, spn, cam)
    print(img, dep, "labels differ on", int((seg_o != seg_r).sum()), "regions differ on", int((fin_o != fin_r).sum()), "neighbour entries differ on",
          int((info_o[:, 18:29] != info_r[:, 18:29]).sum()), "regions", len(np.unique(fin_o[fin_o >= 0])))
    # (the source test's first line -- more than half of the pixels valid, more than five regions -- describes its RGB-D pair, not the agreement.  These inputs are
    # described by what they are for: 7 % to 99 % of the pixels stay valid, 1 to 113 regions; the stepped depth's emptied superpixels are asserted below)
    assert (seg_o >= 0).any() and (seg_o < 0).any()
    if (img, dep) == ("noise_bin", "steps"):
        assert len(np.unique(fin_o[fin_o >= 0])) > 60       # the labelling the region filter's stage test runs on
    assert np.array_equal(seg_o < 0, seg_r < 0) or ((seg_o < 0) != (seg_r < 0)).mean() < 1e-3
    assert (seg_o != seg_r).mean() < 2e-3, (seg_o != seg_r).mean()
    used = info_o[:, 0] > 50
    assert np.abs(info_o[used, 0] - info_r[used, 0]).max() <= 0.02 * info_o[used, 0].max()
    assert np.allclose(info_o[used, 7:15], info_r[used, 7:15], rtol=2e-3, atol=2e-3)
    both = (fin_o >= 0) & (fin_r >= 0)
    pairs = np.stack([fin_o[both], fin_r[both]], 1)
    uniq, cnt = np.unique(pairs, axis=0, return_counts=True)
    best_for_o = {}
    for (a_, b_), c_ in zip(uniq.tolist(), cnt.tolist()):
        if c_ > best_for_o.get(a_, (None, 0))[1]:
            best_for_o[a_] = (b_, c_)
    agree = sum(c_ for (a_, b_), c_ in zip(uniq.tolist(), cnt.tolist()) if best_for_o[a_][0] == b_)
    assert agree / both.sum() > 0.98, agree / both.sum()


@pytest.mark.parametrize("img", ["noise_bin", "stripes1", "blobs"])
def test_steps_depth_empties_superpixels(merged, img):
    """The re-clustering against a stepped depth leaves more than 100 of the 300 superpixels without a pixel (measured: 125 to 227)."""
    _, seg_o, _, info_o = merged[(img, "steps")]
    empty = int((info_o[:, 0] == 0).sum())
    print(img, "emptied superpixels", empty)
    assert empty > 100, empty
    assert np.array_equal(info_o[:, 0].astype(np.int64), np.bincount(seg_o[seg_o >= 0], minlength=300))


def test_oracle_drops_foreign_ids_like_invalid_ones(orc, gold):
    """Ids below zero, equal to spn and far above it are dropped by kernel A before anything indexes with them: the merge equals the one of the same labelling with
    -1 in their place (the GPU test relies on this for both sides)."""
    w, h = 320, 240
    o = _oracle(orc, w, h)
    seg0 = gold["noise_bin_320x240"].astype(np.int32)
    a, b = sc.sprinkle(seg0, 300)
    ra, rb = o.merge_superpixels(sc.depth("tilt", w, h), a), o.merge_superpixels(sc.depth("tilt", w, h), b)
    for x, y in zip(ra, rb):
        assert np.array_equal(np.isnan(x), np.isnan(y)) and np.array_equal(np.nan_to_num(x), np.nan_to_num(y))
    assert (ra[0][b < 0] == -1).all()
    o.close()
