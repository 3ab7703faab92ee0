"""The superpixel path (ifx_slic.hip: SLIC, mergeSuperPixel, the region filter) on the adversarial inputs of tests/slic_cases.py, against the CPU oracle and
the labels of the reference's own gSLICr functions (tests/golden/slic_cases_ref.npz).  Every other superpixel test runs on the reference's RGB-D pair or on frames
of the synthetic scene, where none of the following occurs:

 * exact distance ties in k_slic_assoc (uniform images: the pixel at x = 16 is as far from the centre at 8 as from the one at 24; the first of the nine candidates
   in loop order wins, find_center_association_shared, gSLICr_seg_engine_shared.h);
 * neighbour lists past their cap of eleven (k_sp_first_avg keeps the first eleven ids in ascending order), hence ONE-WAY entries -- a lists b, b's capped list
   has no a -- in both one-block connect kernels, which restate connectSuperPixel's sequential deletion (InstanceFusion_superpixel.cpp:227-400) as propagation;
 * superpixels that lose every pixel in the re-clustering, and SLIC labels that own no pixel;
 * the hand-over between the two connect kernels: 640x480 has S = 1200 superpixels, the last size of k_sp_connect (lists in LDS), 640x496 has S = 1240, the
   first of k_sp_connect_big.

What the stored labels give (from tests/golden/slic_cases_ref.npz: superpixels with more than eleven distinct 4-neighbours / most neighbours of one / labels
without a pixel):
   64x48 and 72x56, all twelve images: 0 over the cap (noise and noise_bin reach exactly 11, stripes1 9, stripes3 8, the others 6 or 7), no empty label
   320x240   const 0 / 6 / 0    checker8off 0 / 8 / 0    stripes1 13 / 13 / 0    noise_bin 288 / 35 / 0    blobs 0 / 8 / 0
   328x248   const 0 / 6 / 0    checker8off 0 / 8 / 0    stripes1 18 / 14 / 4    noise_bin 290 / 31 / 0    blobs 0 / 8 / 0
and, after the merge at 320x240 against the stepped depth, superpixels left without a pixel (info[:, 0] == 0): noise_bin 227, stripes1 148, blobs 126 of 300
(tests/test_slic_cases_cpu.py asserts these conditions from the stored labels).

Only the stage entries are called on the small handles -- gSLICrInterface, mergeSuperPixel, maskSuperPixelFilter_OverSeg; no frame is processed on them."""
import os

import numpy as np
import pytest

import slic_cases as sc
from conftest import SMALL

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MERGE_IMAGES = ("noise", "noise_bin", "stripes1", "blobs", "const")


@pytest.fixture(scope="module")
def ifx():
    import instancefusion_amd as m

    m.lib()
    return m


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(os.path.join(ROOT, "tests", "golden", "slic_cases_ref.npz")))


@pytest.fixture(scope="module")
def handles(ifx, orc):
    """One HIP handle and one oracle per image size, shared by the tests of this module (buffers reused from call to call, as in a run)."""
    made = {}

    def get(w, h):
        if (w, h) not in made:
            g = ifx.ElasticFusion(w=w, h=h, max_surfels=1000, **sc.camera(w, h))
            made[(w, h)] = (g, ifx.InstanceFusion(g), orc.Oracle(w=w, h=h, max_surfels=1000, **sc.camera(w, h)))
        return made[(w, h)][1:]

    yield get
    for g, _, o in made.values():
        g.close(); o.close()


def nan_equal(a, b):
    return np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(np.nan_to_num(a), np.nan_to_num(b))


def _spn(w, h):
    return max((w * h) // 256, (w // 16) * (h // 16))


_labels = {}


def slic_both(get, name, w, h):
    """SLIC labels of one image on both sides (asserted equal), computed once per module."""
    if (name, w, h) not in _labels:
        inst, o = get(w, h)
        rgb = sc.image(name, w, h)
        seg_g, n_g = inst.gSLICrInterface(rgb)
        seg_o, n_o = o.slic_segment(rgb)
        assert n_g == n_o == (w // 16) * (h // 16)
        assert np.array_equal(seg_g, seg_o), (name, w, h, int((seg_g != seg_o).sum()))
        seg_g.setflags(write=False)
        _labels[(name, w, h)] = seg_g
    return _labels[(name, w, h)]


# ---------------------------------------------------------------- SLIC labels
@pytest.mark.parametrize("w,h", sc.TINY_SIZES + sc.MID_SIZES, ids=lambda v: str(v))
def test_slic_labels(handles, gold, w, h):
    inst, o = handles(w, h)
    names = sc.IMAGES if (w, h) in sc.TINY_SIZES else sc.MID_STORED + ("noise",)
    stored = 0
    for name in names:
        seg = slic_both(handles, name, w, h)
        assert seg.min() >= 0 and seg.max() < (w // 16) * (h // 16)
        if sc.key(name, w, h) in gold:
            stored += 1
            diff = seg != gold[sc.key(name, w, h)].astype(np.int32)
            assert not diff.any(), (name, w, h, int(diff.sum()), np.argwhere(diff)[:4].tolist())
    assert stored == (12 if (w, h) in sc.TINY_SIZES else 5)
    # again on the same handle, in reverse order: the centre and label buffers carry nothing over from the image before
    for name in reversed(names):
        seg2, _ = inst.gSLICrInterface(sc.image(name, w, h))
        assert np.array_equal(seg2, slic_both(handles, name, w, h)), (name, w, h)


# ---------------------------------------------------------------- merge
def check_merge(inst, o, dep, seg, what, twice=True):
    s_g, f_g, i_g = inst.mergeSuperPixel(dep, seg)
    s_o, f_o, i_o = o.merge_superpixels(dep, seg)
    assert np.array_equal(s_g, s_o), (what, "re-clustered labels", int((s_g != s_o).sum()))
    assert np.array_equal(f_g, f_o), (what, "region ids", int((f_g != f_o).sum()))
    assert nan_equal(i_g, i_o), (what, "statistics table", np.argwhere(np.nan_to_num(i_g) != np.nan_to_num(i_o))[:6].tolist())
    if twice:       # twice on the same handle: the sums, the neighbour bit matrix and the edge table are rebuilt, not accumulated
        s_2, f_2, i_2 = inst.mergeSuperPixel(dep, seg)
        assert np.array_equal(s_2, s_g) and np.array_equal(f_2, f_g) and nan_equal(i_2, i_g), what
    return s_g, f_g, i_g


@pytest.mark.parametrize("name", MERGE_IMAGES)
@pytest.mark.parametrize("w,h", sc.MID_SIZES, ids=lambda v: str(v))
def test_merge(handles, w, h, name):
    inst, o = handles(w, h)
    seg = slic_both(handles, name, w, h)
    spn = _spn(w, h)
    for dname in sc.DEPTHS:
        dep = sc.depth(dname, w, h)
        s, f, info = check_merge(inst, o, dep, seg, (name, dname, w, h))
        if dname == "zero":
            assert (s == -1).all() and (f == -1).all()
        else:
            assert (s >= 0).any()
        if dname == "steps" and name != "const":
            assert (info[:, 0] == 0).sum() > spn // 3      # emptied superpixels (measured at 320x240: 126 to 227 of 300)
    # foreign ids are dropped by k_sp_posnor before anything indexes with them: the same result as with -1 in their place, on both sides
    ragged, plain = sc.sprinkle(seg, spn)
    dep = sc.depth("tilt", w, h)
    got = check_merge(inst, o, dep, ragged, (name, "ragged", w, h), twice=False)
    want = check_merge(inst, o, dep, plain, (name, "ragged as -1", w, h), twice=False)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and nan_equal(got[2], want[2])
    assert (got[0][plain < 0] == -1).all()


# ---------------------------------------------------------------- the two connect kernels at their hand-over
@pytest.mark.parametrize("name", ["noise_bin", "blobs"])
@pytest.mark.parametrize("w,h", sc.HANDOVER_SIZES, ids=lambda v: str(v))
def test_connect_kernels_at_their_hand_over(handles, w, h, name):
    inst, o = handles(w, h)
    spn = _spn(w, h)
    assert spn == (1200 if h == 480 else 1240)      # merge_run: S <= 1200 -> k_sp_connect, above -> k_sp_connect_big
    seg = slic_both(handles, name, w, h)
    if name == "noise_bin":     # the condition: lists capped nearly everywhere (the floor of two thirds as at 320x240; measured 1225 of 1240 at 640x496)
        over = int((sc.neighbour_counts(seg, spn) > 11).sum())
        assert over >= 2 * spn // 3, over
    regions = 0
    for dname in ("tilt", "steps", "holes"):
        s, f, info = check_merge(inst, o, sc.depth(dname, w, h), seg, (name, dname, w, h))
        assert info.shape[0] == spn
        regions = max(regions, len(np.unique(f[f >= 0])))
        fo = info[:, 29].astype(np.int32)
        assert np.all(fo <= np.arange(spn)) and np.array_equal(fo[fo], fo)
    assert regions > 60, regions


# ---------------------------------------------------------------- region filter, stage call
@pytest.mark.parametrize("w,h", sc.MID_SIZES, ids=lambda v: str(v))
def test_region_filter_stage_call(handles, w, h):
    """ifx_mask_superpixel_filter on a labelling with emptied superpixels, dropped pixels and more than 60 regions; 40 masks, so the chunks of 32 are crossed."""
    inst, o = handles(w, h)
    spn = _spn(w, h)
    seg = slic_both(handles, "noise_bin", w, h)
    s, fin, info = check_merge(inst, o, sc.depth("steps", w, h), seg, ("noise_bin", "steps", w, h), twice=False)
    assert (info[:, 0] == 0).sum() > 100 and (fin < 0).any() and len(np.unique(fin[fin >= 0])) > 60
    rng = np.random.RandomState(31)
    masks = np.zeros((40, h, w), np.uint8)
    masks[0, h // 5: h // 2, w // 4: w // 2] = 255
    masks[1, h // 2:, : w // 3] = 255
    masks[2] = (rng.rand(h, w) < 0.85) * 255
    masks[3] = 255
    # masks[4] stays empty
    for i in range(5, 40):
        x0, y0 = rng.randint(0, w - 40), rng.randint(0, h - 40)
        masks[i, y0:y0 + rng.randint(10, 40), x0:x0 + rng.randint(10, 40)] = 255
    got = inst.maskSuperPixelFilter_OverSeg(fin, masks)
    want = o.mask_superpixel_filter(fin, masks)
    assert np.array_equal(got, want), [int((got[i] != want[i]).sum()) for i in range(40)]
    assert not got[4].any() and np.array_equal(got[3] != 0, fin >= 0) and 0 < (got[2] != 0).sum() and (got[5:] != 0).any()
    # the re-clustered labels as keys (emptied ids never occur, ids up to spn - 1 do), and foreign ids sprinkled in
    assert np.array_equal(inst.maskSuperPixelFilter_OverSeg(s, masks), o.mask_superpixel_filter(s, masks))
    ragged, _ = sc.sprinkle(fin, spn)
    assert np.array_equal(inst.maskSuperPixelFilter_OverSeg(ragged, masks), o.mask_superpixel_filter(ragged, masks))
    assert np.array_equal(inst.maskSuperPixelFilter_OverSeg(fin, masks), got)


# ---------------------------------------------------------------- the production filter (k_sp_count on the re-clustered labels, folded through final_of)
@pytest.mark.parametrize("name", ["checker8off", "blobs", "stripes1", "noise_bin"])
def test_production_filter_through_whole_calls(ifx, orc, small_stream, name):
    """test_segmentation_with_superpixels_exact's map; the calls' colour image replaced, the depth stays frame 5's.  On the oracle alone: checker8off registers 3
    instances and labels 627 surfels, blobs 2 and 563; stripes1 and noise_bin refine every mask away -- the table stays empty and the votes must still be equal.  Then one call with masks that cut through the regions."""
    from instancefusion_amd import synth

    st = small_stream
    g = ifx.ElasticFusion(**SMALL, max_surfels=400000)
    g.set_option("compact_every_frame", 1)
    o = orc.Oracle(**SMALL, max_surfels=400000)
    inst = ifx.InstanceFusion(g)
    for i in range(6):
        po = o.process_frame(st["rgb"][i], st["depth"][i])
        g.processFrame(st["rgb"][i], st["depth"][i])
    m = o.download(); m["pc"][:, 3] = 20.0
    o.upload(m); g.upload(m)
    o.set_pose(po, o.tick); g.set_pose(po, o.tick)
    g.processFrame(st["rgb"][5], st["depth"][5], inPose=po); o.process_frame(st["rgb"][5], st["depth"][5], in_pose=po)
    assert g.count == o.count and np.array_equal(g.image("ids_after"), o.image("ids_after"))
    masks, cls = synth.canned_masks(st["obj"][5], st["scene"])
    rgb = sc.image(name, SMALL["w"], SMALL["h"])
    for frame in (50, 60):
        inst.ProcessSegmentation(rgb, st["depth"][5], masks, cls, frame, superpixels=True)
        o.process_segmentation(rgb, st["depth"][5], masks, cls, frame, flags=2)
        assert np.array_equal(inst.getInstanceTable(), o.instance_table())
        assert np.array_equal(inst.labels(), o.labels())
        assert np.array_equal(g.download()["votes"], o.download()["votes"])
    if name in ("checker8off", "blobs"):
        assert (o.labels() >= 0).sum() >= 300 and (o.instance_table() >= 0).sum() >= 2
    else:
        assert (o.instance_table() == -1).all() and (o.labels() < 0).all()
    # The canned masks are the objects' own outlines: a region lies inside one or outside it, and so does the region's first superpixel -- counts that were never
    # folded through final_of would decide the same.  Masks that cut through the regions: the 75 % rule then depends on the whole region's count.
    h, w = SMALL["h"], SMALL["w"]
    cut = np.zeros((4, h, w), np.uint8)
    cut[0, :, : int(w * 0.55)] = 255
    cut[1, int(h * 0.4):, int(w * 0.45):] = 255
    cut[2] = np.roll(masks[0], 10, axis=1)
    cut[3] = (np.random.RandomState(41).rand(h, w) < 0.8) * 255
    before = o.download()["votes"].copy()
    inst.ProcessSegmentation(rgb, st["depth"][5], cut, cls[:4], 70, superpixels=True)
    o.process_segmentation(rgb, st["depth"][5], cut, cls[:4], 70, flags=2)
    assert np.array_equal(inst.getInstanceTable(), o.instance_table())
    assert np.array_equal(inst.labels(), o.labels())
    assert np.array_equal(g.download()["votes"], o.download()["votes"])
    if name != "noise_bin":     # (there nothing registers with these masks either: 118 regions on 43 % of the pixels)
        assert (o.download()["votes"] != before).sum() > 10000     # the call voted (on the oracle alone: 15114 to 17289 surfel votes changed)
    g.close(); o.close()
