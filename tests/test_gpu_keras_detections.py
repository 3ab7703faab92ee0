"""ifx_keras_detections on the device (refine_detections_graph of the Keras Mask R-CNN and the box conversion behind it): detections, normalised boxes, ROI rows,
count and the padding behind the count equal to the numpy statement (tests/keras_layers_numpy.py) bit for bit, compared as uint32: a case by hand, the reference's
size, directed cases (all background, min_confidence 0 and a NaN score, a score at min_confidence, arg-max ties, coordinates on k + 0.5, the per-class cap, the
cut across classes with equal scores on it, zero-area boxes, a NaN delta, the window clip); NULL outputs, guard bands, refusals, the Python method; the chain into
process_segmentation_unmolded; and a map that does not notice the three calls on a side stream."""
import ctypes as C

import numpy as np
import pytest

import keras_layers_gpu as kg
import keras_layers_numpy as kl
from keras_layers_gpu import F, cuda

pytestmark = pytest.mark.gpu

IMG = (1024, 1024)
WIN = (0, 0, 1024, 1024)


@pytest.fixture(scope="module")
def ifx():
    import instancefusion_amd as m

    m.lib()
    return m


@pytest.fixture(scope="module")
def ef(ifx):
    e = ifx.ElasticFusion(**kg.Q, max_surfels=100000)
    yield e
    e.close()


def _check(ifx, ef, rois, probs, deltas, window=WIN, image=IMG, minconf=0.7, thr=0.3, M=100, **kw):
    import torch

    bufs = kg.raw_detections(ifx, ef, cuda(rois), cuda(probs), cuda(deltas), window, image, minconf, thr, M, **kw)
    torch.cuda.synchronize()
    ref = kl.keras_detections(rois, probs, deltas, window, image, minconf, thr, M)
    kg.detections_equal(kg.read_detections(bufs, M), ref, M, **kw)
    return ref


def _case(seed, R, Cn, peak=0.9, bg=0.3):
    """rois inside the unit square, peaked probability rows (a share `bg` of them background), N(0, 1) deltas"""
    rng = np.random.default_rng(seed)
    side = np.exp(rng.uniform(np.log(0.03), np.log(0.6), (R, 2)))
    p = rng.uniform(0, 1, (R, 2)) * (1 - side)
    rois = np.concatenate([p, p + side], axis=1).astype(F)
    probs = rng.random((R, Cn)) * (1 - peak) / Cn
    cls = np.where(rng.random(R) < bg, 0, rng.integers(1, Cn, R))
    probs[np.arange(R), cls] += peak * rng.uniform(0.6, 1.0, R)
    deltas = rng.standard_normal((R, Cn, 4)).astype(F)
    return rois, probs.astype(F), deltas


def test_by_hand(ifx, ef):
    """R = 17, C = 3 on a 64 x 64 image with zero deltas: background rows, rows below the confidence, two stacks of overlapping boxes per class"""
    R = 17
    rois = np.zeros((R, 4), F)
    probs = np.zeros((R, 3), F)
    for r in range(R):
        k = r % 4
        rois[r] = [k / 8 + r / 512, k / 8, k / 8 + 0.25, k / 8 + 0.25]
        c = (0, 1, 2, 1)[r % 4] if r < 12 else 2
        probs[r, c] = 0.5 + r / 40
        probs[r, (c + 1) % 3] = 0.05
    deltas = np.zeros((R, 3, 4), F)
    ref = _check(ifx, ef, rois, probs, deltas, (0, 0, 64, 64), (64, 64), 0.7, 0.3, 10)
    det, norm, index = ref
    # rows 0 .. 7 are below 0.7, row 8 is background; 12 (class 2, 16's box) and 10 (class 2, IoU 14/15 with 14's) are suppressed; 11 and 9 (class 1) are disjoint
    assert index.tolist() == [16, 15, 14, 13, 11, 9] and det[:, 4].tolist() == [2.0, 2.0, 2.0, 2.0, 1.0, 1.0]
    assert det[0, :4].tolist() == [2.0, 0.0, 16.0, 16.0] and norm[0].tolist() == [0.03125, 0.0, 0.25, 0.25]


def test_reference_size(ifx, ef):
    """R = 1000, C = 81, the reference's thresholds"""
    ref = _check(ifx, ef, *_case(1, 1000, 81))
    assert ref[0].shape[0] == 100
    ref = _check(ifx, ef, *_case(2, 1000, 81, bg=0.97), M=100)
    assert 0 < ref[0].shape[0] < 100


def test_all_background(ifx, ef):
    rois, probs, deltas = _case(3, 200, 5)
    probs[:, 0] = 2.0
    ref = _check(ifx, ef, rois, probs, deltas)
    assert ref[0].shape[0] == 0


def test_min_confidence_zero_and_nan_scores(ifx, ef):
    """min_confidence 0: the score test is skipped; rows whose probabilities hold NaNs -- in class 0 (the row is background), elsewhere (never the maximum)"""
    rois, probs, deltas = _case(4, 300, 7, peak=0.5)
    probs[::9, 0] = np.nan
    probs[4::9, 3] = np.nan
    probs[5::31] = np.nan
    low = _check(ifx, ef, rois, probs, deltas, minconf=0.0, thr=0.5, M=300)
    high = _check(ifx, ef, rois, probs, deltas, minconf=0.4, thr=0.5, M=300)
    assert low[0].shape[0] > high[0].shape[0] > 0 and not np.isnan(low[0]).any()


def test_score_exactly_at_min_confidence_and_argmax_ties(ifx, ef):
    rois, probs, deltas = _case(5, 64, 4)
    probs[:] = 0
    probs[:, 2] = F(0.7)                                # exactly at the threshold: kept
    probs[::2, 3] = F(0.7)                              # tie between 2 and 3: the first wins
    probs[1::8, 2] = np.nextafter(F(0.7), F(0))         # one step below: dropped
    probs[3::8, 0] = F(0.7)                             # tie with class 0: background wins
    ref = _check(ifx, ef, rois, probs, deltas, minconf=0.7, thr=1.0, M=64)
    assert ref[0].shape[0] == 64 - 16 and (ref[0][:, 4] == 2).all() and (ref[0][:, 5] == F(0.7)).all()
    assert np.array_equal(ref[2], np.setdiff1d(np.arange(64), np.concatenate([np.arange(1, 64, 8), np.arange(3, 64, 8)])))     # equal scores: ascending row


def test_coordinates_on_half_round_to_even(ifx, ef):
    """a power-of-two image, zero deltas, rois (2k + 1) / (2 H): every coordinate lands on k + 0.5 exactly"""
    H = 64
    k = np.arange(24)
    rois = np.stack([(2 * k + 1) / (2.0 * H), (2 * k + 3) / (2.0 * H), (2 * k + 41) / (2.0 * H), (2 * k + 47) / (2.0 * H)], axis=1).astype(F)
    probs = np.tile(np.asarray([[0.05, 0.95]], F), (24, 1))
    probs[:, 1] -= (k / 1000).astype(F)
    ref = _check(ifx, ef, rois, probs, np.zeros((24, 2, 4), F), (0, 0, H, H), (H, H), 0.5, 1.0, 24)
    assert ref[2].tolist() == k.tolist()
    assert ref[0][:, 0].tolist() == [float(2 * ((v + 1) // 2)) for v in k]                 # k + 0.5 -> the even neighbour
    assert (ref[0][:, :4] % 2 == 0).all()


def _disjoint(R, Cn, cls):
    k = np.arange(R)
    y, x = (k // 20) * 48 + 8, (k % 20) * 48 + 8
    rois = (np.stack([y, x, y + 32, x + 32], axis=1) / 1024.0).astype(F)
    probs = np.full((R, Cn), 0.001, F)
    probs[k, cls] = 0.9
    return rois, probs, np.zeros((R, Cn, 4), F)


def test_per_class_cap(ifx, ef):
    """300 disjoint boxes of one class, descending scores, max_instances 100: the first hundred"""
    rois, probs, deltas = _disjoint(300, 3, np.full(300, 2))
    probs[:, 2] -= (np.arange(300) / 1000).astype(F)
    ref = _check(ifx, ef, rois, probs, deltas, M=100)
    assert ref[2].tolist() == list(range(100))


def test_cut_across_classes_with_equal_scores_on_it(ifx, ef):
    """two classes of 80 boxes each, max_instances 100, four distinct scores: the cut falls inside a run of equal scores, ascending row decides"""
    cls = np.where(np.arange(160) % 2 == 0, 1, 2)
    rois, probs, deltas = _disjoint(160, 3, cls)
    probs[np.arange(160), cls] = (0.9 - 0.05 * (np.arange(160) // 40)).astype(F)
    ref = _check(ifx, ef, rois, probs, deltas, M=100)
    assert ref[2].tolist() == list(range(100)) and ref[0][99, 5] == ref[0][80, 5] == probs[100, cls[100]]
    assert sorted(np.unique(ref[0][:, 4]).tolist()) == [1.0, 2.0]


def test_identical_zero_area_boxes_are_all_kept(ifx, ef):
    """rois that round to lines and points, forty of them identical: area 0, no pair suppresses"""
    rois, probs, deltas = _disjoint(60, 3, np.full(60, 1))
    rois[:, 2] = rois[:, 0]                             # zero height
    rois[20:] = rois[20]
    probs[:, 1] -= (np.arange(60) / 1000).astype(F)
    ref = _check(ifx, ef, rois, probs, deltas, M=100)
    assert ref[2].tolist() == list(range(60))


def test_nan_delta_drops_the_row_and_the_window_clips(ifx, ef):
    rois, probs, deltas = _case(6, 400, 9, bg=0.1)
    cls = kl.first_max(probs)
    deltas[np.arange(0, 400, 7), cls[::7], 1] = np.nan
    deltas[np.arange(3, 400, 11), cls[3::11], 2] = F(5000)                  # EXP overflows: an infinite height, NaN corners
    win = (100, 200, 900, 700)
    ref = _check(ifx, ef, rois, probs, deltas, window=win, minconf=0.3, thr=0.5, M=400)
    assert ref[0].shape[0] > 20 and not set(ref[2]) & set(range(0, 400, 7))
    b = ref[0][:, :4]
    assert (b[:, [0, 2]] >= 100).all() and (b[:, [0, 2]] <= 900).all() and (b[:, [1, 3]] >= 200).all() and (b[:, [1, 3]] <= 700).all()
    assert (b[:, 0] == 100).any() and (b[:, 3] == 700).any()


def test_null_outputs(ifx, ef):
    case = _case(7, 500, 11)
    for norm, index in ((False, True), (True, False), (False, False)):
        _check(ifx, ef, *case, norm=norm, index=index)


def test_python_method_and_refusals(ifx, ef):
    import torch

    rois, probs, deltas = _case(8, 700, 81)
    ref = kl.keras_detections(rois, probs, deltas, WIN, IMG)
    d = (cuda(rois), cuda(probs), cuda(deltas))
    det, norm, index = ef.keras_detections(*d, WIN, IMG)
    kg.same_floats(det.cpu().numpy(), ref[0])
    kg.same_floats(norm.cpu().numpy(), ref[1])
    assert np.array_equal(index.cpu().numpy(), ref[2])
    side = torch.cuda.Stream()
    buf = torch.full((2 * kg.GUARD + 600,), -7.5, device="cuda")
    out = buf[kg.GUARD:-kg.GUARD].view(100, 6)
    torch.cuda.synchronize()
    pd, pn, pi, cnt = ef.keras_detections(*d, WIN, IMG, out=out, padded=True, stream=side)
    side.synchronize()
    assert pd is out
    kg.detections_equal((kg.payload(buf, -7.5).reshape(100, 6), pn.cpu().numpy(), pi.cpu().numpy(), int(cnt.item())), ref, 100)
    case2 = _case(9, 700, 81)
    win2 = (10, 20, 1000, 900)
    ref2 = kl.keras_detections(*case2, win2, IMG)
    bd, bn, bi, bc = ef.keras_detections(cuda(np.stack([rois, case2[0]])), cuda(np.stack([probs, case2[1]])), cuda(np.stack([deltas, case2[2]])), [WIN, win2], IMG)
    assert tuple(bd.shape) == (2, 100, 6) and tuple(bc.shape) == (2,)
    for k, r in enumerate((ref, ref2)):
        kg.detections_equal((bd[k].cpu().numpy(), bn[k].cpu().numpy(), bi[k].cpu().numpy(), int(bc[k].item())), r, 100)
    with pytest.raises(TypeError):
        ef.keras_detections(d[0], d[1].double(), d[2], WIN, IMG)
    with pytest.raises(ValueError):
        ef.keras_detections(d[0][:-1], d[1], d[2], WIN, IMG)
    with pytest.raises(ValueError):
        ef.keras_detections(d[0], d[1], d[2].reshape(700, 4, 81), WIN, IMG)
    with pytest.raises(ValueError):
        ef.keras_detections(d[0], d[1], d[2], (0, 0, 5), IMG)
    with pytest.raises(ValueError):
        ef.keras_detections(d[0], d[1], d[2], WIN, IMG, out=torch.empty((100, 5), device="cuda"))

    ptr = [C.c_void_p(t.data_ptr()) for t in d]
    o = [torch.full((600,), -7.5, device="cuda"), torch.full((1,), -77, dtype=torch.int32, device="cuda")]
    po, pc = (C.c_void_p(t.data_ptr()) for t in o)
    good = dict(R=700, Cn=81, M=100, image=IMG, window=WIN)

    def call(r=ptr[0], p=ptr[1], dl=ptr[2], out=po, c=pc, params=True, **kw):
        a = dict(good, **kw)
        q = kg.detection_params(ifx, a["window"], a["image"], 0.7, 0.3, a["M"])
        return ef.L.ifx_keras_detections(ef.handle, r, p, dl, a["R"], a["Cn"], C.byref(q) if params else None, out, None, None, c, None)

    bad = [dict(R=0), dict(R=8193), dict(Cn=1), dict(Cn=1025), dict(M=0), dict(M=8193), dict(image=(0, 5)), dict(image=(5, 0)), dict(window=(0, 0, np.nan, 5)),
           dict(window=(0, 0, 5, np.inf)), dict(window=(-2e7, 0, 5, 5)), dict(r=None), dict(p=None), dict(dl=None), dict(out=None), dict(c=None), dict(params=False)]
    for kw in bad:
        assert call(**kw) == kg.E_INVALID, kw
        assert ef.L.ifx_last_error(ef.handle).startswith(b"ifx_keras_detections: "), kw
    torch.cuda.synchronize()
    assert (o[0] == -7.5).all() and (o[1] == -77).all()
    assert call() == 0
    torch.cuda.synchronize()
    pdet = kl.detections_padded(ref, 100)
    kg.same_floats(o[0].cpu().numpy().reshape(100, 6), pdet[0])
    assert int(o[1].item()) == pdet[3]


def test_chain_into_process_segmentation_unmolded(ifx):
    """keras_detections' padded output and a random [R,28,28,C] mask tensor go straight into process_segmentation_unmolded on a 160 x 120 map; the votes equal those
    of the same call fed the numpy statement's detections: the formats meet without glue"""
    import torch

    from instancefusion_amd import synth

    W, H = kg.Q["w"], kg.Q["h"]
    st = synth.make_stream(3, W, H, kg.Q["fx"], kg.Q["fy"], kg.Q["cx"], kg.Q["cy"], noise=True)
    size = ifx.molded_input_size(W, H, 128, 160)
    S, window = int(size[2]), tuple(int(v) for v in size[4:8])
    R, Cn, M = 60, 9, 16
    rois, probs, deltas = _case(10, R, Cn, bg=0.2)
    deltas *= F(0.3)
    rng = np.random.default_rng(11)
    masks = rng.random((M, 28, 28, Cn)).astype(F)
    ref = kl.detections_padded(kl.keras_detections(rois, probs, deltas, window, (S, S), 0.5, 0.3, M), M)
    assert ref[3] >= 4
    votes = []
    for device_layer in (True, False):
        e = ifx.ElasticFusion(**kg.Q, max_surfels=200000)
        inst = ifx.InstanceFusion(e)
        for i in range(3):
            e.processFrame(st["rgb"][i], st["depth"][i])
        if device_layer:
            det, _, _, count = e.keras_detections(cuda(rois), cuda(probs), cuda(deltas), window, (S, S), 0.5, 0.3, M, padded=True)
        else:
            det = cuda(ref[0])
        inst.process_segmentation_unmolded(det, cuda(masks), window, 2)
        torch.cuda.synchronize()
        if device_layer:
            assert int(count.item()) == ref[3] and np.array_equal(kg.bits(det.cpu().numpy()), kg.bits(ref[0]))
        votes.append((inst.labels().copy(), e.download()["votes"].copy()))
        e.close()
    assert np.array_equal(votes[0][0], votes[1][0]) and np.array_equal(votes[0][1], votes[1][1])
    assert (votes[0][1] != 0).any()


def test_the_map_does_not_notice(ifx):
    """two handles through the same three frames; on one of them the three calls run on a side stream between the second frame and the third: the third frame's
    pose, the map's count and every map field are those of the other"""
    import torch

    from instancefusion_amd import synth

    st = synth.make_stream(3, kg.Q["w"], kg.Q["h"], kg.Q["fx"], kg.Q["fy"], kg.Q["cx"], kg.Q["cy"], noise=True)
    pcase = kg.proposal_case(50, 20000)
    pref = kl.keras_proposals(*pcase, IMG, 6000, 200, 0.7)
    dcase = _case(51, 300, 21)
    dref = kl.keras_detections(*dcase, WIN, IMG)
    rng = np.random.default_rng(52)
    maps = [rng.standard_normal((1, s, s, 8)).astype(F) for s in (16, 8, 4, 2)]
    results = []
    for with_calls in (False, True):
        e = ifx.ElasticFusion(**kg.Q, max_surfels=200000)
        for i in range(2):
            e.processFrame(st["rgb"][i], st["depth"][i])
        if with_calls:
            side = torch.cuda.Stream()
            dp, dd, dm = [cuda(a) for a in pcase], [cuda(a) for a in dcase], [cuda(m) for m in maps]
            torch.cuda.synchronize()
            props, pidx = e.keras_proposals(*dp, IMG, proposal_count=200, stream=side)
            with torch.cuda.stream(side):
                pooled = e.pyramid_roi_align(dm, props[None].contiguous(), (512, 512), (7, 7), stream=side)
            det, norm, didx = e.keras_detections(*dd, WIN, IMG, stream=side)
            side.synchronize()
            kg.same_floats(props.cpu().numpy(), pref[0])
            assert np.array_equal(pidx.cpu().numpy(), pref[1]) and np.array_equal(didx.cpu().numpy(), dref[2])
            want, _ = kl.pyramid_roi_align(maps, pref[0][None], (512, 512), (7, 7))
            assert np.array_equal(kg.bits(pooled.cpu().numpy()), kg.bits(want))
        pose = e.processFrame(st["rgb"][2], st["depth"][2])
        results.append((np.asarray(pose).copy(), e.count, e.download()))
        e.close()
    (pa, ca, ma), (pb, cb, mb) = results
    assert np.array_equal(pa, pb) and ca == cb and ca > 0
    for k in ma:
        assert np.array_equal(ma[k], mb[k]), k
