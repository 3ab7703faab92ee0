"""The detector's two operators on the device (ifx_roi_align_forward / ifx_nms): equal to the numpy statement (tests/detector_ops_numpy.py, itself held against
maskrcnn-benchmark's CPU operators in test_detector_ops_cpu.py) -- ROIAlign in every bit, NMS in every kept index -- on the golden cases and at the sizes where
the kernels change path; the streams; every refusal, which leaves the handle usable; and a map that does not notice."""
import ctypes as C
import os

import numpy as np
import pytest

import detector_ops_numpy as dn
from conftest import ROOT

pytestmark = pytest.mark.gpu

E_INVALID = -1
Q = dict(w=160, h=120, fx=132.0, fy=132.0, cx=80.0, cy=60.0)
GOLDEN = os.path.join(ROOT, "tests", "golden", "detector_ops_ref.npz")


@pytest.fixture(scope="module")
def ifx():
    import instancefusion_amd as m

    m.lib()
    return m


@pytest.fixture(scope="module")
def ef(ifx):
    """a handle that never sees a frame: the operators need none"""
    e = ifx.ElasticFusion(**Q, max_surfels=100000)
    yield e
    e.close()


@pytest.fixture(scope="module")
def golden():
    return dict(np.load(GOLDEN))


def _cuda(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _bits_equal(got, ref):
    return got.shape == ref.shape and got.dtype == ref.dtype == np.float32 and np.array_equal(got.view(np.uint32), ref.view(np.uint32))


def _check_roi_align(ef, inp, rois, scale, ph, pw, ratio):
    got = ef.roi_align_forward(_cuda(inp), _cuda(rois), scale, ph, pw, ratio).cpu().numpy()
    ref = dn.roi_align_forward(inp, rois, np.float32(scale), ph, pw, ratio)
    assert _bits_equal(got, ref), (got.shape, int((got.view(np.uint32) != ref.view(np.uint32)).sum()))
    return got


def _rois(rng, n, B, W, H, scale):
    """n ROIs around a W x H map at `scale`, some of them leaving it"""
    iw, ih = W / scale, H / scale
    x0, y0 = rng.uniform(-0.2 * iw, 0.9 * iw, n), rng.uniform(-0.2 * ih, 0.9 * ih, n)
    return np.stack([rng.integers(0, B, n).astype(np.float64), x0, y0, x0 + rng.uniform(0, 0.8 * iw, n), y0 + rng.uniform(0, 0.8 * ih, n)], axis=1).astype(np.float32)


# ---------------------------------------------------------------------------------------------------------------------------------------------- ROIAlign

def test_roi_align_golden_cases(ef, golden):
    """the reference's own outputs, bit for bit (and so the statement's)"""
    for k in range(int(golden["counts"][0])):
        scale, ph, pw, ratio = golden[f"roi{k}_par"]
        got = ef.roi_align_forward(_cuda(golden[f"roi{k}_input"]), _cuda(golden[f"roi{k}_rois"]), float(scale), int(ph), int(pw), int(ratio)).cpu().numpy()
        assert _bits_equal(got, golden[f"roi{k}_out"]), k


@pytest.mark.parametrize("channels", [1, 64, 257])
def test_roi_align_channel_runs(ef, channels):
    """one channel, exactly a block's run of 64, and 257 = four runs and one channel of a fifth"""
    rng = np.random.default_rng(channels)
    inp = rng.standard_normal((2, channels, 19, 23)).astype(np.float32)
    _check_roi_align(ef, inp, _rois(rng, 5, 2, 23, 19, 0.25), 0.25, 7, 7, 2)
    _check_roi_align(ef, inp, _rois(rng, 3, 2, 23, 19, 0.25), 0.25, 2, 3, 0)


@pytest.mark.parametrize("n", [0, 1, 65])
def test_roi_align_roi_counts(ef, n):
    rng = np.random.default_rng(100 + n)
    inp = rng.standard_normal((1, 3, 17, 13)).astype(np.float32)
    got = _check_roi_align(ef, inp, _rois(rng, n, 1, 13, 17, 0.5).reshape(n, 5), 0.5, 7, 7, 2)
    assert got.shape == (n, 3, 7, 7)


def test_roi_align_batch_index(ef):
    """index 1 of 2 reads the second image; an index outside 0 .. batch - 1 gives zeros"""
    rng = np.random.default_rng(3)
    inp = rng.standard_normal((2, 5, 9, 11)).astype(np.float32)
    rois = np.asarray([[1, 2, 1, 30, 25], [0, 2, 1, 30, 25], [2, 2, 1, 30, 25], [-1, 2, 1, 30, 25], [1e9, 2, 1, 30, 25], [-0.5, 2, 1, 30, 25], [1.9, 2, 1, 30, 25]], np.float32)
    got = _check_roi_align(ef, inp, rois, 0.25, 3, 3, 2)
    assert got[0].any() and not np.array_equal(got[0], got[1])
    assert not got[2].any() and not got[3].any() and not got[4].any()
    assert np.array_equal(got[5], got[1]) and np.array_equal(got[6], got[0])          # (int) truncates toward zero


def test_roi_align_one_row_one_column(ef):
    rng = np.random.default_rng(4)
    for shape in ((1, 3, 1, 12), (1, 3, 12, 1), (1, 2, 1, 1)):
        inp = rng.standard_normal(shape).astype(np.float32)
        rois = _rois(rng, 6, 1, shape[3], shape[2], 0.5)
        for ratio in (0, 2):
            _check_roi_align(ef, inp, rois, 0.5, 2, 3, ratio)


def test_roi_align_adaptive_grids(ef):
    """sampling_ratio 0: a 12 x 9 grid per bin; and grids whose axis tables no longer fit the block's LDS (more than 512 samples on an axis), on either axis and both"""
    rng = np.random.default_rng(5)
    inp = rng.standard_normal((1, 2, 33, 29)).astype(np.float32)
    rois = np.asarray([[0, 1.5, 2.25, 19.0, 25.75]], np.float32)                    # 23.5 / 2 -> 12 rows, 17.5 / 2 -> 9 columns
    assert int(np.ceil(np.float32(23.5) / 2)) == 12 and int(np.ceil(np.float32(17.5) / 2)) == 9
    _check_roi_align(ef, inp, rois, 1.0, 2, 2, 0)
    big = np.asarray([[0, -100, -120, 480, 470],      # 14 x 43 = 602 rows of samples, 14 x 42 = 588 columns
                      [0, 3, -120, 20, 470],          # rows only
                      [0, -100, 4, 480, 30],          # columns only
                      [0, 2, 3, 25, 30]], np.float32)
    got = _check_roi_align(ef, inp, big, 1.0, 14, 14, 0)
    assert got[0].any() and got[1].any() and got[2].any()


def test_roi_align_outside_and_reversed(ef):
    rng = np.random.default_rng(6)
    inp = rng.standard_normal((1, 4, 10, 14)).astype(np.float32)
    rois = np.asarray([[0, -400, -300, -200, -100], [0, 300, 200, 500, 400], [0, 40, 30, 8, 6], [0, 40, 6, 8, 30], [0, 56, 40, 56, 40], [0, -4, -4, 0, 0]], np.float32)
    for ratio in (0, 2):
        got = _check_roi_align(ef, inp, rois, 0.25, 7, 7, ratio)
        assert not got[:2].any() and not np.signbit(got[:2]).any()              # +0, not -0
        assert got[2].any()                                                    # a reversed ROI is 1 x 1 at its start corner


def test_roi_align_guard_bands_out_and_stream(ef):
    """out= inside a larger buffer: the floats on both sides keep their values; the call on a side stream is ordered on that stream alone"""
    import torch

    rng = np.random.default_rng(7)
    inp = rng.standard_normal((1, 70, 12, 9)).astype(np.float32)
    rois = _rois(rng, 9, 1, 9, 12, 0.5)
    ref = dn.roi_align_forward(inp, rois, np.float32(0.5), 7, 7, 2)
    guard = 4096
    buf = torch.full((2 * guard + ref.size,), -7.5, device="cuda")
    out = buf[guard:guard + ref.size].view(ref.shape)
    ret = ef.roi_align_forward(_cuda(inp), _cuda(rois), 0.5, 7, 7, 2, out=out)
    assert ret is out
    host = buf.cpu().numpy()
    assert (host[:guard] == -7.5).all() and (host[guard + ref.size:] == -7.5).all()
    assert _bits_equal(host[guard:guard + ref.size].reshape(ref.shape), ref)
    side = torch.cuda.Stream()
    d_in, d_rois = _cuda(inp), _cuda(rois)
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        a = ef.roi_align_forward(d_in, d_rois, 0.5, 7, 7, 2)                      # the current stream
    b = ef.roi_align_forward(d_in, d_rois, 0.5, 7, 7, 2, stream=side)             # named
    side.synchronize()
    assert _bits_equal(a.cpu().numpy(), ref) and _bits_equal(b.cpu().numpy(), ref)


# --------------------------------------------------------------------------------------------------------------------------------------------------- NMS

def _boxes(rng, n, density=1.0):
    extent = 20.0 + 12.0 * np.sqrt(n) / density
    c = rng.uniform(0, extent, (n, 2))
    return np.concatenate([c, c + rng.uniform(4, 40, (n, 2))], axis=1).astype(np.float32)


def _check_nms(ef, boxes, scores, thr, groups=None):
    import torch

    n = boxes.shape[0]
    d_groups = None if groups is None else _cuda(np.asarray(groups, np.int32))
    keep, count = ef.nms(_cuda(boxes), _cuda(scores), thr, groups=d_groups, padded=True)
    got = ef.nms(_cuda(boxes), _cuda(scores), thr, groups=d_groups)
    ref = dn.nms(boxes, scores, np.float32(thr), groups)
    assert got.dtype == torch.int64 and keep.dtype == torch.int64 and count.dtype == torch.int32
    assert np.array_equal(got.cpu().numpy(), ref), (n, got.numel(), ref.size)
    keep, count = keep.cpu().numpy(), int(count.item())
    assert count == ref.size and keep.shape == (n,)
    assert np.array_equal(keep[:count], ref) and (keep[count:] == -1).all()            # -1 behind the count
    return ref


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 128, 129, 1000, 4097, 8192])
def test_nms_sizes(ef, n):
    rng = np.random.default_rng(n)
    boxes = _boxes(rng, n, density=2.0).reshape(n, 4)
    scores = rng.random(n).astype(np.float32)
    ref = _check_nms(ef, boxes, scores, 0.5)
    assert n < 64 or 0.2 * n < ref.size < n                                            # (suppression is at work, and not all of it)


def test_nms_identical_and_disjoint(ef):
    rng = np.random.default_rng(11)
    n = 300
    same = np.tile(np.asarray([[5, 6, 50, 40]], np.float32), (n, 1))
    scores = rng.random(n).astype(np.float32)
    ref = _check_nms(ef, same, scores, 0.5)
    assert ref.tolist() == [int(np.argmax(scores))]
    grid = np.stack(np.meshgrid(np.arange(20), np.arange(15)), axis=-1).reshape(-1, 2).astype(np.float32) * 50
    apart = np.concatenate([grid, grid + 30], axis=1)
    assert _check_nms(ef, apart, scores, 0.0).size == n                                # IoU 0 is not > 0: all kept


def test_nms_chain_across_blocks(ef):
    """A suppresses B, B overlaps C, A does not: C is kept -- with A, B and C in three different 64-blocks of the sorted order"""
    n = 200
    grid = np.stack(np.meshgrid(np.arange(20), np.arange(10)), axis=-1).reshape(-1, 2).astype(np.float32) * 100 + 1000
    boxes = np.concatenate([grid, grid + 20], axis=1)
    a, b, c = 10, 70, 140
    boxes[a], boxes[b], boxes[c] = (0, 0, 19, 9), (8, 0, 27, 9), (16, 0, 35, 9)
    scores = (n - np.arange(n)).astype(np.float32)                                     # sorted position = index
    ref = _check_nms(ef, boxes, scores, 0.4)
    assert a in ref and c in ref and b not in ref and ref.size == n - 1
    perm = np.random.default_rng(12).permutation(n)                                    # the same boxes in another input order
    ref2 = _check_nms(ef, boxes[perm], scores[perm], 0.4)
    assert sorted(perm[ref2].tolist()) == ref.tolist()


def test_nms_equal_scores_nan_scores_nan_boxes(ef):
    rng = np.random.default_rng(13)
    n = 333
    boxes = _boxes(rng, n, density=3.0)
    scores = rng.integers(0, 6, n).astype(np.float32) / 4                              # six values: long runs of equal scores, broken by index
    scores[5] = -0.0
    _check_nms(ef, boxes, scores, 0.3)
    _check_nms(ef, boxes, np.zeros(n, np.float32), 0.3)
    s2 = rng.random(n).astype(np.float32)
    s2[::5] = np.nan                                                                   # visited last, by index
    s2[7], s2[8] = np.inf, -np.inf
    ref = _check_nms(ef, boxes, s2, 0.3)
    b2 = boxes.copy()
    b2[3::11, 0] = np.nan                                                              # a NaN coordinate: neither suppresses nor is suppressed
    b2[4::17] = np.nan
    b2[6, 2] = np.inf
    ref = _check_nms(ef, b2, s2, 0.3)
    assert set(range(3, n, 11)) <= set(ref.tolist()) and set(range(4, n, 17)) <= set(ref.tolist())
    same = np.tile(np.asarray([[3, 3, 20, 20]], np.float32), (130, 1))
    assert _check_nms(ef, same, np.full(130, 0.7, np.float32), 0.5).tolist() == [0]
    # IoU exactly at the threshold is kept (nms.cu's >)
    assert _check_nms(ef, np.asarray([[0, 0, 9, 9], [0, 0, 9, 4]], np.float32), np.asarray([2, 1], np.float32), 0.5).tolist() == [0, 1]


def test_nms_groups_are_the_per_class_loop(ef):
    """81 groups over 1000 boxes in one call against the box head's loop: one ungrouped call per group"""
    rng = np.random.default_rng(14)
    n = 1000
    boxes = _boxes(rng, n, density=4.0)
    scores = rng.random(n).astype(np.float32)
    groups = rng.integers(0, 81, n).astype(np.int32)
    ref = _check_nms(ef, boxes, scores, 0.5, groups)
    d_boxes, d_scores = _cuda(boxes), _cuda(scores)
    parts = []
    for g in range(81):
        idx = np.nonzero(groups == g)[0]
        if idx.size:
            parts.append(idx[ef.nms(d_boxes[idx], d_scores[idx], 0.5).cpu().numpy()])
    assert np.array_equal(np.sort(np.concatenate(parts)), ref)
    assert ref.size > dn.nms(boxes, scores, np.float32(0.5)).size


def test_nms_two_streams_back_to_back_and_padded(ef):
    """two calls on two streams with nothing in between share the handle's scratch: the second waits for the first on the device; padded=True returns without a
    host synchronisation and is read later"""
    import torch

    rng = np.random.default_rng(15)
    cases = []
    for n in (4097, 1500, 4000, 700):
        boxes, scores = _boxes(rng, n, density=2.0), rng.random(n).astype(np.float32)
        cases.append((_cuda(boxes), _cuda(scores), dn.nms(boxes, scores, np.float32(0.5))))
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    torch.cuda.synchronize()
    outs = [ef.nms(b, s, 0.5, stream=(s1, s2)[i % 2], padded=True) for i, (b, s, _) in enumerate(cases)]
    outs.append(ef.nms(cases[0][0], cases[0][1], 0.5, padded=True))                    # and the current stream
    torch.cuda.synchronize()
    for (keep, count), (_, _, ref) in zip(outs, cases + cases[:1]):
        c = int(count.item())
        assert c == ref.size and np.array_equal(keep[:c].cpu().numpy(), ref) and bool((keep[c:] == -1).all())


# --------------------------------------------------------------------------------------------------------------------------------------------- interfaces

def test_refusals_leave_the_handle_usable(ifx, ef):
    import torch

    L = ifx.lib()
    inp, rois, out = torch.zeros(1, 2, 4, 4, device="cuda"), torch.zeros(3, 5, device="cuda"), torch.zeros(3, 2, 2, 2, device="cuda")
    P = lambda t: C.c_void_p(t.data_ptr())

    def ra(d_in=P(inp), batch=1, channels=2, height=4, width=4, d_rois=P(rois), n=3, scale=0.5, ph=2, pw=2, ratio=2, d_out=P(out)):
        return L.ifx_roi_align_forward(ef.handle, d_in, batch, channels, height, width, d_rois, n, scale, ph, pw, ratio, d_out, None)

    bad = [dict(d_in=None), dict(d_rois=None), dict(d_out=None), dict(n=-1), dict(batch=0), dict(channels=0), dict(height=0), dict(width=0), dict(ph=0), dict(pw=0),
           dict(ratio=-1), dict(scale=float("nan")), dict(scale=float("inf")), dict(scale=float("-inf"))]
    for kw in bad:
        assert ra(**kw) == E_INVALID, kw
        assert b"ifx_roi_align_forward" in L.ifx_last_error(ef.handle)
    assert ra(n=0, d_in=None, d_rois=None, d_out=None) == 0                            # n == 0 succeeds and writes nothing
    assert ra() == 0
    boxes, scores, groups = torch.zeros(5, 4, device="cuda"), torch.zeros(5, device="cuda"), torch.zeros(5, dtype=torch.int32, device="cuda")
    keep, count = torch.zeros(5, dtype=torch.int64, device="cuda"), torch.full((1,), -9, dtype=torch.int32, device="cuda")

    def nms(d_boxes=P(boxes), d_scores=P(scores), d_groups=P(groups), n=5, thr=0.5, d_keep=P(keep), d_count=P(count)):
        return L.ifx_nms(ef.handle, d_boxes, d_scores, d_groups, n, thr, d_keep, d_count, None)

    for kw in (dict(n=-1), dict(n=8193), dict(d_boxes=None), dict(d_scores=None), dict(d_keep=None), dict(d_count=None), dict(thr=float("nan"))):
        assert nms(**kw) == E_INVALID, kw
        assert b"ifx_nms" in L.ifx_last_error(ef.handle)
    torch.cuda.synchronize()
    assert int(count.item()) == -9                                                     # nothing was enqueued
    assert nms(n=0, d_boxes=None, d_scores=None, d_keep=None) == 0
    torch.cuda.synchronize()
    assert int(count.item()) == 0                                                      # n == 0 writes count = 0
    assert nms(d_groups=None) == 0                                                     # groups may be NULL
    torch.cuda.synchronize()
    assert int(count.item()) == 1 and keep.tolist() == [0, -1, -1, -1, -1]
    assert nms(thr=float("inf")) == 0
    torch.cuda.synchronize()
    assert int(count.item()) == 5


def test_python_argument_checks(ifx, ef):
    import torch

    inp, rois = torch.zeros(1, 2, 4, 4, device="cuda"), torch.zeros(3, 5, device="cuda")
    boxes, scores = torch.zeros(5, 4, device="cuda"), torch.zeros(5, device="cuda")
    for bad in (inp.half(), inp.double()):
        with pytest.raises(TypeError):
            ef.roi_align_forward(bad, rois, 1.0, 2, 2, 2)
    with pytest.raises(TypeError):
        ef.roi_align_forward(inp, rois.half(), 1.0, 2, 2, 2)
    with pytest.raises(TypeError):
        ef.roi_align_forward(inp, rois, 1.0, 2, 2, 2, out=torch.zeros(3, 2, 2, 2, device="cuda", dtype=torch.float16))
    with pytest.raises(TypeError):
        ef.roi_align_forward(inp.cpu().numpy(), rois, 1.0, 2, 2, 2)
    for kw in (dict(input=inp.cpu()), dict(rois=rois.cpu()), dict(input=inp[0]), dict(rois=torch.zeros(3, 4, device="cuda")), dict(input=inp.transpose(2, 3)[:, :, :, :3]),
               dict(rois=torch.zeros(5, 3, device="cuda").t()), dict(out=torch.zeros(3, 2, 2, 3, device="cuda")), dict(out=torch.zeros(3, 2, 2, 2))):
        args = dict(input=inp, rois=rois, spatial_scale=1.0, pooled_h=2, pooled_w=2, sampling_ratio=2)
        args.update(kw)
        with pytest.raises(ValueError):
            ef.roi_align_forward(**args)
    for kw in (dict(boxes=boxes.half()), dict(scores=scores.half()), dict(scores=scores.double()), dict(groups=torch.zeros(5, dtype=torch.int64, device="cuda")),
               dict(groups=torch.zeros(5, device="cuda"))):
        args = dict(boxes=boxes, scores=scores, threshold=0.5)
        args.update(kw)
        with pytest.raises(TypeError):
            ef.nms(**args)
    for kw in (dict(boxes=boxes.cpu()), dict(scores=scores.cpu()), dict(boxes=torch.zeros(5, 5, device="cuda")), dict(scores=torch.zeros(4, device="cuda")),
               dict(scores=torch.zeros(5, 1, device="cuda")), dict(boxes=torch.zeros(4, 5, device="cuda").t()), dict(groups=torch.zeros(6, dtype=torch.int32, device="cuda")),
               dict(groups=torch.zeros(5, dtype=torch.int32))):
        args = dict(boxes=boxes, scores=scores, threshold=0.5)
        args.update(kw)
        with pytest.raises(ValueError):
            ef.nms(**args)
    with pytest.raises(ifx.IfxError):
        ef.nms(torch.zeros(8193, 4, device="cuda"), torch.zeros(8193, device="cuda"), 0.5)
    assert ef.nms(boxes, scores, 0.5).tolist() == [0]                                  # and the handle goes on


def test_detector_ops_stands_in_for_the_extension_module(ifx, ef):
    rng = np.random.default_rng(16)
    ops = ifx.detector_ops(ef)
    boxes, scores = _boxes(rng, 200, density=3.0), rng.random(200).astype(np.float32)
    assert np.array_equal(ops.nms(_cuda(boxes), _cuda(scores), 0.5).cpu().numpy(), dn.nms(boxes, scores, np.float32(0.5)))
    inp = rng.standard_normal((1, 3, 9, 8)).astype(np.float32)
    rois = _rois(rng, 4, 1, 8, 9, 0.25)
    assert _bits_equal(ops.roi_align_forward(_cuda(inp), _cuda(rois), 0.25, 7, 7, 2).cpu().numpy(), dn.roi_align_forward(inp, rois, np.float32(0.25), 7, 7, 2))
    for name in ("roi_align_backward", "roi_pool_forward", "roi_pool_backward", "sigmoid_focal_loss_forward", "sigmoid_focal_loss_backward"):
        with pytest.raises(NotImplementedError, match="inference only"):
            getattr(ops, name)(None)
    with pytest.raises(AttributeError):
        ops.no_such_operator


def test_the_map_does_not_notice(ifx):
    """two handles through the same three frames; on one of them both operators run (null stream, side stream) between the last frame and
    process_segmentation_rois: labels, instance table and map are those of the other"""
    import torch

    from instancefusion_amd import synth

    st = synth.make_stream(3, Q["w"], Q["h"], Q["fx"], Q["fy"], Q["cx"], Q["cy"], noise=True)
    rng = np.random.default_rng(17)
    M, n = 28, 3
    y, x = np.mgrid[0:M, 0:M]
    roi_masks = np.stack([(np.hypot(x - 13.5, y - 13.5) < r).astype(np.float32) * 0.9 for r in (9, 11, 13)])
    seg_boxes = np.asarray([[20, 15, 80, 70], [70, 40, 140, 110], [30, 60, 90, 115]], np.float32)
    cls = np.asarray([3, 7, 11], np.int32)
    results = []
    for with_ops in (False, True):
        e = ifx.ElasticFusion(**Q, max_surfels=200000)
        inst = ifx.InstanceFusion(e)
        for i in range(3):
            e.processFrame(st["rgb"][i], st["depth"][i])
        if with_ops:
            boxes, scores = _boxes(rng, 500), rng.random(500).astype(np.float32)
            side = torch.cuda.Stream()
            k1 = e.nms(_cuda(boxes), _cuda(scores), 0.5)
            k2 = e.nms(_cuda(boxes), _cuda(scores), 0.5, stream=side)
            inp = rng.standard_normal((1, 8, 30, 40)).astype(np.float32)
            rois = _rois(rng, 10, 1, 40, 30, 0.25)
            r1 = e.roi_align_forward(_cuda(inp), _cuda(rois), 0.25, 7, 7, 2)
            side.synchronize()
            assert np.array_equal(k1.cpu().numpy(), dn.nms(boxes, scores, np.float32(0.5))) and torch.equal(k1, k2)
            assert _bits_equal(r1.cpu().numpy(), dn.roi_align_forward(inp, rois, np.float32(0.25), 7, 7, 2))
        inst.process_segmentation_rois(_cuda(roi_masks), _cuda(seg_boxes), _cuda(cls), 2)
        results.append((inst.labels(), np.asarray(inst.getInstanceTable()), e.download()))
        e.close()
    (la, ta, ma), (lb, tb, mb) = results
    assert la.size > 0 and np.array_equal(la, lb)
    assert np.array_equal(ta, tb)
    for k in ma:
        assert np.array_equal(ma[k], mb[k]), k
