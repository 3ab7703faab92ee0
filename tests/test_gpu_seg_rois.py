"""The mask head's ROI masks and boxes pasted on the GPU (ifx_paste_roi_masks / ifx_process_segmentation_rois / ifx_process_segmentation_deferred_rois): the stage
call pixel for pixel against the float32 statement (tests/roi_paste_numpy.py) and against maskrcnn-benchmark's own masks (tests/golden/roi_paste_ref.npz, ties at
the threshold excepted); the full and the deferred call bit for bit against the existing device entries fed the pasted masks; the producer stream; the refusals."""
import ctypes as C

import numpy as np
import pytest

import roi_paste_numpy as rp
from conftest import SMALL

pytestmark = pytest.mark.gpu

MAP_KEYS = ("pc", "nr", "col", "tm", "ic", "votes")
TINY = dict(w=160, h=120, fx=132.0, fy=132.0, cx=80.0, cy=60.0)
NARROW = dict(w=100, h=76, fx=82.0, fy=82.0, cx=50.0, cy=38.0)    # a width that is no multiple of the 16 pixels a thread owns


@pytest.fixture(scope="module")
def ifx():
    import instancefusion_amd as m

    m.lib()
    return m


@pytest.fixture(scope="module")
def handles(ifx):
    """One handle per image size of the stage tests (no frame is processed on them)."""
    made = {}

    def get(**k):
        key = (k["w"], k["h"])
        if key not in made:
            made[key] = ifx.ElasticFusion(**k, max_surfels=100000)
        return ifx.InstanceFusion(made[key])

    yield get
    for e in made.values():
        e.close()


def _misaligned(t):
    """The same values in a contiguous tensor that starts one element past an aligned address."""
    import torch

    buf = torch.zeros(t.numel() + 1, dtype=t.dtype, device=t.device)
    v = buf[1:].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 != 0
    return v


def _smooth(rng, n, M):
    """n smooth M x M probability fields, none of whose samples is exactly 0.5 or 0.25"""
    y, x = np.mgrid[0:M, 0:M].astype(np.float64) / max(M - 1, 1)
    out = np.zeros((n, M, M), np.float32)
    for i in range(n):
        cx, cy = rng.uniform(0.3, 0.7, 2)
        p = 1.0 / (1.0 + np.exp((np.hypot(x - cx, y - cy) - rng.uniform(0.25, 0.6)) * rng.uniform(6, 20)))
        p += 0.1 * np.cos(rng.uniform(-9, 9) * x + rng.uniform(-9, 9) * y)
        out[i] = np.clip(p, 0.0, 1.0)
    out[out == np.float32(0.5)] = np.float32(0.51)
    out[out == np.float32(0.25)] = np.float32(0.26)
    return out


def _stage(inst, rois, boxes, cls, thr, misaligned=False):
    import torch

    tr, tb = torch.from_numpy(rois).cuda(), torch.from_numpy(boxes).cuda()
    if misaligned:
        tr, tb = _misaligned(tr), _misaligned(tb)
    return inst.paste_roi_masks(tr, tb, cls, threshold=thr)


def _check_stage(inst, rois, boxes, cls, thr, misaligned=False):
    W, H = inst.ef.w, inst.ef.h
    got = _stage(inst, rois, boxes, cls, thr, misaligned)
    want = rp.paste_rois(rois, boxes, cls, W, H, thr)
    for g, w, what in zip(got, want, ("ori", "clean", "order", "class ids")):
        assert g.dtype == w.dtype and g.shape == w.shape, what
        assert np.array_equal(g, w), (what, np.argwhere(g != w)[:5])
    return got


def _mixed_case(rng, M, W, H, thr):
    """The edge cases of one call: (rois, boxes, class ids)"""
    t = np.float32(thr)
    boxes = [
        [50, 40, 50, 40],                        # one pixel
        [0, 0, W - 1, H - 1],                    # the expansion leaves the image on all four sides
        [-20.5, 30, 25, 70.25],                  # partly outside: left
        [W - 30, 20.5, W + 40, 60],              # right
        [60, -15, 100.75, 22],                   # top
        [30.5, H - 25, 70, H + 30],              # bottom
        [90, 50, 60, 80],                        # x1 < x0
        [np.nan, 10, 40, 40],                    # NaN box: empty
        [W + 10, 10, W + 50, 40],                # wholly outside: empty
        [20, 20, 51, 47],                        # two ROIs of equal area: the same ROI and box size, shifted by whole pixels
        [70, 60, 101, 87],
        [10.25, 70.5, 45.5, 110.75],             # all below the threshold
        [100, 10, 150.5, 58],                    # samples exactly at the threshold, 2 x 2 plateaus among them
        [40.5, 35.5, 95.5, 100.5],               # a NaN sample
        [5.3, 5.4, 5.6, 5.9],                    # sub-pixel
        [0, 0, np.inf, 30],                      # infinite coordinate: empty
    ]
    n = len(boxes)
    rois = _smooth(rng, n, M)
    if M == 1:
        rois = np.clip(rois, np.float32(0.8), None)      # (one sample: keep it above both thresholds, or most of the masks are empty)
    rois[10] = rois[9]
    rois[11] = np.minimum(rois[11], t) * np.float32(0.9)
    rois[12][rng.random((M, M)) < 0.3] = t
    if M >= 4:
        rois[12][1:3, 1:3] = t
        rois[12][M - 2:, M - 2:] = t
    rois[13][M // 2, M // 2] = np.nan
    return rois, np.asarray(boxes, np.float32), (100 + np.arange(n)).astype(np.int32)


@pytest.mark.parametrize("M", [1, 14, 28, 29, 64])
def test_stage_equals_the_statement(handles, M):
    """One call with every edge case of the rule at 160x120, aligned and one float past alignment, thresholds 0.5 and 0.25; the same at a width of 100."""
    rng = np.random.default_rng(100 + M)
    inst = handles(**TINY)
    for thr, misaligned in ((0.5, False), (0.25, True)):
        rois, boxes, cls = _mixed_case(rng, M, 160, 120, thr)
        ori, clean, order, _ = _check_stage(inst, rois, boxes, cls, thr, misaligned)
        area = (ori != 0).reshape(len(order), -1).sum(axis=1)
        assert (np.diff(area) <= 0).all() and area[0] > 1000 and (area == 0).sum() >= 4
        r9, r10 = int(np.nonzero(order == 9)[0][0]), int(np.nonzero(order == 10)[0][0])
        assert area[r9] == area[r10] > 0 and r10 == r9 + 1                           # equal areas keep their input order
        assert (clean != ori).any()
    rois, boxes, cls = _mixed_case(rng, M, 100, 76, 0.5)
    _check_stage(handles(**NARROW), rois, boxes, cls, 0.5)


def test_stage_none_one_and_many(handles):
    """n = 0, n = 1 and n = 256 tiny ROIs (boxes of 0 .. 6 pixels scattered over the image, many of equal area)."""
    import torch

    rng = np.random.default_rng(7)
    inst = handles(**TINY)
    out = inst.paste_roi_masks(torch.zeros((0, 28, 28), device="cuda"), torch.zeros((0, 4), device="cuda"), np.zeros(0, np.int32), threshold=0.5)
    assert out[0].shape == (0, 120, 160) and out[2].shape == (0,)
    _check_stage(inst, _smooth(rng, 1, 28), np.asarray([[30.5, 20, 90, 77.5]], np.float32), np.asarray([5], np.int32), 0.5)
    n = 256
    xy = np.stack([rng.uniform(-3, 160, n), rng.uniform(-3, 120, n)], axis=1)
    boxes = np.concatenate([xy, xy + rng.integers(0, 7, (n, 2))], axis=1).astype(np.float32)
    ori, _, order, cls = _check_stage(inst, np.clip(_smooth(rng, n, 7) + 0.3, 0, 1).astype(np.float32), boxes, np.arange(n, dtype=np.int32), 0.5)
    assert sorted(order.tolist()) == list(range(n)) and np.array_equal(cls, order)
    assert len(set((ori != 0).reshape(n, -1).sum(axis=1).tolist())) < n // 2     # ties: the order is the stable one


def test_stage_equals_the_reference_outside_the_tie_band(handles):
    """The fixture's inputs, one call per (size, M, threshold): every pixel farther than 2^-22 from the threshold equals maskrcnn-benchmark's own mask; the band
    holds at most 1 of every 10^5 box pixels."""
    cases = rp.load_fixture()
    groups = {}
    for c in cases:
        groups.setdefault((c["W"], c["H"], c["M"], c["thr"]), []).append(c)
    box_px = band_px = 0
    for (W, H, M, thr), g in groups.items():
        inst = handles(**(TINY if W == 160 else SMALL))
        rois, boxes = np.stack([c["roi"] for c in g]), np.stack([c["box"] for c in g])
        ori, _, order, _ = _stage(inst, rois, boxes, np.arange(len(g), dtype=np.int32), thr)
        assert sorted(order.tolist()) == list(range(len(g)))
        for rank, src in enumerate(order):
            c = g[src]
            _, band = rp.paste_roi(c["roi"], c["box"], W, H, thr, with_band=True)
            rect, _ = rp.paste_values(c["roi"], c["box"], W, H)
            box_px += (rect[1] - rect[0]) * (rect[3] - rect[2])
            band_px += int(band.sum())
            diff = ((ori[rank] != 0) != c["ref"]) & ~band
            assert not diff.any(), (W, H, M, thr, c["box"], np.argwhere(diff)[:4])
    print(f"{box_px} box pixels, {band_px} within 2^-22 of the threshold")
    assert box_px > 1000000 and band_px * 100000 <= box_px, (band_px, box_px)


# ---- the full calls against the existing device entries on twins

def _prepared(a):
    m = a.download()
    m["pc"][:, 3] = 20.0
    return m


def _twins(ifx, st, n_frames=8, clear_votes=False, **opts):
    """test_gpu_seg_device_masks._twins: two handles on the same labelled-ready map (every surfel stable after frame 3)"""
    a = ifx.ElasticFusion(**SMALL, max_surfels=400000)
    b = ifx.ElasticFusion(**SMALL, max_surfels=400000)
    for e in (a, b):
        for k, v in opts.items():
            e.set_option(k, v)
    for i in range(n_frames):
        pa = a.processFrame(st["rgb"][i], st["depth"][i]); pb = b.processFrame(st["rgb"][i], st["depth"][i])
        assert np.array_equal(pa, pb)
        if i == 3:
            m = _prepared(a)
            if clear_votes:
                m["votes"][:] = 0.0
            for e in (a, b):
                e.upload(m); e.set_pose(pa, a.tick)
    return a, b, ifx.InstanceFusion(a), ifx.InstanceFusion(b)


def _same(ia, ib, what):
    assert np.array_equal(ia.getInstanceTable(), ib.getInstanceTable()), what
    assert np.array_equal(ia.getLoopClosureInstanceTable(), ib.getLoopClosureInstanceTable()), what
    assert np.array_equal(ia.labels(), ib.labels()), what


def _same_maps(a, b):
    ma, mb = a.download(), b.download()
    for k in MAP_KEYS:
        assert np.array_equal(ma[k], mb[k]), k


def _roi_case(st, i, rng):
    """The canned masks of frame i as a mask head would hand them over -- tight boxes, 28 x 28 area averages, shuffled -- and the statement's paste of them
    (uint8 0/255, the same order): (rois, boxes, class ids, pasted)."""
    from instancefusion_amd import synth

    masks, cls = synth.canned_masks(st["obj"][i], st["scene"])
    rois, boxes = rp.rois_from_masks(masks)
    perm = rng.permutation(len(masks))
    rois, boxes, cls, masks = rois[perm], boxes[perm], np.asarray(cls, np.int32)[perm], masks[perm]
    pasted = np.stack([rp.paste_roi(r, b, SMALL["w"], SMALL["h"], 0.5) for r, b in zip(rois, boxes)])
    for p, m in zip(pasted, masks):
        if (m != 0).sum() > 50:
            assert ((p != 0) & (m != 0)).sum() / ((p != 0) | (m != 0)).sum() > 0.8    # (the ROI form is a faithful one of the canned mask)
    return rois, boxes, cls, pasted


def test_full_call_equals_the_device_entry_on_pasted_masks(ifx, small_stream):
    """Twins at frames 4..7, superpixels on and off, one call with the kNN smoothing: ROIs on one, the device entry fed the statement's paste on the other."""
    import torch

    st = small_stream
    rng = np.random.default_rng(21)
    a = ifx.ElasticFusion(**SMALL, max_surfels=400000)
    b = ifx.ElasticFusion(**SMALL, max_surfels=400000)
    ia, ib = ifx.InstanceFusion(a), ifx.InstanceFusion(b)
    for i in range(8):
        pa = a.processFrame(st["rgb"][i], st["depth"][i]); pb = b.processFrame(st["rgb"][i], st["depth"][i])
        assert np.array_equal(pa, pb)
        if i == 3:
            m = _prepared(a)
            for e in (a, b):
                e.upload(m); e.set_pose(pa, a.tick)
        if i >= 4:
            rois, boxes, cls, pasted = _roi_case(st, i, rng)
            kw = dict(isflann=(i == 6), superpixels=(i != 5))
            t = torch.from_numpy(rois).cuda()
            ia.process_segmentation_rois(t.unsqueeze(1) if i == 7 else t, torch.from_numpy(boxes).cuda(), cls, 100 + 3 * i, **kw)
            ib.process_segmentation_device(torch.from_numpy(pasted).cuda(), cls, 100 + 3 * i, **kw)
            _same(ia, ib, i)
    assert (ia.labels() >= 0).sum() > 100
    assert (ia.getInstanceTable() >= 0).sum() >= 2
    _same_maps(a, b)
    assert np.array_equal(ia.renderProjectMap(), ib.renderProjectMap())
    a.close(); b.close()


def test_deferred_rois(ifx, small_stream):
    """Lag 0: snapshot + deferred ROI call equals the ordinary ROI call.  Lag 4 with the camera moving: equals the deferred device entry fed the pasted masks."""
    import torch

    st = small_stream
    rng = np.random.default_rng(22)
    a, b, ia, ib = _twins(ifx, st, 5, clear_votes=True)
    for k, sp in enumerate((True, False)):
        rois, boxes, cls, _ = _roi_case(st, 4, rng)
        tr, tb = torch.from_numpy(rois).cuda(), torch.from_numpy(boxes).cuda()
        t = ia.snapshot(superpixels=sp)
        ia.process_segmentation_deferred_rois(t, tr, tb, cls, 100 + 3 * k, superpixels=sp)
        assert ia.snapshot_stats(t)["in_use"] == 0          # a successful call releases its ticket
        ib.process_segmentation_rois(tr, tb, cls, 100 + 3 * k, superpixels=sp)
        _same(ia, ib, ("lag 0", sp))
    assert (ia.getInstanceTable() >= 0).sum() >= 1
    _same_maps(a, b)
    pose5 = None
    for i in range(5, 10):
        pa = a.processFrame(st["rgb"][i], st["depth"][i]); pb = b.processFrame(st["rgb"][i], st["depth"][i])
        assert np.array_equal(pa, pb)
        if i == 5:
            pose5 = pa.copy()
            ta, tb_ = ia.snapshot(superpixels=True), ib.snapshot(superpixels=True)
    assert not np.array_equal(pose5, pa)                       # the camera moved
    rois, boxes, cls, pasted = _roi_case(st, 5, rng)
    ia.process_segmentation_deferred_rois(ta, torch.from_numpy(rois).cuda(), torch.from_numpy(boxes).cuda(), cls, 200, superpixels=True)
    ib.process_segmentation_deferred_device(tb_, torch.from_numpy(pasted).cuda(), cls, 200, superpixels=True)
    _same(ia, ib, "lag 4")
    assert (ia.labels() >= 0).sum() > 100
    _same_maps(a, b)
    a.close(); b.close()


def test_rois_written_on_a_producer_stream(ifx, small_stream):
    """ROI masks, boxes and class ids written into zeroed tensors on a side stream behind several milliseconds of other work there; the call gets that stream and
    no host synchronisation: it must wait on the device (a call that does not reads zeros and registers nothing)."""
    import torch

    st = small_stream
    a, b, ia, ib = _twins(ifx, st)
    rois, boxes, cls, pasted = _roi_case(st, 7, np.random.default_rng(23))
    src_r, src_b, src_c = torch.from_numpy(rois).cuda(), torch.from_numpy(boxes).cuda(), torch.from_numpy(cls).cuda()
    dst_r, dst_b, dst_c = torch.zeros_like(src_r), torch.zeros_like(src_b), torch.zeros_like(src_c)
    x = torch.randn(4096, 4096, device="cuda") / 64.0
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        y = x
        for _ in range(8):
            y = y @ x
        one = (y[0, 0] == y[0, 0]).to(torch.float32)           # (depends on the chain's result; 1 unless the chain produced NaN)
        dst_r.copy_(src_r * one)
        dst_b.copy_(src_b * one)
        dst_c.copy_(src_c)
    ia.process_segmentation_rois(dst_r, dst_b, dst_c, 100, superpixels=True, stream=s)
    ib.process_segmentation_device(torch.from_numpy(pasted).cuda(), cls, 100, superpixels=True)
    torch.cuda.synchronize()
    assert torch.equal(dst_r, src_r) and torch.equal(dst_b, src_b)
    assert (ib.getInstanceTable() >= 0).sum() >= 1            # (zeros would register nothing)
    _same(ia, ib, "producer stream")
    _same_maps(a, b)
    a.close(); b.close()


def test_refusals_leave_the_handle_usable(ifx, small_stream):
    """Sharded handle -> IFX_E_STATE; M = 0 or 65, n = 257, null pointers -> IFX_E_INVALID; TypeError / ValueError in Python for a wrong dtype, shape or device.
    After each refusal a valid call on the same handle still equals its twin."""
    import torch

    st = small_stream
    L = ifx.lib()
    rois, boxes, cls, pasted = _roi_case(st, 7, np.random.default_rng(24))
    n = len(cls)
    d_r, d_b, d_c = torch.from_numpy(rois).cuda(), torch.from_numpy(boxes).cuda(), torch.from_numpy(cls).cuda()
    d_p = torch.from_numpy(pasted).cuda()
    big_r, big_b, big_c = torch.zeros((257, 4, 4), device="cuda"), torch.zeros((257, 4), device="cuda"), torch.zeros(257, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    P = lambda t: C.c_void_p(t.data_ptr())

    e = ifx.ElasticFusion(**SMALL, max_surfels=100000, n_ranks=-1, rank=0)
    try:
        r = L.ifx_process_segmentation_rois(e.handle, P(d_r), 28, P(d_b), 0.5, P(d_c), n, 100, 0, None)
        assert r == -4 and b"sharded" in L.ifx_last_error(e.handle)
        assert L.ifx_paste_roi_masks(e.handle, P(d_r), 28, P(d_b), 0.5, P(d_c), n, None, None, None, None, None) == -4
        assert L.ifx_process_segmentation_deferred_rois(e.handle, 0, P(d_r), 28, P(d_b), 0.5, P(d_c), n, 100, 0, None) == -4
        with pytest.raises(ifx.IfxError, match=r"\(-4\)"):
            ifx.InstanceFusion(e).process_segmentation_rois(d_r, d_b, cls, 100)
    finally:
        e.close()

    a, b, ia, ib = _twins(ifx, st)
    frame = 100

    def valid_call(what):
        nonlocal frame
        ia.process_segmentation_rois(d_r, d_b, cls, frame, superpixels=True)
        ib.process_segmentation_device(d_p, cls, frame, superpixels=True)
        _same(ia, ib, what)
        frame += 3

    refusals = [
        ("M = 0", (P(d_r), 0, P(d_b), P(d_c), n)),
        ("M = 65", (P(d_r), 65, P(d_b), P(d_c), n)),
        ("n = 257", (P(big_r), 4, P(big_b), P(big_c), 257)),
        ("n < 0", (P(d_r), 28, P(d_b), P(d_c), -1)),
        ("null ROI masks", (None, 28, P(d_b), P(d_c), n)),
        ("null boxes", (P(d_r), 28, None, P(d_c), n)),
        ("null class ids", (P(d_r), 28, P(d_b), None, n)),
    ]
    for what, (pr, M, pb, pc, nn) in refusals:
        assert L.ifx_process_segmentation_rois(a.handle, pr, M, pb, 0.5, pc, nn, frame, 2, None) == -1, what
        assert L.ifx_paste_roi_masks(a.handle, pr, M, pb, 0.5, pc, nn, None, None, None, None, None) == -1, what
        t = ia.snapshot()
        assert L.ifx_process_segmentation_deferred_rois(a.handle, t, pr, M, pb, 0.5, pc, nn, frame, 0, None) == -1, what
        ia.release_snapshot(t)
        valid_call(what)
    with pytest.raises(ValueError):
        ia.process_segmentation_rois(torch.from_numpy(rois), d_b, cls, frame)                               # CPU tensor
    with pytest.raises(ValueError):
        ia.process_segmentation_rois(d_r, torch.from_numpy(boxes), cls, frame)
    valid_call("device")
    with pytest.raises(ValueError):
        ia.process_segmentation_rois(d_r[:, :, :-1], d_b, cls, frame)                                       # not square
    with pytest.raises(ValueError):
        ia.process_segmentation_rois(d_r.unsqueeze(0), d_b, cls, frame)                                     # [1,N,M,M]
    with pytest.raises(ValueError):
        ia.process_segmentation_rois(torch.zeros((n, 65, 65), device="cuda"), d_b, cls, frame)              # M = 65
    with pytest.raises(ValueError):
        ia.process_segmentation_rois(d_r, d_b[:, :3], cls, frame)                                           # boxes [N,3]
    with pytest.raises(ValueError):
        ia.process_segmentation_rois(d_r, d_b[:-1], cls, frame)                                             # boxes of another length
    with pytest.raises(ValueError):
        ia.paste_roi_masks(d_r, d_b, cls[:-1])                                                              # class ids of another length
    valid_call("shape")
    with pytest.raises(TypeError):
        ia.process_segmentation_rois(d_r.to(torch.float64), d_b, cls, frame)                                # dtype
    with pytest.raises(TypeError):
        ia.process_segmentation_rois(d_r, d_b.to(torch.float16), cls, frame)
    with pytest.raises(TypeError):
        ia.process_segmentation_deferred_rois(0, (d_r > 0.5), d_b, cls, frame)
    with pytest.raises(TypeError):
        ia.process_segmentation_rois(rois, d_b, cls, frame)                                                 # not a tensor
    valid_call("dtype")
    assert (ib.getInstanceTable() >= 0).sum() >= 2
    _same_maps(a, b)
    a.close(); b.close()
