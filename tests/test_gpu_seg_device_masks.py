"""The segmentation call on masks already on the GPU (ifx_process_segmentation_device / InstanceFusion.process_segmentation_device) against the host entry fed what
the reference's Mask-RCNN bridge hands over (build/mask_ori.py:87-124: binarised to 0/255, then a STABLE sort by area, descending): instance tables, labels,
colours and every map array bit for bit, for every accepted format, any input order, masks written on another stream, and the resident-frame path at 640x480."""
import ctypes as C

import numpy as np
import pytest

from conftest import SMALL

pytestmark = pytest.mark.gpu

MAP_KEYS = ("pc", "nr", "col", "tm", "ic", "votes")


@pytest.fixture(scope="module")
def ifx():
    import instancefusion_amd as m

    m.lib()
    return m


def bridge(masks, class_ids):
    """The bridge's two steps, literally (build/mask_ori.py:87-124): maskNP[maskOri != 0] = 255, then sorted(results, key=lambda x: np.sum(x[0]), reverse=True)."""
    results = []
    for maskOri, c in zip(masks, class_ids):
        maskNP = np.zeros(maskOri.shape, np.uint8)
        maskNP[maskOri != 0] = 255
        results.append((maskNP, int(c)))
    results = sorted(results, key=lambda x: np.sum(x[0]), reverse=True)
    if not results:
        return np.zeros((0,) + masks.shape[1:], np.uint8), np.zeros(0, np.int32)
    return np.stack([r[0] for r in results]), np.asarray([r[1] for r in results], np.int32)


def _same(ia, ib, what):
    assert np.array_equal(ia.getInstanceTable(), ib.getInstanceTable()), what
    assert np.array_equal(ia.getLoopClosureInstanceTable(), ib.getLoopClosureInstanceTable()), what
    assert np.array_equal(ia.labels(), ib.labels()), what


def _same_maps(a, b):
    ma, mb = a.download(), b.download()
    for k in MAP_KEYS:
        assert np.array_equal(ma[k], mb[k]), k


def _twins(ifx, st, n_frames=8, **opts):
    """Two handles on the same labelled-ready map (every surfel stable after frame 3, as test_gpu_parity's schedule test)."""
    a = ifx.ElasticFusion(**SMALL, max_surfels=400000)
    b = ifx.ElasticFusion(**SMALL, max_surfels=400000)
    for e in (a, b):
        for k, v in opts.items():
            e.set_option(k, v)
    for i in range(n_frames):
        pa = a.processFrame(st["rgb"][i], st["depth"][i]); pb = b.processFrame(st["rgb"][i], st["depth"][i])
        assert np.array_equal(pa, pb)
        if i == 3:
            m = a.download(); m["pc"][:, 3] = 20.0
            for e in (a, b):
                e.upload(m); e.set_pose(pa, a.tick)
    return a, b, ifx.InstanceFusion(a), ifx.InstanceFusion(b)


@pytest.mark.parametrize("ff_rounds", [0, 2])
@pytest.mark.parametrize("seg_device", [1, 0])
def test_device_masks_equal_host_entry(ifx, small_stream, seg_device, ff_rounds):
    """test_segmentation_device_schedule_equals_host_schedule's sequence on twins: device uint8 tensors on one, the host entry with the same numpy masks on the
    other (both on the resident frame) -- calls with superpixels, one with the kNN smoothing, then new classes until the table evicts.  ff_rounds = 2 only moves
    the gate of the flood fill's fixed schedule to its second launch: on this scene (every edge two-way) the first relaxation changes nothing, and the launch
    counts of the first call, printed below, are 2 ff_relax and 1 ff_count with seg_device 1 (4 and 1 by default; 7 and 1 on the host-driven schedule, which
    ignores the option) -- the host-driven resume of an incomplete fill does not run here (tests/test_gpu_flood_fill_cases.py::test_serpentine_inside_a_call)."""
    import torch

    from instancefusion_amd import synth

    st = small_stream
    a = ifx.ElasticFusion(**SMALL, max_surfels=400000)
    b = ifx.ElasticFusion(**SMALL, max_surfels=400000)
    for e in (a, b):
        e.set_option("seg_device", seg_device); e.set_option("ff_rounds", ff_rounds)
    ia, ib = ifx.InstanceFusion(a), ifx.InstanceFusion(b)
    for i in range(8):
        pa = a.processFrame(st["rgb"][i], st["depth"][i]); pb = b.processFrame(st["rgb"][i], st["depth"][i])
        assert np.array_equal(pa, pb)
        if i == 3:
            m = a.download(); m["pc"][:, 3] = 20.0
            for e in (a, b):
                e.upload(m); e.set_pose(pa, a.tick)
        if i >= 4:
            masks, cls = synth.canned_masks(st["obj"][i], st["scene"])
            flann = i == 6
            if i == 4:      # the launch counts of one call, read once (see the docstring)
                a.set_option("kernel_timing", 1); a.kernel_ms("__reset__")
            ia.process_segmentation_device(torch.from_numpy(masks).cuda(), cls, 100 + 3 * i, isflann=flann, superpixels=True)
            if i == 4:
                print("seg_device", seg_device, "ff_rounds", ff_rounds, ": ff_relax launches", a.kernel_ms("ff_relax")[1], "ff_count launches", a.kernel_ms("ff_count")[1])
                a.set_option("kernel_timing", 0)
            ib.ProcessSegmentation(None, None, masks, cls, 100 + 3 * i, isflann=flann, superpixels=True)
            _same(ia, ib, i)
    assert (ia.labels() >= 0).sum() > 100
    i = 7
    masks, cls = synth.canned_masks(st["obj"][i], st["scene"])
    nm = masks.shape[0]
    d_masks = torch.from_numpy(masks).cuda()
    evicted = False
    for call in range(60):
        classes = (1000 + call * nm + np.arange(nm)).astype(np.int32)
        before = (ib.getInstanceTable() >= 0).sum()
        ia.process_segmentation_device(d_masks, torch.from_numpy(classes).cuda(), 300 + 3 * call)
        ib.ProcessSegmentation(None, None, masks, classes, 300 + 3 * call)
        _same(ia, ib, call)
        evicted = evicted or (ib.getInstanceTable() >= 0).sum() < before
        if evicted:
            break
    assert evicted
    _same_maps(a, b)
    assert np.array_equal(ia.renderProjectMap(), ib.renderProjectMap())
    a.close(); b.close()


def _bridge_case(st, i, rng):
    """Shuffled canned masks of frame i plus a mask of the same area as another one, placed before it, and an empty one: (bool masks, class ids)."""
    from instancefusion_amd import synth

    masks, cls = synth.canned_masks(st["obj"][i], st["scene"])
    raw = [m > 0 for m in masks]
    classes = [int(c) for c in cls]
    assert len(raw) >= 3
    tie = np.roll(raw[1], 6, axis=1)                     # same area as raw[1], overlapping it: which comes first changes the overlap clean and the votes
    assert tie.sum() == raw[1].sum() > 0
    raw.insert(1, tie); classes.insert(1, 77)            # the tie BEFORE its twin in the input
    raw.append(np.zeros_like(raw[0])); classes.append(78)
    perm = rng.permutation(len(raw))
    bm = np.stack([raw[k] for k in perm])
    bc = np.asarray([classes[k] for k in perm], np.int32)
    ti, tw = int(np.nonzero(perm == 1)[0][0]), int(np.nonzero(perm == 2)[0][0])
    if ti > tw:                                          # keep the tie before its twin after the shuffle too
        bm[[ti, tw]] = bm[[tw, ti]]; bc[[ti, tw]] = bc[[tw, ti]]
    return bm, bc


def _as_format(bm, fmt, rng, thr=0.5):
    """The same geometry as the detector may hand it over: bool, uint8 with arbitrary non-zero inside values, float32 probabilities (inside (thr, 1], outside
    [0, thr], some exactly thr)."""
    if fmt == "bool":
        return bm.copy()
    if fmt == "uint8":
        return np.where(bm, rng.integers(1, 256, bm.shape), 0).astype(np.uint8)
    lo = np.nextafter(np.float32(thr), np.float32(2))
    inside = np.maximum(rng.uniform(thr, 1.0, bm.shape).astype(np.float32), lo)
    outside = rng.uniform(0.0, thr, bm.shape).astype(np.float32)
    outside[rng.random(bm.shape) < 0.1] = np.float32(thr)
    out = np.where(bm, inside, outside).astype(np.float32)
    assert ((out > np.float32(thr)) == bm).all() and (out == np.float32(thr)).any()
    return out


def _misaligned(t):
    """The same values in a contiguous tensor that starts one element past an aligned address (16-B loads impossible)."""
    import torch

    buf = torch.zeros(t.numel() + 1, dtype=t.dtype, device=t.device)
    v = buf[1:].view(t.shape)
    v.copy_(t)
    return v


def test_bridge_order_and_formats(ifx, small_stream):
    """Shuffled masks with a tie and an empty mask as bool, uint8 and float32 probabilities (aligned, misaligned, [N,1,H,W]): the host entry fed the literal bridge
    expression of the same masks gives the same result."""
    import torch

    st = small_stream
    rng = np.random.default_rng(11)
    a, b, ia, ib = _twins(ifx, st)
    frame = 100
    cases = [("bool", False, False, 0.5), ("uint8", False, False, 0.5), ("float32", False, False, 0.5), ("uint8", True, False, 0.5),
             ("float32", True, True, 0.5), ("float32", False, True, 0.25), ("uint8", False, True, 0.5)]
    for k, (fmt, misaligned, four_d, thr) in enumerate(cases):
        i = 5 + (k % 3)
        bm, bc = _bridge_case(st, i, rng)
        raw = _as_format(bm, fmt, rng, thr)
        t = torch.from_numpy(raw).cuda()
        if four_d:
            t = t.unsqueeze(1)
        if misaligned:
            t = _misaligned(t)
            assert t.data_ptr() % 16 != 0
        cls = torch.from_numpy(bc.astype(np.int64)).cuda() if k % 2 else bc.tolist()
        sp = k % 2 == 0
        ia.process_segmentation_device(t, cls, frame, superpixels=sp, threshold=thr)
        hm, hc = bridge(bm, bc)
        ib.ProcessSegmentation(None, None, hm, hc, frame, superpixels=sp)
        _same(ia, ib, (k, fmt))
        frame += 3
    assert (ib.getInstanceTable() >= 0).sum() >= 3
    assert (ia.labels() >= 0).sum() > 100
    _same_maps(a, b)
    a.close(); b.close()


def test_masks_written_on_a_producer_stream(ifx, small_stream):
    """Masks and class ids written into zeroed tensors on a side stream behind several milliseconds of other work there; the call gets that stream and no host
    synchronisation: it must wait on the device (a call that does not reads zeros)."""
    import torch

    from instancefusion_amd import synth

    st = small_stream
    a, b, ia, ib = _twins(ifx, st)
    masks, cls = synth.canned_masks(st["obj"][7], st["scene"])
    src, cls_src = torch.from_numpy(masks).cuda(), torch.from_numpy(cls).cuda()
    dst, cls_dst = torch.zeros_like(src), torch.zeros_like(cls_src)
    x = torch.randn(4096, 4096, device="cuda") / 64.0
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        y = x
        for _ in range(8):
            y = y @ x
        dst.copy_(src * (y[0, 0] == y[0, 0]).to(torch.uint8))   # (depends on the chain's result; NaN-safe: 1 unless the chain produced NaN)
        cls_dst.copy_(cls_src)
    ia.process_segmentation_device(dst, cls_dst, 100, superpixels=True, stream=s)
    ib.ProcessSegmentation(None, None, masks, cls, 100, superpixels=True)
    torch.cuda.synchronize()
    assert torch.equal(dst, src)
    assert (ib.getInstanceTable() >= 0).sum() >= 1          # (zeros would register nothing)
    _same(ia, ib, "producer stream")
    _same_maps(a, b)
    a.close(); b.close()


def test_resident_frame_path_640x480(ifx):
    """Frames through enqueue_frame_device + hint_next_frame_device (the call then runs on the third stream beside the next frame's tracker, the superpixels run
    ahead on the side stream): device-mask calls on shuffled masks against the host entry on the bridge of the same masks."""
    import torch

    from instancefusion_amd import synth

    n, W, H = 12, 640, 480
    st = synth.make_stream(n, W, H, 528.0, 528.0, 320.0, 240.0, noise=True)
    d_rgb = torch.from_numpy(st["rgb"][:n].copy()).cuda()
    d_dep = torch.from_numpy(st["depth"][:n].view(np.int16).copy()).cuda()
    torch.cuda.synchronize()
    outs = []
    for dev in (True, False):
        rng = np.random.default_rng(3)
        g = ifx.ElasticFusion(w=W, h=H, fx=528.0, fy=528.0, cx=320.0, cy=240.0, max_surfels=2_000_000, confidence=2.0)
        inst = ifx.InstanceFusion(g)
        g.set_option("slic_ahead", 2)
        seen = []
        for i in range(n):
            if i + 1 < n:
                g.hint_next_frame_device(d_rgb[i + 1].data_ptr(), d_dep[i + 1].data_ptr())
            g.enqueue_frame_device(d_rgb[i].data_ptr(), d_dep[i].data_ptr(), i)
            inst.whetherDoSegmentation(-(1 << 30))
            if i == 3:   # every surfel stable from here on, so that the calls label (the announced frame's parked tracker is dropped by the upload)
                g.sync()
                m = g.download(); m["pc"][:, 3] = 20.0
                pose = g.getCurrPose()
                g.upload(m); g.set_pose(pose, g.tick); g.combined_predict(pose, g.tick, g.tick)
            if i in (5, 7, 8, 10):
                mk, cl = synth.canned_masks(st["obj"][i], st["scene"])
                perm = rng.permutation(len(mk))
                if dev:
                    inst.process_segmentation_device(torch.from_numpy(mk[perm]).cuda(), cl[perm], 10 + i, superpixels=True)
                else:
                    hm, hc = bridge(mk[perm], cl[perm])
                    inst.ProcessSegmentation(None, None, hm, hc, 10 + i, superpixels=True)
                seen.append((inst.getInstanceTable(), inst.getLoopClosureInstanceTable(), inst.labels()))
        g.sync()
        outs.append((seen, g.trajectory(), g.download(), inst.labels(), g.image("ids_after"), g.superpixel_ahead_stats()))
        g.close()
    a, b = outs
    for k, (x, y) in enumerate(zip(a[0], b[0])):
        assert all(np.array_equal(p, q) for p, q in zip(x, y)), k
    assert np.array_equal(a[1], b[1]) and np.array_equal(a[3], b[3]) and np.array_equal(a[4], b[4])
    assert all(np.array_equal(a[2][k], b[2][k]) for k in MAP_KEYS)
    assert a[5]["runs"] == b[5]["runs"] and a[5]["used"] == b[5]["used"] and a[5]["used"] >= 1, (a[5], b[5])
    assert (a[3] >= 0).sum() > 100


def test_refusals_leave_the_handle_usable(ifx, small_stream):
    """Sharded handle -> IFX_E_STATE; n = 257, an unknown format, null pointers -> IFX_E_INVALID; TypeError / ValueError in Python for a CPU tensor, a wrong shape
    or dtype.  After each refusal a valid call on the same handle still equals its twin."""
    import torch

    from instancefusion_amd import synth

    st = small_stream
    L = ifx.lib()
    masks, cls = synth.canned_masks(st["obj"][7], st["scene"])
    n = masks.shape[0]
    d_m, d_c = torch.from_numpy(masks).cuda(), torch.from_numpy(cls).cuda()
    big = torch.zeros((257,) + masks.shape[1:], dtype=torch.uint8, device="cuda")
    big_c = torch.zeros(257, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()

    e = ifx.ElasticFusion(**SMALL, max_surfels=100000, n_ranks=-1, rank=0)
    try:
        r = L.ifx_process_segmentation_device(e.handle, C.c_void_p(d_m.data_ptr()), ifx.MASK_U8, 0.5, C.c_void_p(d_c.data_ptr()), n, 100, 0, None)
        assert r == -4 and b"sharded" in L.ifx_last_error(e.handle)
        with pytest.raises(ifx.IfxError, match=r"\(-4\)"):
            ifx.InstanceFusion(e).process_segmentation_device(d_m, cls, 100)
    finally:
        e.close()

    a, b, ia, ib = _twins(ifx, st)
    frame = 100

    def valid_call(what):
        nonlocal frame
        ia.process_segmentation_device(d_m, cls, frame, superpixels=True)
        ib.ProcessSegmentation(None, None, masks, cls, frame, superpixels=True)
        _same(ia, ib, what)
        frame += 3

    refusals = [
        ("n = 257", (C.c_void_p(big.data_ptr()), ifx.MASK_U8, 0.5, C.c_void_p(big_c.data_ptr()), 257)),
        ("n < 0", (C.c_void_p(d_m.data_ptr()), ifx.MASK_U8, 0.5, C.c_void_p(d_c.data_ptr()), -1)),
        ("format", (C.c_void_p(d_m.data_ptr()), 7, 0.5, C.c_void_p(d_c.data_ptr()), n)),
        ("null masks", (None, ifx.MASK_U8, 0.5, C.c_void_p(d_c.data_ptr()), n)),
        ("null class ids", (C.c_void_p(d_m.data_ptr()), ifx.MASK_F32, 0.5, None, n)),
    ]
    for what, (pm, fmt, thr, pc, nn) in refusals:
        r = L.ifx_process_segmentation_device(a.handle, pm, fmt, thr, pc, nn, frame, 2, None)
        assert r == -1, (what, r)
        valid_call(what)
    with pytest.raises(ValueError):
        ia.process_segmentation_device(torch.from_numpy(masks), cls, frame)                                 # CPU tensor
    valid_call("cpu tensor")
    with pytest.raises(ValueError):
        ia.process_segmentation_device(d_m[:, :-1], cls, frame)                                             # wrong shape
    with pytest.raises(ValueError):
        ia.process_segmentation_device(d_m.unsqueeze(0), cls, frame)                                         # [1,N,H,W]
    valid_call("shape")
    with pytest.raises(TypeError):
        ia.process_segmentation_device(d_m.to(torch.float64), cls, frame)                                   # dtype
    with pytest.raises(TypeError):
        ia.process_segmentation_device(d_m.to(torch.int32), cls, frame)
    with pytest.raises(ValueError):
        ia.process_segmentation_device(d_m, cls[:-1], frame)                                                # class ids of another length
    valid_call("dtype")
    assert (ib.getInstanceTable() >= 0).sum() >= 2
    _same_maps(a, b)
    a.close(); b.close()
