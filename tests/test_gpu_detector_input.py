"""The detector's input made on the device (ifx_detector_input / ifx_detector_input_image): bit for bit the numpy statement of the reference's CPU transform
(tests/detector_input_numpy.py, itself held against maskrcnn-benchmark's size functions, Pillow and CPU torch in test_detector_input_cpu.py) -- on explicit
images through the stage call, on the resident frame (also with the next frame announced), on a snapshot's frame three frames later without disturbing the
deferred call, on a consumer stream without host synchronisation; and every refusal leaves the handle usable."""
import ctypes as C

import numpy as np
import pytest

import detector_input_numpy as dn
from conftest import SMALL

pytestmark = pytest.mark.gpu

E_INVALID, E_STATE = -1, -4
Q = dict(w=160, h=120, fx=132.0, fy=132.0, cx=80.0, cy=60.0)
MEAN_255, STD_255 = (102.9801, 115.9465, 122.7717), (57.375, 57.12, 58.395)
MEAN_01, STD_01 = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
# (w, h, min_size, max_size, size_divisible)
STAGE_CASES = [(20, 12, 32, None, 0), (64, 48, 56, None, 32), (64, 48, 48, None, 0), (48, 64, 56, None, 32), (160, 120, 40, None, 32), (160, 120, 16, None, 0),
               (160, 120, 100, 120, 32), (70, 50, 64, None, 32)]


@pytest.fixture(scope="module")
def ifx():
    import instancefusion_amd as m

    m.lib()
    return m


@pytest.fixture(scope="module")
def stage_handle(ifx):
    """a handle that never sees a frame: the stage call needs none"""
    e = ifx.ElasticFusion(**Q, max_surfels=100000)
    yield e
    e.close()


@pytest.fixture(scope="module")
def quarter_stream():
    from instancefusion_amd import synth

    return synth.make_stream(5, Q["w"], Q["h"], Q["fx"], Q["fy"], Q["cx"], Q["cy"], noise=True)


def _images(w, h):
    rng = np.random.default_rng(w * 1000 + h)
    g = np.add.outer(np.arange(h) * 3, np.arange(w) * 2)
    return {"random": rng.integers(0, 256, (h, w, 3), dtype=np.uint8),
            "gradient": np.stack([g % 256, (g * 2 + 40) % 256, 255 - g % 256], axis=2).astype(np.uint8),
            "zeros": np.zeros((h, w, 3), np.uint8), "full": np.full((h, w, 3), 255, np.uint8)}


def _params(flags):
    to255, swap = bool(flags & 2), bool(flags & 1)
    return dict(mean=MEAN_255 if to255 else MEAN_01, std=STD_255 if to255 else STD_01, to_bgr255=to255, swap_rb=swap)


def _statement(small, size, flags):
    """the float tail and the padding on an image the statement has resized already (one resize serves the four flag combinations)"""
    ow, oh, Wp, Hp = size
    p = _params(flags)
    out = np.zeros((1, 3, Hp, Wp), np.float32)
    out[0, :, :oh, :ow] = dn.float_tail(small.transpose(2, 0, 1), p["mean"], p["std"], p["to_bgr255"], p["swap_rb"])
    return out


def _equal(got, ref):
    return got.shape == ref.shape and got.dtype == ref.dtype == np.float32 and np.array_equal(got, ref)


@pytest.mark.parametrize("case", STAGE_CASES, ids=lambda c: "x".join(str(v) for v in c))
def test_stage_call_equals_the_statement(ifx, stage_handle, case):
    """ifx_detector_input_image on random / gradient / all-0 / all-255 images x the four flag combinations: every float equal, the padding exactly 0.0"""
    import torch

    w, h, mn, mx, d = case
    size = dn.input_size(w, h, mn, mx, d)
    ow, oh, Wp, Hp = size
    assert ifx.detector_input_size(w, h, mn, mx, d) == size
    for name, img in _images(w, h).items():
        small = dn.resize(img, ow, oh)
        d_img = torch.from_numpy(img).cuda()
        for flags in range(4):
            t, (goh, gow) = ifx.detector_input_image(stage_handle, d_img, min_size=mn, max_size=mx, size_divisible=d, **_params(flags))
            torch.cuda.synchronize()
            got = t.cpu().numpy()
            ref = _statement(small, size, flags)
            assert (goh, gow) == (oh, ow) and tuple(t.shape) == (1, 3, Hp, Wp)
            assert _equal(got, ref), (case, name, flags, int((got != ref).sum()))
            pad = np.concatenate([got[0, :, :, ow:].reshape(-1), got[0, :, oh:, :].reshape(-1)])
            assert not pad.view(np.uint32).any(), (case, name, flags)          # literal +0.0


def test_unaligned_output_and_guard_bands(ifx, stage_handle):
    """W' a multiple of 4 but the pointer 4 bytes off a 16-byte boundary: the 4-byte store path writes the same floats; nothing is written outside the tensor"""
    import torch

    w, h, mn, d = 70, 50, 64, 32
    size = dn.input_size(w, h, mn, None, d)
    ow, oh, Wp, Hp = size
    img = _images(w, h)["random"]
    ref = _statement(dn.resize(img, ow, oh), size, 3)
    n = 3 * Hp * Wp
    buf = torch.full((n + 64,), -7.0, dtype=torch.float32, device="cuda")
    for off in (32, 33):
        buf.fill_(-7.0)
        out = buf[off:off + n].view(1, 3, Hp, Wp)
        assert (out.data_ptr() % 16 == 0) == (off == 32)
        t, _ = ifx.detector_input_image(stage_handle, torch.from_numpy(img).cuda(), min_size=mn, size_divisible=d, out=out, **_params(3))
        torch.cuda.synchronize()
        assert t.data_ptr() == out.data_ptr()
        host = buf.cpu().numpy()
        assert _equal(host[off:off + n].reshape(1, 3, Hp, Wp), ref), off
        assert (host[:off] == -7.0).all() and (host[off + n:] == -7.0).all(), off
    with pytest.raises(ValueError):
        ifx.detector_input_image(stage_handle, torch.from_numpy(img).cuda(), min_size=mn, size_divisible=d, out=torch.zeros(1, 3, Hp, Wp + 1, device="cuda"))
    with pytest.raises(TypeError):
        ifx.detector_input_image(stage_handle, torch.from_numpy(img).cuda(), min_size=mn, size_divisible=d, out=torch.zeros(1, 3, Hp, Wp, device="cuda", dtype=torch.float64))
    with pytest.raises(ValueError):
        ifx.detector_input_image(stage_handle, torch.from_numpy(img).cuda(), min_size=mn, size_divisible=d, out=torch.zeros(1, 3, Hp, Wp))


def test_more_sizes_than_the_table_cache_holds(ifx, stage_handle):
    """the handle keeps the tap tables of eight (w, h, ow, oh); twelve sizes in turn, twice: evicted tables are rebuilt and every result is the statement's"""
    import torch

    img = _images(64, 48)["random"]
    d_img = torch.from_numpy(img).cuda()
    refs = {mn: dn.detector_input(img, min_size=mn, size_divisible=0, **_params(1))[0] for mn in range(30, 54, 2)}
    for _ in range(2):
        for mn, ref in refs.items():
            t, _ = ifx.detector_input_image(stage_handle, d_img, min_size=mn, size_divisible=0, **_params(1))
            torch.cuda.synchronize()
            assert _equal(t.cpu().numpy(), ref), mn


def test_resident_frame(ifx, quarter_stream):
    """160 x 120: after two frames the call gives the statement on the frame fed last; with frame t + 1 announced before frame t is enqueued
    (ifx_hint_next_frame_device) it is still frame t's, and after frame t + 1 it is that frame's (the announced copy-in waited for the read)."""
    import torch

    st = quarter_stream
    kw = dict(min_size=100, size_divisible=32, **_params(3))
    refs = [dn.detector_input(st["rgb"][i], **kw) for i in range(5)]
    e = ifx.ElasticFusion(**Q, max_surfels=200000)
    inst = ifx.InstanceFusion(e)
    assert inst.detector_input_size(100, None, 32) == (133, 100, 160, 128)
    for i in range(2):
        e.processFrame(st["rgb"][i], st["depth"][i])
    t, size = inst.detector_input(**kw)
    torch.cuda.synchronize()
    assert size == refs[1][1] == (100, 133)
    assert _equal(t.cpu().numpy(), refs[1][0])
    e.close()
    e = ifx.ElasticFusion(**Q, max_surfels=200000)
    inst = ifx.InstanceFusion(e)
    d_rgb = torch.from_numpy(st["rgb"].copy()).cuda()
    d_dep = torch.from_numpy(st["depth"].view(np.int16).copy()).cuda()
    torch.cuda.synchronize()
    outs = []
    for i in (0, 1):
        e.enqueue_frame_device(d_rgb[i].data_ptr(), d_dep[i].data_ptr(), i)
    for i in (2, 3):
        e.hint_next_frame_device(d_rgb[i + 1].data_ptr(), d_dep[i + 1].data_ptr())      # frame i + 1 is announced: its copy-in may start under frame i
        e.enqueue_frame_device(d_rgb[i].data_ptr(), d_dep[i].data_ptr(), i)
        outs.append(inst.detector_input(**kw)[0])                                       # (no host synchronisation in between)
    e.enqueue_frame_device(d_rgb[4].data_ptr(), d_dep[4].data_ptr(), 4)
    outs.append(inst.detector_input(**kw)[0])
    torch.cuda.synchronize()
    for i, t in zip((2, 3, 4), outs):
        assert _equal(t.cpu().numpy(), refs[i][0]), i
    e.close()


def _prepared_run(ifx, st, with_detector_input):
    """frames 0..8 of the 320 x 240 stream, every surfel stable after frame 3 (test_gpu_seg_deferred's preparation), a snapshot with its frame after frame 5"""
    import torch

    e = ifx.ElasticFusion(**SMALL, max_surfels=400000)
    inst = ifx.InstanceFusion(e)
    poses, ticket, got = [], None, None
    for i in range(9):
        p = e.processFrame(st["rgb"][i], st["depth"][i])
        poses.append(p.copy())
        if i == 3:
            m = e.download()
            m["pc"][:, 3] = 20.0
            m["votes"][:] = 0.0
            e.upload(m); e.set_pose(p, e.tick)
        if i == 5:
            ticket = inst.snapshot(superpixels=True)
    if with_detector_input:
        t, size = inst.detector_input(ticket, min_size=200, size_divisible=32, **_params(2))
        torch.cuda.synchronize()
        got = (t.cpu().numpy(), size)
    return e, inst, ticket, poses, got


def test_ticket_frame_and_undisturbed_deferred_call(ifx, small_stream):
    """snapshot(superpixels=True) at frame 5, three more frames: detector_input(ticket) is the statement on frame 5's image, the ticket is still valid, and the
    deferred call on it gives the labels, tables and map of a run that never called detector_input, with equal poses"""
    from instancefusion_amd import synth

    st = small_stream
    a, ia, ta, pa, got = _prepared_run(ifx, st, True)
    b, ib, tb, pb, _ = _prepared_run(ifx, st, False)
    ref, size = dn.detector_input(st["rgb"][5], min_size=200, size_divisible=32, **_params(2))
    assert got[1] == size == (200, 266)
    assert _equal(got[0], ref)
    assert not _equal(got[0], dn.detector_input(st["rgb"][8], min_size=200, size_divisible=32, **_params(2))[0])      # (the resident frame is another one)
    assert ia.snapshot_stats(ta)["in_use"] == 1                  # not released
    for x, y in zip(pa, pb):
        assert np.array_equal(x, y)
    masks, cls = synth.canned_masks(st["obj"][5], st["scene"])
    ia.process_segmentation_deferred(ta, masks, cls, 100, superpixels=True)
    ib.process_segmentation_deferred(tb, masks, cls, 100, superpixels=True)
    assert np.array_equal(ia.labels(), ib.labels()) and (ia.labels() >= 0).sum() >= 100
    assert np.array_equal(ia.getInstanceTable(), ib.getInstanceTable())
    assert np.array_equal(ia.getLoopClosureInstanceTable(), ib.getLoopClosureInstanceTable())
    ma, mb = a.download(), b.download()
    for k in ("pc", "nr", "col", "tm", "ic", "votes"):
        assert np.array_equal(ma[k], mb[k]), k
    a.close(); b.close()


def test_consumer_stream(ifx, quarter_stream):
    """stream = a torch side stream: a clone enqueued on that stream with no host synchronisation in front of it sees the finished tensor; a second call into the
    same tensor waits for that clone (the entry's event) and the second clone sees the second result"""
    import torch

    st = quarter_stream
    e = ifx.ElasticFusion(**Q, max_surfels=200000)
    inst = ifx.InstanceFusion(e)
    for i in range(2):
        e.processFrame(st["rgb"][i], st["depth"][i])
    side = torch.cuda.Stream()
    kw1 = dict(min_size=120, size_divisible=32, **_params(3))
    kw2 = dict(min_size=120, size_divisible=32, **_params(0))
    out, _ = inst.detector_input(stream=side, **kw1)
    with torch.cuda.stream(side):
        c1 = out.clone()
    out2, _ = inst.detector_input(stream=side, out=out, **kw2)
    with torch.cuda.stream(side):
        c2 = out2.clone()
    torch.cuda.synchronize()
    assert out2.data_ptr() == out.data_ptr()
    assert _equal(c1.cpu().numpy(), dn.detector_input(st["rgb"][1], **kw1)[0])
    assert _equal(c2.cpu().numpy(), dn.detector_input(st["rgb"][1], **kw2)[0])
    e.close()


def test_refusals(ifx, quarter_stream):
    """every refusal of include/ifx_c_api.h, each followed by a successful call on the same handle"""
    import torch

    from instancefusion_amd import sharded

    st = quarter_stream
    L = ifx.lib()
    kw = dict(min_size=100, size_divisible=32, **_params(3))
    ref = dn.detector_input(st["rgb"][1], **kw)[0]
    good = ifx.detector_prep(**kw)
    n = ref.size
    d_out = torch.zeros(n, dtype=torch.float32, device="cuda")
    d_img = torch.from_numpy(st["rgb"][1].copy()).cuda()
    torch.cuda.synchronize()
    e = ifx.ElasticFusion(**Q, max_surfels=200000)
    inst = ifx.InstanceFusion(e)

    def resident(p=good, ticket=-1, out=d_out.data_ptr(), floats=n, h=None):
        return L.ifx_detector_input((h or e).handle, ticket, None if p is None else C.byref(p), C.c_void_p(out), floats, None)

    def image(h, p=good, rgb=d_img.data_ptr(), out=d_out.data_ptr(), floats=n):
        return L.ifx_detector_input_image(h.handle, C.c_void_p(rgb), Q["w"], Q["h"], None if p is None else C.byref(p), C.c_void_p(out), floats, None)

    def works(h=None, through_image=False):
        d_out.zero_()
        torch.cuda.synchronize()
        assert (image(h or e) if through_image else resident(h=h)) == 0
        torch.cuda.synchronize()
        assert _equal(d_out.cpu().numpy().reshape(ref.shape), ref)

    assert resident() == E_STATE and b"no frame" in L.ifx_last_error(e.handle)          # no frame processed yet ...
    works(through_image=True)                                                          # ... which the stage call does not need
    for i in range(2):
        e.processFrame(st["rgb"][i], st["depth"][i])
    works()

    def bad(**kw2):
        p = ifx.detector_prep(**{**kw, **kw2})
        return p

    flags4 = ifx.detector_prep(**kw); flags4.flags = 4
    invalid = [("NULL parameters", lambda f: f(p=None)), ("NULL output", lambda f: f(out=None)), ("min_size < 1", lambda f: f(p=bad(min_size=0))),
               ("size_divisible < 0", lambda f: f(p=bad(size_divisible=-1))), ("unknown flag bits", lambda f: f(p=flags4)),
               ("a std entry of 0", lambda f: f(p=bad(std=(1.0, 1.0, 0.0)))), ("out_floats too small", lambda f: f(floats=n - 1)),
               ("scale above 8", lambda f: f(p=bad(min_size=14)))]                      # 120 / 14 = 8.57
    for what, call in invalid:
        assert call(resident) == E_INVALID, what
        works()
        assert call(lambda **k: image(e, **k)) == E_INVALID, what
        works(through_image=True)
    assert image(e, rgb=None) == E_INVALID
    works(through_image=True)
    assert resident(p=bad(min_size=15)) == 0                                            # exactly 8: accepted
    assert resident(ticket=12345) == E_INVALID                                          # unknown ticket
    works()
    t_plain, t_frame = inst.snapshot(), inst.snapshot(superpixels=True)
    assert resident(ticket=t_plain) == E_STATE and b"without its frame" in L.ifx_last_error(e.handle)
    works()
    assert resident(ticket=t_frame) == 0
    inst.release_snapshot(t_plain)
    assert resident(ticket=t_plain) == E_INVALID                                        # released ticket
    works()
    m = e.download()
    pose, tick = e.getCurrPose(), e.tick
    e.upload(m); e.set_pose(pose, tick)
    assert resident(ticket=t_frame) == E_STATE and b"uploaded" in L.ifx_last_error(e.handle)      # voided by ifx_map_upload
    works()
    inst.release_snapshot(t_frame)
    e.camera_count(2)
    assert resident() == E_STATE and b"camera" in L.ifx_last_error(e.handle)            # more than one camera context
    works(through_image=True)
    e.close()
    ef = ifx.ElasticFusion(**Q, max_surfels=200000, n_ranks=-1, rank=0)                 # a sharded handle: a world of one
    sharded.OwnerShardedElasticFusion(ef, None)
    assert resident(h=ef) == E_STATE and b"sharded" in L.ifx_last_error(ef.handle)
    assert resident(h=ef, ticket=0) == E_STATE
    works(h=ef, through_image=True)
    ef.close()
