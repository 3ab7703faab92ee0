"""The default detector's input on the GPU (ifx_detector_input_molded / ifx_detector_input_molded_image): bit for bit against the numpy statement
(tests/molded_input_numpy.py, itself held against the reference's utils.resize_image in tests/test_unmold_cpu.py) -- both pad axes, downscale, upscale and no
resize, both layouts; the resident frame against the image entry; and one round trip: the window it returns feeds unmold_detections."""
import ctypes as C

import numpy as np
import pytest

import molded_input_numpy as mi
import unmold_numpy as un

pytestmark = pytest.mark.gpu

Q = dict(w=160, h=120, fx=132.0, fy=132.0, cx=80.0, cy=60.0)
DIMS = [(128, 128), (200, 256), (0, 160), (100, 101)]                # 0.8 down, 1.6 up, s == 1, and an odd S whose top pad is no multiple of anything


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


def _image(w, h):
    rng = np.random.default_rng(w * 1000 + h)
    img = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    img[: h // 4] = 255
    img[h // 4: h // 3] = 0
    return img


def _bits(a):
    return np.ascontiguousarray(a).view(np.int32)


@pytest.mark.parametrize("dims", DIMS, ids=lambda d: f"{d[0]}-{d[1]}")
def test_image_entry_equals_the_statement(ifx, stage_handle, dims):
    """160 x 120 (pad above and below) and 120 x 160 (pad left and right), channels last and first, the default mean and one with a zero and a negative entry"""
    import torch

    mn, mx = dims
    for (w, h) in ((160, 120), (120, 160), (100, 76)):
        img = _image(w, h)
        d_img = torch.from_numpy(img).cuda()
        for mean in (mi.MEAN_PIXEL, (0.0, -7.25, 300.5)):
            for last in (True, False):
                ref, window = mi.molded_input(img, mn, mx, mean, channels_last=last)
                t, win, scale = ifx.detector_input_molded_image(stage_handle, d_img, mn, mx, mean=mean, channels_last=last)
                torch.cuda.synchronize()
                got = t.cpu().numpy()[0]
                assert win == window and got.shape == ref.shape and got.dtype == np.float32
                assert np.array_equal(_bits(got), _bits(ref)), (w, h, mn, mx, mean, last, int((_bits(got) != _bits(ref)).sum()))
    if dims == (128, 128):
        assert win == (15, 0, 112, 128) and abs(scale - 1.28) < 1e-12          # 100 x 76: 128 x 97, (128 - 97) // 2 = 15
    # an output tensor to reuse, its guard bands untouched
    buf = torch.full((3 * mx * mx + 64,), 7.0, device="cuda")
    out = buf[32:32 + 3 * mx * mx].view(1, mx, mx, 3)
    t, _, _ = ifx.detector_input_molded_image(stage_handle, torch.from_numpy(_image(160, 120)).cuda(), mn, mx, out=out)
    torch.cuda.synchronize()
    assert t.data_ptr() == out.data_ptr() and (buf[:32] == 7.0).all() and (buf[-32:] == 7.0).all()
    assert np.array_equal(_bits(t.cpu().numpy()[0]), _bits(mi.molded_input(_image(160, 120), mn, mx)[0]))


def test_resident_frame_equals_the_image_entry_and_the_round_trip(ifx):
    """After two frames the resident-frame entry gives what the image entry gives on that frame (and the statement); its window feeds unmold_detections, whose
    boxes come back in frame pixels; refusals leave the handle usable."""
    import torch

    from instancefusion_amd import synth

    st = synth.make_stream(2, Q["w"], Q["h"], Q["fx"], Q["fy"], Q["cx"], Q["cy"], noise=True)
    e = ifx.ElasticFusion(**Q, max_surfels=200000)
    inst = ifx.InstanceFusion(e)
    L = ifx.lib()
    try:
        mean3 = (C.c_double * 3)(*mi.MEAN_PIXEL)
        out = torch.zeros((1, 128, 128, 3), device="cuda")
        assert L.ifx_detector_input_molded(e.handle, -1, 128, 128, mean3, 0, C.c_void_p(out.data_ptr()), int(out.numel()), None) == -4      # no frame yet
        assert L.ifx_last_error(e.handle).startswith(b"ifx_detector_input_molded")
        for i in range(2):
            e.processFrame(st["rgb"][i], st["depth"][i])
        assert inst.molded_input_size(128, 128) == (128, 96, 128, 128, 16, 0, 112, 128)
        for last in (True, False):
            t, window, scale = inst.detector_input_molded(min_dim=128, max_dim=128, channels_last=last)
            t2, window2, _ = ifx.detector_input_molded_image(e, torch.from_numpy(st["rgb"][1]).cuda(), 128, 128, channels_last=last)
            torch.cuda.synchronize()
            assert window == window2 == (16, 0, 112, 128) and scale == 0.8
            assert torch.equal(t.view(torch.int32), t2.view(torch.int32))
            assert np.array_equal(_bits(t.cpu().numpy()[0]), _bits(mi.molded_input(st["rgb"][1], 128, 128, channels_last=last)[0]))
        for bad in ((-1, 128, 128, None, 0, out), (-1, 128, 128, mean3, 2, out), (-1, 128, 0, mean3, 0, out), (-1, 0, 19, mean3, 0, out), (-1, 200, 256, mean3, 0, out)):
            tk, mn, mx, mp, lay, o = bad
            assert L.ifx_detector_input_molded(e.handle, tk, mn, mx, mp, lay, C.c_void_p(o.data_ptr()), int(o.numel()), None) == -1, bad[:5]
            assert L.ifx_last_error(e.handle).startswith(b"ifx_detector_input_molded"), bad[:5]
        assert L.ifx_detector_input_molded_image(e.handle, None, 160, 120, 128, 128, mean3, 0, C.c_void_p(out.data_ptr()), int(out.numel()), None) == -1
        # the round trip: a detection drawn in the molded image comes back in frame pixels
        det = np.zeros((3, 6), np.float32)
        det[0] = (16 + 0.8 * 30 + 0.2, 0.8 * 40 + 0.2, 16 + 0.8 * 90 + 0.2, 0.8 * 100 + 0.2, 1, 0.9)
        masks = np.random.default_rng(7).random((3, 28, 28, 3)).astype(np.float32)
        g = e.unmold_detections(torch.from_numpy(det).cuda(), torch.from_numpy(masks).cuda(), window, (Q["w"], Q["h"]))
        w = un.unmold_detections(det, masks, window, Q["w"], Q["h"])
        assert g[2].cpu().numpy().tolist() == [[30, 40, 90, 100]] and np.array_equal(g[0].cpu().numpy(), w[0][:1]) and w[5] == 1
        t, _, _ = inst.detector_input_molded(min_dim=128, max_dim=128)                  # still usable
        torch.cuda.synchronize()
        assert np.array_equal(_bits(t.cpu().numpy()[0]), _bits(mi.molded_input(st["rgb"][1], 128, 128)[0]))
    finally:
        e.close()
