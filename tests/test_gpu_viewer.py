"""ifx_render_view on the GPU (ifx_map.hip k_view_quad / k_view_big / k_view_resolve): the viewer's surfel pass from any camera.

Every case asks for array equality with tests/viewer_numpy.py -- ids as integers, rgba bit for bit.  Maps are uploaded (ifx_map_upload: a slot is a row of the
uploaded map); no frames run unless stated.  The share of the golden scenes equal to GL itself is then tests/test_viewer_rule_cpu.py's, by transitivity."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT, SMALL
import viewer_numpy as V

pytestmark = pytest.mark.gpu

GOLD = os.path.join(ROOT, "tests", "golden", "gl_viewer_scenes.npz")
REPLAY = os.path.join(ROOT, "instancefusion_amd", "ifx_replay")
FRAME = dict(w=160, h=120, fx=132.0, fy=132.0, cx=80.0, cy=60.0)      # the handles' frame size: unrelated to any viewport below
THR = 3.0


@pytest.fixture(scope="module")
def ifx():
    import instancefusion_amd as m

    m.lib()
    return m


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(GOLD))


@pytest.fixture(scope="module")
def handle(ifx):
    e = ifx.ElasticFusion(**FRAME, max_surfels=1 << 16, confidence=THR)
    yield e
    e.close()


def full_map(m):
    n = m["pc"].shape[0]
    out = {k: np.ascontiguousarray(m[k], np.float32) for k in ("pc", "nr", "col", "tm")}
    out["ic"] = np.zeros((n, 4), np.float32)
    out["votes"] = np.zeros((n, 48), np.float32)
    return out


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def check(e, m, mvp, size, what, threshold=THR, color_type=0, unstable=0, draw_window=0, time=17, time_delta=200, clear_rgb=(1.0, 1.0, 1.0), upload=True):
    """upload, draw on the GPU and with the numpy rule, ask for equal arrays; returns (rgba, ids, big quads on the GPU)"""
    if upload:
        e.upload(full_map(m))
    w, h = size
    info = {}
    want_rgba, want_ids = V.render_view(m, mvp, w, h, threshold, color_type, unstable, draw_window, time, time_delta, clear_rgb=clear_rgb, info=info)
    rgba, ids = e.render_view(mvp, size, color_type=color_type, threshold=threshold, unstable=unstable, draw_window=draw_window, time=time, time_delta=time_delta, clear_rgb=clear_rgb)
    big = e.L.ifx_render_view_big_quads(e.handle)
    assert ids.shape == (h, w) and rgba.shape == (h, w, 4)
    assert np.array_equal(ids, want_ids), (what, int((ids != want_ids).sum()))
    assert np.array_equal(bits(rgba), bits(want_rgba)), (what, int((bits(rgba) != bits(want_rgba)).any(-1).sum()))
    assert big == info["big"], (what, big, info["big"])
    return rgba, ids, big


# ------------------------------------------------------------------ the golden scenes
def test_golden_scenes_equal_the_rule(handle, gold):
    m = {k: gold[k] for k in ("pc", "nr", "col", "tm")}
    w, h = (int(v) for v in gold["size"])
    handle.upload(full_map(m))
    for name in gold["scenes"]:
        ct, unstable, window, t, tdelta = (int(v) for v in gold[f"{name}__flags"])
        rgba, ids, big = check(handle, m, gold[f"{name}__mvp"], (w, h), str(name), float(gold[f"{name}__threshold"]), ct, unstable, window, t, tdelta, clear_rgb=(0, 0, 0), upload=False)
        gl = gold[f"{name}__gl_ids"]
        print(f"{name}: {float((ids == gl).mean() * 100):.3f} % of the pixels equal to GL, {big} quads drawn by a workgroup each")
        assert (ids >= 0).sum() > 4000
    assert big > 0      # camera (c): the big-quad path carried part of the image


def test_viewports_unrelated_to_the_frame(handle, gold):
    """61x37, 1x1, 257x3 on a 160x120 handle; after a 640x480 call (the key image regrows; the close camera fills it) 61x37 again: no stale keys"""
    m = {k: gold[k] for k in ("pc", "nr", "col", "tm")}
    handle.upload(full_map(m))
    mvp = gold["c_close__mvp"]
    first = None
    for size in ((61, 37), (1, 1), (257, 3), (640, 480), (61, 37)):
        rgba, ids, _ = check(handle, m, mvp, size, f"viewport {size}", color_type=4, upload=False)
        if size == (61, 37):
            if first is None:
                first = (rgba, ids)
            else:
                assert np.array_equal(ids, first[1]) and np.array_equal(bits(rgba), bits(first[0]))
    check(handle, m, gold["a_type0__mvp"], (640, 480), "tracked pose at 640x480", color_type=2, upload=False)


# ------------------------------------------------------------------ hand-made maps
def cam(near=0.1, far=1000.0, w=64, h=48, f=60.0, fy=None):
    import instancefusion_amd as ifx
    return ifx.viewer_mvp(f, f if fy is None else fy, w / 2.0, h / 2.0, w, h, near, far, np.eye(4))


def surfels(rows):
    """rows: (x, y, z, confidence, nx, ny, nz, radius, colour word, instance word, init time, last time)"""
    a = np.array(rows, np.float32).reshape(-1, 12)
    return dict(pc=a[:, 0:4].copy(), nr=a[:, 4:8].copy(), col=a[:, 8:10].copy(), tm=a[:, 10:12].copy())


def rgbw(r, g, b):
    return float((r << 16) | (g << 8) | b)


FACING = (0.0, 0.0, -1.0)


def test_one_quad_covers_the_viewport(handle):
    m = surfels([(0, 0, 0.5, 10, *FACING, 1.0, rgbw(200, 10, 10), rgbw(1, 2, 3), 1, 1)])
    _, ids, big = check(handle, m, cam(), (64, 48), "whole viewport", color_type=2)
    assert big == 1 and np.all(ids == 0)


@pytest.mark.parametrize("pixels", [256, 257])
def test_hand_over_between_the_two_paths(handle, pixels):
    """A box of exactly 256 pixels is drawn by its thread, one of 257 by a workgroup.  257 is prime: the box is one row of a 320x8 viewport under a camera
    whose vertical focal length is tiny (the MVP is any 4x4)."""
    w, h = 320, 8
    mvp = cam(w=w, h=h, f=100.0, fy=0.25)
    found = None
    for off in (0.0, 0.005):
        for r in np.linspace(0.88, 0.93, 501):
            m = surfels([(off, 2.0, 1.0, 10, *FACING, r, rgbw(0, 200, 0), rgbw(9, 9, 9), 1, 1)])      # fy * y / z = 0.5: the centre of a pixel row
            ok, _, _, _, _, (x0, x1, y0, y1), _ = V.view_setup(m["pc"], m["nr"], m["col"], mvp, w, h, THR, 0)
            if ok[0] and y0[0] == y1[0] and x1[0] - x0[0] + 1 == pixels:
                found = m
                break
        if found is not None:
            break
    assert found is not None
    _, ids, big = check(handle, found, mvp, (w, h), f"box of {pixels}", color_type=2)
    assert big == (1 if pixels > 256 else 0)
    assert (ids == 0).sum() > 150      # the disc inside the quad: 2 r f px of the row


@pytest.mark.parametrize("order", [(0, 1), (1, 0)])
def test_tie_goes_to_the_lower_slot(handle, order):
    rows = [(0, 0, 1.0, 10, *FACING, 0.1, rgbw(255, 0, 0), rgbw(1, 1, 1), 1, 1), (0, 0, 1.0, 10, *FACING, 0.1, rgbw(0, 0, 255), rgbw(2, 2, 2), 1, 1)]
    m = surfels([rows[order[0]], rows[order[1]]])
    rgba, ids, _ = check(handle, m, cam(), (64, 48), f"tie {order}", color_type=2)
    assert (ids == 0).sum() > 50 and not (ids == 1).any()
    assert (rgba[ids == 0][0, 0] > rgba[ids == 0][0, 2]) == (order[0] == 0)      # the colour is the first uploaded surfel's


@pytest.mark.parametrize("small_z", [1.0, 3.0])
def test_small_and_big_quads_meet_in_the_key_image(handle, small_z):
    m = surfels([(0, 0, 2.0, 10, *FACING, 2.0, rgbw(10, 200, 10), rgbw(1, 1, 1), 1, 1), (0.05, 0.02, small_z, 10, *FACING, 0.04 * small_z, rgbw(200, 10, 10), rgbw(2, 2, 2), 1, 1)])
    _, ids, big = check(handle, m, cam(), (64, 48), f"small quad at {small_z}", color_type=2)
    assert big == 1 and ((ids == 1).sum() > 5) == (small_z < 2.0) and (ids == 0).sum() > 2000


def edge_on_row(z, r=0.25):
    return (0.3, 0.0, z, 10, 1.0, 0.0, 0.0, r, rgbw(5, 5, 200), rgbw(3, 3, 3), 1, 1)      # normal along x: the corners -x / +x lie at z -+ about r


def test_corner_at_w_zero_and_behind(handle):
    """normal (1, 0, 0): x = (0, -1, 1) / sqrt 2 * r * 1.41421356, so corner p - x has w = p.z - x.z: exactly 0, one ulp behind, one ulp in front"""
    f32 = np.float32
    with np.errstate(all="ignore"):
        az = ((f32(1.0) * (f32(1.0) / np.sqrt(f32(2.0)))) * f32(0.25)) * f32(1.41421356)
    for z in (az, np.nextafter(az, f32(0)), np.nextafter(az, f32(1))):
        m = surfels([edge_on_row(float(z)), (-0.2, 0.1, 1.0, 10, *FACING, 0.1, rgbw(1, 200, 1), rgbw(4, 4, 4), 1, 1)])
        assert m["pc"][0, 2] == z
        _, ids, _ = check(handle, m, cam(), (64, 48), f"corner w at {z!r}", color_type=2)
        assert not (ids == 0).any() and (ids == 1).any()      # at or behind w = 0: not drawn; one ulp in front: far outside the guard band


def test_far_and_near_planes(handle):
    m = surfels([(0, 0, 20.0, 10, *FACING, 2.0, rgbw(200, 0, 0), rgbw(1, 1, 1), 1, 1),                 # wholly beyond far = 10
                 (-0.03, 0.0, 0.1, 10, 0.0, 0.6, -0.8, 0.02, rgbw(0, 200, 0), rgbw(2, 2, 2), 1, 1),     # tilted about x: straddles near = 0.1, every corner at w > 0
                 (0.5, 0.3, 5.0, 10, *FACING, 0.3, rgbw(0, 0, 200), rgbw(3, 3, 3), 1, 1)])
    _, ids, _ = check(handle, m, cam(near=0.1, far=10.0), (64, 48), "near and far", color_type=2)
    assert not (ids == 0).any() and (ids == 1).any() and (ids == 2).any()
    # the straddling quad is cut by the depth clip: fewer pixels than under a near plane in front of it
    _, ids2, _ = check(handle, m, cam(near=0.01, far=10.0), (64, 48), "near plane pulled in", color_type=2, upload=False)
    assert (ids2 == 1).sum() > (ids == 1).sum()


def test_degenerate_surfels(handle):
    m = surfels([(0, 0, 1.0, 10, 0.0, 0.0, 0.0, 0.1, rgbw(200, 0, 0), rgbw(1, 1, 1), 1, 1),           # zero normal: NaN axes
                 (0.2, 0, 1.0, 10, *FACING, 0.0, rgbw(0, 200, 0), rgbw(2, 2, 2), 1, 1),               # radius 0
                 (-0.2, 0, 1.0, 10, *FACING, 0.1, rgbw(0, 0, 200), -1.0, 1, 1),                       # instance colour -1
                 (0, 0.2, 1.0, 10, 0.0, 0.0, 1.0, 0.1, rgbw(200, 200, 0), rgbw(4, 4, 4), 1, 1),       # back-facing: drawn (nothing enables face culling)
                 (0, -0.2, 1.0, 1.0, *FACING, 0.05, rgbw(0, 200, 200), rgbw(5, 5, 5), 1, 1)])         # unstable: drawn only with unstable = 1 (zw 0.90 + radius < 1)
    _, ids, _ = check(handle, m, cam(), (64, 48), "degenerate", color_type=2)
    assert set(np.unique(ids)) == {-1, 3}
    _, ids, _ = check(handle, m, cam(), (64, 48), "degenerate, unstable = 1", color_type=4, unstable=1, upload=False)
    assert set(np.unique(ids)) == {-1, 3, 4}


def test_unstable_surfel_is_pushed_back_by_its_radius(handle):
    m = surfels([(0, 0, 1.0, 10, *FACING, 0.1, rgbw(200, 0, 0), rgbw(1, 1, 1), 1, 1), (0, 0, 0.99, 1.0, *FACING, 0.05, rgbw(0, 200, 0), rgbw(2, 2, 2), 1, 1)])
    _, ids, _ = check(handle, m, cam(), (64, 48), "unstable in front", color_type=2, unstable=1)
    assert (ids == 0).any() and not (ids == 1).any()      # in front by less than its radius: behind after the push
    _, ids, _ = check(handle, m, cam(), (64, 48), "both stable", threshold=0.5, color_type=2, upload=False)
    assert (ids == 1).any()


def test_time_ramp_divides_by_zero_at_time_one(handle):
    m = surfels([(-0.2, 0, 1.0, 10, *FACING, 0.1, 0, rgbw(1, 1, 1), 1, 1), (0.2, 0, 1.0, 10, *FACING, 0.1, 0, rgbw(2, 2, 2), 3, 3), (0, 0.25, 1.0, 10, *FACING, 0.1, 0, rgbw(2, 2, 2), 0, 0)])
    rgba, ids, _ = check(handle, m, cam(), (64, 48), "ramp at time 1", color_type=3, time=1)
    assert (ids == 0).any() and (ids == 1).any() and (ids == 2).any()
    for t in (2, 17):
        check(handle, m, cam(), (64, 48), f"ramp at time {t}", color_type=3, time=t, draw_window=1, time_delta=1, upload=False)


def test_sixty_four_random_surfels_every_flag(handle):
    rs = np.random.default_rng(5)
    n = 64
    nrm = rs.normal(size=(n, 3)); nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    m = dict(pc=np.c_[rs.uniform(-1, 1, n), rs.uniform(-0.7, 0.7, n), rs.uniform(0.05, 4.0, n), rs.choice([1.0, 10.0], n)].astype(np.float32),
             nr=np.c_[nrm, rs.uniform(0.01, 0.4, n)].astype(np.float32),
             col=np.c_[rs.integers(0, 1 << 24, n), np.where(rs.random(n) < 0.8, rs.integers(0, 1 << 24, n), -1)].astype(np.float32),
             tm=np.c_[rs.integers(1, 17, n), rs.integers(1, 17, n)].astype(np.float32))
    handle.upload(full_map(m))
    seen_big = 0
    for ct in range(5):
        for unstable in (0, 1):
            _, ids, big = check(handle, m, cam(), (64, 48), f"random type {ct} unstable {unstable}", color_type=ct, unstable=unstable, draw_window=ct % 2, time=17, time_delta=5, upload=False)
            seen_big += big
            assert len(np.unique(ids)) > 8
    assert seen_big > 0


# ------------------------------------------------------------------ the call itself
def test_empty_map(ifx):
    e = ifx.ElasticFusion(**FRAME, max_surfels=1 << 12)
    try:
        rgba, ids = e.render_view(cam(), (64, 48), clear_rgb=(0.25, 0.5, 0.75))
        assert np.all(ids == -1)
        assert np.array_equal(rgba, np.broadcast_to(np.array([0.25, 0.5, 0.75, 0.0], np.float32), (48, 64, 4)))
        assert e.L.ifx_render_view_big_quads(e.handle) == 0
    finally:
        e.close()


def test_device_outputs_equal_host_outputs(handle, gold):
    import torch

    m = {k: gold[k] for k in ("pc", "nr", "col", "tm")}
    handle.upload(full_map(m))
    kw = dict(color_type=4, threshold=THR, time=17, time_delta=200)
    rgba, ids = handle.render_view(gold["c_close__mvp"], (160, 120), **kw)
    d_rgba, d_ids = handle.render_view(gold["c_close__mvp"], (160, 120), device=True, **kw)
    assert d_rgba.is_cuda and d_ids.dtype == torch.int32
    assert np.array_equal(d_ids.cpu().numpy(), ids) and np.array_equal(bits(d_rgba.cpu().numpy()), bits(rgba))
    # host and device outputs of one call; either image alone
    p = ifx_params(handle, gold["c_close__mvp"], 160, 120, color_type=4)
    h_rgba, h_ids = np.zeros((120, 160, 4), np.float32), np.zeros((120, 160), np.int32)
    t_rgba, t_ids = torch.zeros((120, 160, 4), dtype=torch.float32, device="cuda"), torch.zeros((120, 160), dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    assert handle.L.ifx_render_view(handle.handle, C.byref(p), h_rgba.ctypes.data_as(C.c_void_p), None, None, C.c_void_p(t_ids.data_ptr())) == 0
    handle.sync()
    assert np.array_equal(bits(h_rgba), bits(rgba)) and np.array_equal(t_ids.cpu().numpy(), ids)
    assert handle.L.ifx_render_view(handle.handle, C.byref(p), None, h_ids.ctypes.data_as(C.c_void_p), C.c_void_p(t_rgba.data_ptr()), None) == 0
    handle.sync()
    assert np.array_equal(h_ids, ids) and np.array_equal(bits(t_rgba.cpu().numpy()), bits(rgba))
    assert handle.L.ifx_render_view(handle.handle, C.byref(p), None, None, None, None) == 0


def ifx_params(e, mvp, w, h, color_type=0, threshold=THR):
    import instancefusion_amd as ifx

    p = ifx.ViewParams()
    p.mvp[:] = [float(v) for v in np.asarray(mvp, np.float32).reshape(16)]
    p.w, p.h, p.threshold, p.color_type, p.unstable, p.draw_window, p.time, p.time_delta = w, h, threshold, color_type, 0, 0, 17, 200
    p.clear_rgb[:] = [1.0, 1.0, 1.0]
    return p


def test_refusals_write_nothing(ifx, handle):
    handle.upload(full_map(surfels([(0, 0, 0.5, 10, *FACING, 1.0, rgbw(200, 10, 10), rgbw(1, 2, 3), 1, 1)])))
    rgba, ids = np.full((48, 64, 4), 7.0, np.float32), np.full((48, 64), 7, np.int32)

    def call(e, p):
        return e.L.ifx_render_view(e.handle, C.byref(p), rgba.ctypes.data_as(C.c_void_p), ids.ctypes.data_as(C.c_void_p), None, None)

    bad = []
    for w, h in ((0, 48), (64, 0), (4097, 48), (64, 4097), (-1, 48)):
        bad.append(ifx_params(handle, cam(), w, h))
    for ct in (-1, 5):
        bad.append(ifx_params(handle, cam(), 64, 48, color_type=ct))
    for v in (float("nan"), float("inf")):
        mvp = cam().copy(); mvp[2, 1] = v
        bad.append(ifx_params(handle, mvp, 64, 48))
    for p in bad:
        assert call(handle, p) == -1      # IFX_E_INVALID
        assert np.all(rgba == 7.0) and np.all(ids == 7)
    good = ifx_params(handle, cam(), 64, 48)
    s = ifx.ElasticFusion(**SMALL, max_surfels=100000, n_ranks=-1, rank=0)
    try:
        assert call(s, good) == -4        # IFX_E_STATE: a sharded handle
        assert np.all(rgba == 7.0) and np.all(ids == 7)
        with pytest.raises(ifx.IfxError, match=r"\(-4\)"):
            s.render_view(cam(), (64, 48))
    finally:
        s.close()
    assert call(handle, good) == 0 and np.all(ids == 0)
    # NaN threshold, time < 0, time_delta < 0: the handle's own values
    p = ifx_params(handle, cam(), 64, 48, threshold=float("nan"))
    p.time, p.time_delta = -1, -1
    assert call(handle, p) == 0 and np.all(ids == 0)      # confidence 10 > the handle's 3


def test_read_only_between_frames(ifx):
    """20 frames on two handles; one draws a view between frame 10 and frame 11: poses, map, ids_after and labels stay bit-identical"""
    from instancefusion_amd import synth

    nf = 20
    st = synth.make_stream(nf, FRAME["w"], FRAME["h"], FRAME["fx"], FRAME["fy"], FRAME["cx"], FRAME["cy"], noise=True)
    a, b = (ifx.ElasticFusion(**FRAME, max_surfels=200000, confidence=THR) for _ in range(2))
    try:
        ia, ib = ifx.InstanceFusion(a), ifx.InstanceFusion(b)
        calls = 0
        for i in range(nf):
            pa, pb = a.processFrame(st["rgb"][i], st["depth"][i]), b.processFrame(st["rgb"][i], st["depth"][i])
            assert np.array_equal(pa, pb), i
            if i >= 4 and i % 3 == 1:
                masks, cls = synth.canned_masks(st["obj"][i], st["scene"])
                ia.ProcessSegmentation(st["rgb"][i], st["depth"][i], masks, cls, i)
                ib.ProcessSegmentation(st["rgb"][i], st["depth"][i], masks, cls, i)
                calls += 1
            if i == 9:
                mvp = ifx.viewer_mvp(105.0, 105.0, 80.0, 60.0, 160, 120, 0.1, 1000.0, pa)
                rgba, ids = a.render_view(mvp, (200, 150), draw_instances=True, unstable=True, draw_window=True)
                assert (ids >= 0).sum() > 5000
                rgba2, ids2 = a.render_view(mvp, (200, 150), draw_instances=True, unstable=True, draw_window=True)      # the call after it gives the same result
                assert np.array_equal(ids, ids2) and np.array_equal(bits(rgba), bits(rgba2))
        assert calls >= 4
        assert np.array_equal(a.image("ids_after"), b.image("ids_after"))
        assert np.array_equal(ia.labels(), ib.labels())
        ma, mb = a.download(), b.download()
        for k in ma:
            assert np.array_equal(bits(ma[k]), bits(mb[k])), k
        assert ma["pc"].shape[0] > 5000
        # the live map through the rule: slots are the downloaded map's rows once compacted
        mvp = ifx.viewer_mvp(105.0, 105.0, 80.0, 60.0, 160, 120, 0.1, 1000.0, a.getCurrPose())
        rgba, ids = a.render_view(mvp, (160, 120), color_type=2)
        want_rgba, want_ids = V.render_view(ma, mvp, 160, 120, THR, 2, 0, 0, a.tick, 200)
        assert np.array_equal(ids, want_ids) and np.array_equal(bits(rgba), bits(want_rgba))
    finally:
        a.close(); b.close()


def test_replay_view_ppm_equals_python(small_stream, tmp_path):
    """ifx_replay --view-ppm (ElasticFusionInterface::RenderMapToBuffer, viewerMvp) against tools/run_log.py --view-ppm (ElasticFusion.render_view, viewer_mvp)
    over the same .klg: the same bytes, from the default camera and from a given one"""
    import importlib.util

    from instancefusion_amd import logio

    st = small_stream
    klg = str(tmp_path / "s.klg")
    wr = logio.RawLogWriter(klg, depth="zlib", image="jpeg", jpeg_quality=95)
    for i in range(8):
        wr.add(33333 * i, st["rgb"][i], st["depth"][i])
    wr.close()
    common = ["--width", str(SMALL["w"]), "--height", str(SMALL["h"]), "--fx", str(SMALL["fx"]), "--fy", str(SMALL["fy"]), "--cx", str(SMALL["cx"]),
              "--cy", str(SMALL["cy"]), "--max-surfels", "400000", "--confidence", "2", "--no-close-loops"]
    spec = importlib.util.spec_from_file_location("run_log", os.path.join(ROOT, "tools", "run_log.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    views = {"gui": ["--view-size", "160x120"],
             "posed": ["--view-size", "200x90", "--view-instances", "--view-pose", "0.8660254 0 0.5 -0.4 0 1 0 0.05 -0.5 0 0.8660254 -0.6 0 0 0 1"]}
    for name, extra in views.items():
        out_c, out_p = str(tmp_path / f"C_{name}"), str(tmp_path / f"P_{name}")
        r = subprocess.run([REPLAY, klg] + common + ["--out", out_c, "--view-ppm", out_c + ".ppm"] + extra, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr
        assert mod.main([klg] + common + ["--out", out_p, "--view-ppm", out_p + ".ppm"] + extra) == 0
        c, p = open(out_c + ".ppm", "rb").read(), open(out_p + ".ppm", "rb").read()
        w, h = (int(v) for v in extra[1].split("x"))
        head = f"P6\n{w} {h}\n255\n".encode()
        assert c.startswith(head) and len(c) == len(head) + w * h * 3
        assert c == p, name
        img = np.frombuffer(c[len(head):], np.uint8).reshape(h, w, 3)
        drawn = (img != 255).any(-1)
        assert drawn.sum() > w * h // 10 and not drawn.all()      # the map is in view, on the GUI's white
