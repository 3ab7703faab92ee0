"""The view-list walk's owner lookup (k_raster_view, instancefusion_amd/csrc/ifx_walk_owner.h) on hand-built maps.

A lane of the walk finds the record of its candidate pixel through a table, a max-scan and a carry; k_raster_list, the per-pass path's rasteriser (option
view_list 0), walks every box with its own lane and has no such search.  For each map the frame path through the view list -- id image on the sampled lattice
(lazy_ids 1: records of area 1-2, up to 64 box starts a step; the lattice test without a division) or whole (lazy_ids 0), clean pass inside the walk
(clean_raster 1, k_raster_view<false, true>) or in front of it (0, k_raster_view<false, false>) -- is held bit for bit to the per-pass path of the same library and
to the CPU oracle: the prediction images, the id image (the frame's own lattice pixels read as the frame left them, then the whole image, which a lazy handle
completes with one more walk of the same list), the surfel count and every map array, after each of three frames at a held pose.

Maps and the cases of tests/cpp/walk_owner_check.cpp they put on the GPU:
  one_pixel   every slot a disc inside one pixel: 64 box starts per step                                   "all ones"
  close_up    discs that cover the whole image (one box over 300 steps) among one-pixel discs              "one area among ones", "large boxes"
  culled_runs runs of 1, 63, 64, 65 entries the walk culls (below the confidence threshold; behind the     "empty run across a boundary", "single lane 0 / 63",
              camera) between drawn ones                                                                   "sum on a step boundary"
  id_only     stable surfels outside the time window (id-only records; lattice records under lazy_ids)     "random" (areas 0, 1, 2 and large mixed)
              interleaved with window surfels of several sizes
  short       a map shorter than one wave                                                                  "single lane 0", "one area alone"
With a wrong carry in the kernel (lane 0's mark instead of lane 63's leaving a step; tried once while developing, not kept) close_up, culled_runs and id_only
fail on every form -- a box that reaches over a step boundary is drawn with the wrong record -- while one_pixel passes (no box crosses a boundary), and
short fails only through its one large disc."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

W, H = 160, 120
K = dict(fx=132.0, fy=132.0, cx=80.0, cy=60.0)
TICK = 1000
MAP_KEYS = ("pc", "nr", "col", "tm", "ic", "votes")
FORMS = {   # name -> options of the view-list frame path
    "lattice+clean": dict(view_list=1, lazy_ids=1, clean_raster=1),
    "whole+clean": dict(view_list=1, lazy_ids=0, clean_raster=1),
    "lattice": dict(view_list=1, lazy_ids=1, clean_raster=0),
    "whole": dict(view_list=1, lazy_ids=0, clean_raster=0),
    "per_pass": dict(view_list=0, lazy_ids=0, clean_raster=0),
}


@pytest.fixture(scope="module")
def ifx():
    import instancefusion_amd as m

    m.lib()
    return m


@pytest.fixture(scope="module")
def frames():
    from instancefusion_amd import synth

    return synth.make_stream(4, W, H, K["fx"], K["fy"], K["cx"], K["cy"], noise=True)


def _surfels(px, py, z, r_px, conf, last, normal=(0.0, 0.0, -1.0)):
    """camera-frame surfels (the pose is the identity) centred on pixel centres (px + 0.5, py + 0.5) at depth z with a radius of r_px pixels, facing the camera"""
    px, py, z, r_px, conf, last = (np.broadcast_to(np.asarray(a, np.float64), np.shape(px)).copy() for a in (px, py, z, r_px, conf, last))
    n = px.size
    pc = np.stack([(px + 0.5 - K["cx"]) / K["fx"] * z, (py + 0.5 - K["cy"]) / K["fy"] * z, z, conf], 1)
    nr = np.concatenate([np.tile(np.asarray(normal, np.float64), (n, 1)), (r_px * np.abs(z) / K["fx"])[:, None]], 1)
    tm = np.stack([last - 5, last], 1)
    return pc, nr, tm


def _finish(parts, order=None):
    pc, nr, tm = (np.concatenate([p[k] for p in parts], 0) for k in range(3))
    if order is not None:
        pc, nr, tm = pc[order], nr[order], tm[order]
    n = pc.shape[0]
    col = np.stack([np.full(n, float((200 << 16) + (120 << 8) + 40)), np.zeros(n)], 1)
    return dict(pc=pc.astype(np.float32), nr=nr.astype(np.float32), col=col.astype(np.float32), tm=tm.astype(np.float32), ic=np.zeros((n, 4), np.float32),
                votes=np.zeros((n, 48), np.float32))


def _grid(step=1, x0=0, y0=0):
    ys, xs = np.mgrid[y0:H:step, x0:W:step]
    return xs.ravel().astype(np.float64), ys.ravel().astype(np.float64)


def map_one_pixel():
    xs, ys = _grid()
    return _finish([_surfels(xs, ys, 1.0 + 0.001 * ((xs * 7 + ys * 3) % 11), 0.3, 20.0, TICK - 1)])


def map_close_up():
    xs, ys = _grid(2)
    tiny = _surfels(xs, ys, 1.0, 0.3, 20.0, TICK - 1)
    # three discs over the whole image: behind the tiny ones, between, and a tilted one in front of part of them; first, in the middle and last of the slot order
    big = [_surfels([80.0], [60.0], [2.0], [140.0], [20.0], [TICK - 1]), _surfels([30.0], [100.0], [1.5], [120.0], [20.0], [TICK - 2]),
           _surfels([120.0], [20.0], [0.9], [60.0], [20.0], [TICK - 1], normal=(0.6, 0.0, -0.8))]
    n = xs.size
    order = np.concatenate([[n], np.arange(0, 2501), [n + 1], np.arange(2501, n), [n + 2]])
    return _finish([tiny] + big, order)


def map_culled_runs():
    # drawn, then a run the walk culls, then drawn, ...: run lengths 1, 63, 64, 65 in turn, the culled ones alternately below the confidence threshold (listed for the
    # clean pass, not drawn) and behind the camera; drawn discs of 1, 9 and ~80 pixels so that the box in front of a run ends before, on and behind a step boundary
    kinds, k = [], 0
    for rep in range(12):
        for run in (1, 63, 64, 65):
            kinds += [1 + (k % 3)] * (1 + k % 4) + [0 if (k % 2 == 0) else -1] * run
            k += 1
    kinds = np.asarray(kinds + [1, 2, 3])
    n = kinds.size
    i = np.arange(n)
    px, py = (i * 37) % W, (i * 11) % H
    r_px = np.where(kinds == 1, 0.3, np.where(kinds == 2, 1.4, 5.0))
    z = np.where(kinds == -1, -1.0, 1.0 + 0.01 * (i % 7))
    conf = np.where(kinds == 0, 5.0, 20.0)
    return _finish([_surfels(px.astype(np.float64), py.astype(np.float64), z, r_px, conf, TICK - 1)])


def map_id_only():
    rng = np.random.RandomState(5)
    n = 6000
    px, py = rng.randint(0, W, n).astype(np.float64), rng.randint(0, H, n).astype(np.float64)
    r_px = rng.choice([0.3, 0.3, 1.4, 6.0, 14.0, 30.0], n)
    old = rng.uniform(size=n) < 0.5                       # last seen 300 frames ago: outside the time window of 200, id render only
    conf = np.where(rng.uniform(size=n) < 0.2, 5.0, 20.0)
    conf = np.where(old, 20.0, conf)
    return _finish([_surfels(px, py, 1.0 + rng.uniform(0, 1, n), r_px, conf, np.where(old, TICK - 300.0, TICK - 1.0))])


def map_short():
    return _finish([_surfels([10.0, 11.0, 80.0, 150.0, 3.0], [10.0, 10.0, 60.0, 110.0, 118.0], [1.0, 1.0, 1.2, 1.0, 1.0], [0.3, 0.3, 50.0, 1.4, 0.3], [20.0, 5.0, 20.0, 20.0, 20.0],
                              [TICK - 1, TICK - 1, TICK - 1, TICK - 300, TICK - 1])])


MAPS = dict(one_pixel=map_one_pixel, close_up=map_close_up, culled_runs=map_culled_runs, id_only=map_id_only, short=map_short)


def _raw_ids(hip, ifx, e, d_ids):
    """the id image as the frame left it (no completion): on a lazy handle only the lattice pixels are the frame's"""
    e.sync()
    a = np.zeros((H, W), np.int32)
    assert hip.hipMemcpy(a.ctypes.data, d_ids, a.nbytes, 2) == 0
    return a


@pytest.mark.parametrize("name", list(MAPS))
def test_view_list_walk_equals_per_pass_path_and_oracle(ifx, orc, frames, name):
    hip = C.CDLL("libamdhip64.so")
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    st, m = frames, MAPS[name]()
    pose = np.eye(4, dtype=np.float32)
    efs = {k: ifx.ElasticFusion(w=W, h=H, max_surfels=200000, **K) for k in FORMS}
    o = orc.Oracle(w=W, h=H, max_surfels=200000, **K)
    try:
        d_ids = {}
        for k, e in efs.items():
            for opt, v in FORMS[k].items():
                e.set_option(opt, v)
            e.processFrame(st["rgb"][0], st["depth"][0])       # as bench.py brings its map in: a first frame, the map, the pose and clock, one prediction
            e.upload(m); e.set_pose(pose, TICK); e.combined_predict(pose, TICK, TICK)
            d_ids[k] = ifx.lib().ifx_ids_after(e.handle)
        o.process_frame(st["rgb"][0], st["depth"][0])
        o.upload(m); o.set_pose(pose, TICK); o.combined_predict(pose, TICK, TICK)
        drawn = 0
        for i in (1, 2, 3):
            for e in efs.values():
                e.processFrame(st["rgb"][i], st["depth"][i], inPose=pose)
            o.process_frame(st["rgb"][i], st["depth"][i], in_pose=pose)
            same_slots = all(e.slots == e.count for e in efs.values())   # no tombstone yet: the id images name the rows of the oracle's map
            want_ids = o.image("ids_after")
            for k, e in efs.items():
                if FORMS[k]["lazy_ids"] and FORMS[k]["view_list"]:
                    raw = _raw_ids(hip, ifx, e, d_ids[k])
                    assert np.array_equal(raw[::10, ::10], _raw_ids(hip, ifx, efs["per_pass"], d_ids["per_pass"])[::10, ::10]), (name, i, k, "lattice vs per-pass")
                    if same_slots:
                        assert np.array_equal(raw[::10, ::10], want_ids[::10, ::10]), (name, i, k, "lattice vs oracle")
            ids = {k: e.image("ids_after") for k, e in efs.items()}
            for k, e in efs.items():
                assert e.count == o.count == efs["per_pass"].count, (name, i, k, e.count, o.count)
                for img in ("pred_vertex", "pred_normal", "pred_image"):
                    got = e.image(img)
                    assert np.array_equal(got, efs["per_pass"].image(img)), (name, i, k, img, "vs per-pass")
                    assert np.array_equal(got, o.image(img)), (name, i, k, img, "vs oracle")
                assert np.array_equal(ids[k], ids["per_pass"]), (name, i, k, "ids vs per-pass", int((ids[k] != ids["per_pass"]).sum()))
                if same_slots:
                    assert np.array_equal(ids[k], want_ids), (name, i, k, "ids vs oracle", int((ids[k] != want_ids).sum()))
            drawn += int((want_ids > 0).sum())
            mo = o.download()
            for k, e in efs.items():
                mg = e.download()
                for key in MAP_KEYS:
                    assert np.array_equal(mg[key], mo[key]), (name, i, k, key)
        assert drawn > 0, name
        vs = efs["lattice+clean"].view_list_stats()
        assert vs["scans"] >= 1, vs                            # the frames really took the view list
    finally:
        for e in efs.values():
            e.close()
        o.close()
