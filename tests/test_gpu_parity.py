"""GPU parity tests: the HIP path (libifx.so through its C-ABI) against the CPU oracle on identical
seeded inputs.  Integer / index / byte outputs must match exactly; float outputs computed by the
same per-element formula must match exactly too (both sides are built without FMA contraction and
share the deterministic expf); the tracker's reductions are exact, order-independent sums on both sides, so the
29 / 11 floats of the normal equations, the poses (conftest.assert_pose_equal: bit-equal, at most one f32 ulp where the
6x6 solve's pivoting differs), the map sizes, the id images and the labels are compared for EQUALITY over whole runs."""
import ctypes as C

import os

import numpy as np
import pytest

from conftest import SMALL, assert_pose_equal
from gputest_protocol import HALF_K, protocol_inputs

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ifx():
    import instancefusion_amd as m

    m.lib()
    return m


def nan_equal(a, b):
    return np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(np.nan_to_num(a), np.nan_to_num(b))


def orc_trk_buf(orc, t, name, level, w, h):
    specs = {"vmap_curr": (np.float32, (3, h, w)), "nmap_curr": (np.float32, (3, h, w)), "vmap_prev": (np.float32, (3, h, w)),
             "nmap_prev": (np.float32, (3, h, w)), "last_depth": (np.float32, (h, w)), "last_img": (np.uint8, (h, w)), "next_img": (np.uint8, (h, w)),
             "lastnext_img": (np.uint8, (h, w)), "didx": (np.int16, (h, w)), "didy": (np.int16, (h, w)), "cloud": (np.float32, (h, w, 3)),
             "depth_tmp": (np.uint16, (h, w))}
    dt, shp = specs[name]
    p = orc.lib().orc_tracker_buffer(t, name.encode(), level)
    n = int(np.prod(shp)) * np.dtype(dt).itemsize
    return np.frombuffer((C.c_char * n).from_address(p), dt).reshape(shp).copy()


# ---------------------------------------------------------------- a2: preprocessing
def test_preprocess_exact(ifx, orc, small_stream):
    g = ifx.ElasticFusion(**SMALL, max_surfels=1000)
    o = orc.Oracle(**SMALL, max_surfels=400000)
    rgb, dep = small_stream["rgb"][3], small_stream["depth"][3].copy()
    dep[:7, :9] = 0          # holes
    dep[100:110, 50:60] = 150  # below the 300 mm gate
    g.set_frame(rgb, dep)
    o.process_frame(rgb, dep)
    for name in ("depth_filtered", "depth_metric", "depth_metric_filtered"):
        assert np.array_equal(g.image(name), o.image(name)), name
    g.close(); o.close()


# ---------------------------------------------------------------- a3-a8: tracker on the reference's RGB-D pair
def test_tracker_gputest_pair(ifx, orc, gputest_pair, oracle_pins):
    L = orc.lib()
    h, w = gputest_pair[1].shape
    V, N, rgba, prev, depth_mm, rgb = protocol_inputs(*gputest_pair)
    g = ifx.ElasticFusion(w=w, h=h, max_surfels=1000, **HALF_K)
    pose, diag = g.track_pair(V, N, rgba, prev, depth_mm, rgb, np.eye(4))
    # real sensor data, against a LIVE oracle tracker on the same pair.  The sums of the normal equations are exact on both sides (bit-identical); what is left between
    # the two is the f64 rounding of the 6x6 solve (unpivoted on the device, pivoted in the oracle), which almost never survives the cast to f32: assert_pose_equal
    # (bit-equal, one f32 ulp at most -- and counted).  Errors and counts of the last iteration (diag) are functions of the exact sums: equal.
    t = L.orc_tracker_create(w, h, HALF_K["fx"], HALF_K["fy"], HALF_K["cx"], HALF_K["cy"])
    L.orc_tracker_init_first_rgb(t, orc.ptr(prev))
    p0 = np.eye(4, dtype=np.float32).reshape(16).copy()
    L.orc_tracker_init_model(t, orc.ptr(V), orc.ptr(N), orc.ptr(rgba), orc.ptr(p0))
    L.orc_tracker_init_frame(t, orc.ptr(depth_mm), orc.ptr(rgb), 20.0)
    dio = np.zeros(8, np.float32)
    L.orc_tracker_run(t, orc.ptr(p0), 10.0, 1, 0, 1, orc.ptr(dio))
    assert_pose_equal(pose, p0.reshape(4, 4), "the reference's RGB-D pair")
    assert np.array_equal(diag[:6], dio[:6]), (diag, dio)
    assert np.abs(pose - oracle_pins["pose_pyr"]).max() < 1e-6    # (and the committed regression pin of the oracle, tests/golden/oracle_pins.npz)
    # pyramid buffers against the live oracle tracker
    for lvl in range(3):
        lw, lh = w >> lvl, h >> lvl
        for name in ("vmap_curr", "nmap_curr", "vmap_prev", "nmap_prev", "last_depth", "last_img", "didx", "didy", "depth_tmp"):
            a, b = g.tracker_buffer(name, lvl), orc_trk_buf(orc, t, name, lvl, lw, lh)
            if a.dtype == np.float32:
                if name in ("vmap_curr", "nmap_curr"):   # only the x plane is defined where invalid (cudafuncs.cu:130,161)
                    bad = np.isnan(b[0])
                    assert np.array_equal(np.isnan(a[0]), bad), (name, lvl)
                    assert np.array_equal(a[:, ~bad], b[:, ~bad]), (name, lvl)
                else:
                    assert nan_equal(a, b), (name, lvl)
            else:
                assert np.array_equal(a, b), (name, lvl)
        # this frame's intensity pyramid: the oracle swapped it into "lastnext" after the run (so3), the HIP path keeps it
        # in the frame slot, where it is the next frame's "previous image"
        assert np.array_equal(g.tracker_buffer("next_img", lvl), orc_trk_buf(orc, t, "lastnext_img", lvl, lw, lh))
    L.orc_tracker_destroy(t)
    g.close()


def test_build_pyramids_stage_call(ifx, orc, gputest_pair):
    """ifx_build_pyramids (the pyramid builders of EF/Cuda/cudafuncs.cuh:64-183 as one stage call on DEVICE pointers) on the reference's RGB-D pair: every output buffer
    of every level against the oracle tracker's (createVMap / createNMap / pyrDown / intensity + pyrDownUcharGauss / Sobel; copyMaps + resize + tranformMaps /
    verticesToDepth + pyrDownGaussF / projectToPointCloud), with a model pose that is not the identity."""
    import torch

    L = orc.lib()
    h, w = gputest_pair[1].shape
    V, N, rgba, prev, depth_mm, rgb = protocol_inputs(*gputest_pair)
    ang = 0.3
    pose = np.eye(4, dtype=np.float32)
    pose[:3, :3] = np.array([[np.cos(ang), 0, np.sin(ang)], [0, 1, 0], [-np.sin(ang), 0, np.cos(ang)]], np.float32)
    pose[:3, 3] = (0.3, -0.2, 1.1)
    t = L.orc_tracker_create(w, h, HALF_K["fx"], HALF_K["fy"], HALF_K["cx"], HALF_K["cy"])
    L.orc_tracker_init_first_rgb(t, orc.ptr(prev))
    p0 = pose.reshape(16).copy()
    L.orc_tracker_init_model(t, orc.ptr(V), orc.ptr(N), orc.ptr(rgba), orc.ptr(p0))
    L.orc_tracker_init_frame(t, orc.ptr(depth_mm), orc.ptr(rgb), 20.0)
    L.orc_project_cloud.argtypes = [C.c_void_p, C.c_int, C.c_int] + [C.c_float] * 4 + [C.c_void_p]
    g = ifx.ElasticFusion(w=w, h=h, max_surfels=1000, **HALF_K)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.int16) if a.dtype == np.uint16 else np.ascontiguousarray(a)).cuda()
    d_in = [dev(depth_mm), dev(rgb), dev(V), dev(N), dev(rgba)]
    spec = dict(depth=(torch.int16, 1), vmap_curr=(torch.float32, 3), nmap_curr=(torch.float32, 3), next_img=(torch.uint8, 1), didx=(torch.int16, 1), didy=(torch.int16, 1),
                vmap_g_prev=(torch.float32, 3), nmap_g_prev=(torch.float32, 3), last_depth=(torch.float32, 1), last_img=(torch.uint8, 1), cloud=(torch.float32, 3))
    bufs = {n: [torch.full((c * (h >> l) * (w >> l),), 77, dtype=dt, device="cuda") for l in range(3)] for n, (dt, c) in spec.items()}
    torch.cuda.synchronize()
    g.build_pyramids(*[x.data_ptr() for x in d_in], model_pose=pose, **{n: [b.data_ptr() for b in v] for n, v in bufs.items()})
    names = dict(depth="depth_tmp", vmap_curr="vmap_curr", nmap_curr="nmap_curr", next_img="next_img", vmap_g_prev="vmap_prev",
                 nmap_g_prev="nmap_prev", last_depth="last_depth", last_img="last_img")
    L.orc_sobel.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    for lvl in range(3):
        lw, lh = w >> lvl, h >> lvl
        div = float(1 << lvl)
        didx = np.zeros((lh, lw), np.int16); didy = np.zeros((lh, lw), np.int16)   # (the oracle tracker takes the derivatives inside its run, RGBDOdometry.cpp:287-293: the same routine here)
        L.orc_sobel(orc.ptr(orc_trk_buf(orc, t, "next_img", lvl, lw, lh)), lw, lh, orc.ptr(didx), orc.ptr(didy))
        assert np.array_equal(bufs["didx"][lvl].cpu().numpy().reshape(lh, lw), didx), lvl
        assert np.array_equal(bufs["didy"][lvl].cpu().numpy().reshape(lh, lw), didy), lvl
        for mine, theirs in names.items():
            b = orc_trk_buf(orc, t, theirs, lvl, lw, lh)
            a = bufs[mine][lvl].cpu().numpy().view(b.dtype).reshape(b.shape)
            if mine in ("vmap_curr", "nmap_curr"):   # only the x plane is defined where invalid (cudafuncs.cu:130,161)
                bad = np.isnan(b[0])
                assert np.array_equal(np.isnan(a[0]), bad), (mine, lvl)
                assert np.array_equal(a[:, ~bad], b[:, ~bad]), (mine, lvl)
            elif a.dtype == np.float32:
                assert nan_equal(a, b), (mine, lvl)
            else:
                assert np.array_equal(a, b), (mine, lvl)
        cloud = np.zeros((lh, lw, 3), np.float32)
        L.orc_project_cloud(orc.ptr(orc_trk_buf(orc, t, "last_depth", lvl, lw, lh)), lw, lh, HALF_K["fx"] / div, HALF_K["fy"] / div, HALF_K["cx"] / div, HALF_K["cy"] / div, orc.ptr(cloud))
        assert nan_equal(bufs["cloud"][lvl].cpu().numpy().reshape(lh, lw, 3), cloud), lvl
    # the frame side alone, two outputs only: nothing else is touched
    keep = bufs["vmap_g_prev"][0].clone()
    g.build_pyramids(d_in[0].data_ptr(), d_in[1].data_ptr(), next_img=[b.data_ptr() for b in bufs["next_img"]])
    assert torch.equal(keep.view(torch.int32), bufs["vmap_g_prev"][0].view(torch.int32))   # (bit patterns: the map holds NaNs)
    with pytest.raises(ifx.IfxError):                # half an input group
        g.build_pyramids(d_in[0].data_ptr(), 0, next_img=[b.data_ptr() for b in bufs["next_img"]])
    L.orc_tracker_destroy(t)
    g.close()


def test_reduction_stage_api(ifx, orc, gputest_pair):
    """icpStep / computeRgbResidual / rgbStep / so3Step replacements on device pointers."""
    import torch

    L, G = orc.lib(), ifx.lib()
    h, w = gputest_pair[1].shape
    V, N, rgba, prev, depth_mm, rgb = protocol_inputs(*gputest_pair)
    t = L.orc_tracker_create(w, h, HALF_K["fx"], HALF_K["fy"], HALF_K["cx"], HALF_K["cy"])
    L.orc_tracker_init_first_rgb(t, orc.ptr(prev))
    p0 = np.eye(4, dtype=np.float32).reshape(16).copy()
    L.orc_tracker_init_model(t, orc.ptr(V), orc.ptr(N), orc.ptr(rgba), orc.ptr(p0))
    L.orc_tracker_init_frame(t, orc.ptr(depth_mm), orc.ptr(rgb), 20.0)
    L.orc_sobel.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    g = ifx.ElasticFusion(w=w, h=h, max_surfels=1000, **HALF_K)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.int16) if a.dtype == np.uint16 else np.ascontiguousarray(a)).cuda()
    ang = 0.01
    Rc = np.array([[np.cos(ang), -np.sin(ang), 0], [np.sin(ang), np.cos(ang), 0], [0, 0, 1]], np.float32)
    tc = np.array([0.004, -0.002, 0.003], np.float32)
    I3 = np.eye(3, dtype=np.float32); z3 = np.zeros(3, np.float32)
    for lvl in range(3):
        lw, lh = w >> lvl, h >> lvl
        div = float(1 << lvl)
        fx, fy, cx, cy = HALF_K["fx"] / div, HALF_K["fy"] / div, HALF_K["cx"] / div, HALF_K["cy"] / div
        b = {n: orc_trk_buf(orc, t, n, lvl, lw, lh) for n in ("vmap_curr", "nmap_curr", "vmap_prev", "nmap_prev", "last_depth", "last_img", "next_img", "lastnext_img")}
        d = {n: dev(np.nan_to_num(v, nan=np.nan)) for n, v in b.items()}
        # --- icp
        L.orc_icp_step.argtypes = [C.c_void_p] * 6 + [C.c_float] * 4 + [C.c_void_p] * 2 + [C.c_float] * 2 + [C.c_int] * 2 + [C.c_void_p]
        ref = np.zeros(29, np.float32); got = np.zeros(29, np.float32)
        sn = np.float32(np.sin(20.0 * 3.14159254 / 180.0))
        L.orc_icp_step(orc.ptr(Rc.reshape(9).copy()), orc.ptr(tc), orc.ptr(b["vmap_curr"]), orc.ptr(b["nmap_curr"]), orc.ptr(I3.reshape(9).copy()), orc.ptr(z3), fx, fy, cx, cy,
                       orc.ptr(b["vmap_prev"]), orc.ptr(b["nmap_prev"]), 0.10, sn, lw, lh, orc.ptr(ref))
        r = G.ifx_icp_step(g.handle, orc.ptr(Rc.reshape(9).copy()), orc.ptr(tc), d["vmap_curr"].data_ptr(), d["nmap_curr"].data_ptr(), orc.ptr(I3.reshape(9).copy()), orc.ptr(z3),
                           fx, fy, cx, cy, d["vmap_prev"].data_ptr(), d["nmap_prev"].data_ptr(), 0.10, sn, lw, lh, orc.ptr(got))
        assert r == 0 and got[28] == ref[28] and ref[28] > 100
        assert np.array_equal(got, ref)            # exact: grid-valued terms summed in f64, the same total in any order (ifx_dev.h / orc_math.h)
        # --- rgb residual + rgb step
        didx = np.zeros((lh, lw), np.int16); didy = np.zeros((lh, lw), np.int16)
        L.orc_sobel(orc.ptr(b["next_img"]), lw, lh, orc.ptr(didx), orc.ptr(didy))
        cloud = np.zeros((lh, lw, 3), np.float32)
        L.orc_project_cloud.argtypes = [C.c_void_p, C.c_int, C.c_int] + [C.c_float] * 4 + [C.c_void_p]
        L.orc_project_cloud(orc.ptr(b["last_depth"]), lw, lh, fx, fy, cx, cy, orc.ptr(cloud))
        K = np.array([[fx, 0, cx], [0, fy, cy], [0, 0, 1]], np.float64)
        krk = (K @ Rc.astype(np.float64).T @ np.linalg.inv(K)).astype(np.float32).reshape(9).copy()
        kt = (K @ (-Rc.astype(np.float64).T @ tc)).astype(np.float32)
        dt_ref = np.zeros((lh, lw), np.dtype([("zx", np.int16), ("zy", np.int16), ("ox", np.int16), ("oy", np.int16), ("diff", np.float32), ("valid", np.int32)]))
        cnt, sig = C.c_int(), C.c_int()
        L.orc_rgb_residual.argtypes = [C.c_float] + [C.c_void_p] * 7 + [C.c_float, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
        min_scale = float((5, 3, 1)[lvl] ** 2 * 64)
        L.orc_rgb_residual(min_scale, orc.ptr(didx), orc.ptr(didy), orc.ptr(b["last_depth"]), orc.ptr(b["last_depth"]), orc.ptr(b["last_img"]), orc.ptr(b["next_img"]),
                           orc.ptr(dt_ref), 0.07, orc.ptr(kt), orc.ptr(krk), lw, lh, C.byref(cnt), C.byref(sig))
        d_didx, d_didy, d_cloud = dev(didx), dev(didy), dev(cloud)
        d_cor = torch.zeros(lw * lh * 2, dtype=torch.int32).cuda()
        gc, gs = C.c_int(), C.c_int()
        r = G.ifx_rgb_residual(g.handle, min_scale, d_didx.data_ptr(), d_didy.data_ptr(), d["last_depth"].data_ptr(), d["last_depth"].data_ptr(), d["last_img"].data_ptr(),
                               d["next_img"].data_ptr(), d_cor.data_ptr(), 0.07, orc.ptr(kt), orc.ptr(krk), lw, lh, C.byref(gc), C.byref(gs))
        assert r == 0 and (gc.value, gs.value) == (cnt.value, sig.value)
        cor = d_cor.cpu().numpy().view(ifx.CORRES_DTYPE).reshape(lh, lw)
        valid = dt_ref["valid"] != 0
        assert np.array_equal(cor["zx"] >= 0, valid)
        assert np.array_equal(cor["zx"][valid], dt_ref["zx"][valid]) and np.array_equal(cor["zy"][valid], dt_ref["zy"][valid])
        assert np.array_equal(cor["diff"][valid], dt_ref["diff"][valid])
        if cnt.value:
            L.orc_rgb_step.argtypes = [C.c_void_p, C.c_float, C.c_void_p, C.c_float, C.c_float, C.c_void_p, C.c_void_p, C.c_float, C.c_int, C.c_int, C.c_void_p]
            sigma = float(np.sqrt(cnt.value))
            L.orc_rgb_step(orc.ptr(dt_ref), sigma, orc.ptr(cloud), fx, fy, orc.ptr(didx), orc.ptr(didy), 0.125, lw, lh, orc.ptr(ref))
            r = G.ifx_rgb_step(g.handle, d_cor.data_ptr(), sigma, d_cloud.data_ptr(), fx, fy, d_didx.data_ptr(), d_didy.data_ptr(), 0.125, lw, lh, orc.ptr(got))
            assert r == 0 and got[28] == ref[28]
            assert np.array_equal(got, ref)
        # --- so3
        Kinv = np.linalg.inv(K)
        Rs = np.array([[1, 0, 0.004], [0, 1, -0.003], [-0.004, 0.003, 1]], np.float64)
        ib = (K @ Rs @ Kinv).astype(np.float32).reshape(9).copy(); kinv = Kinv.astype(np.float32).reshape(9).copy(); krlr = (K @ Rs).astype(np.float32).reshape(9).copy()
        L.orc_so3_step.argtypes = [C.c_void_p] * 5 + [C.c_int, C.c_int, C.c_void_p]
        r11 = np.zeros(11, np.float32); g11 = np.zeros(11, np.float32)
        L.orc_so3_step(orc.ptr(b["lastnext_img"]), orc.ptr(b["next_img"]), orc.ptr(ib), orc.ptr(kinv), orc.ptr(krlr), lw, lh, orc.ptr(r11))
        r = G.ifx_so3_step(g.handle, d["lastnext_img"].data_ptr(), d["next_img"].data_ptr(), orc.ptr(ib), orc.ptr(kinv), orc.ptr(krlr), lw, lh, orc.ptr(g11))
        assert r == 0 and g11[10] == r11[10]
        assert np.array_equal(g11, r11)
    L.orc_tracker_destroy(t)
    g.close()


# ---------------------------------------------------------------- a9-a15: map stages on identical map states
def _run_to_state(ifx, orc, st, n_frames):
    g = ifx.ElasticFusion(**SMALL, max_surfels=400000)
    g.set_option("compact_every_frame", 1)
    o = orc.Oracle(**SMALL, max_surfels=400000)
    for i in range(n_frames):
        o.process_frame(st["rgb"][i], st["depth"][i])
    return g, o


MAP_KEYS = ("pc", "nr", "col", "tm", "ic", "votes")


def test_map_stages_exact(ifx, orc, small_stream):
    st = small_stream
    g, o = _run_to_state(ifx, orc, st, 6)
    m = o.download()
    m["pc"][::3, 3] = 15.0    # make a third of the surfels stable so that splats / id discs are drawn
    o.upload(m); g.upload(m)
    pose = st["poses"][6].astype(np.float32)
    tick = o.tick
    # index map (predictIndices)
    o.predict_indices(pose, tick); g.predict_indices(pose, tick)
    for name in ("index", "index_vc", "index_ct", "index_nr"):
        assert np.array_equal(g.image(name), o.image(name)), name
    assert (o.image("index") > 0).mean() > 0.5
    # splat prediction + fill-in (combinedPredict + FillIn)
    # both sides see frame 6 (upload + preprocessing only; maps untouched) for the fill-in
    g.set_frame(st["rgb"][6], st["depth"][6])
    o.set_frame(st["rgb"][6], st["depth"][6])
    o.combined_predict(pose, tick, tick); g.combined_predict(pose, tick, tick)
    for name in ("pred_vertex", "pred_normal", "pred_image", "pred_inst", "pred_time"):
        assert np.array_equal(g.image(name), o.image(name)), name
    assert (o.image("pred_vertex")[..., 2] > 0).mean() > 0.2
    # id render (renderSurfelIds), both modes
    assert np.array_equal(g.render_ids(pose, 0), o.render_ids(pose, 0))
    assert np.array_equal(g.render_ids(pose, 1), o.render_ids(pose, 1))
    g.close(); o.close()


def test_fuse_and_clean_exact(ifx, orc, small_stream):
    st = small_stream
    g, o = _run_to_state(ifx, orc, st, 6)
    m = o.download()
    g.upload(m)
    pose = st["poses"][6].astype(np.float32)
    tick = o.tick
    g.set_frame(st["rgb"][6], st["depth"][6])
    o.set_frame(st["rgb"][6], st["depth"][6])
    o.predict_indices(pose, tick); g.predict_indices(pose, tick)
    o.fuse(pose, tick, 0.75); g.fuse(pose, tick, 0.75)
    o.predict_indices(pose, tick); g.predict_indices(pose, tick)
    o.clean(pose, tick); g.clean(pose, tick)
    mo, mg = o.download(), g.download()
    assert mo["pc"].shape == mg["pc"].shape and mo["pc"].shape[0] != m["pc"].shape[0]
    for k in MAP_KEYS:
        assert np.array_equal(mo[k], mg[k]), k
    g.close(); o.close()


# ---------------------------------------------------------------- a1: whole frames, a16-a23: instance layer
def test_end_to_end_sequence(ifx, orc, small_stream):
    from instancefusion_amd import synth

    st = small_stream
    g = ifx.ElasticFusion(**SMALL, max_surfels=400000)
    g.set_option("compact_every_frame", 1)
    o = orc.Oracle(**SMALL, max_surfels=400000)
    inst = ifx.InstanceFusion(g)
    err = []
    for i in range(10):
        pg = g.processFrame(st["rgb"][i], st["depth"][i])
        po = o.process_frame(st["rgb"][i], st["depth"][i])
        assert_pose_equal(pg, po, f"frame {i}")
        assert g.count == o.count, i
        assert np.array_equal(g.image("ids_after"), o.image("ids_after")), i
    assert np.allclose(g.trajectory()[-1], pg)
    # instance layer on identical map states: upload the oracle's map into the GPU object
    m = o.download(); m["pc"][:, 3] = np.maximum(m["pc"][:, 3], 12.0)
    o.upload(m); g.upload(m)
    pose = po
    ids_o = o.render_ids(pose, 0); ids_g = g.render_ids(pose, 0)
    assert np.array_equal(ids_o, ids_g)
    # run one more frame with the pose held fixed so that both refresh ids_after from the same state (the pose BEFORE it identical too:
    # the velocity weighting of the fused measurements compares the two)
    g.set_pose(pose, o.tick); o.set_pose(pose, o.tick)
    pg = g.processFrame(st["rgb"][9], st["depth"][9], inPose=pose); po2 = o.process_frame(st["rgb"][9], st["depth"][9], in_pose=pose)
    # identical map, identical pose, identical frame: the precondition of the exact label comparison below is asserted, not assumed
    assert g.count == o.count
    assert np.array_equal(g.image("ids_after"), o.image("ids_after"))
    masks, cls = synth.canned_masks(st["obj"][9], st["scene"])
    assert inst.whetherDoSegmentation(100) == o.should_segment(100)
    for frame in (100, 103):
        inst.ProcessSegmentation(st["rgb"][9], st["depth"][9], masks, cls, frame)
        o.process_segmentation(st["rgb"][9], st["depth"][9], masks, cls, frame)
        assert np.array_equal(inst.getInstanceTable(), o.instance_table())
        lg, lo = inst.labels(), o.labels()
        assert np.array_equal(lg, lo)                      # exact integer match of the instance IDs
        assert np.array_equal(g.download()["votes"], o.download()["votes"])
    assert (lo >= 0).sum() > 100
    assert np.array_equal(inst.maskCleanOverlap(masks), _clean(orc, masks))
    g.close(); o.close()


def test_bootstrap_pose_guess(ifx, orc, small_stream):
    """processFrame(..., inPose, bootstrap=true), EF/ElasticFusion.cpp:334-356: inPose is the tracker's initial guess
    (currPose * inPose), the model maps keep the old pose, the velocity weighting compares with the pose before the guess."""
    st = small_stream
    g = ifx.ElasticFusion(**SMALL, max_surfels=400000)
    g.set_option("compact_every_frame", 1)
    o = orc.Oracle(**SMALL, max_surfels=400000)
    for i in range(4):
        pg = g.processFrame(st["rgb"][i], st["depth"][i]); po = o.process_frame(st["rgb"][i], st["depth"][i])
    # the true relative motion of the next frame as the guess, slightly off
    rel = (np.linalg.inv(st["poses"][3].astype(np.float64)) @ st["poses"][4].astype(np.float64)).astype(np.float32)
    rel[:3, 3] += np.float32([0.002, -0.001, 0.0015])
    pg = g.processFrame(st["rgb"][4], st["depth"][4], inPose=rel, bootstrap=True)
    po = o.process_frame(st["rgb"][4], st["depth"][4], in_pose=rel, bootstrap=True)
    assert_pose_equal(pg, po, "bootstrap frame")
    assert np.abs(pg - st["poses"][4]).max() < 0.02                      # it tracked (a replaced pose would equal pose3 * rel exactly)
    assert np.abs(pg - (st["poses"][3] @ rel)).max() > 1e-6
    # the frames that follow are unaffected by the mode
    pg = g.processFrame(st["rgb"][5], st["depth"][5]); po = o.process_frame(st["rgb"][5], st["depth"][5])
    assert_pose_equal(pg, po, "frame after the bootstrap frame")
    assert g.count == o.count and np.array_equal(g.image("ids_after"), o.image("ids_after"))
    with pytest.raises(ifx.IfxError):
        g.processFrame(st["rgb"][6], st["depth"][6], bootstrap=True)     # assert(inPose) in the reference
    g.close(); o.close()


def test_bounding_boxes_and_instance_point_clouds(ifx, orc, small_stream):
    """f-4: computeMapBoundingBox / getInstancePointCloud (IF/Core/InstanceFusion.cpp:1261-1590) on identical labelled maps: the 648 normal
    votes, the boxes in both frames and the per-instance counts are integers and must match exactly; ground normal, frames and the
    records to float rounding of the tiny host part (same formulas, two compilers)."""
    from instancefusion_amd import synth

    st = small_stream
    g = ifx.ElasticFusion(**SMALL, max_surfels=400000)
    g.set_option("compact_every_frame", 1)
    o = orc.Oracle(**SMALL, max_surfels=400000)
    inst = ifx.InstanceFusion(g)
    for i in range(8):
        po = o.process_frame(st["rgb"][i], st["depth"][i])
    m = o.download(); m["pc"][:, 3] = np.maximum(m["pc"][:, 3], 12.0)
    o.upload(m); g.processFrame(st["rgb"][0], st["depth"][0]); g.upload(m)
    g.set_pose(po, o.tick); o.set_pose(po, o.tick)
    g.processFrame(st["rgb"][7], st["depth"][7], inPose=po); o.process_frame(st["rgb"][7], st["depth"][7], in_pose=po)
    masks, cls = synth.canned_masks(st["obj"][7], st["scene"])
    inst.ProcessSegmentation(st["rgb"][7], st["depth"][7], masks, cls, 100, superpixels=True)
    o.process_segmentation(st["rgb"][7], st["depth"][7], masks, cls, 100, flags=2)
    assert np.array_equal(inst.labels(), o.labels())
    for bt in (True, False):
        bg, ng, cg, mg, vg = inst.computeMapBoundingBox(bt)
        bo, no, co, mo, vo = o.map_bounding_boxes(bt)
        assert np.array_equal(vg, vo) and vo.sum() > 1000                       # the normal votes of the whole map
        assert np.allclose(ng, no, atol=1e-6) and np.allclose(cg, co, atol=1e-6) and np.allclose(mg, mo, atol=1e-5)
        found = bo[:, 0] < 900
        assert found.sum() >= 2 and np.array_equal(found, bg[:, 0] < 900)
        assert np.allclose(bg, bo, atol=2e-5), np.abs(bg - bo).max()            # (integer boxes of frame coordinates that differ by float rounding of the frames)
        assert (bg[found, 1] > bg[found, 0]).all()
    cg, _ = inst.getInstancePointCloud(-1)
    co, _ = o.instance_point_cloud(-1)
    assert np.array_equal(cg, co) and cg.sum() > 100
    q = int(np.argmax(cg))
    cg, rg = inst.getInstancePointCloud(q, True)
    co, ro = o.instance_point_cloud(q, True)
    assert rg.shape == ro.shape == (cg[q], 10)
    assert np.array_equal(rg[:, 0], ro[:, 0]) and np.array_equal(rg[:, 7:], ro[:, 7:])      # slots in map order, colours
    assert np.allclose(rg[:, 1:7], ro[:, 1:7], atol=2e-5)
    lab = inst.labels()
    assert set(rg[:, 0].astype(int).tolist()) <= set(np.nonzero(lab >= 0)[0].tolist())       # every record's slot is a labelled live surfel (compacted store: slot = rank)
    g.close(); o.close()


@pytest.mark.parametrize("ff_rounds", [0, 2])
def test_segmentation_device_schedule_equals_host_schedule(ifx, small_stream, ff_rounds):
    """The segmentation call without the host in the middle of it (default since round 3: compare map, registration and the flood fill's termination on the
    device, one synchronisation at the end) against round 2's host-driven schedule (`seg_device` 0): instance tables, votes, labels and colours bit for bit
    over calls with superpixels, calls that match registered instances, and the eviction of a full table (the device stops at the mask that finds no free
    slot, the host evicts and goes on from there).  ff_rounds = 2 halves the fixed relaxation schedule (default 4).  That is NOT too short here: the room's objects
    stand nearer than 3.37 m (4000 depth units), every edge of the fill is two-way, the union-find start is already the fixpoint and the first relaxation changes
    nothing.  Launch counts of the first call, printed below: 2 ff_relax and 1 ff_count with ff_rounds = 2, 4 and 1 by default -- the tail is issued once, the
    host-driven resume does not run.  What this parameter exercises is a schedule whose LAST launch is the second one (the gate word moves with it); the resume
    itself is driven by tests/test_gpu_flood_fill_cases.py::test_serpentine_inside_a_call."""
    from instancefusion_amd import synth

    st = small_stream
    a = ifx.ElasticFusion(**SMALL, max_surfels=400000)
    b = ifx.ElasticFusion(**SMALL, max_surfels=400000)
    b.set_option("seg_device", 0)
    a.set_option("ff_rounds", ff_rounds)
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
            if i == 4:      # the launch counts of one call, read once (see the docstring)
                a.set_option("kernel_timing", 1); a.kernel_ms("__reset__")
            ia.ProcessSegmentation(st["rgb"][i], st["depth"][i], masks, cls, 100 + 3 * i, superpixels=True)
            if i == 4:
                print("ff_rounds", ff_rounds, ": ff_relax launches", a.kernel_ms("ff_relax")[1], "ff_count launches", a.kernel_ms("ff_count")[1])
                a.set_option("kernel_timing", 0)
            ib.ProcessSegmentation(st["rgb"][i], st["depth"][i], masks, cls, 100 + 3 * i, superpixels=True)
            assert np.array_equal(ia.getInstanceTable(), ib.getInstanceTable()), i
            assert np.array_equal(ia.labels(), ib.labels()), i
    assert (ia.labels() >= 0).sum() > 100
    # fill the table: new classes for every mask until the twenty weakest instances are evicted
    i = 7
    masks, cls = synth.canned_masks(st["obj"][i], st["scene"])
    nm = masks.shape[0]
    evicted = False
    for call in range(60):
        classes = (1000 + call * nm + np.arange(nm)).astype(np.int32)     # never seen before: every usable mask takes a new slot until the table is full
        before = (ib.getInstanceTable() >= 0).sum()
        ia.ProcessSegmentation(st["rgb"][i], st["depth"][i], masks, classes, 300 + 3 * call)
        ib.ProcessSegmentation(st["rgb"][i], st["depth"][i], masks, classes, 300 + 3 * call)
        assert np.array_equal(ia.getInstanceTable(), ib.getInstanceTable()), call
        evicted = evicted or (ib.getInstanceTable() >= 0).sum() < before
        if evicted:
            break
    assert evicted
    ma, mb = a.download(), b.download()
    for k in MAP_KEYS:
        assert np.array_equal(ma[k], mb[k]), k
    assert np.array_equal(ia.labels(), ib.labels())
    a.close(); b.close()


def _clean(orc, masks):
    m = masks.copy()
    L = orc.lib()
    L.orc_mask_clean_overlap.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int]
    L.orc_mask_clean_overlap(orc.ptr(m), m.shape[0], m.shape[2], m.shape[1])
    return m


# ---------------------------------------------------------------- full-size properties (BASELINE sizes)
def test_full_size_properties(ifx):
    from instancefusion_amd import synth

    W, H = 640, 480
    K = dict(fx=528.0, fy=528.0, cx=320.0, cy=240.0)
    st = synth.make_stream(8, W, H, noise=True, **K)
    big = synth.make_map(1_000_000, st["scene"], st["poses_world"][0], 1000)

    def run(compact_every_frame):
        g = ifx.ElasticFusion(w=W, h=H, max_surfels=1_600_000, **K)
        g.set_option("compact_every_frame", compact_every_frame)
        g.processFrame(st["rgb"][0], st["depth"][0])
        g.upload(big); g.set_pose(st["poses"][0], 1000); g.combined_predict(st["poses"][0], 1000, 1000)
        poses = [g.processFrame(st["rgb"][i], st["depth"][i]) for i in range(1, 8)]
        ids = g.image("ids_after")
        slots, live = g.slots, g.count
        assert ids.max() < slots and ids.min() >= 0
        inst = ifx.InstanceFusion(g)
        masks, cls = synth.canned_masks(st["obj"][7], st["scene"])
        inst.ProcessSegmentation(st["rgb"][7], st["depth"][7], masks, cls, 200)
        lab = inst.labels()
        m = g.download()
        g.close()
        return np.stack(poses), m, lab, live

    p1, m1, l1, n1 = run(0)
    p2, m2, l2, n2 = run(1)
    p3, m3, l3, n3 = run(0)
    # determinism: identical inputs -> bit-identical outputs
    assert np.array_equal(p1, p3) and all(np.array_equal(m1[k], m3[k]) for k in MAP_KEYS) and np.array_equal(l1, l3)
    # tombstones + lazy compaction is equivalent to compacting every frame (order-preserving)
    assert np.array_equal(p1, p2) and n1 == n2
    assert all(np.array_equal(m1[k], m2[k]) for k in MAP_KEYS) and np.array_equal(l1, l2)
    # compaction is idempotent and the label scan equals the decoded arg-max
    v = np.trunc(m1["votes"]).astype(np.int64)
    cnt = np.empty((v.shape[0], 96), np.int64)
    cnt[:, 0::2] = (((v >> 16) & 0xFFFF) ^ 0x8000) - 0x8000
    cnt[:, 1::2] = ((v & 0xFFFF) ^ 0x8000) - 0x8000
    assert np.array_equal(l1, np.where(cnt.max(axis=1) > 0, cnt.argmax(axis=1), -1))
    gt = st["poses"][1:8]
    assert np.sqrt(np.mean(np.sum((p1[:, :3, 3] - gt[:, :3, 3]) ** 2, axis=1))) < 0.02


def _label_image(ids, labels):
    """instance label under every pixel (the surfel id image looked up in bestIDInEachSurfel); -2 where no surfel"""
    ids = np.asarray(ids, np.int64)
    ok = (ids > 0) & (ids < len(labels))
    return np.where(ok, np.asarray(labels)[np.where(ok, ids, 0)], -2)


@pytest.mark.timeout(1500)
def test_full_loop_640x480_trajectory_and_labels(ifx, orc):
    """The whole 90-frame camera loop of the benchmark stream at 640x480, HIP against the oracle frame by frame (BASELINE
    configuration 2 without the pre-populated map, so that the oracle finishes in a minute): per-frame pose, RMS over the
    whole trajectory bit-equal (<= 1 ulp; the north star asks 1e-4 m RMS), map sizes / id images / the whole map equal, and the
    instance layer with superpixel refinement at four segmentation calls -- instance tables, labels and the label under every
    pixel equal; a fifth call after re-uploading the map (exercises upload + held pose at this size)."""
    import os

    from instancefusion_amd import synth

    W, H, NF = 640, 480, 90
    K = dict(fx=528.0, fy=528.0, cx=320.0, cy=240.0)
    st = synth.make_stream(NF, W, H, noise=True, loop_len=NF, **K)
    orc.set_threads(orc.usable_cores())
    g = ifx.ElasticFusion(w=W, h=H, max_surfels=3_000_000, **K)
    g.set_option("compact_every_frame", 1)                                # slot numbers = the oracle's indices, so that the id images can be compared (lazy compaction: test_full_size_properties)
    o = orc.Oracle(w=W, h=H, max_surfels=3_000_000, **K)
    inst = ifx.InstanceFusion(g)
    err, rot = [], []
    seg_frames = (30, 50, 70, 89)
    lab_mismatch = []
    for i in range(NF):
        pg = g.processFrame(st["rgb"][i], st["depth"][i]); po = o.process_frame(st["rgb"][i], st["depth"][i])
        err.append(float(np.linalg.norm(pg[:3, 3] - po[:3, 3])))
        rot.append(float(np.abs(pg[:3, :3] - po[:3, :3]).max()))
        assert_pose_equal(pg, po, f"frame {i}")                              # every single frame: bit-equal (<= 1 ulp, counted)
        if i % 15 == 14 or i in seg_frames:
            assert g.count == o.count, (i, g.count, o.count)                 # map sizes equal
            assert np.array_equal(g.image("ids_after"), o.image("ids_after")), i
        if i in seg_frames:
            masks, cls = synth.canned_masks(st["obj"][i], st["scene"])
            assert masks.shape[0] > 0
            inst.ProcessSegmentation(st["rgb"][i], st["depth"][i], masks, cls, i, superpixels=True)
            o.process_segmentation(st["rgb"][i], st["depth"][i], masks, cls, i, flags=2)
            assert np.array_equal(inst.getInstanceTable(), o.instance_table()), i
            lg, lo = inst.labels(), o.labels()
            li_g, li_o = _label_image(g.image("ids_after"), lg), _label_image(o.image("ids_after"), lo)
            lab_mismatch.append(float((li_g != li_o).mean()))
            assert np.array_equal(lg, lo), i                                  # every label of the map, every call
            assert np.array_equal(li_g, li_o), (i, lab_mismatch)
    rms = float(np.sqrt(np.mean(np.square(err))))
    assert rms <= 1e-7, rms                                                  # (north star: 1e-4 m RMS; asserted: <= 1 ulp per pose entry above)
    mg_, mo_ = g.download(), o.download()
    for k in MAP_KEYS:
        assert np.array_equal(mg_[k], mo_[k]), k                             # the whole map after 90 free-running frames, bit for bit
    del mg_, mo_
    gt = st["poses"][:NF]
    traj = g.trajectory()
    assert traj.shape[0] == NF
    ate = float(np.sqrt(np.mean(np.sum((traj[:, :3, 3] - gt[:, :3, 3]) ** 2, axis=1))))
    assert ate < 0.05                                                        # both sides drift alike against the ground truth (the algorithm's own error)
    assert (lo >= 0).sum() > 1000
    # exact label equality needs identical maps: the oracle's map goes into the HIP object, one frame with the pose held, a fifth call
    m = o.download()
    g.upload(m); o.upload(m)
    g.set_pose(po, o.tick); o.set_pose(po, o.tick)
    pg = g.processFrame(st["rgb"][NF - 1], st["depth"][NF - 1], inPose=po); o.process_frame(st["rgb"][NF - 1], st["depth"][NF - 1], in_pose=po)
    assert g.count == o.count and np.array_equal(g.image("ids_after"), o.image("ids_after"))
    masks, cls = synth.canned_masks(st["obj"][NF - 1], st["scene"])
    inst.ProcessSegmentation(st["rgb"][NF - 1], st["depth"][NF - 1], masks, cls, 200, superpixels=True)
    o.process_segmentation(st["rgb"][NF - 1], st["depth"][NF - 1], masks, cls, 200, flags=2)
    assert np.array_equal(inst.getInstanceTable(), o.instance_table())
    assert np.array_equal(inst.labels(), o.labels())                         # exact integer match of the instance IDs
    assert np.array_equal(g.download()["votes"], o.download()["votes"])
    print(f"90-frame loop: pose RMS {rms:.2e} m (max {max(err):.2e}), label-image mismatch {lab_mismatch}, ATE vs ground truth {ate * 1e3:.1f} mm")
    g.close(); o.close()


@pytest.mark.timeout(1500)
def test_bench_configuration_against_the_oracle_directly(ifx, orc):
    """bench.py's OWN configuration against the oracle, with no HIP-vs-HIP link in between: the 90-frame 640x480 loop through ifx_hint_next_frame_device +
    ifx_enqueue_frame_device (frames resident in HBM, one-frame look-ahead, the next frame's tracker parked behind every frame), default options -- lazy tombstone
    compaction, cached view lists aged over several frames, the id image on the sampled lattice, the 6x6 solve in the next launch's prologue -- and three
    segmentation calls on the RESIDENT frame (ProcessSegmentation(None, None, ...): beside the tracker queued ahead).  Every pose against the oracle's as it is produced
    (assert_pose_equal: bit-equal, <= 1 ulp counted), the instance tables at the calls, and at the end the downloaded map, votes and labels array_equal."""
    import torch

    from instancefusion_amd import synth

    W, H, NF = 640, 480, 90
    K = dict(fx=528.0, fy=528.0, cx=320.0, cy=240.0)
    st = synth.make_stream(NF, W, H, noise=True, loop_len=NF, **K)
    orc.set_threads(orc.usable_cores())
    d_rgb = torch.from_numpy(st["rgb"]).cuda()
    d_dep = torch.from_numpy(st["depth"].view(np.int16)).cuda()
    torch.cuda.synchronize()
    g = ifx.ElasticFusion(w=W, h=H, max_surfels=3_000_000, **K)             # every option at its default
    g.set_option("hot_verify", 1)                                            # (debug pass: the gathered copy of the store against the arrays before every frame that trusts it)
    o = orc.Oracle(w=W, h=H, max_surfels=3_000_000, **K)
    inst = ifx.InstanceFusion(g)
    seg_frames = (35, 60, 89)
    scans0 = g.view_list_stats()["scans"]
    for i in range(NF):
        if i + 1 < NF:
            g.hint_next_frame_device(d_rgb[i + 1].data_ptr(), d_dep[i + 1].data_ptr())
        g.enqueue_frame_device(d_rgb[i].data_ptr(), d_dep[i].data_ptr(), i)
        inst.whetherDoSegmentation(100 + i)                                   # the host's per-frame decision point, as in bench.py (waits for the frame's result only)
        po = o.process_frame(st["rgb"][i], st["depth"][i])
        if i in seg_frames:
            masks, cls = synth.canned_masks(st["obj"][i], st["scene"])
            assert masks.shape[0] > 0
            inst.ProcessSegmentation(None, None, masks, cls, i, superpixels=True)
            o.process_segmentation(st["rgb"][i], st["depth"][i], masks, cls, i, flags=2)
            assert np.array_equal(inst.getInstanceTable(), o.instance_table()), i
        assert_pose_equal(g.trajectory(1)[0], po, f"frame {i}")              # (the trajectory ring: no interference with the frames in flight beyond a stream wait)
    vs = g.view_list_stats()
    assert 3 < vs["scans"] - scans0 < NF // 2, vs                            # the lists really were cached over several frames
    assert g.tracker_fallbacks() == 0
    assert g.hot_records_stale() == 0                                        # every writer of the frame path kept the gathered copy coherent over the 90 frames
    assert g.count == o.count
    assert np.array_equal(inst.labels(), o.labels()) and (o.labels() >= 0).sum() > 1000
    mg_, mo_ = g.download(), o.download()
    for k in MAP_KEYS:
        assert np.array_equal(mg_[k], mo_[k]), k
    g.close(); o.close()


def test_map_view_is_valid_until_the_next_frame_call(ifx, small_stream):
    """ifx_map_view hands out MUTABLE pointers (the reference's getMapSurfelsGpu).  Writes made before the next frame call are seen by that frame (the gathered copy of
    the store is rebuilt behind every view); a write through a pointer kept PAST a frame call is outside the contract (include/ifx_c_api.h) -- and the debug pass
    `hot_verify` says so: ifx_hot_records_stale counts the slot."""
    hip = C.CDLL("libamdhip64.so")
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    st = small_stream
    g = ifx.ElasticFusion(**SMALL, max_surfels=400000)
    g.set_option("clean_raster", 1); g.set_option("hot_records", 1)          # (what this test is about, whatever IFX_OPTS switched off for the run: tools/round_extras.sh)
    g.set_option("hot_verify", 1)
    for i in range(4):
        g.processFrame(st["rgb"][i], st["depth"][i])
    assert g.hot_records_stale() == 0
    v = g.map_view()
    rec = np.zeros(4, np.float32)
    slot = v.count // 2
    assert hip.hipMemcpy(rec.ctypes.data, v.d_pos_conf + 16 * slot, 16, 2) == 0
    rec[3] += 0.25                                                            # inside the contract: written before the next frame call
    assert hip.hipMemcpy(v.d_pos_conf + 16 * slot, rec.ctypes.data, 16, 1) == 0
    g.processFrame(st["rgb"][4], st["depth"][4])
    g.processFrame(st["rgb"][5], st["depth"][5])
    assert g.hot_records_stale() == 0
    g.sync()
    assert hip.hipMemcpy(rec.ctypes.data, v.d_pos_conf + 16 * slot, 16, 2) == 0
    rec[3] += 0.25                                                            # outside it: the pointer was kept past two frame calls
    assert hip.hipMemcpy(v.d_pos_conf + 16 * slot, rec.ctypes.data, 16, 1) == 0
    g.processFrame(st["rgb"][6 % st["rgb"].shape[0]], st["depth"][6 % st["rgb"].shape[0]])
    assert g.hot_records_stale() == 1
    g.close()


@pytest.mark.timeout(1500)
def test_config3_5m_map_full_instance_path(ifx, orc):
    """BASELINE configuration 3's workload (rgbd-scenes-v2 is not in the image: the synthetic stream stands in): a 5M-surfel
    map, 640x480, the FULL instance path -- votes, gSLICr superpixels + geometric merging, flood fill, label scan, kNN colour
    smoothing.  Against the oracle on the same 5M map: poses, instance table, labels (exact: both start from the same map and
    the frames before the call keep them identical or the test says so); then size-independent properties of the kNN pass."""
    import os

    from instancefusion_amd import synth

    W, H = 640, 480
    K = dict(fx=528.0, fy=528.0, cx=320.0, cy=240.0)
    N = 5_000_000
    st = synth.make_stream(4, W, H, noise=True, loop_len=90, **K)
    big = synth.make_map(N, st["scene"], st["poses_world"][0], 1000)
    orc.set_threads(orc.usable_cores())
    g = ifx.ElasticFusion(w=W, h=H, max_surfels=N + 600_000, **K)
    g.set_option("compact_every_frame", 1)
    o = orc.Oracle(w=W, h=H, max_surfels=N + 600_000, **K)
    g.processFrame(st["rgb"][0], st["depth"][0]); o.process_frame(st["rgb"][0], st["depth"][0])
    g.upload(big); o.upload(big)
    g.set_pose(st["poses"][0], 1000); o.set_pose(st["poses"][0], 1000)
    g.combined_predict(st["poses"][0], 1000, 1000); o.combined_predict(st["poses"][0], 1000, 1000)
    for name in ("pred_vertex", "pred_normal", "pred_image"):
        assert np.array_equal(g.image(name), o.image(name)), name           # the 5M-surfel prediction itself, bit for bit
    inst = ifx.InstanceFusion(g)
    for i in (1, 2):
        pg = g.processFrame(st["rgb"][i], st["depth"][i]); po = o.process_frame(st["rgb"][i], st["depth"][i])
        assert_pose_equal(pg, po, f"frame {i}")
    assert g.count == o.count and np.array_equal(g.image("ids_after"), o.image("ids_after"))
    masks, cls = synth.canned_masks(st["obj"][2], st["scene"])
    inst.ProcessSegmentation(st["rgb"][2], st["depth"][2], masks, cls, 300, superpixels=True)
    o.process_segmentation(st["rgb"][2], st["depth"][2], masks, cls, 300, flags=2)
    assert np.array_equal(inst.getInstanceTable(), o.instance_table())
    lg, lo = inst.labels(), o.labels()
    assert lg.shape[0] == g.count and np.array_equal(lg, lo)               # exact integer match over all ~5M surfels
    mg = g.download()
    assert np.array_equal(mg["votes"], o.download()["votes"])
    # labels = decoded arg-max of the packed counters (first maximum wins, -1 when nothing is positive)
    for a in range(0, lg.shape[0], 500_000):                                 # in slices: 5M x 96 int64 counters would be 3.8 GB
        v = np.trunc(mg["votes"][a:a + 500_000]).astype(np.int64)
        cnt = np.empty((v.shape[0], 96), np.int64)
        cnt[:, 0::2] = (((v >> 16) & 0xFFFF) ^ 0x8000) - 0x8000
        cnt[:, 1::2] = ((v & 0xFFFF) ^ 0x8000) - 0x8000
        assert np.array_equal(lg[a:a + 500_000], np.where(cnt.max(axis=1) > 0, cnt.argmax(axis=1), -1)), a
    del v, cnt
    # kNN colour smoothing over all 5M surfels (the oracle's brute force is O(N^2): properties instead)
    col0 = mg["col"][:, 1].copy()
    nbr = inst.flannKnnVoteSurfelMap(with_neighbours=True)
    assert nbr.shape == (g.count, 10)
    rng = np.random.RandomState(3)
    pick = rng.randint(0, g.count, 200)
    pos = mg["pc"][:, :3].astype(np.float64)
    for i in pick:                                                          # exact 10 nearest neighbours of sampled surfels against numpy
        d = np.sum((pos - pos[i]) ** 2, axis=1)
        ref = np.argpartition(d, 10)[:10]
        assert np.isclose(np.sort(d[ref])[-1], np.sort(d[nbr[i]])[-1], rtol=1e-6), i
        assert set(nbr[i].tolist()) == set(ref.tolist()) or np.isclose(np.sort(d[ref]), np.sort(d[nbr[i]]), rtol=1e-6).all()
    col1 = g.download()["col"][:, 1]
    palette = set(np.unique(col0).tolist()) | {float(0x717171), 0.0}
    assert set(np.unique(col1).tolist()) <= palette | set(np.unique(col0).tolist())   # smoothing only redistributes existing instance colours
    g.close(); o.close()


def _tracker_variants_equal(ifx, variants):
    from instancefusion_amd import synth

    W, H = 640, 480
    K = dict(fx=528.0, fy=528.0, cx=320.0, cy=240.0)
    st = synth.make_stream(8, W, H, noise=True, loop_len=90, **K)
    out = []
    for opts in variants:
        g = ifx.ElasticFusion(w=W, h=H, max_surfels=1_000_000, **K)
        for k, v in opts.items():
            g.set_option(k, v)
        poses, diags = [], []
        for i in range(8):
            poses.append(g.processFrame(st["rgb"][i], st["depth"][i]))
            diags.append(g.tracker_diag())   # after every frame: the run's diagnostics are written by whichever form ran its last iteration
        out.append((np.stack(poses), g.download(), np.stack(diags).view(np.uint32)))
        g.close()
    for v, other in zip(variants[1:], out[1:]):
        assert np.array_equal(out[0][0], other[0]), (variants[0], v)
        assert all(np.array_equal(out[0][1][k], other[1][k]) for k in MAP_KEYS), (variants[0], v)
        assert np.array_equal(out[0][2], other[2]), (variants[0], v, np.argwhere(out[0][2] != other[2]).tolist())   # every bit of every frame's diagnostics


def test_persistent_level_kernel_is_bit_identical(ifx):
    """All Gauss-Newton iterations of a pyramid level in one persistent launch with grid barriers (option gn_persist, a bit per level; k_gn_level): the same
    rows and the same exact sums as the two launches per iteration -- trajectories and maps bit-identical whichever levels use it (the default is the coarsest
    level only, where the meetings of 75 blocks cost less than launch boundaries).  A barrier that timed out would show up as a different
    pose, and as an error of ifx_sync."""
    big = 1 << 20   # (by default a level uses the kernel only while its grid has at most 128 blocks: lifted here so that every level really runs it)
    _tracker_variants_equal(ifx, [dict(gn_persist=0), dict(gn_persist=7, gn_persist_blocks=big), dict(gn_persist=4), dict(gn_persist=6, gn_persist_blocks=big),
                                  dict(gn_persist=5, gn_persist_blocks=big)])   # (5: a persistent level BEHIND two-launch iterations -- those keep round 3's last-block form)


def test_persistent_level_kernel_fallback_equals_two_launch_form(ifx):
    """A meeting of the persistent level kernel that does not happen must cost time, never the pose: with the test hooks `gn_fault` (block 1 never arrives at
    meeting number n) and `gn_spin_limit` (polls before a meeting gives up) every block leaves the level unpublished and the one-workgroup kernel enqueued behind
    the launch (k_gn_level_solo) re-runs it inside the same frame -- trajectory and map equal the two-launch form's bit for bit, and the fallback is counted
    (ifx_tracker_fallbacks), not raised as an error."""
    from instancefusion_amd import synth

    W, H = 640, 480
    K = dict(fx=528.0, fy=528.0, cx=320.0, cy=240.0)
    st = synth.make_stream(6, W, H, noise=True, loop_len=90, **K)
    out = []
    for opts in (dict(gn_persist=0), dict(gn_persist=4, gn_spin_limit=3000, gn_fault=3), dict(gn_persist=6, gn_persist_blocks=1 << 20, gn_spin_limit=3000, gn_fault=10)):
        g = ifx.ElasticFusion(w=W, h=H, max_surfels=1_000_000, **K)
        for k, v in opts.items():
            g.set_option(k, v)
        poses = np.stack([g.processFrame(st["rgb"][i], st["depth"][i]) for i in range(6)])
        fb = g.tracker_fallbacks()
        out.append((poses, g.download(), fb))
        g.close()
    assert out[0][2] == 0
    assert out[1][2] == 5, out[1][2]          # the coarsest level of every tracked frame (meeting 3 is its second iteration's first)
    assert out[2][2] >= 5, out[2][2]          # meeting 10 lies in the next level: that one falls back (and the run's abort word sends nothing else astray)
    for other in out[1:]:
        assert np.array_equal(out[0][0], other[0])
        assert all(np.array_equal(out[0][1][k], other[1][k]) for k in MAP_KEYS)


def test_gn_prologue_solve_is_bit_identical(ifx):
    """The 6x6 solve of a two-launch Gauss-Newton iteration in the prologue of EVERY block of the next iteration's first launch (option gn_prologue, default since
    round 4: no last-block ticket, no pose round trip through memory between the two launches; sums / residual totals / running increment double-buffered by iteration
    parity) against round 3's last-block form (gn_prologue = 0): the same totals give the same bits -- trajectories and maps identical, with and without the
    persistent kernel in front of the two-launch tail, for the tracker configurations that change the tail's length or the system (no pyramid, fast odometry,
    ICP only, photometric only with its pivoted solve)."""
    for extra in (dict(), dict(gn_persist=4), dict(pyramid=0), dict(fast_odom=1), dict(icp_weight_x1000=100000), dict(icp_weight_x1000=0)):
        _tracker_variants_equal(ifx, [dict(gn_prologue=0, **extra), dict(gn_prologue=1, **extra)])
    # the chain ends where a level's launches get too large for a solve in every block (default 2048 blocks: level 0 of a 1280x960 frame; here lowered so that
    # it ends after the coarsest level / after the two coarse levels of a 640x480 frame): its last iteration in the last-block form, the finer levels as in round 3
    _tracker_variants_equal(ifx, [dict(gn_prologue=0), dict(gn_prologue_blocks=200), dict(gn_prologue_blocks=600), dict(gn_prologue_blocks=200, gn_persist=4)])


@pytest.mark.parametrize("world,zero_dies,lazy_ids", [(2, 0, 0), (3, 0, 0), (2, 1, 0), (3, 1, 0), (2, -1, 0), (2, 30, 0), (3, 1, 1), (2, 30, 1)] +
                         [(2 + i % 3, 1000 + 29 * i, i % 2) for i in range(int(os.environ.get("IFX_SWEEP_SHARDED", "0")))])   # (IFX_SWEEP_SHARDED=N: other scenes / motions, 30 frames each; a one-off wider run)
def test_owner_sharded_map_emulated(ifx, small_stream, world, zero_dies, lazy_ids):
    """The spatially sharded map (ifx_config.n_ranks = G: every rank stores the surfels it owns, 1 / G of the map; key images
    MIN-reduced, winners' attributes SUM-merged between the eight phases of a frame) against one GPU: G handles in one process, the
    all-reduces done by hand.  Poses, prediction / index / id images and -- merged by creation number -- the whole map, bit for bit,
    over first-frame initialisation, an uploaded map, appended surfels, deletions and independent local compactions.
    zero_dies: the reference's "surfel 0" (id 0 = "no surfel": it occludes, but is never associated or voted for) is removed in the middle and the next live
    surfel takes its place (from then on IT is never associated: the measurement at its pixel makes a new surfel instead) -- on one GPU the lowest live slot
    (DevState::first_live), on the sharded map the lowest live creation number of ANY rank (MIN-reduced with the keys of exchanges 0 and 4).
    zero_dies = -1: the same with the rule switched off on the ranks (option own_first_live = 0, round 4's behaviour) -- the maps must then DIFFER: the scenario tests the rule.
    zero_dies = 30: no such scenario, but 30 frames instead of 8.
    lazy_ids = 1: option own_lazy_ids on the ranks -- exchange 4 carries the id keys of the sampled lattice only (asserted on the exchange table); the whole id image, completed
    on demand by an id render + one key exchange (ifx_owner_ids_begin / _resume), must equal the one a second set of ranks WITHOUT the option holds after the same frames."""
    import torch

    from instancefusion_amd import dist as ifd
    from instancefusion_amd import sharded, synth

    st = small_stream
    NF = 8
    src = list(range(NF))
    swept = zero_dies >= 1000
    if zero_dies == 30:   # a LONG life of the map (the stream forth and back): the clean pass's 20-frame age rule at work on shards whose view lists live several frames
        NF, zero_dies = 30, 0
        src = [(i % 18) if (i % 18) < 10 else 18 - (i % 18) for i in range(NF)]
    elif zero_dies >= 1000:   # another scene, another camera motion
        seed_, NF = zero_dies, 30
        zero_dies = 0
        src = list(range(NF))
        prof = ("still", "slow", "nominal", "fast", "jump", "spin", "dolly", "shake")[(seed_ // 29) % 8]
        st = synth.make_stream_from_poses(synth.trajectory_profile(prof, NF, seed_), synth.Scene(seed_), SMALL["w"], SMALL["h"], SMALL["fx"], SMALL["fy"], SMALL["cx"], SMALL["cy"], noise_seed=seed_ + 1)
    d_rgb = torch.from_numpy(st["rgb"][src]).cuda()
    d_dep = torch.from_numpy(st["depth"][src].view(np.int16)).cuda()
    one = ifx.ElasticFusion(**SMALL, max_surfels=400000)
    efs = [ifx.ElasticFusion(**SMALL, max_surfels=400000, n_ranks=world, rank=r) for r in range(world)]
    efs_whole = [ifx.ElasticFusion(**SMALL, max_surfels=400000, n_ranks=world, rank=r) for r in range(world)] if lazy_ids else []
    for e in efs + efs_whole:
        e.set_option("compact_divisor", 16 if e.cfgd["rank"] else 64)     # the ranks compact at different times: ids are creation numbers, nothing to agree on
        if zero_dies < 0:
            e.set_option("own_first_live", 0)
    for e in efs:
        e.set_option("own_lazy_ids", lazy_ids)
        e.set_option("own_key_rs", int(lazy_ids and world == 2))   # (with it: the index keys of exchanges 0 and 2 come back as creation numbers only, op 6)
    P_, L_ = SMALL["w"] * SMALL["h"], -(-SMALL["w"] // 10) * -(-SMALL["h"] // 10)
    poses = []
    for i in range(NF):
        if i == 4:   # an uploaded map in the middle: every rank is handed all rows and keeps its own
            m = one.download()
            conf0 = m["pc"][:, 3].copy()
            m["pc"][::2, 3] = 15.0
            if zero_dies:   # row 0 is marked for removal (copy_unstable.vert: colorTime.w == -1): this frame's clean removes it; and row 1 -- "surfel 0" from then on -- is
                # swapped for a surfel in the middle of the image that every frame so far updated: one that WOULD be associated again (the oracle says: at tick 8)
                q = (np.linalg.inv(poses[-1].astype(np.float64)) @ np.concatenate([m["pc"][:, :3], np.ones((len(m["pc"]), 1), np.float32)], 1).T).T
                u, v = SMALL["fx"] * q[:, 0] / q[:, 2] + SMALL["cx"], SMALL["fy"] * q[:, 1] / q[:, 2] + SMALL["cy"]
                ok = (m["tm"][:, 1] == m["tm"][:, 1].max()) & (q[:, 2] > 0) & (np.abs(u - SMALL["cx"]) < 40) & (np.abs(v - SMALL["cy"]) < 30)
                kz = int(np.argmax(np.where(ok, conf0, -1.0)))   # (the most often updated of them: about a quarter of the surfels in view are updated by any one frame)
                assert ok[kz] and kz > 1
                for k_ in MAP_KEYS:
                    m[k_][[1, kz]] = m[k_][[kz, 1]]
                m["tm"][0, 1] = -1.0
            one.upload(m); one.set_pose(poses[-1], one.tick); one.combined_predict(poses[-1], one.tick, one.tick)
            for e in efs + efs_whole:
                e.upload(m)
                e.set_pose(poses[-1], one.tick)
            own = ifd.owner_of(m["pc"][:, :3], world)
            assert [e.count for e in efs] == [int((own == r).sum()) for r in range(world)]
            sharded.emulate_owner_predict(efs)          # ElasticFusion::predict on the sharded map: local raster, exchange, owned winners, exchange, fill-in
            if lazy_ids:
                sharded.emulate_owner_predict(efs_whole)
        one.enqueue_frame_device(d_rgb[i].data_ptr(), d_dep[i].data_ptr(), i)
        sharded.emulate_owner_ranks(efs, d_rgb[i].data_ptr(), d_dep[i].data_ptr())
        poses.append(one.getCurrPose())
        if lazy_ids:
            sharded.emulate_owner_ranks(efs_whole, d_rgb[i].data_ptr(), d_dep[i].data_ptr())
            if i > 0:   # (the map's first frame draws no id image and exchanges the whole form)
                assert [(b, op) for _, b, op in sharded._exchange_spec(efs[0], 4)] == [((P_ + L_) * 8 + 8, 0)], i
                assert [(b, op) for _, b, op in sharded._exchange_spec(efs_whole[0], 4)] == [(P_ * 16 + 8, 0)], i
                assert [(b, op) for _, b, op in sharded._exchange_spec(efs[0], 2)] == [(P_ * 8 + 8, 6 if world == 2 else 0)], i
            if i > 0 and i % 3 != 1:   # (frames 1, 4, 7, ...: the sparse image is simply overwritten by the next frame)
                with pytest.raises(RuntimeError):
                    efs[0].image("ids_after")          # caller-driven exchanges and no ifx_owner_ids_begin: refused, not silently sparse
                sharded.emulate_owner_ids(efs)
                whole = efs_whole[0].image("ids_after")
                assert i < 5 or swept or (whole > 0).sum() > 1000, (i, int((whole > 0).sum()))   # (a floor of the committed scenario: populated from the uploaded map on, half of its surfels are stable)
                for e in efs + efs_whole[1:]:
                    assert np.array_equal(e.image("ids_after"), whole), (i, e.cfgd["rank"])
        if zero_dies < 0:
            continue
        for e in efs:
            assert np.array_equal(e.getCurrPose(), poses[-1], equal_nan=True), (i, e.cfgd["rank"])
        for name in ("pred_vertex", "pred_normal", "pred_image", "pred_time", "fill_vertex", "fill_image"):
            a = one.image(name)
            for e in efs:
                assert np.array_equal(e.image(name), a, equal_nan=a.dtype.kind == "f"), (i, name, e.cfgd["rank"])
    # the maps: shards merged by creation number == the unsharded map (whose creation numbers are 0..n-1 after the compaction of download())
    ref = one.download()
    parts = [(e.seq(), e.download()) for e in efs]
    seq = np.concatenate([p[0] for p in parts])
    order = np.argsort(seq, kind="stable")
    assert len(np.unique(seq)) == len(seq)
    if zero_dies < 0:   # without the rule the successor goes on being associated on the ranks: another map
        merged_tm = np.concatenate([p[1]["tm"] for p in parts])[order]
        assert merged_tm.shape != ref["tm"].shape or not np.array_equal(merged_tm, ref["tm"])
        for e in efs:
            e.close()
        one.close()
        return
    assert sum(len(p[0]) for p in parts) == ref["pc"].shape[0]
    if zero_dies:
        assert seq.min() > 0
        # the successor was last updated by the frame of the upload at the latest (never associated again), while surfels right behind it went on being updated
        assert ref["tm"][0, 1] <= 5, ref["tm"][0]
    for k in MAP_KEYS:
        merged = np.concatenate([p[1][k] for p in parts])[order]
        assert np.array_equal(merged, ref[k], equal_nan=True), k
    assert min(len(p[0]) for p in parts) > 0.5 * len(seq) / world          # every rank holds about 1 / G of the map
    # ownership is what the hash says, for created and uploaded surfels alike (by their current position for the ones that never moved)
    for e in efs + efs_whole:
        e.close()
    one.close()


@pytest.mark.parametrize("world,lazy_ids", [(2, 0), (3, 0), (2, 1), (3, 1)])
def test_owner_sharded_instance_emulated(ifx, small_stream, world, lazy_ids):
    """The instance layer on the spatially sharded map: whetherDoSegmentation sums (vote mass of the owned surfels summed
    across the ranks), segmentation calls with superpixels (partial boxes MIN / MAX-merged, model depth SUM-merged, votes and label scan on the
    owned surfels) and the eviction of a full instance table (per-instance max / sum of the vote counters merged) against one GPU: decisions,
    instance tables and -- merged by creation number -- votes and labels, bit for bit."""
    import torch

    from instancefusion_amd import sharded, synth

    st = small_stream
    NF = 10
    d_rgb = torch.from_numpy(st["rgb"][:NF]).cuda()
    d_dep = torch.from_numpy(st["depth"][:NF].view(np.int16)).cuda()
    one = ifx.ElasticFusion(**SMALL, max_surfels=400000)
    efs = [ifx.ElasticFusion(**SMALL, max_surfels=400000, n_ranks=world, rank=r) for r in range(world)]
    inst_one, insts = ifx.InstanceFusion(one), [ifx.InstanceFusion(e) for e in efs]
    for e in efs:
        e.set_option("own_lazy_ids", lazy_ids)   # (1: the frames exchange the sampled lattice's id keys; every segmentation call completes the image at an exchange point of its own)
        e.set_option("own_key_rs", lazy_ids)

    def merged(name_of):
        parts = [(e.seq(), name_of(e, x)) for e, x in zip(efs, insts)]
        seq = np.concatenate([p[0] for p in parts])
        return np.concatenate([p[1] for p in parts])[np.argsort(seq, kind="stable")]

    def check(tag):
        assert all(np.array_equal(x.getInstanceTable(), inst_one.getInstanceTable()) for x in insts), tag
        assert np.array_equal(merged(lambda e, x: e.download()["votes"]), one.download()["votes"]), tag
        assert np.array_equal(merged(lambda e, x: x.labels()), inst_one.labels()), tag

    calls = 0
    for i in range(NF):
        if i == 4:   # make the map stable (confidence 20): from here on the id image is populated and the masks find surfels to vote for
            m = one.download()
            m["pc"][:, 3] = 20.0
            pose = one.getCurrPose()
            one.upload(m); one.set_pose(pose, one.tick); one.combined_predict(pose, one.tick, one.tick)
            for e in efs:
                e.upload(m)
                e.set_pose(pose, one.tick)
            sharded.emulate_owner_predict(efs)
        one.enqueue_frame_device(d_rgb[i].data_ptr(), d_dep[i].data_ptr(), i)
        sharded.emulate_owner_ranks(efs, d_rgb[i].data_ptr(), d_dep[i].data_ptr())
        want = inst_one.whetherDoSegmentation(i)
        assert [x.whetherDoSegmentation(i) for x in insts] == [want] * world, i
        if i >= 2 and (want or i % 3 == 0):
            masks, cls = synth.canned_masks(st["obj"][i], st["scene"])
            if masks.shape[0]:
                inst_one.ProcessSegmentation(st["rgb"][i], st["depth"][i], masks, cls, i, superpixels=True)
                sharded.emulate_owner_segmentation(efs, st["rgb"][i], st["depth"][i], masks, cls, i, superpixels=True)
                calls += 1
                check(("call", i))
    assert calls >= 2 and (inst_one.labels() >= 0).sum() > 30       # (a sanity floor of the scenario, not a parity figure: 46 with the window loop as the reference's shaders run it, which removes more duplicates at 320 columns)
    # flannKnnVoteSurfelMap: exact 10-NN over every rank's surfels (exports all-gathered), the owned surfels recoloured
    inst_one.flannKnnVoteSurfelMap()
    sharded.emulate_owner_knn(efs)
    assert np.array_equal(merged(lambda e, x: e.download()["col"]), one.download()["col"])
    assert len(np.unique(one.download()["col"][:, 1])) >= 2      # (the default colour and at least one instance's: a sanity floor of the scenario)
    # a full table: new classes for every mask of every call until the twenty weakest instances are evicted (exchange points 3 and 1 again)
    i = NF - 1
    masks, cls = synth.canned_masks(st["obj"][i], st["scene"])
    nm = masks.shape[0]
    evicted = False
    for call in range(320):      # (as many calls as it takes to fill the 96 slots: a mask or two of the eight register per call on this young map)
        classes = (1 + (call * nm + np.arange(nm)) % 79).astype(np.int32)
        before = (inst_one.getInstanceTable() >= 0).sum()
        inst_one.ProcessSegmentation(st["rgb"][i], st["depth"][i], masks, classes, 200 + 3 * call)
        sharded.emulate_owner_segmentation(efs, st["rgb"][i], st["depth"][i], masks, classes, 200 + 3 * call, superpixels=False)
        evicted = evicted or (inst_one.getInstanceTable() >= 0).sum() < before
        if call % 16 == 15 or evicted:
            check(("eviction", call))
        if evicted:
            break
    assert evicted
    for e in efs:
        e.close()
    one.close()


@pytest.mark.timeout(1500)
@pytest.mark.parametrize("lazy_ids", [0, 1])
def test_config4_1280x960_20m_map_sharded_x4(ifx, lazy_ids):
    """BASELINE configuration 4 at its size: a 1280x960 stream into a 20M-surfel map spatially sharded over FOUR ranks (5M surfels each; the four
    handles live in one process on this GPU, the exchanges of a frame reduced by hand exactly as the collectives would) against ONE handle holding all
    20M surfels.  Over five frames with a segmentation call (superpixels) in between: poses, prediction / fill-in / id images bit for bit every frame,
    whetherDoSegmentation decisions, instance table, and at the end -- merged by creation number -- the whole 20M-surfel map, votes and labels."""
    import torch

    from instancefusion_amd import dist as ifd
    from instancefusion_amd import sharded, synth

    W, H, G, N, NF = 1280, 960, 4, 20_000_000, 5
    K = dict(fx=1056.0, fy=1056.0, cx=640.0, cy=480.0)
    st = synth.make_stream(NF + 1, W, H, noise=True, loop_len=90, **K)
    big = synth.make_map(N, st["scene"], st["poses_world"][0], 1000, fx=K["fx"], fy=K["fy"])
    d_rgb = torch.from_numpy(st["rgb"]).cuda()
    d_dep = torch.from_numpy(st["depth"].view(np.int16)).cuda()
    one = ifx.ElasticFusion(w=W, h=H, max_surfels=N + 3_000_000, **K)
    efs = [ifx.ElasticFusion(w=W, h=H, max_surfels=N // G + 2_500_000, n_ranks=G, rank=r, **K) for r in range(G)]
    inst_one, insts = ifx.InstanceFusion(one), [ifx.InstanceFusion(e) for e in efs]
    for e in efs:
        e.set_option("own_lazy_ids", lazy_ids)   # (1: exchange 4 carries [splat keys | the id keys of the 128 x 96 lattice | word]: 9.9 MB instead of 19.7 MB a frame)
        e.set_option("own_key_rs", lazy_ids)     # (and the index keys of exchanges 0 and 2 come back as creation numbers only)
    # frame 0 initialises the tracker's previous image; then the 20M map replaces the first-frame map on both sides
    one.enqueue_frame_device(d_rgb[0].data_ptr(), d_dep[0].data_ptr(), 0)
    sharded.emulate_owner_ranks(efs, d_rgb[0].data_ptr(), d_dep[0].data_ptr())
    one.upload(big); one.set_pose(st["poses"][0], 1000); one.combined_predict(st["poses"][0], 1000, 1000)
    own = ifd.owner_of(big["pc"][:, :3], G)
    for e in efs:
        e.upload(big); e.set_pose(st["poses"][0], 1000)
    assert [e.count for e in efs] == [int((own == r).sum()) for r in range(G)]
    assert min(e.count for e in efs) > 0.9 * N / G                         # the spatial hash balances: every rank holds about 5M surfels
    del big, own
    sharded.emulate_owner_predict(efs)
    for name in ("pred_vertex", "pred_normal", "pred_image"):
        a = one.image(name)
        assert all(np.array_equal(e.image(name), a) for e in efs), name     # the prediction of the 20M map itself
    seg_at = 3
    for i in range(1, NF + 1):
        one.enqueue_frame_device(d_rgb[i].data_ptr(), d_dep[i].data_ptr(), i)
        sharded.emulate_owner_ranks(efs, d_rgb[i].data_ptr(), d_dep[i].data_ptr())
        pose = one.getCurrPose()
        for e in efs:
            assert np.array_equal(e.getCurrPose(), pose), (i, e.cfgd["rank"])
        for name in ("pred_vertex", "pred_normal", "pred_image", "pred_time", "fill_vertex", "fill_image"):
            a = one.image(name)
            for e in efs:
                assert np.array_equal(e.image(name), a), (i, name, e.cfgd["rank"])
        want = inst_one.whetherDoSegmentation(100 + i)
        assert [x.whetherDoSegmentation(100 + i) for x in insts] == [want] * G, i
        assert [b for _, b, _ in sharded._exchange_spec(efs[0], 4)] == [(W * H + 128 * 96) * 8 + 8 if lazy_ids else W * H * 16 + 8]
        if i == seg_at:
            masks, cls = synth.canned_masks(st["obj"][i], st["scene"])
            assert masks.shape[0] > 0
            inst_one.ProcessSegmentation(st["rgb"][i], st["depth"][i], masks, cls, 100 + i, superpixels=True)
            sharded.emulate_owner_segmentation(efs, st["rgb"][i], st["depth"][i], masks, cls, 100 + i, superpixels=True)
            assert all(np.array_equal(x.getInstanceTable(), inst_one.getInstanceTable()) for x in insts)
    assert np.abs(one.getCurrPose() - st["poses"][NF]).max() < 0.05          # it tracked
    # labels, then the map: shards merged by creation number == the unsharded map
    lab_one = inst_one.labels()
    labs = [x.labels() for x in insts]
    seqs = [e.seq() for e in efs]
    seq = np.concatenate(seqs)
    order = np.argsort(seq, kind="stable")
    assert len(np.unique(seq)) == len(seq) == lab_one.shape[0]
    assert np.array_equal(np.concatenate(labs)[order], lab_one) and (lab_one >= 0).sum() > 1000
    del labs, lab_one
    ref = one.download()
    one.close()
    for k in MAP_KEYS:                                                       # one field at a time: 20M x 48 vote floats are 3.8 GB
        parts = []
        for e in efs:
            m = e.download()
            parts.append(m[k])
            del m
        merged = np.concatenate(parts)[order]
        del parts
        assert np.array_equal(merged, ref.pop(k)), k
        del merged
    for e in efs:
        e.close()


@pytest.mark.parametrize("ahead,lazy_ids", [(False, 0), (True, 0), (True, 1)])
def test_config5_two_streams_one_sharded_map(ifx, ahead, lazy_ids):
    """(ahead = True: rank k runs the tracker of camera k's NEXT frame on its third stream as soon as the camera's context is parked, under the other camera's map phases --
    ifx_owner_track_ahead -- and the frame commits the parked pose block instead of tracking: same poses, same map, and every tracked frame but the first is served that way.)
    BASELINE configuration 5 in small: K = 2 cameras (two stretches of the benchmark trajectory through the same scene) feed ONE map that is spatially
    sharded over G = 2 ranks.  Semantics of a frame set: the K frames are processed in camera order on the one map; every camera tracks against the
    prediction rendered at the end of its own last frame (camera contexts: ifx_camera_count / ifx_camera_select).  On the sharded side camera c is tracked by
    rank c ONLY (ifx_owner_set_tracking_rank: stream k on GPU k, no tracker collective), the pose block is handed to the other rank (exchange 310), and every
    rank runs the frame's map phases on its shard; camera 1 enters with an external pose (its extrinsic calibration: ifx_owner_set_frame_pose).  Against ONE
    handle that time-slices the two cameras over the whole map: every pose, the prediction after every frame and -- merged by creation number -- the map, bit for bit."""
    import torch

    from instancefusion_amd import sharded, synth

    K, G, NS = 2, 2, 7
    W, H = SMALL["w"], SMALL["h"]
    st = synth.make_stream(30, W, H, SMALL["fx"], SMALL["fy"], SMALL["cx"], SMALL["cy"], noise=True, loop_len=90)
    first = (0, 20)                                            # camera c sees frames first[c], first[c] + 1, ... of the loop
    d_rgb = torch.from_numpy(st["rgb"]).cuda()
    d_dep = torch.from_numpy(st["depth"].view(np.int16)).cuda()
    torch.cuda.synchronize()
    one = ifx.ElasticFusion(**SMALL, max_surfels=600000)
    efs = [ifx.ElasticFusion(**SMALL, max_surfels=600000, n_ranks=G, rank=r) for r in range(G)]
    for e in [one] + efs:
        e.camera_count(K)
    for e in efs:
        e.set_option("own_lazy_ids", lazy_ids)   # (a parked id image is a whole one: with the option every camera switch completes the image first -- one id exchange per switch)
    pose_b0 = st["poses"][first[1]].astype(np.float32)         # camera 1's pose in the map frame (= camera 0's first frame): given, not tracked
    for s_ in range(NS):
        for c in range(K):
            i = first[c] + s_
            ext = pose_b0 if (c == 1 and s_ == 0) else None
            one.camera_select(c)
            p1 = one.processFrame(st["rgb"][i], st["depth"][i], inPose=ext)
            if lazy_ids:
                sharded.emulate_owner_ids(efs)
            for e in efs:
                e.camera_select(c)
                e.owner_set_tracking_rank(c)                    # stream c is tracked on rank c only
                if ext is not None:
                    e.owner_set_frame_pose(ext)
            if ahead and (s_ > 0 or c > 0):                     # the camera whose frame was just processed is parked now: its next frame's tracker starts at once, on its rank
                cp, sp = (c - 1, s_) if c > 0 else (K - 1, s_ - 1)
                if sp + 1 < NS:
                    j = first[cp] + sp + 1
                    for e in efs:
                        e.owner_track_ahead(cp, cp, d_rgb[j].data_ptr(), d_dep[j].data_ptr())
            sharded.emulate_owner_ranks(efs, d_rgb[i].data_ptr(), d_dep[i].data_ptr())
            for e in efs:
                assert np.array_equal(e.getCurrPose(), p1), (s_, c, e.cfgd["rank"])
            for name in ("pred_vertex", "pred_normal", "pred_image", "fill_vertex"):   # camera c's prediction is reduced to the rank that tracks it (exchange op 5): checked there
                assert np.array_equal(efs[c].image(name), one.image(name)), (s_, c, name)
            if lazy_ids:
                sharded.emulate_owner_ids(efs)
            assert np.array_equal(efs[1 - c].image("ids_after"), efs[c].image("ids_after"))   # (the id image comes from the exchanged keys: everywhere)
    # both cameras tracked: their trajectories follow the ground truth of their stretch
    assert np.abs(p1 - st["poses"][first[1] + NS - 1]).max() < 0.03
    if ahead:   # every frame from the second set on took its pose from the run ahead (camera 0's first frame is the map's first; camera 1's entered with its extrinsic pose)
        assert [e.owner_track_ahead(-1, 0) for e in efs] == [NS - 1, NS - 1]
    else:
        assert [e.owner_track_ahead(-1, 0) for e in efs] == [0, 0]
    # A camera's prediction is reduced to its tracking rank ONLY (exchange 5, op 5): whoever else tried to track that camera's next frame would do so from partial sums and
    # broadcast the result.  The handles remember the root per camera and EVERY rank refuses alike -- the frame, and a run ahead
    j = first[K - 1] + NS
    for e in efs:   # (camera K - 1 is live, its prediction sits complete on rank K - 1 only)
        e.owner_set_tracking_rank(0)
        with pytest.raises(ifx.IfxError, match="reduced to rank"):
            e.owner_frame_phase(310, d_rgb[j].data_ptr(), d_dep[j].data_ptr())
        e.owner_set_tracking_rank(-1)
        with pytest.raises(ifx.IfxError, match="reduced to rank"):
            e.owner_frame_phase(0, d_rgb[j].data_ptr(), d_dep[j].data_ptr())      # (every rank tracks: the frame starts with phase 0)
        with pytest.raises(ifx.IfxError, match="reduced to rank"):
            e.owner_track_ahead(0, 1, d_rgb[j].data_ptr(), d_dep[j].data_ptr())   # camera 0 (parked): its prediction lives on rank 0
        e.owner_set_tracking_rank(K - 1)
    ref = one.download()
    parts = [(e.seq(), e.download()) for e in efs]
    seq = np.concatenate([p[0] for p in parts])
    order = np.argsort(seq, kind="stable")
    assert len(np.unique(seq)) == len(seq) == ref["pc"].shape[0]
    for k in MAP_KEYS:
        assert np.array_equal(np.concatenate([p[1][k] for p in parts])[order], ref[k]), k
    assert min(len(p[0]) for p in parts) > 0.3 * len(seq) / G
    for e in efs:
        e.close()
    one.close()


def test_camera_contexts_on_the_enqueue_path(ifx):
    """Camera contexts on an UNSHARDED handle fed through the enqueue-only entry (ifx_enqueue_frame_device: the call returns while the frame is still running, the
    camera switch that follows is enqueued behind it) against the same frames through the synchronous entry: every pose and the map, bit for bit."""
    import torch

    from instancefusion_amd import synth

    K, NS = 2, 6
    W, H = SMALL["w"], SMALL["h"]
    st = synth.make_stream(30, W, H, SMALL["fx"], SMALL["fy"], SMALL["cx"], SMALL["cy"], noise=True, loop_len=90)
    first = (0, 15)
    d_rgb = torch.from_numpy(st["rgb"]).cuda()
    d_dep = torch.from_numpy(st["depth"].view(np.int16)).cuda()
    torch.cuda.synchronize()
    outs = []
    for enqueue in (0, 1):
        g = ifx.ElasticFusion(**SMALL, max_surfels=600000)
        g.camera_count(K)
        poses = []
        for s_ in range(NS):
            for c in range(K):
                i = first[c] + s_
                g.camera_select(c)
                if s_ == 0 or not enqueue:   # (a camera's first frame: host entry in both runs -- camera 1 enters with its extrinsic pose)
                    g.processFrame(st["rgb"][i], st["depth"][i], inPose=(st["poses"][i].astype(np.float32) if (c == 1 and s_ == 0) else None))
                else:
                    g.enqueue_frame_device(d_rgb[i].data_ptr(), d_dep[i].data_ptr(), i)
                if not enqueue:
                    poses.append(g.getCurrPose())
        if enqueue:
            g.sync()
        traj = g.trajectory()
        m = g.download()
        outs.append((traj, m, poses))
        g.close()
    a, b = outs
    assert np.array_equal(a[0], b[0])
    assert np.array_equal(np.stack(a[2]), a[0])      # (the trajectory log is the sequence of the frames' poses)
    assert all(np.array_equal(a[1][k], b[1][k]) for k in MAP_KEYS)
    assert np.abs(a[0][-1] - st["poses"][first[1] + NS - 1]).max() < 0.05


@pytest.mark.parametrize("swap,side", [(1, 1), (0, 1), (1, 0)])
def test_config5_three_streams_runs_ahead_per_camera(ifx, swap, side):
    """K = 3 cameras into one sharded map in a world of one (the collectives inside the library), every camera tracked by the one rank: with the run-ahead schedule
    every camera has a run pending at any time -- pose block, event and frame slot parked per camera; the frame binds the run's slot instead of computing its frame
    side again; the run's frame side on the side stream, its tracker on the third -- and the camera switch moves the prediction / fill-in / id blocks by pointer.
    Against the same streams with every frame tracking inside itself: every pose, every prediction, the id image and the whole map, bit for bit; options cam_swap /
    cam_side off give the same again."""
    import torch

    from instancefusion_amd import sharded, synth

    K, NS = 3, 6
    W, H = SMALL["w"], SMALL["h"]
    st = synth.make_stream(40, W, H, SMALL["fx"], SMALL["fy"], SMALL["cx"], SMALL["cy"], noise=True, loop_len=90)
    first = (0, 12, 24)
    d_rgb = torch.from_numpy(st["rgb"]).cuda()
    d_dep = torch.from_numpy(st["depth"].view(np.int16)).cuda()
    torch.cuda.synchronize()
    outs = []
    for ahead in (0, 1):
        ef = ifx.ElasticFusion(**SMALL, max_surfels=600000, n_ranks=-1, rank=0)
        ef.set_option("cam_swap", swap)
        ef.set_option("cam_side", side)
        osh = sharded.OwnerShardedElasticFusion(ef, None)
        ef.camera_count(K)
        poses, preds, diags = [], [], []
        for s_ in range(NS):
            for c in range(K):
                i = first[c] + s_
                ef.camera_select(c)
                ef.owner_set_tracking_rank(0)
                if c > 0 and s_ == 0:
                    ef.owner_set_frame_pose(st["poses"][i].astype(np.float32))
                if ahead and (s_ > 0 or c > 0):   # the camera parked a moment ago: its next frame's tracker starts now
                    cp, sp = (c - 1, s_) if c > 0 else (K - 1, s_ - 1)
                    if sp + 1 < NS:
                        j = first[cp] + sp + 1
                        ef.owner_track_ahead(cp, 0, d_rgb[j].data_ptr(), d_dep[j].data_ptr())
                osh.process_frame_device(d_rgb[i].data_ptr(), d_dep[i].data_ptr())
                poses.append(ef.getCurrPose())
                if s_ > 0:
                    diags.append(ef.tracker_diag())   # (a frame served by a run ahead reports that run's residuals, not the previous camera's)
                if s_ in (1, NS - 1):
                    preds.append((ef.image("pred_vertex"), ef.image("pred_image"), ef.image("fill_vertex"), ef.image("ids_after")))
        served = ef.owner_track_ahead(-1, 0)
        order = np.argsort(ef.seq(), kind="stable")
        m = ef.download()
        outs.append((np.stack(poses), preds, {k: m[k][order] for k in MAP_KEYS}, served, np.stack(diags)))
        ef.close()
    a, b = outs
    assert np.array_equal(a[4], b[4]) and len(np.unique(a[4][:, 0])) > K
    assert a[3] == 0 and b[3] == K * (NS - 1)   # every frame from the second set on took its pose from a run ahead (first set: the map's first frame / the cameras' extrinsic poses)
    assert np.array_equal(a[0], b[0])
    for pa, pb in zip(a[1], b[1]):
        assert all(np.array_equal(x, y) for x, y in zip(pa, pb))
    assert all(np.array_equal(a[2][k], b[2][k]) for k in MAP_KEYS)
    assert np.abs(a[0][-1] - st["poses"][first[K - 1] + NS - 1]).max() < 0.05


@pytest.mark.timeout(3000)
def test_config5_8_streams_50m_map_sharded_x8(ifx):
    """BASELINE configuration 5 AT ITS SIZE, emulated in one process: K = 8 concurrent 640x480 streams (eight stretches of the benchmark trajectory through the same
    scene) into ONE 50M-surfel map that is spatially sharded over G = 8 ranks of ~6.25M surfels -- eight owner handles on this GPU, the collectives done by hand exactly
    as ifx_comm.hip enqueues them (incl. the camera-indexed reduction: camera k's prediction goes to rank k only).  Camera k is tracked by rank k alone and its pose
    block broadcast; cameras 1..7 enter with their extrinsic pose.  Against ONE handle holding all 50M surfels that time-slices the eight cameras: every pose on
    every rank, the prediction after every frame on the rank that consumes it, the whetherDoSegmentation decisions, a segmentation call with superpixels (instance
    table), and at the end -- merged by creation number, one field at a time -- labels and the whole map, votes included, bit for bit."""
    import gc

    import torch

    from instancefusion_amd import dist as ifd
    from instancefusion_amd import sharded, synth

    W, H, K_, G, N, NS = 640, 480, 8, 8, 50_000_000, 2
    Kc = dict(fx=528.0, fy=528.0, cx=320.0, cy=240.0)
    first = [10 * c for c in range(K_)]                        # camera c sees frames first[c] + 1, first[c] + 2, ... of the 90-frame loop
    st = synth.make_stream(first[-1] + NS + 2, W, H, noise=True, loop_len=90, **Kc)
    big = synth.make_map(N, st["scene"], st["poses_world"][0], 1000)
    d_rgb = torch.from_numpy(st["rgb"]).cuda()
    d_dep = torch.from_numpy(st["depth"].view(np.int16)).cuda()
    one = ifx.ElasticFusion(w=W, h=H, max_surfels=N + 2_000_000, **Kc)
    efs = [ifx.ElasticFusion(w=W, h=H, max_surfels=N // G + 1_500_000, n_ranks=G, rank=r, **Kc) for r in range(G)]
    inst_one, insts = ifx.InstanceFusion(one), [ifx.InstanceFusion(e) for e in efs]
    for e in [one] + efs:
        e.camera_count(K_)
    # camera 0's frame 0 initialises the tracker's previous image; then the 50M map replaces the first-frame map on both sides
    one.enqueue_frame_device(d_rgb[0].data_ptr(), d_dep[0].data_ptr(), 0)
    sharded.emulate_owner_ranks(efs, d_rgb[0].data_ptr(), d_dep[0].data_ptr())
    one.upload(big); one.set_pose(st["poses"][0], 1000); one.combined_predict(st["poses"][0], 1000, 1000)
    own = ifd.owner_of(big["pc"][:, :3], G)
    for e in efs:
        e.upload(big); e.set_pose(st["poses"][0], 1000)
    counts = [e.count for e in efs]
    assert counts == [int((own == r).sum()) for r in range(G)]
    assert min(counts) > 0.9 * N / G and max(counts) < 1.1 * N / G      # the spatial hash balances: every rank holds about 6.25M surfels
    del big, own
    gc.collect()
    sharded.emulate_owner_predict(efs)
    assert all(np.array_equal(e.image("pred_vertex"), one.image("pred_vertex")) for e in efs)   # the prediction of the 50M map itself
    seg_done = False
    for s_ in range(NS):
        for c in range(K_):
            i = first[c] + 1 + s_
            ext = st["poses"][i].astype(np.float32) if (c > 0 and s_ == 0) else None   # a camera enters with its extrinsic calibration, then tracks
            one.camera_select(c)
            p1 = one.processFrame(st["rgb"][i], st["depth"][i], inPose=ext)
            for e in efs:
                e.camera_select(c)
                e.owner_set_tracking_rank(c)                    # stream c is tracked on rank c only
                if ext is not None:
                    e.owner_set_frame_pose(ext)
            sharded.emulate_owner_ranks(efs, d_rgb[i].data_ptr(), d_dep[i].data_ptr())
            for e in efs:
                assert np.array_equal(e.getCurrPose(), p1), (s_, c, e.cfgd["rank"])
            for name in ("pred_vertex", "pred_normal", "pred_image", "pred_time", "fill_vertex", "fill_image"):
                assert np.array_equal(efs[c].image(name), one.image(name)), (s_, c, name)
            want = inst_one.whetherDoSegmentation(100 + 8 * s_ + c)
            assert [x.whetherDoSegmentation(100 + 8 * s_ + c) for x in insts] == [want] * G, (s_, c)
            if s_ == 1 and c == 3 and not seg_done:              # one segmentation call, on camera 3's frame
                masks, cls = synth.canned_masks(st["obj"][i], st["scene"])
                assert masks.shape[0] > 0
                inst_one.ProcessSegmentation(st["rgb"][i], st["depth"][i], masks, cls, 100 + 8 * s_ + c, superpixels=True)
                sharded.emulate_owner_segmentation(efs, st["rgb"][i], st["depth"][i], masks, cls, 100 + 8 * s_ + c, superpixels=True)
                assert all(np.array_equal(x.getInstanceTable(), inst_one.getInstanceTable()) for x in insts)
                seg_done = True
            if s_ == NS - 1:
                assert np.abs(p1 - st["poses"][i]).max() < 0.05, c       # every camera tracked its stretch
    assert seg_done
    # labels, then the map: shards merged by creation number == the unsharded map
    lab_one = inst_one.labels()
    labs = np.concatenate([x.labels() for x in insts])
    seq = np.concatenate([e.seq() for e in efs])
    order = np.argsort(seq, kind="stable")
    assert len(np.unique(seq)) == len(seq) == lab_one.shape[0]
    assert np.array_equal(labs[order], lab_one) and (lab_one >= 0).sum() > 1000
    inv = np.empty(len(order), np.int64)
    inv[order] = np.arange(len(order))                                       # row j of the concatenated shards is row inv[j] of the unsharded map
    bounds = np.cumsum([0] + [e.count for e in efs])
    del labs, lab_one, seq, order
    gc.collect()
    for k in MAP_KEYS:                                                       # one field at a time, one shard at a time: 50M x 48 vote floats are 9.6 GB
        ref = one.download(fields=(k,))[k]
        for r, e in enumerate(efs):
            part = e.download(fields=(k,))[k]
            assert part.shape[0] == bounds[r + 1] - bounds[r]
            assert np.array_equal(part, ref[inv[bounds[r]:bounds[r + 1]]]), (k, r)
            del part
        del ref
        gc.collect()
    for e in efs:
        e.close()
    one.close()


@pytest.mark.parametrize("earlyz,lds", [(1, 0), (0, 0), (0, 1)])
def test_view_list_path_equals_per_pass_culls(ifx, earlyz, lds):
    """The frame path through the cached view list (one scan of the store per ~6 frames, list-driven index / clean / raster passes,
    flattened rasteriser, early-z) against the round-1 path (three culls over all slots per frame): poses, maps, id images and
    labels bit for bit, over enough frames for several list rebuilds, appended surfels, deletions and a lazy compaction."""
    from instancefusion_amd import synth

    W, H = 640, 480
    K = dict(fx=528.0, fy=528.0, cx=320.0, cy=240.0)
    NF = 26
    st = synth.make_stream(NF, W, H, noise=True, loop_len=90, **K)
    big = synth.make_map(400_000, st["scene"], st["poses_world"][0], 1000)

    def run(view):
        g = ifx.ElasticFusion(w=W, h=H, max_surfels=1_600_000, **K)
        g.set_option("view_list", view)
        g.set_option("raster_earlyz", earlyz)
        g.set_option("raster_lds", lds)                # per-wave depth test in LDS in front of the global atomics
        # Compactions inside the run, at the SAME frames on both paths: the id images are compared as slot numbers, and WHEN the lazy rule (tombstones > slots / divisor)
        # fires depends on when tombstones are written -- the view-list path writes those of slots no list holds at its next scan, up to VL_MAX_AGE frames after the
        # per-pass path (results equal either way: the lazy rule itself runs against the oracle in test_long_run_with_calls_on_the_resident_frame_path).
        g.set_option("compact_divisor", 1)
        g.processFrame(st["rgb"][0], st["depth"][0])
        g.upload(big); g.set_pose(st["poses"][0], 1000); g.combined_predict(st["poses"][0], 1000, 1000)
        inst = ifx.InstanceFusion(g)
        poses, ids = [], []
        for i in range(1, NF):
            poses.append(g.processFrame(st["rgb"][i], st["depth"][i]))
            if i in (9, 17):
                g.compact()
            if i % 6 == 0:
                ids.append(g.image("ids_after").copy())
            if i == 12:
                masks, cls = synth.canned_masks(st["obj"][i], st["scene"])
                inst.ProcessSegmentation(st["rgb"][i], st["depth"][i], masks, cls, 200, superpixels=True)
        slots, live = g.slots, g.count
        lab = inst.labels()
        m = g.download()
        g.close()
        return np.stack(poses), ids, lab, m, slots, live

    a, b = run(1), run(0)
    assert np.array_equal(a[0], b[0])
    assert all(np.array_equal(x, y) for x, y in zip(a[1], b[1]))
    assert np.array_equal(a[2], b[2]) and a[5] == b[5]
    assert all(np.array_equal(a[3][k], b[3][k]) for k in MAP_KEYS)
    assert a[3]["pc"].shape[0] > 400_000 and (a[2] >= 0).sum() > 100


def test_view_list_survives_a_full_map(ifx, small_stream):
    """A store that fills up while the cached view list is on: new surfels that do not fit get NO list position (an advisor finding of
    round 2: reserved-but-unwritten entries were dereferenced by the list walkers), the frames report IFX_E_CAPACITY, and the handle
    keeps working -- ids and list lengths stay inside the store, the map downloads finite, a compaction + more frames run."""
    st = small_stream
    cap = 30_000
    g = ifx.ElasticFusion(**SMALL, max_surfels=cap)
    full = 0
    for rep in range(3):
        for i in range(10):
            try:
                g.processFrame(st["rgb"][i], st["depth"][i], inPose=st["poses"][i] if rep else None)
            except ifx.IfxError as e:
                assert "capacity" in str(e)
                full += 1
            vs = g.view_list_stats()
            assert 0 <= vs["window"] <= cap and 0 <= vs["outside"] <= cap, vs
            ids = g.image("ids_after")
            assert ids.min() >= 0 and ids.max() < cap
    assert full > 0
    with pytest.raises(ifx.IfxError, match="capacity"):    # the flag is sticky until a map is uploaded: whole-map consumers refuse too
        g.download()
    # an uploaded map clears it; the handle tracks and fuses again
    from instancefusion_amd import synth
    small = synth.make_map(5_000, st["scene"], st["poses_world"][0], 1000)
    g.upload(small); g.set_pose(st["poses"][0], 1000)
    for i in range(1, 4):
        g.processFrame(st["rgb"][i], st["depth"][i], inPose=st["poses"][i])
    m = g.download()
    assert 5_000 < m["pc"].shape[0] <= cap and np.isfinite(m["pc"]).all() and np.isfinite(m["nr"]).all()
    g.close()


def test_reference_passes_toggle_keeps_the_view_list_honest(ifx, orc, small_stream):
    """Switching `reference_passes` on takes the frames off the view-list path; switching it back must not let a device-side "valid"
    describe a list the host never built (advisor finding of round 2: the passes then walked an almost empty list).  Against the
    oracle frame by frame across both switches: poses, map sizes and id images equal."""
    st = small_stream
    g = ifx.ElasticFusion(**SMALL, max_surfels=400000)
    g.set_option("compact_every_frame", 0)
    o = orc.Oracle(**SMALL, max_surfels=400000)
    for i in range(10):
        if i == 3:
            g.set_option("reference_passes", 1)
        if i == 6:
            g.set_option("reference_passes", 0)
        pg = g.processFrame(st["rgb"][i], st["depth"][i]); po = o.process_frame(st["rgb"][i], st["depth"][i])
        assert_pose_equal(pg, po, f"frame {i}")
        assert g.count == o.count, i
    mg, mo = g.download(), o.download()
    for k in MAP_KEYS:
        assert np.array_equal(mg[k], mo[k]), k
    g.close(); o.close()


# ---------------------------------------------------------------- a20, a21: superpixel refinement
def _slic_cases(gputest_pair):
    from instancefusion_amd import synth

    c1, d1, c2, d2 = gputest_pair
    st = synth.make_stream(2, 640, 480, 528.0, 528.0, 320.0, 240.0, noise=True)
    return {"c1": (c1, d1 // 5), "c2": (c2, d2 // 5), "synth": (st["rgb"][1], st["depth"][1])}


def test_superpixel_stages_exact(ifx, orc, gputest_pair):
    """SLIC labels equal the labels of the reference's own per-pixel functions (golden fixture) and the
    oracle's; re-clustered labels, merged region ids, the 30-float statistics table and the filtered
    masks equal the oracle's bit for bit (fixed-point sums make the statistics order-independent)."""
    import os

    gold = dict(np.load(os.path.join(os.path.dirname(__file__), "golden", "slic_ref.npz")))
    rng = np.random.RandomState(11)
    for name, (rgb, dep) in _slic_cases(gputest_pair).items():
        h, w = rgb.shape[:2]
        K = dict(fx=528.0 * w / 640, fy=528.0 * w / 640, cx=w / 2.0, cy=h / 2.0)
        g = ifx.ElasticFusion(w=w, h=h, max_surfels=1000, **K)
        o = orc.Oracle(w=w, h=h, max_surfels=1000, **K)
        inst = ifx.InstanceFusion(g)
        seg_g, n_g = inst.gSLICrInterface(rgb)
        seg_o, n_o = o.slic_segment(rgb)
        assert n_g == n_o == (w // 16) * (h // 16)
        assert np.array_equal(seg_g, gold[name + "_ref_labels"].astype(np.int32)), name
        assert np.array_equal(seg_g, seg_o), name
        s_g, f_g, i_g = inst.mergeSuperPixel(dep, seg_g)
        s_o, f_o, i_o = o.merge_superpixels(dep, seg_o)
        assert np.array_equal(s_g, s_o) and np.array_equal(f_g, f_o), name
        assert nan_equal(i_g, i_o), name
        assert np.array_equal(f_g, gold[name + "_merge_final"].astype(np.int32)), name
        # twice on the same handle: buffers are reused, result unchanged (determinism of the atomics)
        s_g2, f_g2, i_g2 = inst.mergeSuperPixel(dep, seg_g)
        assert np.array_equal(f_g2, f_g) and nan_equal(i_g2, i_g)
        masks = np.zeros((5, h, w), np.uint8)
        masks[0, h // 5: h // 2, w // 4: w // 2] = 255
        masks[1, h // 2:, : w // 3] = 255
        masks[2] = (rng.rand(h, w) < 0.8) * 255
        masks[3] = 255
        assert np.array_equal(inst.maskSuperPixelFilter_OverSeg(f_g, masks), o.mask_superpixel_filter(f_o, masks)), name
        # ragged labelling: invalid ids and ids >= spNum are dropped by the filter on both sides
        f_bad = f_g.copy(); f_bad[::7, ::5] = -1; f_bad[3::11, 2::9] = 10 ** 6
        assert np.array_equal(inst.maskSuperPixelFilter_OverSeg(f_bad, masks), o.mask_superpixel_filter(f_bad, masks)), name
        # depth holes / all-zero depth: nothing survives
        s0, f0, _ = inst.mergeSuperPixel(np.zeros_like(dep), seg_g)
        assert (s0 == -1).all() and (f0 == -1).all()
        g.close(); o.close()


def test_segmentation_with_superpixels_exact(ifx, orc, small_stream):
    from instancefusion_amd import synth

    st = small_stream
    g = ifx.ElasticFusion(**SMALL, max_surfels=400000)
    g.set_option("compact_every_frame", 1)     # slot ids == the oracle's compacted indices
    o = orc.Oracle(**SMALL, max_surfels=400000)
    inst = ifx.InstanceFusion(g)
    for i in range(6):
        po = o.process_frame(st["rgb"][i], st["depth"][i])
        g.processFrame(st["rgb"][i], st["depth"][i])
    m = o.download(); m["pc"][:, 3] = 20.0
    o.upload(m); g.upload(m)
    pose = po
    o.set_pose(pose, o.tick); g.set_pose(pose, o.tick)      # same previous pose -> same fusion weight
    g.processFrame(st["rgb"][5], st["depth"][5], inPose=pose); o.process_frame(st["rgb"][5], st["depth"][5], in_pose=pose)
    assert g.count == o.count and np.array_equal(g.image("ids_after"), o.image("ids_after"))
    masks, cls = synth.canned_masks(st["obj"][5], st["scene"])
    for frame in (50, 60):
        inst.ProcessSegmentation(st["rgb"][5], st["depth"][5], masks, cls, frame, superpixels=True)
        o.process_segmentation(st["rgb"][5], st["depth"][5], masks, cls, frame, flags=2)
        assert np.array_equal(inst.getInstanceTable(), o.instance_table())
        assert np.array_equal(inst.labels(), o.labels())
        assert np.array_equal(g.download()["votes"], o.download()["votes"])
    assert (o.labels() >= 0).sum() > 100
    g.close(); o.close()


# ---------------------------------------------------------------- frame look-ahead (side stream) must not change results
@pytest.mark.parametrize("flann", [False, True])
def test_lookahead_equivalence(ifx, small_stream, flann):
    """Every way of feeding the frames -- one stream, two streams, the next frame announced (its tracker enqueued ahead, a segmentation call then runs BESIDE it on the third
    stream), prefetched, announced wrongly, with a compaction before every frame -- gives the same trajectory, map, id image and decisions; segmentation calls with
    superpixels (and, flann: the kNN smoothing, whose forced view-list scan then runs beside the tracker too) at frames where the map has stable surfels."""
    import torch

    from instancefusion_amd import synth

    n = 14
    st = synth.make_stream(n, SMALL["w"], SMALL["h"], SMALL["fx"], SMALL["fy"], SMALL["cx"], SMALL["cy"], noise=True)
    d_rgb = torch.from_numpy(st["rgb"][:n].copy()).cuda()
    d_dep = torch.from_numpy(st["depth"][:n].view(np.int16).copy()).cuda()
    torch.cuda.synchronize()

    from instancefusion_amd import synth

    def run(mode):
        seg = []
        g = ifx.ElasticFusion(**SMALL, max_surfels=400000, confidence=2.0)
        inst = ifx.InstanceFusion(g)
        if mode == "single":
            g.set_option("two_streams", 0)
        if mode == "hint_no_track_ahead":
            g.set_option("track_ahead", 0)
        if mode == "hint_housekeeping":
            g.set_option("compact_divisor", 1 << 30)   # compaction before every frame that follows one with a deletion
        if mode == "hint_result_launch":
            g.set_option("fold_result", 0)             # the frame result by a launch of its own instead of the last block of the prediction's resolve
        for i in range(n):
            if mode.startswith("hint") and i + 1 < n:
                g.hint_next_frame_device(d_rgb[i + 1].data_ptr(), d_dep[i + 1].data_ptr())
            g.enqueue_frame_device(d_rgb[i].data_ptr(), d_dep[i].data_ptr(), i)
            if mode == "prefetch" and i + 1 < n:
                g.prefetch_frame_device(d_rgb[i + 1].data_ptr(), d_dep[i + 1].data_ptr())
            if mode == "wrong_hint" and i + 1 < n:   # a look-ahead that does not come true is recomputed
                g.prefetch_frame_device(d_rgb[0].data_ptr(), d_dep[0].data_ptr())
            seg.append(inst.whetherDoSegmentation(10 + i))   # host decision between frames, as in the reference's main loop
            if i in (5, 9, 12):   # and segmentation calls while the next frame's tracker may already be queued
                mk, cl = synth.canned_masks(st["obj"][i], st["scene"])
                res = mode == "hint_resident"   # (the frame's images from their frame slot instead of host copies)
                inst.ProcessSegmentation(None if res else st["rgb"][i], None if res else st["depth"][i], mk, cl, 10 + i, superpixels=True, isflann=flann)
        g.sync()
        traj, m, ids, lab = g.trajectory(), g.download(), g.image("ids_after"), inst.labels()
        g.close()
        return traj, m, ids, seg, lab

    ref = run("single")
    assert (ref[4] >= 0).sum() > 100   # the calls labelled something
    for mode in ("plain", "hint", "hint_resident", "hint_no_track_ahead", "prefetch", "wrong_hint", "hint_housekeeping", "hint_result_launch"):
        t, m, ids, seg, lab = run(mode)
        assert np.array_equal(lab, ref[4]), mode
        assert seg == ref[3], mode
        assert np.array_equal(t, ref[0]), mode
        assert all(np.array_equal(m[k], ref[1][k]) for k in MAP_KEYS), mode
        if mode != "hint_housekeeping":      # compaction renumbers the slots the id image refers to
            assert np.array_equal(ids, ref[2]), mode
        else:
            assert np.array_equal(ids > 0, ref[2] > 0)
    # and the host-buffer entry point gives the same trajectory
    if not flann:
        g = ifx.ElasticFusion(**SMALL, max_surfels=400000, confidence=2.0)
        poses = np.stack([g.processFrame(st["rgb"][i], st["depth"][i]) for i in range(n)])
        g.close()
        assert np.array_equal(poses, ref[0][:n])


def test_superpixels_ahead_of_a_call_change_nothing(ifx):
    """When whetherDoSegmentation's cadence announces a call for the next frame and that frame is announced too, its SLIC + superpixel merge run ahead on the side stream
    (ifx_superpixel_ahead_stats) and the call waits for one event instead.  Here with option slic_ahead = 2 (a run ahead for EVERY announced frame): calls that use
    such a run, runs whose call never comes, calls whose frame had none -- the same decisions, map, votes, labels and id image as with the look-ahead switched off.
    (The cadence-driven default is what bench.py's fast-cadence leg runs: its JSON carries runs / used_by_a_call.)"""
    import torch

    from instancefusion_amd import synth

    n = 16
    st = synth.make_stream(n, SMALL["w"], SMALL["h"], SMALL["fx"], SMALL["fy"], SMALL["cx"], SMALL["cy"], noise=True)
    d_rgb = torch.from_numpy(st["rgb"][:n].copy()).cuda()
    d_dep = torch.from_numpy(st["depth"][:n].view(np.int16).copy()).cuda()
    torch.cuda.synchronize()
    outs = []
    for ahead in (0, 2):
        g = ifx.ElasticFusion(**SMALL, max_surfels=400000, confidence=2.0)
        inst = ifx.InstanceFusion(g)
        g.set_option("slic_ahead", ahead)
        fired = []
        for i in range(n):
            if i == 8:                    # frame 9 is announced WRONGLY (another frame's images): the superpixels run ahead on those must not serve frame 9's call
                g.hint_next_frame_device(d_rgb[0].data_ptr(), d_dep[0].data_ptr())
            elif i + 1 < n and i != 10:   # (frame 11 is not announced: its call finds no run ahead)
                g.hint_next_frame_device(d_rgb[i + 1].data_ptr(), d_dep[i + 1].data_ptr())
            g.enqueue_frame_device(d_rgb[i].data_ptr(), d_dep[i].data_ptr(), i)
            fired.append(inst.whetherDoSegmentation(-(1 << 30)))   # (a frame number that never fires: with slic_ahead = 2 every decision point starts a run for the announced frame)
            if i in (5, 7, 9, 11, 12):    # 5, 7: served by a run ahead; 9: its run was for the wrong images; 11: not announced; 12: its run was displaced by 11's in-call superpixels
                mk, cl = synth.canned_masks(st["obj"][i], st["scene"])
                inst.ProcessSegmentation(None, None, mk, cl, 10 + i, superpixels=True)
        g.sync()
        stats = g.superpixel_ahead_stats()
        outs.append((fired, g.trajectory(), g.download(), inst.labels(), g.image("ids_after"), stats))
        g.close()
    a, b = outs
    assert a[5]["runs"] == 0 and a[5]["used"] == 0
    assert b[5]["runs"] >= 5 and b[5]["used"] == 2, b[5]
    assert a[0] == b[0]
    assert np.array_equal(a[1], b[1]) and np.array_equal(a[3], b[3]) and np.array_equal(a[4], b[4])
    assert (a[3] >= 0).sum() > 100
    assert all(np.array_equal(a[2][k], b[2][k]) for k in a[2]), [k for k in a[2] if not np.array_equal(a[2][k], b[2][k])]


def test_host_entry_returning_with_the_pose_changes_nothing(ifx, small_stream):
    """Option host_entry_async: ifx_process_frame returns when the frame's pose is known (read back right behind the tracker) and the map passes finish under the
    caller's copy of the next frame; the frame's housekeeping decision moves to the start of the next call.  A loop of frames only, with compactions forced often:
    the same poses from every call, the same map and the same coverage of the id image as with the fully synchronous entry (the slot numbers in the last id image may
    differ: the last frame's compaction is still pending in the one mode and done in the other)."""
    st = small_stream
    outs = []
    order = list(range(10)) + list(range(8, -1, -1))
    for mode in (0, 1, 2, 3):   # 2: the synchronous entry with every next frame announced from host memory (ifx_hint_next_frame); 3: the same on the early-return entry
        g = ifx.ElasticFusion(**SMALL, max_surfels=400000, confidence=2.0)
        g.set_option("host_entry_async", mode & 1)
        g.set_option("compact_divisor", 64)
        poses = []
        for j, i in enumerate(order):
            if mode >= 2 and j + 1 < len(order):
                g.hint_next_frame(st["rgb"][order[j + 1]], st["depth"][order[j + 1]])
            poses.append(g.processFrame(st["rgb"][i], st["depth"][i]))
        la = g.lookahead_stats()
        if mode == 2:   # every frame but the first two came prepared AND tracked ahead (frame 1 is announced during the map's first frame, which has no tracker to park behind)
            assert la["host_hinted"] == len(order) - 1 and la["side_prepared"] == len(order) - 1 and la["tracked_ahead"] >= len(order) - 2, la
        elif mode < 2:
            assert la["host_hinted"] == 0 and la["tracked_ahead"] == 0, la
        ids, slots, m = g.image("ids_after"), g.slots, g.download()
        outs.append((np.stack(poses), ids, slots, m))
        g.close()
    a = outs[0]
    for b in outs[1:]:
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1] > 0, b[1] > 0)
        assert all(np.array_equal(a[3][k], b[3][k]) for k in MAP_KEYS)
    assert a[3]["pc"].shape[0] > 50000


def test_segmentation_call_on_the_resident_frame(ifx):
    """ifx_process_segmentation with rgb = depth = NULL refines the masks on the frame most recently processed, still resident in its frame slot: the same
    tables, votes, labels and colours as with the host copies of that frame handed over (the reference's signature)."""
    from instancefusion_amd import synth

    W, H = 320, 240
    K = dict(fx=264.0, fy=264.0, cx=160.0, cy=120.0)
    st = synth.make_stream(16, W, H, noise=True, loop_len=90, **K)
    outs = []
    for resident in (False, True):
        g = ifx.ElasticFusion(w=W, h=H, max_surfels=400_000, confidence=2.0, **K)
        inst = ifx.InstanceFusion(g)
        for i in range(16):
            g.processFrame(st["rgb"][i], st["depth"][i])
            if i in (7, 11, 15):
                mk, cl = synth.canned_masks(st["obj"][i], st["scene"])
                inst.ProcessSegmentation(None if resident else st["rgb"][i], None if resident else st["depth"][i], mk, cl, i + 1, superpixels=True)
        outs.append((g.download(), inst.labels(), inst.getInstanceTable()))
        g.close()
    assert all(np.array_equal(outs[0][0][k], outs[1][0][k]) for k in MAP_KEYS)
    assert np.array_equal(outs[0][1], outs[1][1]) and (outs[0][1] >= 0).any()
    assert np.array_equal(np.asarray(outs[0][2]), np.asarray(outs[1][2]))


# ---------------------------------------------------------------- a19: flood fill of the masks on the device
def test_flood_fill_exact(ifx, orc):
    """The device label propagation (label = earliest pixel that reaches me) against the oracle's sequential
    breadth-first fill: shapes that need many tile-to-tile hand-offs (spiral), one-way edges (depth beyond 4 m where
    the threshold depends on the source pixel), several regions per mask, holes in the model depth, skipped masks."""
    w, h = 320, 240
    K = dict(fx=264.0, fy=264.0, cx=160.0, cy=120.0)
    g = ifx.ElasticFusion(w=w, h=h, max_surfels=1000, **K)
    o = orc.Oracle(w=w, h=h, max_surfels=1000, **K)
    inst = ifx.InstanceFusion(g)
    rng = np.random.RandomState(4)
    yy, xx = np.mgrid[0:h, 0:w]
    depth = (2000 + 3 * xx + 2 * yy + rng.randint(-20, 21, (h, w))).astype(np.uint16)
    depth[rng.rand(h, w) < 0.02] = 0                       # holes
    far = (4500 + 25 * xx + rng.randint(-150, 151, (h, w))).astype(np.uint16)   # 4.5 .. 12.5 m: thresholds 87 .. 420, one-way edges
    masks = np.zeros((7, h, w), np.uint8)
    # 0: spiral corridor, 3 px wide
    sp = np.zeros((h, w), bool)
    l, t, r, b = 10, 10, w - 10, h - 10
    while r - l > 16 and b - t > 16:
        sp[t:t + 3, l:r] = True; sp[t:b, r - 3:r] = True; sp[b - 3:b, l + 8:r] = True; sp[t + 8:b, l + 8:l + 11] = True
        l += 8; t += 8; r -= 8; b -= 8
    masks[0][sp] = 255
    masks[1, 40:200, 50:280] = 255                          # big block with holes
    masks[2, 20:100, 20:120] = 255; masks[2, 130:220, 180:300] = 255   # two separate regions: 47 % / 53 %
    masks[3, 60:180, 100:110] = 255                         # thin
    masks[4] = (rng.rand(h, w) < 0.5) * 255                 # salt and pepper: hundreds of tiny regions -> nothing above 25 %
    masks[5, 30:210, 30:290] = 255                          # far-depth mask (uses `far` below)
    masks[6, 5:50, 5:50] = 255                              # skipped
    ori = masks.copy()
    ori[1, 30:210, 40:290] = 255                            # original mask larger than the refined one
    un = np.zeros(7, np.uint8); un[6] = 1
    for name, dmap in (("near", depth), ("far", far)):
        mg, ug = inst.maskGeometricFilter(dmap, masks, ori, un)
        mo, uo = o.mask_geometric_filter(dmap, masks, ori, un)
        assert np.array_equal(ug, uo), name
        for i in range(7):
            assert np.array_equal(mg[i], mo[i]), (name, i)
        assert np.array_equal(mg[6], masks[6])
        if name == "near":   # the spiral is one region that survives; salt-and-pepper has no region above 25 %
            assert mo[0].any() and uo[0] == 0 and uo[4] == 1 and uo[2] == 0
        else:
            assert mo[5].any()
    g.close(); o.close()


# ---------------------------------------------------------------- sizes: ragged (not a multiple of the tile sizes) and BASELINE config 4 (1280x960)
@pytest.mark.parametrize("w,h,frames", [(328, 248, 4), (1280, 960, 2)])
def test_other_resolutions_against_oracle(ifx, orc, w, h, frames):
    from instancefusion_amd import synth

    K = dict(fx=528.0 * w / 640, fy=528.0 * w / 640, cx=w / 2.0, cy=h / 2.0)
    st = synth.make_stream(frames, w, h, noise=True, **K)
    g = ifx.ElasticFusion(w=w, h=h, max_surfels=w * h * 2, **K)
    g.set_option("compact_every_frame", 1)
    o = orc.Oracle(w=w, h=h, max_surfels=w * h * 2, **K)
    inst = ifx.InstanceFusion(g)
    for i in range(frames):
        pg = g.processFrame(st["rgb"][i], st["depth"][i])
        po = o.process_frame(st["rgb"][i], st["depth"][i])
        assert_pose_equal(pg, po, f"frame {i}")
        for name in ("depth_filtered", "depth_metric", "depth_metric_filtered"):
            assert np.array_equal(g.image(name), o.image(name)), (i, name)
    assert g.count == o.count
    assert np.array_equal(g.image("ids_after"), o.image("ids_after"))
    # identical map state -> identical integer outputs of the map stages at this size
    m = o.download()
    g.upload(m); o.upload(m)
    assert np.array_equal(g.render_ids(po, 0), o.render_ids(po, 0))
    # superpixel stages at this size (ragged: the last partial cell column / row has no centre of its own)
    seg_g, n_g = inst.gSLICrInterface(st["rgb"][0])
    seg_o, n_o = o.slic_segment(st["rgb"][0])
    assert n_g == n_o == (w // 16) * (h // 16) and np.array_equal(seg_g, seg_o)
    s_g, f_g, i_g = inst.mergeSuperPixel(st["depth"][0], seg_g)
    s_o, f_o, i_o = o.merge_superpixels(st["depth"][0], seg_o)
    assert np.array_equal(s_g, s_o) and np.array_equal(f_g, f_o) and nan_equal(i_g, i_o)
    mk, cl = synth.canned_masks(st["obj"][0], st["scene"])
    if mk.shape[0]:
        assert np.array_equal(inst.maskSuperPixelFilter_OverSeg(f_g, mk), o.mask_superpixel_filter(f_o, mk))
        dm = (st["depth"][0].astype(np.float32) * 1.186).astype(np.uint16)
        a, ua = inst.maskGeometricFilter(dm, mk, mk)
        b, ub = o.mask_geometric_filter(dm, mk, mk)
        assert np.array_equal(a, b) and np.array_equal(ua, ub)
    g.close(); o.close()


def test_empty_inputs(ifx, small_stream):
    """No masks, an all-zero depth frame, a segmentation call on an empty map: nothing crashes, nothing changes."""
    st = small_stream
    g = ifx.ElasticFusion(**SMALL, max_surfels=200000)
    inst = ifx.InstanceFusion(g)
    inst.ProcessSegmentation(st["rgb"][0], st["depth"][0], np.zeros((0, SMALL["h"], SMALL["w"]), np.uint8), np.zeros(0, np.int32), 0, superpixels=True)
    p0 = g.processFrame(st["rgb"][0], np.zeros_like(st["depth"][0]))          # empty first frame -> empty map
    assert g.count == 0 and np.array_equal(p0, np.eye(4, dtype=np.float32))
    inst.ProcessSegmentation(st["rgb"][0], st["depth"][0], np.full((1, SMALL["h"], SMALL["w"]), 255, np.uint8), np.array([3], np.int32), 1, superpixels=True)
    assert (inst.getInstanceTable() == -1).all()
    g.close()


# ---------------------------------------------------------------- 8f-2: kNN smoothing of the instance colours
def test_knn_vote_exact(ifx, orc):
    from instancefusion_amd import synth

    w, h = 320, 240
    K = dict(fx=264.0, fy=264.0, cx=160.0, cy=120.0)
    n = 20000
    st = synth.make_stream(1, w, h, noise=False, **K)
    m = synth.make_map(n, st["scene"], st["poses_world"][0], 10)
    rng = np.random.RandomState(2)
    lab = rng.randint(-1, 6, n).astype(np.int32)
    lab[rng.rand(n) < 0.5] = -1
    votes = np.zeros((n, 48), np.float32)
    for i in np.nonzero(lab >= 0)[0]:
        a, b = (7, 0) if lab[i] % 2 == 0 else (0, 7)
        votes[i, lab[i] // 2] = orc.lib().orc_vote_encode(a, b)
    m["votes"] = votes
    m["pc"][5000:5010, :3] = m["pc"][4999, :3]            # coincident points: distance ties broken by index
    g = ifx.ElasticFusion(w=w, h=h, max_surfels=n + 100, **K)
    o = orc.Oracle(w=w, h=h, max_surfels=n + 100, **K)
    inst = ifx.InstanceFusion(g)
    g.processFrame(st["rgb"][0], np.zeros_like(st["depth"][0])); o.process_frame(st["rgb"][0], np.zeros_like(st["depth"][0]))
    g.upload(m); o.upload(m)
    masks = np.zeros((1, h, w), np.uint8)
    o.set_ids_after(np.zeros((h, w), np.int32))
    # flags bit0 = isflann: label scan, then the smoothing, inside the segmentation call
    inst.ProcessSegmentation(st["rgb"][0], st["depth"][0], masks, np.array([1], np.int32), 0, isflann=True)
    o.process_segmentation(st["rgb"][0], st["depth"][0], masks, np.array([1], np.int32), 0, flags=1)
    assert np.array_equal(inst.labels(), o.labels()) and np.array_equal(o.labels(), lab)
    cg, co = g.download()["col"], o.download()["col"]
    assert np.array_equal(cg, co)
    assert (co[:, 1] != 0).sum() > n // 4
    # the stage on its own, with the neighbour lists
    ng = inst.flannKnnVoteSurfelMap(with_neighbours=True)
    no = o.knn_vote(with_neighbours=True)
    assert np.array_equal(ng[:n], no)
    assert np.array_equal(g.download()["col"], o.download()["col"])
    g.close(); o.close()


def test_knn_against_reference_flann_golden(ifx):
    """The HIP grid search against the neighbour lists of the reference's vendored FLANN 1.8.4 (tests/golden/knn_ref.npz)."""
    import os

    gold = np.load(os.path.join(os.path.dirname(__file__), "golden", "knn_ref.npz"))
    pos, ref_idx = gold["pos"], gold["idx"].astype(np.int64)
    n = pos.shape[0]
    g = ifx.ElasticFusion(w=320, h=240, fx=264.0, fy=264.0, cx=160.0, cy=120.0, max_surfels=n + 10)
    m = dict(pc=np.concatenate([pos, np.full((n, 1), 20.0, np.float32)], 1), nr=np.tile(np.array([0, 0, 1, 0.01], np.float32), (n, 1)), col=np.zeros((n, 2), np.float32),
             tm=np.ones((n, 2), np.float32), ic=np.zeros((n, 4), np.float32), votes=np.zeros((n, 48), np.float32))
    g.upload(m)
    mine = ifx.InstanceFusion(g).flannKnnVoteSurfelMap(with_neighbours=True)[:n].astype(np.int64)
    p64 = pos.astype(np.float64)
    dm = np.sort(((p64[mine] - p64[:, None, :]) ** 2).sum(-1), axis=1)
    dr = np.sort(((p64[ref_idx] - p64[:, None, :]) ** 2).sum(-1), axis=1)
    assert np.array_equal(dm, dr)                                     # same distances: equal up to the order / choice of equidistant points
    strict = (np.diff(dr, axis=1) > 0).all(axis=1)
    assert strict.mean() > 0.95 and np.array_equal(mine[strict], ref_idx[strict])
    g.close()


# ---------------------------------------------------------------- tracker configurations other than the default (BASELINE config 1: single-scale ICP)
@pytest.mark.parametrize("name,kw", [
    ("single_scale_icp_only", dict(pyramid=0, icp_weight=100.0, so3=0)),     # RGBDOdometry iterations {10,0,0}, icp && !rgb
    ("rgb_only", dict(icp_weight=0.0)),                                     # !icp && rgb
    ("fast_odometry", dict(fast_odom=1)),                                   # iterations {3,5,4}
    ("no_so3", dict(so3=0)),
    ("tight_time_window", dict(time_delta=3, confidence=2.0)),              # surfels leave the active window / become stable quickly
])
def test_tracker_and_map_configurations(ifx, orc, small_stream, name, kw):
    st = small_stream
    g = ifx.ElasticFusion(**SMALL, max_surfels=400000, **kw)
    g.set_option("compact_every_frame", 1)
    o = orc.Oracle(**SMALL, max_surfels=400000, **kw)
    # (The photometric term alone -- about 1 500 correspondences on this stream -- leaves directions of the 6x6 system almost unobservable; both sides take the PIVOTED
    # LDLT there, EF/Utils/RGBDOdometry.cpp:552, on bit-identical exact sums: the poses are held to the same standard as every other configuration.)
    for i in range(6):
        pg = g.processFrame(st["rgb"][i], st["depth"][i])
        po = o.process_frame(st["rgb"][i], st["depth"][i])
        assert_pose_equal(pg, po, f"{name} frame {i}")
        assert np.array_equal(g.tracker_diag()[:6], o.tracker_diag()[:6]), (name, i)
    assert g.count == o.count, name
    assert np.array_equal(g.image("ids_after"), o.image("ids_after")), name
    mg, mo = g.download(), o.download()
    for k in ("pc", "nr", "col", "tm", "ic", "votes"):
        assert np.array_equal(mg[k], mo[k]), (name, k)
    g.close(); o.close()


def test_config1_single_scale_icp_at_640x480_resident_frames(ifx, orc):
    """BASELINE configuration 1 at its stated size: 640x480, single-scale ICP (RGBDOdometry iterations {10, 0, 0}: pyramid off, icp && !rgb, no SO(3) pre-alignment,
    EF/Utils/RGBDOdometry.cpp:384-386, 541-565), surfel fusion only (no instance call), on the resident-frame path bench.py uses (next frame announced, tracker
    parked): 24 frames, every pose, then count and the whole map against the oracle.  (dyson_lab.klg is not in the image: the synthetic stream stands in.)"""
    import torch

    from instancefusion_amd import synth

    Wb, Hb, NFb = 640, 480, 24
    Kb = dict(fx=528.0, fy=528.0, cx=320.0, cy=240.0)
    kw = dict(pyramid=0, icp_weight=100.0, so3=0)
    st = synth.make_stream(NFb, Wb, Hb, noise=True, **Kb)
    orc.set_threads(orc.usable_cores())
    d_rgb = torch.from_numpy(st["rgb"]).cuda()
    d_dep = torch.from_numpy(st["depth"].view(np.int16)).cuda()
    torch.cuda.synchronize()
    g = ifx.ElasticFusion(w=Wb, h=Hb, max_surfels=2_000_000, **Kb, **kw)
    o = orc.Oracle(w=Wb, h=Hb, max_surfels=2_000_000, **Kb, **kw)
    for i in range(NFb):
        if i + 1 < NFb:
            g.hint_next_frame_device(d_rgb[i + 1].data_ptr(), d_dep[i + 1].data_ptr())
        g.enqueue_frame_device(d_rgb[i].data_ptr(), d_dep[i].data_ptr(), i)
        po = o.process_frame(st["rgb"][i], st["depth"][i])
        assert_pose_equal(g.trajectory(1)[0], po, f"configuration 1, frame {i}")
    assert g.lookahead_stats()["tracked_ahead"] >= NFb - 3, g.lookahead_stats()
    assert g.count == o.count
    mg, mo = g.download(), o.download()
    for k in ("pc", "nr", "col", "tm", "ic", "votes"):
        assert np.array_equal(mg[k], mo[k]), k
    assert g.tracker_range_exceeded() == 0
    g.close(); o.close()


def test_many_masks_overseg_filter(ifx, orc, gputest_pair):
    """More than 32 masks: the per-mask bit sets of the region counter are processed in chunks of 32."""
    import os

    gold = dict(np.load(os.path.join(os.path.dirname(__file__), "golden", "slic_ref.npz")))
    c1, d1 = gputest_pair[0], gputest_pair[1] // 5
    h, w = c1.shape[:2]
    K = dict(fx=264.0, fy=264.0, cx=160.0, cy=120.0)
    g = ifx.ElasticFusion(w=w, h=h, max_surfels=1000, **K)
    o = orc.Oracle(w=w, h=h, max_surfels=1000, **K)
    inst = ifx.InstanceFusion(g)
    fin = gold["c1_merge_final"].astype(np.int32)
    rng = np.random.RandomState(8)
    masks = np.zeros((70, h, w), np.uint8)
    for i in range(70):
        x0, y0 = rng.randint(0, w - 40), rng.randint(0, h - 40)
        masks[i, y0:y0 + rng.randint(10, 40), x0:x0 + rng.randint(10, 40)] = 255
    masks[33] = 255; masks[64] = (fin >= 0) * 255
    assert np.array_equal(inst.maskSuperPixelFilter_OverSeg(fin, masks), o.mask_superpixel_filter(fin, masks))
    assert np.array_equal(inst.maskCleanOverlap(masks), _clean(orc, masks))
    g.close(); o.close()


# ---------------------------------------------------------------- a23: instance table eviction (96 slots full -> the 20 weakest instances are dropped)
def test_instance_table_eviction_exact(ifx, orc, small_stream):
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
    assert np.array_equal(g.image("ids_after"), o.image("ids_after"))
    masks, cls = synth.canned_masks(st["obj"][5], st["scene"])
    nm = masks.shape[0]
    assert nm >= 4
    evicted = False
    for call in range(30):
        classes = (1 + (call * nm + np.arange(nm)) % 79).astype(np.int32)      # a new class for every mask of every call: nothing matches
        if (call + 2) * nm > 96 and not evicted:
            # the calls around the eviction see surfels WITHOUT a colour yet (col.y = 0, as new frames leave them): colours are assigned once, so a label scan that ran
            # before the eviction (the device-side schedule enqueues its tail before the host knows the table is full) would leave colours of evicted instances behind
            m = o.download(); m["col"][:, 1] = 0.0
            o.upload(m); g.upload(m)
            o.set_pose(po, o.tick); g.set_pose(po, o.tick)
            g.processFrame(st["rgb"][5], st["depth"][5], inPose=po); o.process_frame(st["rgb"][5], st["depth"][5], in_pose=po)
        inst.ProcessSegmentation(st["rgb"][5], st["depth"][5], masks, classes, 100 + 3 * call)
        o.process_segmentation(st["rgb"][5], st["depth"][5], masks, classes, 100 + 3 * call)
        tg, to = inst.getInstanceTable(), o.instance_table()
        assert np.array_equal(tg, to), call
        if (to >= 0).sum() < 96 and call * nm > 96:
            evicted = True
        mg_, mo_ = g.download(), o.download()
        assert np.array_equal(mg_["votes"], mo_["votes"]), call
        assert np.array_equal(mg_["col"], mo_["col"]), call                    # instance colours too (ifx_map_bounding_boxes keys membership on them)
        assert np.array_equal(inst.labels(), o.labels()), call
    assert evicted
    lc = inst.getLoopClosureInstanceTable()
    assert lc.shape == (96, 5) and np.array_equal(lc[:, 3] >= 0, to >= 0)
    # InstanceFusion::renderProjectMap: the instance colour under every pixel
    pm_g, pm_o = inst.renderProjectMap(), o.render_project_map()
    assert np.array_equal(pm_g, pm_o) and (pm_o[..., :3].sum(axis=2) > 0).mean() > 0.05 and (pm_o[..., 3] == 1).all()
    g.close(); o.close()


def test_knn_vote_with_tombstones(ifx, orc, small_stream):
    """The smoothing on a map with dead slots (no compaction) equals the oracle's on the compacted map."""
    from instancefusion_amd import synth

    st = small_stream
    kw = dict(time_delta=3, confidence=2.0)
    g = ifx.ElasticFusion(**SMALL, max_surfels=400000, **kw)
    o = orc.Oracle(**SMALL, max_surfels=400000, **kw)
    inst = ifx.InstanceFusion(g)
    for i in range(6):
        po = o.process_frame(st["rgb"][i], st["depth"][i])
        g.processFrame(st["rgb"][i], st["depth"][i])
    m = o.download()
    o.upload(m); g.upload(m)                       # identical maps; from here on the pose is held, so both sides stay identical
    o.set_pose(po, o.tick); g.set_pose(po, o.tick)
    for i in (6, 7):
        g.processFrame(st["rgb"][i], st["depth"][i], inPose=po); o.process_frame(st["rgb"][i], st["depth"][i], in_pose=po)
    assert g.slots > g.count                       # tombstones present on the device (young unstable surfels died)
    assert g.count == o.count
    masks, cls = synth.canned_masks(st["obj"][7], st["scene"])
    inst.ProcessSegmentation(st["rgb"][7], st["depth"][7], masks, cls, 50, isflann=True)
    o.process_segmentation(st["rgb"][7], st["depth"][7], masks, cls, 50, flags=1)
    assert np.array_equal(inst.labels(), o.labels())
    mg, mo = g.download(), o.download()
    assert all(np.array_equal(mg[k], mo[k]) for k in MAP_KEYS)
    g.close(); o.close()


# ---------------------------------------------------------------- 8f-1: log replay end to end (tools/run_log.py)
def test_run_log_replay(ifx, small_stream, tmp_path):
    import importlib.util
    import os

    from instancefusion_amd import logio, synth

    st = small_stream
    n = 8
    klg = str(tmp_path / "s.klg")
    wr = logio.RawLogWriter(klg, depth="zlib", image="jpeg", jpeg_quality=100)
    for i in range(n + 1):                                   # the reader never delivers the last frame
        wr.add(33333 * i, st["rgb"][min(i, n - 1)], st["depth"][min(i, n - 1)])
    wr.close()
    mdir = tmp_path / "masks"
    mdir.mkdir()
    for i in range(n):
        mk, cl = synth.canned_masks(st["obj"][i], st["scene"])
        np.savez(mdir / f"{i:06d}.npz", masks=mk, class_ids=cl)
    spec = importlib.util.spec_from_file_location("run_log", os.path.join(os.path.dirname(os.path.dirname(__file__)), "tools", "run_log.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    out = str(tmp_path / "Result")
    rc = mod.main([klg, "--width", str(SMALL["w"]), "--height", str(SMALL["h"]), "--fx", str(SMALL["fx"]), "--fy", str(SMALL["fy"]), "--cx", str(SMALL["cx"]),
                   "--cy", str(SMALL["cy"]), "--max-surfels", "400000", "--masks", str(mdir), "--out", out, "--flann-every", "2"])
    assert rc == 0
    traj = np.loadtxt(out + ".freiburg")
    assert traj.shape == (n, 8) and np.allclose(traj[:, 0], 0.033333 * np.arange(n), atol=1e-6)
    # same poses as feeding the decoded frames directly
    rd = logio.RawLogReader(klg, SMALL["w"], SMALL["h"])
    g = ifx.ElasticFusion(**SMALL, max_surfels=400000)
    k = 0
    while rd.hasMore():
        rd.getNext()
        p = g.processFrame(rd.rgb, rd.depth)
        assert np.allclose(traj[k, 1:4], p[:3, 3], atol=2e-6), k
        k += 1
    g.close()
    for suffix in (".ply", "_Instance.ply"):
        raw = open(out + suffix, "rb").read()
        head, body = raw.split(b"end_header\n", 1)
        nv = int(head.split(b"element vertex ")[1].split(b"\n")[0])
        assert len(body) == nv * 31


# ---------------------------------------------------------------- 8e: sharded projection, emulated on one GPU
@pytest.mark.parametrize("world", [2, 3])
def test_sharded_projection_emulated(ifx, small_stream, world):
    """G handles of one process act as ranks 0..G-1 (each projects only its slice of the slots); the all-reduce(MIN) of the
    key images is replaced by an element-wise minimum.  Every replica must equal the single-handle run bit for bit."""
    import torch

    from instancefusion_amd import sharded, synth

    st = small_stream
    n = 7
    d_rgb = torch.from_numpy(st["rgb"][:n].copy()).cuda()
    d_dep = torch.from_numpy(st["depth"][:n].view(np.int16).copy()).cuda()
    torch.cuda.synchronize()
    ref = ifx.ElasticFusion(**SMALL, max_surfels=400000)
    ref.set_option("two_streams", 0)
    rinst = ifx.InstanceFusion(ref)
    efs = [ifx.ElasticFusion(**SMALL, max_surfels=400000) for _ in range(world)]
    insts = [ifx.InstanceFusion(e) for e in efs]
    for r, e in enumerate(efs):
        e._chk(e.L.ifx_set_shard(e.handle, r, world), "ifx_set_shard")
    xs = None
    for i in range(n):
        ref.enqueue_frame_device(d_rgb[i].data_ptr(), d_dep[i].data_ptr(), i)
        xs = sharded.emulate_ranks(efs, d_rgb[i].data_ptr(), d_dep[i].data_ptr(), xs)
        seg = rinst.whetherDoSegmentation(10 + i)
        assert all(x.whetherDoSegmentation(10 + i) == seg for x in insts), i
        if i == 4:   # the instance layer runs replicated on identical inputs
            mk, cl = synth.canned_masks(st["obj"][4], st["scene"])
            for x in [rinst] + insts:
                x.ProcessSegmentation(st["rgb"][4], st["depth"][4], mk, cl, 14, superpixels=True)
    ref.sync()
    t0, m0, i0, l0 = ref.trajectory(), ref.download(), ref.image("ids_after"), rinst.labels()
    for r, (e, x) in enumerate(zip(efs, insts)):
        e.sync()
        assert np.array_equal(e.trajectory(), t0), r
        assert np.array_equal(e.image("ids_after"), i0), r
        m = e.download()
        assert all(np.array_equal(m[k], m0[k]) for k in MAP_KEYS), r
        assert np.array_equal(x.labels(), l0), r
        e.close()
    ref.close()


def test_sharded_world_of_one(ifx, small_stream):
    """ShardedElasticFusion with a single rank (no process group): the phase API alone equals the normal entry point."""
    import torch

    from instancefusion_amd import sharded

    st = small_stream
    d_rgb = torch.from_numpy(st["rgb"][:5].copy()).cuda()
    d_dep = torch.from_numpy(st["depth"][:5].view(np.int16).copy()).cuda()
    torch.cuda.synchronize()
    a = ifx.ElasticFusion(**SMALL, max_surfels=400000)
    b = ifx.ElasticFusion(**SMALL, max_surfels=400000)
    sb = sharded.ShardedElasticFusion(b, 0, 1, None)
    for i in range(5):
        a.enqueue_frame_device(d_rgb[i].data_ptr(), d_dep[i].data_ptr(), i)
        sb.process_frame_device(d_rgb[i].data_ptr(), d_dep[i].data_ptr())
    a.sync(); b.sync()
    assert np.array_equal(a.trajectory(), b.trajectory())
    ma, mb = a.download(), b.download()
    assert all(np.array_equal(ma[k], mb[k]) for k in MAP_KEYS)
    a.close(); b.close()


def test_sharded_rccl_world_of_one(ifx, small_stream):
    """The real exchange path -- torch.distributed 'nccl' (RCCL) all-reduce(MIN) enqueued on the handle's own stream -- with a
    process group of one rank: exercises the stream hand-over and the RCCL call; the result must equal the plain entry point."""
    import os
    import socket

    import torch
    import torch.distributed as dist

    from instancefusion_amd import sharded

    st = small_stream
    d_rgb = torch.from_numpy(st["rgb"][:5].copy()).cuda()
    d_dep = torch.from_numpy(st["depth"][:5].view(np.int16).copy()).cuda()
    torch.cuda.synchronize()
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("nccl", rank=0, world_size=1)
    try:
        a = ifx.ElasticFusion(**SMALL, max_surfels=400000)
        b = ifx.ElasticFusion(**SMALL, max_surfels=400000)
        sb = sharded.ShardedElasticFusion(b, 0, 1, dist)
        for i in range(5):
            a.enqueue_frame_device(d_rgb[i].data_ptr(), d_dep[i].data_ptr(), i)
            sb.process_frame_device(d_rgb[i].data_ptr(), d_dep[i].data_ptr())
        a.sync(); b.sync(); torch.cuda.synchronize()
        assert np.array_equal(a.trajectory(), b.trajectory())
        ma, mb = a.download(), b.download()
        assert all(np.array_equal(ma[k], mb[k]) for k in MAP_KEYS)
        assert np.array_equal(a.image("ids_after"), b.image("ids_after"))
        a.close(); b.close()
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("lazy_ids", [0, 1, 2, 3, 4])
def test_owner_sharded_rccl_world_of_one_in_library(ifx, small_stream, lazy_ids):
    """The spatially sharded map with the collectives INSIDE libifx.so (csrc/ifx_comm.hip), on real RCCL: a world of one (ifx_config.n_ranks = -1:
    creation-number ids, owner filter, every exchange point of a frame / predict / segmentation call / kNN smoothing issued as a one-rank
    ncclAllReduce / ncclAllGather on the handle's stream by the library itself).  One library call per frame; against the unsharded handle:
    poses, prediction / fill-in / id images, instance table, and -- by creation number -- the whole map, votes, labels and colours, bit for bit.
    Also the host-pointer entry (ifx_owner_process_frame) and the exchange statistics: six collectives and 80 bytes per pixel per frame."""
    import torch

    from instancefusion_amd import sharded, synth

    st = small_stream
    NF = 9
    d_rgb = torch.from_numpy(st["rgb"][:NF].copy()).cuda()
    d_dep = torch.from_numpy(st["depth"][:NF].view(np.int16).copy()).cuda()
    torch.cuda.synchronize()
    one = ifx.ElasticFusion(**SMALL, max_surfels=400000)
    ef = ifx.ElasticFusion(**SMALL, max_surfels=400000, n_ranks=-1, rank=0)
    osh = sharded.OwnerShardedElasticFusion(ef, None)            # ifx_comm_unique_id + ifx_owner_init_comm: ncclCommInitRank(1, id, 0)
    ef.set_option("own_lazy_ids", int(lazy_ids in (1, 2)))       # (1: 72 B per pixel + the lattice; the whole id image on demand, the exchange enqueued by the library in place)
    ef.set_option("own_key_rs", int(lazy_ids == 2))              # (2: also the index keys as ncclReduceScatter + ncclAllGather of the creation numbers: eight collectives, 68 B per pixel in all-reduce-equivalent bytes)
    ef.set_option("own_track_rows", int(lazy_ids >= 3))          # (3: the tracker's reductions over this rank's pixel blocks, the 2 x 29 exact sums ncclAllReduce'd in f64 -- 38 more collectives of 1 KB a frame;
    ef.set_option("own_track_rows_emulate", 3 if lazy_ids == 4 else 0)   # 4: this one rank playing three in turn into the same rows: the partition covers every block once.  Same poses, same map.)
    inst_one, inst = ifx.InstanceFusion(one), ifx.InstanceFusion(ef)
    P = SMALL["w"] * SMALL["h"]

    def by_seq(x):
        return x[np.argsort(ef.seq(), kind="stable")]

    for i in range(NF):
        if i == 4:   # an uploaded, stable map: upload keeps the owned rows (all of them here), predict runs with its two exchanges inside the library
            m = one.download(); m["pc"][:, 3] = 20.0
            pose = one.getCurrPose()
            one.upload(m); one.set_pose(pose, one.tick); one.combined_predict(pose, one.tick, one.tick)
            ef.upload(m); ef.set_pose(pose, one.tick)
            osh.predict()
        if i == 6:   # the reference-shaped entry: host pointers, one synchronisation, currPose back
            one.processFrame(st["rgb"][i], st["depth"][i])
            pg = osh.process_frame(st["rgb"][i], st["depth"][i])
            assert np.array_equal(pg, one.getCurrPose())
        else:
            if i == 7:
                osh.exchange_stats(reset=True)
            one.enqueue_frame_device(d_rgb[i].data_ptr(), d_dep[i].data_ptr(), i)
            if i + 1 < NF and i + 1 != 6 and lazy_ids < 3:   # the one-frame look-ahead of the sharded path: the next frame's image-only work on the side stream, its tracker parked behind this frame
                ef.hint_next_frame_device(d_rgb[i + 1].data_ptr(), d_dep[i + 1].data_ptr())   # (frame 4's parked tracker is dropped by the upload, others by the segmentation calls' map accesses: both paths run)
            osh.process_frame_device(d_rgb[i].data_ptr(), d_dep[i].data_ptr())
            if i == 7:
                xs = osh.exchange_stats()
                L = -(-SMALL["w"] // 10) * -(-SMALL["h"] // 10)
                rows = 38 if lazy_ids >= 3 else 0   # (19 iterations x 2 all-reduces of one accumulator row block: 4 replicas x 32 doubles)
                assert xs["collectives"] == (6, 6, 8, 6, 6)[lazy_ids] + rows and xs["bytes"] == (80 * P, 72 * P + 8 * L, 68 * P + 8 * L - 4, 80 * P, 80 * P)[lazy_ids] + 16 + 24 + rows * 1024, xs     # keys 8 + 8 + 16, association verdicts 2 (8 B per measurement pixel), clean taps 16, prediction 30 (its vertex is rebuilt from the key), + the 16-byte tail, + the 8-byte "surfel 0" word behind the keys of exchanges 0, 2 and 4
        assert np.array_equal(ef.getCurrPose(), one.getCurrPose()), i
        for name in ("pred_vertex", "pred_normal", "pred_image", "pred_time", "fill_vertex", "fill_image"):
            assert np.array_equal(ef.image(name), one.image(name)), (i, name)
        want = inst_one.whetherDoSegmentation(i)
        assert inst.whetherDoSegmentation(i) == want, i
        if i >= 5:
            masks, cls = synth.canned_masks(st["obj"][i], st["scene"])
            inst_one.ProcessSegmentation(st["rgb"][i], st["depth"][i], masks, cls, i, superpixels=True)
            osh.process_segmentation(st["rgb"][i], st["depth"][i], masks, cls, i, superpixels=True)
            assert np.array_equal(inst.getInstanceTable(), inst_one.getInstanceTable()), i
            assert np.array_equal(by_seq(inst.labels()), inst_one.labels()), i
    assert (inst_one.labels() >= 0).sum() > 100
    inst_one.flannKnnVoteSurfelMap()
    osh.knn_vote_colour()                                       # the all-gather of the slots inside the library
    ref, got = one.download(), ef.download()
    order = np.argsort(ef.seq(), kind="stable")
    assert len(order) == ref["pc"].shape[0]
    for k in MAP_KEYS:
        assert np.array_equal(got[k][order], ref[k]), k
    assert len(np.unique(ref["col"][:, 1])) > 2
    ef.close(); one.close()


# ---------------------------------------------------------------- 8f-3a: local loop-closure detection (INACTIVE prediction + model-to-model tracking + gates)
def test_loop_closure_detection(ifx, orc, small_stream):
    """EF/ElasticFusion.cpp:453-566 without ferns.  A 3-frame time window makes most of the map 'inactive' from the fourth
    frame on, so the model-to-model tracker has something to align on the 10-frame stream played forth and back."""
    st = small_stream
    kw = dict(time_delta=3, confidence=2.0)
    thr = 35000 * (SMALL["w"] * SMALL["h"]) // (640 * 480)
    g = ifx.ElasticFusion(**SMALL, max_surfels=400000, **kw)
    g0 = ifx.ElasticFusion(**SMALL, max_surfels=400000, **kw)          # same run without the detection
    o = orc.Oracle(**SMALL, max_surfels=400000, **kw)
    for e in (g, g0):
        e.set_option("compact_every_frame", 1)
    g.set_loop_closure(True, thr, 1e-4, 1e-5)
    o.set_loop_closure(True, thr, 1e-4, 1e-5)
    seq = list(range(10)) + list(range(8, 2, -1))
    n_ran = 0
    po = None
    for k, i in enumerate(seq):
        strict = k >= 10
        if k >= 3:
            # Both sides start every frame from the oracle's map and pose: this configuration (3-frame window) tracks against a sparse
            # prediction and free-running trajectories drift apart by > 1e-4 within ten frames, which is not what is tested here.
            m, tick0, po_prev = o.download(), o.tick, po
        po = o.process_frame(st["rgb"][i], st["depth"][i])
        if k >= 3:
            for e in (g, g0):
                e.upload(m); e.set_pose(po_prev, tick0)
        # frames 3..9: the GPU tracks by itself (poses agree to ~1e-6, not bit for bit); frames 10..: it is handed the oracle's pose, so that
        # the renders the model-to-model tracker aligns are identical on both sides
        pg = g.processFrame(st["rgb"][i], st["depth"][i], inPose=po if strict else None)
        p0 = g0.processFrame(st["rgb"][i], st["depth"][i], inPose=po if strict else None)
        assert np.array_equal(pg, p0), k                               # the detection has no side effect on the frame
        assert np.abs(pg - po).max() < 1e-4, k
        dg, do = g.loop_closure_diag(), o.loop_closure_diag()
        assert dg["ran"] == do["ran"], (k, dg, do)
        if k == 2:                                                     # every surfel stable from here on (only stable ones are predicted)
            m = o.download(); m["pc"][:, 3] = 20.0; o.upload(m)
        if k < 3:
            assert not dg["ran"] and dg["inactive_pixels"] == 0 and not dg["accepted"]
            assert k == 0 or np.array_equal(dg["est_pose"], pg)      # (the first frame only initialises the map)
            continue
        n_ran += dg["ran"]
        assert dg["cov_ok"] == do["cov_ok"] and dg["accepted"] == do["accepted"], (k, dg, do)
        if strict:
            for name in ("old_vertex", "old_normal", "old_image", "old_time"):
                assert np.array_equal(g.image(name), o.image(name)), (k, name)
            assert dg["inactive_pixels"] == do["inactive_pixels"] > 1000 and dg["icp_count"] == do["icp_count"], (k, dg, do)
            assert abs(dg["icp_error"] - do["icp_error"]) <= 1e-3 * do["icp_error"], (k, dg, do)
            assert abs(dg["cov_max"] - do["cov_max"]) <= 1e-3 * abs(do["cov_max"]), (k, dg, do)
            assert np.abs(dg["est_pose"] - do["est_pose"]).max() < 2e-5, k
        else:
            # a 1e-7 difference of the pose moves a few pixels of the two renders (u8 colours, z-buffer winners) and the alignment of two
            # noisy renders answers with up to a few 1e-4: gates and sums are compared tightly, the estimate loosely
            assert abs(dg["inactive_pixels"] - do["inactive_pixels"]) <= max(4, do["inactive_pixels"] // 1000), (k, dg, do)
            assert abs(dg["icp_count"] - do["icp_count"]) <= max(8.0, do["icp_count"] * 0.002), (k, dg, do)
            assert abs(dg["icp_error"] - do["icp_error"]) <= 0.01 * do["icp_error"], (k, dg, do)
            assert abs(dg["cov_max"] - do["cov_max"]) <= 0.01 * abs(do["cov_max"]), (k, dg, do)
            assert np.abs(dg["est_pose"] - do["est_pose"]).max() < 1e-3, k
    assert n_ran >= 10
    assert g.loop_closure_diag()["candidates"] == o.loop_closure_diag()["candidates"] > 0
    assert g.count == g0.count and all(np.array_equal(a, b) for a, b in zip(g.download().values(), g0.download().values()))
    g.close(); g0.close(); o.close()


@pytest.mark.parametrize("world", [2, 1])
def test_owner_sharded_loop_closure_detection(ifx, small_stream, world):
    """Local loop-closure DETECTION on the spatially sharded map (EF/ElasticFusion.cpp:453-566; VERDICT round 2, missing item 3): every rank rasters the
    ACTIVE and the INACTIVE render of its shard from one scan, the two key images are MIN-reduced, the owners' winners of both renders SUM-merged, and the
    model-to-model tracker + gates run replicated on the exchanged images.  Against the unsharded handle with the same detection: verdict (ran, inactive
    pixels, ICP count / error, covariance gate, accepted, estimated pose, candidates) and the old_* / act_* images bit for bit on every frame; poses and
    the merged map unaffected.  world = 2: two handles of one process, exchanges by hand; world = 1: a world of one on real RCCL through the in-library path."""
    import torch

    from instancefusion_amd import sharded

    st = small_stream
    kw = dict(time_delta=3, confidence=2.0)
    thr = 35000 * (SMALL["w"] * SMALL["h"]) // (640 * 480)
    seq = list(range(10)) + list(range(8, 2, -1))
    d_rgb = torch.from_numpy(st["rgb"][:10].copy()).cuda()
    d_dep = torch.from_numpy(st["depth"][:10].view(np.int16).copy()).cuda()
    torch.cuda.synchronize()
    one = ifx.ElasticFusion(**SMALL, max_surfels=400000, **kw)
    one.set_loop_closure(True, thr, 1e-4, 1e-5)
    if world == 1:
        efs = [ifx.ElasticFusion(**SMALL, max_surfels=400000, n_ranks=-1, rank=0, **kw)]
        osh = sharded.OwnerShardedElasticFusion(efs[0], None)
    else:
        efs = [ifx.ElasticFusion(**SMALL, max_surfels=400000, n_ranks=world, rank=r, **kw) for r in range(world)]
    for e in efs:
        e.set_loop_closure(True, thr, 1e-4, 1e-5)
    n_ran = 0
    for k, i in enumerate(seq):
        if k == 3:   # every surfel stable from here on (only stable ones are predicted); the renders then have something to show
            m = one.download(); m["pc"][:, 3] = 20.0
            pose, tick = one.getCurrPose(), one.tick
            one.upload(m); one.set_pose(pose, tick); one.combined_predict(pose, tick, tick)
            for e in efs:
                e.upload(m); e.set_pose(pose, tick)
            if world == 1:
                osh.predict()
            else:
                sharded.emulate_owner_predict(efs)
        one.enqueue_frame_device(d_rgb[i].data_ptr(), d_dep[i].data_ptr(), k)
        if world == 1:
            osh.process_frame_device(d_rgb[i].data_ptr(), d_dep[i].data_ptr())
        else:
            sharded.emulate_owner_ranks(efs, d_rgb[i].data_ptr(), d_dep[i].data_ptr())
        d1 = one.loop_closure_diag()
        for e in efs:
            assert np.array_equal(e.getCurrPose(), one.getCurrPose()), (k, e.cfgd["rank"])
            de = e.loop_closure_diag()
            for key in d1:
                assert np.array_equal(np.asarray(de[key]), np.asarray(d1[key])), (k, key, de, d1)
            if d1["ran"]:
                for name in ("old_vertex", "old_normal", "old_image", "old_time", "act_vertex", "act_normal", "act_image"):
                    assert np.array_equal(e.image(name), one.image(name)), (k, name)
        n_ran += int(d1["ran"])
    assert n_ran >= 8 and one.loop_closure_diag()["candidates"] > 0
    ref = one.download()
    parts = [(e.seq(), e.download()) for e in efs]
    order = np.argsort(np.concatenate([p[0] for p in parts]), kind="stable")
    for key in MAP_KEYS:
        assert np.array_equal(np.concatenate([p[1][key] for p in parts])[order], ref[key]), key
    for e in efs:
        e.close()
    one.close()


def test_loop_closure_detection_nothing_inactive(ifx, small_stream):
    """Default 200-frame window: nothing can be inactive on a short stream -> the block is skipped, results and candidates untouched;
    with an uploaded map (unknown times) the INACTIVE render runs, finds nothing and the tracker kernels return at once."""
    st = small_stream
    g = ifx.ElasticFusion(**SMALL, max_surfels=400000)
    g0 = ifx.ElasticFusion(**SMALL, max_surfels=400000)
    g.set_loop_closure(True)
    for i in range(5):
        assert np.array_equal(g.processFrame(st["rgb"][i], st["depth"][i]), g0.processFrame(st["rgb"][i], st["depth"][i]))
        d = g.loop_closure_diag()
        assert not d["ran"] and d["candidates"] == 0
    m = g.download()
    g.upload(m); g0.upload(m)
    for i in range(5, 8):
        assert np.array_equal(g.processFrame(st["rgb"][i], st["depth"][i]), g0.processFrame(st["rgb"][i], st["depth"][i]))
        d = g.loop_closure_diag()
        assert not d["ran"] and d["inactive_pixels"] == 0 and not d["accepted"]
    assert all(np.array_equal(a, b) for a, b in zip(g.download().values(), g0.download().values()))
    g.close(); g0.close()


# ---------------------------------------------------------------- a9 / a14: the tiled rasteriser against the global-atomic one
@pytest.mark.parametrize("res", [(320, 240), (328, 248)])
def test_tiled_rasteriser_equals_atomic_rasteriser(ifx, small_stream, res):
    """k_tile_* (key tiles resolved in LDS, on by default from 1 Mpixel) and k_raster_list (global atomics) must draw the same images: trajectories, maps,
    predictions and id images bit for bit over several frames, also on an image whose size is no multiple of the tile size."""
    from instancefusion_amd import synth

    w, h = res
    K = dict(fx=264.0, fy=264.0, cx=w / 2.0, cy=h / 2.0)
    st = small_stream if res == (320, 240) else synth.make_stream(6, w, h, noise=True, **K)
    a = ifx.ElasticFusion(w=w, h=h, max_surfels=400000, confidence=2.0, **K)
    b = ifx.ElasticFusion(w=w, h=h, max_surfels=400000, confidence=2.0, **K)
    a.set_option("raster_tiles", 0); b.set_option("raster_tiles", 1)
    for k in range(6):
        assert np.array_equal(a.processFrame(st["rgb"][k], st["depth"][k]), b.processFrame(st["rgb"][k], st["depth"][k])), k
        for name in ("ids_after", "pred_vertex", "pred_normal", "pred_image", "pred_time", "fill_vertex"):
            assert np.array_equal(a.image(name), b.image(name)), (k, name)
    ma, mb = a.download(), b.download()
    assert all(np.array_equal(ma[key], mb[key]) for key in MAP_KEYS) and (a.image("ids_after") > 0).mean() > 0.3
    a.close(); b.close()


# ---------------------------------------------------------------- 8f-3: deformation hooks (graph application inside clean, graph sampling, constraint samples)
def _random_graph(samples, rng, rot=0.05, trans=0.02):
    import math

    g = np.zeros((samples.shape[0], 16), np.float32)
    g[:, :3] = samples[:, :3]; g[:, 15] = samples[:, 3]
    for i in range(len(g)):
        a = rng.uniform(-rot, rot, 3)
        Rx = np.array([[1, 0, 0], [0, math.cos(a[0]), -math.sin(a[0])], [0, math.sin(a[0]), math.cos(a[0])]])
        Ry = np.array([[math.cos(a[1]), 0, math.sin(a[1])], [0, 1, 0], [-math.sin(a[1]), 0, math.cos(a[1])]])
        Rz = np.array([[math.cos(a[2]), -math.sin(a[2]), 0], [math.sin(a[2]), math.cos(a[2]), 0], [0, 0, 1]])
        g[i, 3:12] = (Rz @ Ry @ Rx).T.reshape(9)
        g[i, 12:15] = rng.uniform(-trans, trans, 3)
    return g


@pytest.mark.parametrize("is_fern", [True, False])
def test_deformation_application_exact(ifx, orc, small_stream, is_fern):
    """GlobalModel::clean with a deformation graph (copy_unstable.vert:178-374) on identical maps: positions, normals and time stamps bit for bit,
    incl. the time-stamp refresh against the re-rendered INACTIVE depth (local loop closure, is_fern = False)."""
    st = small_stream
    kw = dict(time_delta=3, confidence=2.0)
    o = orc.Oracle(**SMALL, max_surfels=400000, **kw)
    g = ifx.ElasticFusion(**SMALL, max_surfels=400000, **kw)
    o.set_loop_closure(True); g.set_loop_closure(True)
    for k in range(7):
        pose = o.process_frame(st["rgb"][k], st["depth"][k])
        if k == 2:
            m = o.download(); m["pc"][:, 3] = 20.0; o.upload(m)
    # the GPU runs its own frames too (so that its store has tombstones and its own slot numbering), then takes the oracle's map
    for k in range(4):
        g.processFrame(st["rgb"][k], st["depth"][k])
    m0 = o.download()
    g.upload(m0)
    tick = o.tick
    g.set_pose(pose, tick)
    so, sg = o.sample_graph_model(), g.sample_graph_model()
    assert np.array_equal(so, sg) and so.shape[0] >= 5
    graph = _random_graph(so, np.random.RandomState(11))
    pose2 = pose.copy(); pose2[:3, 3] += np.array([0.004, -0.003, 0.002], np.float32)      # the adopted pose differs from the tracked one
    for e in (o, g):
        e.set_frame(st["rgb"][7], st["depth"][7])                      # the order of a frame: index map, fuse, index map, clean (with the graph)
        e.predict_indices(pose2, tick)
        e.fuse(pose2, tick, 1.0)
        e.predict_indices(pose2, tick)
        e.set_deformation(graph, is_fern=is_fern)
        e.clean(pose2, tick)
    mo, mg = o.download(), g.download()
    assert mo["pc"].shape == mg["pc"].shape
    for key in MAP_KEYS:
        assert np.array_equal(mo[key], mg[key]), key
    assert np.abs(mo["pc"][: len(m0["pc"]), :3] - m0["pc"][: len(mo["pc"]), :3]).max() > 1e-3 or len(mo["pc"]) != len(m0["pc"])      # something moved
    if not is_fern:
        assert (mo["tm"][:, 1] == tick).sum() > (m0["tm"][:, 1] == tick).sum()          # moved stable surfels in front of the old model were re-activated
    # the graph is consumed by one clean
    for e in (o, g):
        e.predict_indices(pose2, tick); e.fuse(pose2, tick, 1.0); e.predict_indices(pose2, tick); e.clean(pose2, tick)
    assert all(np.array_equal(o.download()[key], g.download()[key]) for key in MAP_KEYS)
    o.close(); g.close()


def test_deformation_large_graph(ifx, orc, small_stream):
    """1000 nodes (the reference allows < 1024): 64 KB of graph in LDS, deep binary search, every surfel has 20 time neighbours on both sides."""
    st = small_stream
    o = orc.Oracle(**SMALL, max_surfels=400000, confidence=2.0)
    g = ifx.ElasticFusion(**SMALL, max_surfels=400000, confidence=2.0)
    for k in range(5):
        pose = o.process_frame(st["rgb"][k], st["depth"][k])
    m0 = o.download()
    g.processFrame(st["rgb"][0], st["depth"][0])
    g.upload(m0); g.set_pose(pose, o.tick)
    rng = np.random.RandomState(3)
    pick = np.sort(rng.choice(len(m0["pc"]), 1000, replace=False))                 # map order = time order
    samples = np.concatenate([m0["pc"][pick, :3], m0["tm"][pick, :1]], 1)
    assert (np.diff(samples[:, 3]) >= 0).all()
    graph = _random_graph(samples, rng, rot=0.02, trans=0.01)
    for e in (o, g):
        e.set_frame(st["rgb"][5], st["depth"][5])
        e.predict_indices(pose, o.tick); e.fuse(pose, o.tick, 1.0); e.predict_indices(pose, o.tick)
        e.set_deformation(graph, is_fern=True)
        e.clean(pose, o.tick)
    mo, mg = o.download(), g.download()
    for key in MAP_KEYS:
        assert np.array_equal(mo[key], mg[key]), key
    with pytest.raises(ifx.IfxError):
        g.set_deformation(np.zeros((1024, 16), np.float32))                        # GlobalModel::MAX_NODES
    with pytest.raises(ifx.IfxError):
        g.set_deformation(graph[::-1].copy())                                      # not sorted by time
    o.close(); g.close()


def test_sample_graph_with_tombstones(ifx, small_stream):
    """Deformation::sampleGraphModel numbers the surfels of the compacted map; the store keeps tombstones: the sample must not depend on them."""
    st = small_stream
    a = ifx.ElasticFusion(**SMALL, max_surfels=400000, confidence=2.0, time_delta=3)
    b = ifx.ElasticFusion(**SMALL, max_surfels=400000, confidence=2.0, time_delta=3)
    b.set_option("compact_every_frame", 1)
    for k in range(8):
        a.processFrame(st["rgb"][k], st["depth"][k]); b.processFrame(st["rgb"][k], st["depth"][k])
    assert a.slots > b.slots == b.count == a.count                     # a holds tombstones
    sa, sb = a.sample_graph_model(), b.sample_graph_model()
    assert sa.shape[0] == (a.count + 4999) // 5000 and np.array_equal(sa, sb)
    m = b.download()
    assert np.array_equal(sb[:, :3], m["pc"][::5000, :3]) and np.array_equal(sb[:, 3], m["tm"][::5000, 0])
    a.close(); b.close()


def test_loop_closure_callback_end_to_end(ifx, orc, small_stream):
    """An accepted candidate calls back into the host (EF/ElasticFusion.cpp:566-613): constraint samples, graph sample, a deformation graph
    (here a stand-in for the reference's optimiser: rigid nodes carrying the mean constraint offset), currPose = estPose -- same callback on both sides."""
    st = small_stream
    kw = dict(time_delta=3, confidence=2.0)
    thr = 35000 * (SMALL["w"] * SMALL["h"]) // (640 * 480)
    o = orc.Oracle(**SMALL, max_surfels=400000, **kw)
    g = ifx.ElasticFusion(**SMALL, max_surfels=400000, **kw)
    g.set_option("compact_every_frame", 1)
    o.set_loop_closure(True, thr, 1e-4, 1e-5); g.set_loop_closure(True, thr, 1e-4, 1e-5)
    log = {"o": [], "g": []}
    tracked = [None]

    def make_cb(tag):
        def cb(e, lc):
            if tag == "o":
                tracked[0] = e.get_pose()       # the pose the frame was tracked to (before currPose = estPose)
            src, dst, tm = e.loop_closure_constraints()
            s = e.sample_graph_model()
            log[tag].append((src, dst, tm, s, lc))
            if len(log[tag]) > 1:          # deform on the first candidate only
                return
            graph = np.zeros((s.shape[0], 16), np.float32)
            graph[:, :3] = s[:, :3]; graph[:, 3] = graph[:, 7] = graph[:, 11] = 1.0; graph[:, 15] = s[:, 3]
            graph[:, 12:15] = (dst - src).mean(axis=0) if len(src) else 0.0
            e.set_deformation(graph, is_fern=False)
            e.adopt_estimated_pose()
        return cb

    o.set_loop_closure_callback(make_cb("o")); g.set_loop_closure_callback(make_cb("g"))
    po = None
    for k in range(9):
        if k >= 3:
            m, tick0, po_prev = o.download(), o.tick, po
        tracked[0] = None
        po = o.process_frame(st["rgb"][k], st["depth"][k])
        if k >= 3:
            g.upload(m); g.set_pose(po_prev, tick0)
        # the GPU is handed the pose the oracle tracked (the renders the candidate is judged on are then identical); when the callback adopts
        # the estimated pose the frame continues with it on both sides
        pg = g.processFrame(st["rgb"][k], st["depth"][k], inPose=None if k < 3 else (tracked[0] if tracked[0] is not None else po))
        if k == 2:
            m = o.download(); m["pc"][:, 3] = 20.0; o.upload(m)
        assert np.abs(pg - po).max() < 5e-5, k
    assert len(log["o"]) == len(log["g"]) >= 2
    so, sg = log["o"][0], log["g"][0]
    assert np.array_equal(so[2], sg[2]) and len(so[2]) > 20                 # constraint times
    assert np.array_equal(so[0], sg[0]) and np.abs(so[1] - sg[1]).max() < 5e-5   # src = currPose * v exact, dst = estPose * v to the estimate's tolerance
    assert np.array_equal(so[3], sg[3])                                   # graph samples
    assert g.count == o.count
    mo, mg = o.download(), g.download()
    assert np.abs(mo["pc"] - mg["pc"]).max() < 2e-4 and np.array_equal(mo["tm"][:, 0], mg["tm"][:, 0])
    o.close(); g.close()



# ---------------------------------------------------------------- 8f-3: the GPU contacts of the fern data base (EF/Ferns.cpp)
def test_fern_callback_global_deformation(ifx, orc, small_stream):
    """The place of Ferns::findFrame and the global deformation inside a frame (EF/ElasticFusion.cpp:457-514): the callback runs every frame on the
    predict() at the tracked pose (its resampled fill-in images are what findFrame reads), a produced graph is applied by this frame's clean as a
    fern deformation, currPose = recoveryPose, and the local detection of that frame is skipped (:516).  Same callback on both sides, exact."""
    st = small_stream
    kw = dict(time_delta=3, confidence=2.0)
    o = orc.Oracle(**SMALL, max_surfels=400000, **kw)
    g = ifx.ElasticFusion(**SMALL, max_surfels=400000, **kw)
    g.set_option("compact_every_frame", 1)
    o.set_loop_closure(True); g.set_loop_closure(True)
    log = {"o": [], "g": []}
    tracked = [None]
    DEFORM_AT = 4   # callback number (= frame index 5)

    def make_cb(tag):
        def cb(e):
            if tag == "o":
                tracked[0] = e.get_pose()
            log[tag].append(e.fern_frame())
            if len(log[tag]) != DEFORM_AT:
                return False
            s = e.sample_graph_model()
            e.set_deformation(_random_graph(s, np.random.RandomState(5)), is_fern=True)
            p2 = tracked[0].copy(); p2[:3, 3] += np.array([0.003, -0.002, 0.004], np.float32)
            e.adopt_pose(p2)
            return True
        return cb

    with pytest.raises(RuntimeError):
        g.adopt_pose(np.eye(4, dtype=np.float32))                      # only inside the callback
    o.set_fern_callback(make_cb("o")); g.set_fern_callback(make_cb("g"))
    po = None
    for k in range(8):
        if k >= 1:
            m, tick0, po_prev = o.download(), o.tick, po
        po = o.process_frame(st["rgb"][k], st["depth"][k])
        if k >= 1:
            g.upload(m); g.set_pose(po_prev, tick0)
        pg = g.processFrame(st["rgb"][k], st["depth"][k], inPose=None if k < 1 else tracked[0])
        assert len(log["o"]) == len(log["g"]) == k, k                  # every frame after the first
        if k >= 1:
            assert np.array_equal(pg, po), k
            for a, b in zip(log["o"][-1], log["g"][-1]):                # findFrame's four images
                assert np.array_equal(a, b), k
            assert (log["g"][-1][1][..., 2] > 0).mean() > 0.9
            do, dg = o.loop_closure_diag(), g.loop_closure_diag()
            assert do["ran"] == dg["ran"] == (len(log["g"]) != DEFORM_AT and do["inactive_pixels"] > 0), k
            if len(log["g"]) == DEFORM_AT:
                assert np.abs(pg[:3, 3] - tracked[0][:3, 3]).max() > 1e-3      # the adopted pose
            mo, mg = o.download(), g.download()
            for key in MAP_KEYS:
                assert np.array_equal(mo[key], mg[key]), (k, key)
        g.fern_frame_async()                                            # the same read-back enqueued behind the frame and fetched later
        for a, b in zip(o.fern_frame(), g.fern_frame()):                # addFrame's four images (end-of-frame predict)
            assert np.array_equal(a, b), k
        for a, b in zip(o.fern_frame(), g.fern_frame_fetch()):
            assert np.array_equal(a, b), k
        if k == 2:                                                      # everything stable from here on: an old model comes into being
            m2 = o.download(); m2["pc"][:, 3] = 20.0; o.upload(m2)
    assert len(log["g"]) > DEFORM_AT
    o.close(); g.close()


def test_fern_hooks(ifx, orc, small_stream):
    """(1) the resampled fill-in / instance images Ferns::addFrame and findFrame read back; (2) the ICP-only, single-scale tracker on two small
    renders (keyframe against current frame, Ferns.cpp:558-592) against the oracle's tracker fed the same maps."""
    st = small_stream
    W, H = SMALL["w"], SMALL["h"]
    g = ifx.ElasticFusion(**SMALL, max_surfels=400000)
    frames = []
    for k in range(4):
        pose = g.processFrame(st["rgb"][k], st["depth"][k])
        img, v, n, inst = g.fern_frame()
        rw, rh = W // 8, H // 8
        ys = (np.arange(rh) * H + H // 2) // rh
        xs = (np.arange(rw) * W + W // 2) // rw
        assert np.array_equal(img, g.image("fill_image")[ys][:, xs][..., :3]) and np.array_equal(inst, g.image("pred_inst")[ys][:, xs][..., :3])
        assert np.array_equal(v, g.image("fill_vertex")[ys][:, xs]) and np.array_equal(n, g.image("fill_normal")[ys][:, xs])
        assert (v[..., 2] > 0).mean() > 0.9
        # for the tracker below: the same maps at 1/4 (80 x 60, the fern resolution of a 640 x 480 stream; 40 x 30 is not a valid pyramid size)
        y4, x4 = (np.arange(H // 4) * H + H // 2) // (H // 4), (np.arange(W // 4) * W + W // 2) // (W // 4)
        frames.append((pose.copy(), g.image("fill_vertex")[y4][:, x4].copy(), g.image("fill_normal")[y4][:, x4].copy(), g.image("fill_image")[y4][:, x4][..., :3].copy()))
    # keyframe = frame 1, current = frame 3; handle configured as Ferns::findFrame drives its RGBDOdometry
    KS = dict(w=W // 4, h=H // 4, fx=SMALL["fx"] / 4, fy=SMALL["fy"] / 4, cx=SMALL["cx"] / 4, cy=SMALL["cy"] / 4)
    small = ifx.ElasticFusion(**KS, max_surfels=1000, icp_weight=100.0, pyramid=0, so3=0)
    (pm, vm, nm, im), (pc_, vc, nc, ic_) = frames[1], frames[3]
    est_g, dg = small.track_maps(vm, nm, vc, nc, pm)
    L = orc.lib()
    t = L.orc_tracker_create(KS["w"], KS["h"], KS["fx"], KS["fy"], KS["cx"], KS["cy"])
    rgba0 = np.zeros((KS["h"], KS["w"], 4), np.uint8)
    pose_o = np.ascontiguousarray(pm, np.float32).reshape(16).copy()
    diag_o = np.zeros(8, np.float32)
    L.orc_tracker_init_model(t, orc.ptr(np.ascontiguousarray(vm)), orc.ptr(np.ascontiguousarray(nm)), orc.ptr(rgba0), orc.ptr(pose_o))
    L.orc_tracker_init_frame_maps.argtypes = [C.c_void_p] * 4
    L.orc_tracker_init_frame_maps(t, orc.ptr(np.ascontiguousarray(vc)), orc.ptr(np.ascontiguousarray(nc)), orc.ptr(rgba0))
    L.orc_tracker_run(t, orc.ptr(pose_o), 100.0, 0, 0, 0, orc.ptr(diag_o))
    L.orc_tracker_destroy(t)
    assert dg[1] == diag_o[1] > 300 and abs(dg[0] - diag_o[0]) <= 1e-3 * diag_o[0]
    assert np.abs(est_g - pose_o.reshape(4, 4)).max() < 1e-5
    assert np.abs(est_g - pm).max() > 1e-4                                  # it did move away from its start
    # with images and the default weights (ICP + RGB, 3 levels): the model-to-model configuration on host maps, at 1/2 resolution (at 80 x 60 the coarsest
    # level has 300 pixels and its 6x6 system is so poorly conditioned that the unpivoted device solve and the pivoted oracle solve part ways)
    y2, x2 = (np.arange(H // 2) * H + H // 2) // (H // 2), (np.arange(W // 2) * W + W // 2) // (W // 2)
    KH = dict(w=W // 2, h=H // 2, fx=SMALL["fx"] / 2, fy=SMALL["fy"] / 2, cx=SMALL["cx"] / 2, cy=SMALL["cy"] / 2)
    g2 = ifx.ElasticFusion(**SMALL, max_surfels=400000)
    half = []
    for k in range(3):
        pose = g2.processFrame(st["rgb"][k], st["depth"][k])
        half.append((pose.copy(), g2.image("fill_vertex")[y2][:, x2].copy(), g2.image("fill_normal")[y2][:, x2].copy(), g2.image("fill_image")[y2][:, x2].copy()))
    g2.close()
    (pm, vm, nm, im), (pc_, vc, nc, ic_) = half[1], half[2]
    full = ifx.ElasticFusion(**KH, max_surfels=1000, so3=0)
    est2, d2 = full.track_maps(vm, nm, vc, nc, pm, model_rgba=im, cur_rgba=ic_)
    t = L.orc_tracker_create(KH["w"], KH["h"], KH["fx"], KH["fy"], KH["cx"], KH["cy"])
    pose_o2 = np.ascontiguousarray(pm, np.float32).reshape(16).copy()
    L.orc_tracker_init_model(t, orc.ptr(np.ascontiguousarray(vm)), orc.ptr(np.ascontiguousarray(nm)), orc.ptr(np.ascontiguousarray(im)), orc.ptr(pose_o2))
    L.orc_tracker_init_frame_maps(t, orc.ptr(np.ascontiguousarray(vc)), orc.ptr(np.ascontiguousarray(nc)), orc.ptr(np.ascontiguousarray(ic_)))
    L.orc_tracker_run(t, orc.ptr(pose_o2), 10.0, 1, 0, 0, orc.ptr(diag_o))
    for l in range(3):                                                    # the second tracker's pyramids, buffer by buffer
        for name, dt, ch in (("vmap_curr", np.float32, 3), ("nmap_prev", np.float32, 3), ("next_depth", np.float32, 1), ("last_img", np.uint8, 1), ("didx", np.int16, 1)):
            w_, h_ = KH["w"] >> l, KH["h"] >> l
            n_ = w_ * h_ * ch * np.dtype(dt).itemsize
            a = np.frombuffer((C.c_char * n_).from_address(L.orc_tracker_buffer(t, name.encode(), l)), dt).reshape((ch, h_, w_) if ch > 1 else (h_, w_))
            assert nan_equal(a.astype(np.float64), full.tracker_buffer(name, l, m2m=True).astype(np.float64)), (l, name)
    L.orc_tracker_destroy(t)
    assert abs(d2[1] - diag_o[1]) <= max(2.0, 0.002 * diag_o[1]) and d2[3] == diag_o[3] and np.abs(est2 - pose_o2.reshape(4, 4)).max() < 2e-5
    g.close(); small.close(); full.close()


def test_loop_closure_scheduling_equivalence(ifx, small_stream):
    """The model-to-model tracker runs on a stream of its own, under the map passes and the next frame's tracker: every scheduling variant (one
    stream, plain, announced next frame, host-buffer entry point) must give the same verdict sequence bit for bit -- and the same frames as without
    the detection."""
    import torch

    st = small_stream
    seq = list(range(10)) + list(range(8, 0, -1))
    n = len(seq)
    d_rgb = torch.from_numpy(st["rgb"][seq].copy()).cuda()
    d_dep = torch.from_numpy(st["depth"][seq].view(np.int16).copy()).cuda()
    torch.cuda.synchronize()
    kw = dict(time_delta=3, confidence=1.5)
    thr = 35000 * (SMALL["w"] * SMALL["h"]) // (640 * 480)

    def run(mode):
        g = ifx.ElasticFusion(**SMALL, max_surfels=400000, **kw)
        if mode != "off":
            g.set_loop_closure(True, thr, 1e-4, 1e-5)
        if mode == "single":
            g.set_option("two_streams", 0)
        verdicts = []
        for i in range(n):
            if mode == "host":
                g.processFrame(st["rgb"][seq[i]], st["depth"][seq[i]])
            else:
                if mode == "hint" and i + 1 < n:
                    g.hint_next_frame_device(d_rgb[i + 1].data_ptr(), d_dep[i + 1].data_ptr())
                g.enqueue_frame_device(d_rgb[i].data_ptr(), d_dep[i].data_ptr(), i)
            if mode != "off" and (mode in ("host", "single") or i % 3 == 2):      # reading the verdict waits for the third stream: not after every frame
                d = g.loop_closure_diag()
                verdicts.append((i, d["ran"], d["inactive_pixels"], d["icp_count"], d["icp_error"], d["accepted"], d["est_pose"].tobytes()))
        g.sync()
        d = g.loop_closure_diag() if mode != "off" else None
        out = (g.trajectory(), g.download(), g.image("ids_after"), verdicts, d["candidates"] if d else 0)
        g.close()
        return out

    ref = run("single")
    assert ref[4] >= 0 and any(v[1] for v in ref[3]) and any(v[2] > 1000 for v in ref[3])       # the tracker did run on populated renders
    for mode in ("plain", "hint", "host", "off"):
        t, m, ids, verdicts, cand = run(mode)
        assert np.array_equal(t[:n], ref[0][:n]), mode
        assert all(np.array_equal(m[k], ref[1][k]) for k in MAP_KEYS) and np.array_equal(ids, ref[2]), mode
        if mode == "off":
            continue
        assert cand == ref[4], mode
        want = {v[0]: v for v in ref[3]}
        for v in verdicts:
            assert v == want[v[0]], (mode, v[0])


# ---------------------------------------------------------------- a1: the instanceGT argument of processFrame + computePrecisionAndRecall (evaluateAndSave)
def test_instance_ground_truth_and_precision_recall(ifx, orc, small_stream):
    from instancefusion_amd import synth

    st = small_stream
    g = ifx.ElasticFusion(**SMALL, max_surfels=400000, confidence=2.0)
    g.set_option("compact_every_frame", 1)
    o = orc.Oracle(**SMALL, max_surfels=400000, confidence=2.0)
    inst = ifx.InstanceFusion(g)
    for k in range(6):
        gt = (st["obj"][k] % 250).astype(np.uint8) if k >= 1 else None          # no ground truth for the first frames, then one per frame
        g.set_instance_gt(gt); o.set_instance_gt(gt)
        po = o.process_frame(st["rgb"][k], st["depth"][k])
        g.processFrame(st["rgb"][k], st["depth"][k])
    m = o.download(); m["pc"][:, 3] = 20.0                                       # every surfel stable, so that the segmentation below labels some
    g.upload(m); o.upload(m); g.set_pose(po, o.tick); o.set_pose(po, o.tick)     # identical maps from here on
    g.processFrame(st["rgb"][5], st["depth"][5], inPose=po); o.process_frame(st["rgb"][5], st["depth"][5], in_pose=po)
    mg, mo = g.download(), o.download()
    assert np.array_equal(mg["ic"], mo["ic"])
    w = mo["ic"][:, 3]
    assert (w == -1).any() and (w >= 0).sum() > 1000 and set(np.unique(w[w >= 0]).astype(int)) <= set(np.unique(st["obj"][1:6] % 250).astype(int))
    masks, cls = synth.canned_masks(st["obj"][5], st["scene"])
    inst.ProcessSegmentation(st["rgb"][5], st["depth"][5], masks, cls, 5)
    o.process_segmentation(st["rgb"][5], st["depth"][5], masks, cls, 5)
    pg, po_ = inst.precision_recall(), o.precision_recall()
    for a, b in zip(pg, po_):
        assert np.array_equal(a, b)
    assert po_[1].sum() == (w >= 0).sum() and po_[0].sum() > 0 and po_[2].sum() > 0
    g.set_instance_gt(None); o.set_instance_gt(None)                             # switched off: new surfels carry -2 again
    g.processFrame(st["rgb"][6], st["depth"][6], inPose=po); o.process_frame(st["rgb"][6], st["depth"][6], in_pose=po)
    assert np.array_equal(g.download()["ic"], o.download()["ic"]) and (o.download()["ic"][:, 3] == -2).any()
    g.close(); o.close()
