"""Relocalisation (`reloc`) and frame-to-frame RGB (`frameToFrameRGB`) on the GPU: the passthrough fill-in kernel, the tracking gate and the frame path built on
them, against the reference driver of tests/reloc_reference.py (the CPU oracle's stage calls in the reference's order)."""
import numpy as np
import pytest

import reloc_reference as rr
from conftest import SMALL, assert_pose_equal

pytestmark = pytest.mark.gpu

MAP_KEYS = ("pc", "nr", "col", "tm", "ic", "votes")
E_INVALID, E_STATE = -1, -4


@pytest.fixture(scope="module")
def ifx():
    import instancefusion_amd as m

    m.lib()
    return m


def _same(a, b):
    """equal bit for bit, but for the sign of a NaN: a normal over a hole in the depth is 0 * inf on both sides, and the two processors' default NaNs differ in the sign bit"""
    return np.array_equal(a, b, equal_nan=np.issubdtype(np.asarray(a).dtype, np.floating))


def _maps_equal(mg, mo, what):
    assert mg["pc"].shape == mo["pc"].shape, (what, mg["pc"].shape, mo["pc"].shape)
    for k in MAP_KEYS:
        assert np.array_equal(mg[k], mo[k]), f"map field {k} differs {what}"


# ------------------------------------------------------------------ 1. the scenario
@pytest.mark.parametrize("compact_every_frame", [1, 0])
def test_scenario_lost_and_recovered(ifx, orc, compact_every_frame):
    """24 frames at 160x120; the depth of frames 6-17 is masked down to a 32x24 window: frames 6-18 fail the gate, the map is lost at frame 16, the fern callback of
    frame 19 adopts a pose, frame 20 confirms it and fuses again.  Per frame: pose, return code, verdict, tick and surfel count are the driver's; the whole map after
    frames 15, 19 and 23; with compact_every_frame (slot numbers = the oracle's indices) also ids_after after frame 23.  compact_every_frame = 0 is the default frame
    path: cached view lists, hot records and the fused clean + raster walk live through fourteen skipped frames."""
    st, recs, maps, ids, d = rr.scenario_run(orc)
    g = ifx.ElasticFusion(max_surfels=1 << 18, time_delta=200, **rr.SCENARIO)
    g.set_option("compact_every_frame", compact_every_frame)
    g.set_loop_closure(True)
    g.set_option("reloc", 1)
    frame = {"i": 0}
    seen = {}

    def fern(ef):
        i = frame["i"]
        if ef.reloc_state()["lost"]:
            seen[i] = ef.fern_frame()
        if i == rr.ADOPT_FRAME:
            ef.adopt_pose(st["poses"][i])
        return False

    g.set_fern_callback(fern)
    for i in range(rr.SCENARIO_FRAMES):
        frame["i"] = i
        r = recs[i]
        pg = g.processFrame(st["rgb"][i], st["depth"][i])
        assert_pose_equal(pg, r["pose"], f"frame {i}")
        s = g.reloc_state()
        print(f"frame {i:2d}: status {g.last_frame_status} ok {int(s['ok'])} lost {int(s['lost'])} rec {int(s['last_frame_recovery'])} count {s['tracking_count']} err {s['icp_error']:.3e} "
              f"cov {s['cov_diag'].max():.3e} tick {g.tick} surfels {g.count} fused {int(s['fused'])}")
        assert g.last_frame_status == r["status"], i
        if i > 0:
            assert (s["ok"], s["lost"], s["last_frame_recovery"], s["tracking_count"]) == (r["ok"], r["lost"], r["recovery"], r["count"]), (i, s, r)
            assert s["fused"] == r["fused"], i
        assert g.tick == r["tick"], (i, g.tick, r["tick"])
        assert g.count == r["surfels"], (i, g.count, r["surfels"])
        if i in maps:
            _maps_equal(g.download(), maps[i], f"after frame {i}")
    assert [i for i, r in enumerate(recs) if r["status"] == 1] == [16, 17, 18, 19]
    assert sorted(seen) == [16, 17, 18, 19], "the fern callback ran on every lost frame"
    for i, got in seen.items():   # while lost the fern data base sees the raw frame
        want = d.raw_fern_frame(st["rgb"][i], st["depth"][i], np.eye(4))
        for a, b, name in zip(got, want, ("image", "vertex", "normal", "instances")):
            assert _same(a, b), f"fern frame ({name}) of lost frame {i}"
    if compact_every_frame:
        assert np.array_equal(g.image("ids_after"), ids), "ids_after after frame 23"
    assert len(g.trajectory()) == rr.SCENARIO_FRAMES, "the trajectory takes a pose every frame"


def test_options_are_refused_where_not_offered(ifx):
    g = ifx.ElasticFusion(max_surfels=1000, **rr.SCENARIO)
    g.camera_count(2)
    for name in ("reloc", "frame_to_frame_rgb"):
        assert g.L.ifx_set_option(g.handle, name.encode(), 1) == E_STATE, name
    g.close()


# ------------------------------------------------------------------ 2. every frame OK
def test_all_frames_ok_changes_nothing(ifx, orc, small_stream):
    """small_stream with `reloc` on and off: poses, map and id image equal bit for bit, and equal to the oracle's."""
    st = small_stream
    o = orc.Oracle(max_surfels=400000, time_delta=200, **SMALL)
    o.set_loop_closure(True)
    runs = []
    for reloc in (0, 1):
        g = ifx.ElasticFusion(max_surfels=400000, time_delta=200, **SMALL)
        g.set_option("compact_every_frame", 1)
        g.set_loop_closure(True)
        g.set_option("reloc", reloc)
        poses = [g.processFrame(st["rgb"][i], st["depth"][i]) for i in range(10)]
        if reloc:
            s = g.reloc_state()
            assert s["ok"] and not s["lost"] and s["tracking_count"] == 0 and s["fused"] and g.last_frame_status == 0
        runs.append((poses, g.download(), g.image("ids_after"), g.tick))
        g.close()
    for i in range(10):
        po = o.process_frame(st["rgb"][i], st["depth"][i])
        assert np.array_equal(runs[0][0][i], runs[1][0][i]), f"pose of frame {i} with reloc on / off"
        assert_pose_equal(runs[1][0][i], po, f"frame {i}")
    _maps_equal(runs[0][1], runs[1][1], "with reloc on / off")
    _maps_equal(runs[1][1], o.download(), "against the oracle")
    assert np.array_equal(runs[0][2], runs[1][2]) and np.array_equal(runs[1][2], o.image("ids_after"))
    assert runs[0][3] == runs[1][3] == o.tick


# ------------------------------------------------------------------ 3. the passthrough stage
@pytest.mark.parametrize("w,h", [(160, 120), (168, 124)])   # 168 x 124: partial edge blocks in both grid dimensions (64 x 4 pixels per block)
def test_passthrough_stage(ifx, orc, w, h):
    from instancefusion_amd import synth

    K = dict(w=w, h=h, fx=132.0, fy=132.0, cx=w / 2.0, cy=h / 2.0)
    st = synth.make_stream(3, w, h, K["fx"], K["fy"], K["cx"], K["cy"], noise=True)
    g = ifx.ElasticFusion(max_surfels=1 << 17, **K)
    for i in range(2):
        pose = g.processFrame(st["rgb"][i], st["depth"][i])
    m = g.download()
    m["pc"][:, 3] = 20.0                       # every surfel stable: the prediction draws them
    g.upload(m)
    g.set_pose(pose, g.tick)
    T = g.tick
    dep = st["depth"][2].copy()
    dep[h // 3: h // 2, w // 4: w // 2] = 0   # a hole: zero depth passes through as the empty vertex it is
    g.set_frame(st["rgb"][2], dep)
    e = orc.Oracle(max_surfels=16, **K)       # never received a surfel: the empty-sample branch at every pixel
    e.set_frame(st["rgb"][2], dep)
    e.combined_predict(pose, T, T)
    raw = {k: e.image(k) for k in ("fill_vertex", "fill_normal", "fill_image")}
    names = ("fill_vertex", "fill_normal", "fill_image", "pred_vertex", "pred_normal", "pred_image", "pred_time")
    g.combined_predict(pose, T, T)
    base = {k: g.image(k) for k in names}
    assert (base["pred_vertex"][..., 2] != 0).mean() > 0.5, "the map covers the view: mask 0 and the passthrough differ"
    assert np.isnan(raw["fill_normal"]).any() and not _same(base["fill_vertex"], raw["fill_vertex"]) and not np.array_equal(base["fill_image"], raw["fill_image"])
    for mask in (3, 2, 1):
        g.combined_predict(pose, T, T, passthrough=mask)
        got = {k: g.image(k) for k in names}
        for k in ("fill_vertex", "fill_normal"):
            assert _same(got[k], (raw if mask & 1 else base)[k]), (mask, k)
        assert np.array_equal(got["fill_image"], (raw if mask & 2 else base)["fill_image"]), mask
        for k in names[3:]:
            assert _same(got[k], base[k]), (mask, k)
    g.combined_predict(pose, T, T, passthrough=0)
    for k in names:
        assert _same(g.image(k), base[k]), k
    eye = np.eye(4, dtype=np.float32)
    assert g.L.ifx_combined_predict_ex(g.handle, eye.ctypes.data, 2, 2, 4) == E_INVALID, "a mask outside 0..3"


# ------------------------------------------------------------------ 4. the gate stage
def _numpy_gate(A, err, state):
    cov = np.diag(np.linalg.inv(np.asarray(A, np.float64)))
    ok, lost, rec, count = rr.gate(err, cov, *state)
    return ok, (lost, rec, count), cov


I6 = np.eye(6)
ONE_BAD = np.diag([1e5, 1e5, 5e3, 1e5, 1e5, 1e5])
GOOD_ERR, BAD_ERR = np.float32(5e-5), np.float32(3e-4)


def _check(g, A, err, state, cov_rtol=1e-12):
    ok, st, cov = g.reloc_gate(A, err, state)
    wok, wst, wcov = _numpy_gate(A, err, state)
    assert (ok, st) == (wok, wst), (A.diagonal(), err, state, ok, st, wok, wst)
    assert np.allclose(cov, wcov, rtol=cov_rtol, atol=0), (cov, wcov)
    return ok, st


def test_gate_stage(ifx, orc):
    g = ifx.ElasticFusion(max_surfels=1000, **rr.SCENARIO)
    fresh = (False, False, 0)
    assert _check(g, 1e5 * I6, GOOD_ERR, fresh) == (True, (False, False, 0))
    assert _check(g, ONE_BAD, GOOD_ERR, fresh) == (False, (False, False, 1)), "the covariance gate fails alone"
    assert _check(g, 1e4 * I6, GOOD_ERR, fresh) == (True, (False, False, 0)), "a covariance of exactly 1e-4 is not greater"
    assert np.diag(np.linalg.inv(1e4 * I6)).max() == 1e-4
    assert _check(g, 1e5 * I6, np.float32(1e-4), fresh) == (False, (False, False, 1)), "an error of exactly 1e-4f is not below"
    assert _check(g, 1e5 * I6, np.float32(np.nan), fresh) == (False, (False, False, 1)), "a NaN error is not ok"
    assert _check(g, 1e5 * I6, np.nextafter(np.float32(1e-4), np.float32(0)), fresh) == (True, (False, False, 0))
    # a general (non-diagonal, pivoting) matrix
    rng = np.random.RandomState(3)
    M = rng.randn(6, 6)
    A = M @ M.T * 1e5 + 1e4 * I6
    A[[0, 3]] = A[[3, 0]]
    _check(g, A, GOOD_ERR, fresh, cov_rtol=1e-12 * np.linalg.cond(A))
    # ten failures then an OK: the count is back at 0, never lost
    s = fresh
    for k in range(10):
        ok, s = _check(g, ONE_BAD if k % 2 else 1e5 * I6, GOOD_ERR if k % 2 else BAD_ERR, s)
        assert not ok and s == (False, False, k + 1)
    assert _check(g, 1e5 * I6, GOOD_ERR, s) == (True, (False, False, 0))
    # eleven failures: lost on the eleventh
    s = fresh
    for k in range(11):
        ok, s = _check(g, 1e5 * I6, BAD_ERR, s)
        assert s == (k == 10, False, k + 1)
    # lost without lastFrameRecovery: the state is untouched for any input
    for A, err in ((1e5 * I6, GOOD_ERR), (ONE_BAD, GOOD_ERR), (1e5 * I6, BAD_ERR), (1e5 * I6, np.float32(np.nan))):
        ok, s2 = _check(g, A, err, (True, False, 11))
        assert s2 == (True, False, 11)
    # lost with lastFrameRecovery: cleared only when error and covariance both pass; lastFrameRecovery cleared either way
    assert _check(g, 1e5 * I6, GOOD_ERR, (True, True, 11)) == (True, (False, False, 0))
    assert _check(g, ONE_BAD, GOOD_ERR, (True, True, 11)) == (False, (True, False, 11))
    assert _check(g, 1e5 * I6, BAD_ERR, (True, True, 11)) == (False, (True, False, 11))
    # a tracked matrix of the scenario (frame 9: the worst conditioned of its run, cond 1.5e3) against orc_tracker_covariance
    st, recs, maps, ids, d = rr.scenario_run(orc)
    r = recs[9]
    ORACLE_VS_NUMPY = 3.45e-15   # largest relative difference between the oracle's inverse and numpy's on this matrix, measured on the CPU
    measured = np.max(np.abs(np.diag(r["cov"]) - np.diag(np.linalg.inv(r["lastA"]))) / np.abs(np.diag(r["cov"])))
    print(f"oracle inverse against numpy on the tracked matrix: {measured:.3e}")
    ok, s3, cov = g.reloc_gate(r["lastA"], r["err"], (False, False, 3))
    print(f"device inverse against the oracle's: {np.max(np.abs(cov - np.diag(r['cov'])) / np.abs(np.diag(r['cov']))):.3e}")
    assert np.allclose(cov, np.diag(r["cov"]), rtol=4 * ORACLE_VS_NUMPY, atol=0)
    assert (ok, s3) == (False, (False, False, 4))


# ------------------------------------------------------------------ 5. frame-to-frame RGB
F2F_CONFIDENCE = 2.5   # confidence threshold of this test's maps: surfels are stable, and drawn, from frame 5 on


def test_frame_to_frame_rgb(ifx, orc):
    """Eight frames of the scenario's stream (its depth as rendered: every frame tracks).  The driver takes the previous raw frame, alpha 255, as the tracker's
    model image; poses per frame and the final map are bit-equal, and the option gives the same run with `reloc` on (every frame OK).  With the default confidence
    threshold (10) a map built from scratch draws nothing for its first ten frames, and the fill-in image is the raw frame with or without the option; at 2.5 the
    prediction carries colour from frame 5 on, and the driver's poses of frames 6 and 7 differ from those of the same driver without the option (measured on the CPU:
    2.2e-4 and 6.8e-3 in the largest entry).  ICP errors of this run on the CPU: 5.2e-5 to 9.2e-5, every frame OK."""
    from instancefusion_amd import synth

    K = rr.SCENARIO
    st = synth.make_stream(rr.SCENARIO_FRAMES, K["w"], K["h"], K["fx"], K["fy"], K["cx"], K["cy"], noise=True)
    d = rr.RelocReference(orc, reloc=True, frame_to_frame_rgb=True, confidence=F2F_CONFIDENCE, **K)
    plain = rr.RelocReference(orc, reloc=True, frame_to_frame_rgb=False, confidence=F2F_CONFIDENCE, **K)
    want, differ = [], []
    for i in range(8):
        r, rp = (drv.frame(st["rgb"][i], st["depth"][i]) for drv in (d, plain))
        assert r["ok"] and r["fused"] and not r["lost"], (i, r["err"], r["cov_diag"])
        want.append(r["pose"])
        if not np.array_equal(r["pose"], rp["pose"]):
            differ.append(i)
    assert differ == [6, 7], "the option changes the run: the test would pass without it otherwise"
    mo = d.o.download()
    raw = d.raw_images(st["rgb"][7], st["depth"][7], want[7])
    for reloc in (0, 1):
        g = ifx.ElasticFusion(max_surfels=1 << 18, time_delta=200, confidence=F2F_CONFIDENCE, frame_to_frame_rgb=True, reloc=bool(reloc), **K)
        g.set_option("compact_every_frame", 1)
        g.set_loop_closure(True)
        for i in range(8):
            assert_pose_equal(g.processFrame(st["rgb"][i], st["depth"][i]), want[i], f"frame {i}, reloc {reloc}")
            assert g.last_frame_status == 0
        _maps_equal(g.download(), mo, f"frame-to-frame RGB, reloc {reloc}")
        assert np.array_equal(g.image("fill_image"), raw["image"]), "the fill image is the raw frame"
        g.close()
