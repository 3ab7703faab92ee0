"""Reference driver for the relocalisation mode (`reloc`) and `frameToFrameRGB` of ElasticFusion::processFrame.

The CPU oracle has neither option, so the expected values of tests/test_reloc_cpu.py and tests/test_gpu_reloc.py come from this composition of the oracle's
stage calls in the reference's order (EF/ElasticFusion.cpp:330-431, 453-484, 620, 700-763).  Per frame:

  1. orc_set_frame;
  2. a fresh orc_tracker: init_first_rgb(previous frame), init_model(fill_* if the prediction is not dense enough else pred_*; with frameToFrameRGB the image is
     always the fill-in image), init_frame(filtered depth, rgb, 20), run, orc_tracker_covariance;
  3. the gate of :371-423, here in Python (`gate`);
  4. a frame that fuses: orc_process_frame(in_pose = the tracked pose) -- with no option set this reproduces orc_process_frame's own poses bit for bit;
  5. a skipped frame: the pose is adopted, predict() with the window (0, tick) after a recovery, and the tick advances unless lost;
  6. the passthrough fill-in images come from a second Oracle that never received a surfel: its fill-in takes the empty-sample branch at every pixel, which is the
     shaders' passthrough branch (`sample.z == 0 || passthrough == 1`, EF/Shaders/FillIn.cpp:65-195).

Test infrastructure only."""
from __future__ import annotations

import ctypes as C

import numpy as np

ERR_GATE = np.float32(1e-4)   # frameToModel.lastICPError < 1e-4f
COV_GATE = 1e-04              # covariance(i, i) > 1e-04, f64


def gate(err, cov_diag, lost, recovery, count):
    """EF/ElasticFusion.cpp:371-423.  Returns (ok, lost, lastFrameRecovery, trackingCount)."""
    ok = bool(np.float32(err) < ERR_GATE)   # NaN: False
    cov_ok = not any(float(c) > COV_GATE for c in cov_diag)
    if not lost:
        ok = ok and cov_ok
        if not ok:
            count += 1
            if count > 10:
                lost = True
        else:
            count = 0
    elif recovery:
        ok = ok and cov_ok
        if ok:
            lost, count = False, 0
        recovery = False
    return ok, lost, recovery, count


def dense_enough(pred_image):
    """ElasticFusion::denseEnough (EF/ElasticFusion.cpp:252-267) on the (w/20 x h/20) nearest resample"""
    h, w = pred_image.shape[:2]
    rw, rh = w // 20, h // 20
    sx = (np.arange(rw) * w + w // 2) // rw
    sy = (np.arange(rh) * h + h // 2) // rh
    s = pred_image[np.ix_(sy, sx)][..., :3]
    lit = int(((s[..., 0] > 0) & (s[..., 1] > 0) & (s[..., 2] > 0)).sum())
    return np.float32(lit) / np.float32(rw * rh) > np.float32(0.75)


class RelocReference:
    def __init__(self, ol, w, h, fx, fy, cx, cy, max_surfels=1 << 18, reloc=True, frame_to_frame_rgb=False, loop_closure=True, time_delta=200, **cfg):
        self.ol, self.L = ol, ol.lib()
        self.K = dict(w=w, h=h, fx=fx, fy=fy, cx=cx, cy=cy)
        self.o = ol.Oracle(max_surfels=max_surfels, time_delta=time_delta, **self.K, **cfg)
        self.empty = ol.Oracle(max_surfels=16, time_delta=time_delta, **self.K, **cfg)   # never receives a surfel
        self.loop_closure = loop_closure
        if loop_closure:
            self.o.set_loop_closure(True)
        self.reloc, self.f2f = reloc, frame_to_frame_rgb
        self.lost, self.recovery, self.count = False, False, 0
        self.prev_rgb = None
        self.fill = None   # the fill-in images of the last predict(), passthrough applied

    # -- passthrough
    def raw_images(self, rgb, depth, pose):
        """fill_vertex / fill_normal / fill_image of a map without surfels: the frame itself"""
        self.empty.set_frame(rgb, depth)
        self.empty.combined_predict(pose, 1, 1)
        return {k: self.empty.image("fill_" + k) for k in ("vertex", "normal", "image")}

    def raw_fern_frame(self, rgb, depth, pose):
        self.raw_images(rgb, depth, pose)
        return self.empty.fern_frame()

    def _take_fill(self, rgb, depth, pose):
        mask = 3 if self.lost else (2 if self.f2f else 0)
        self.fill = {k: self.o.image("fill_" + k) for k in ("vertex", "normal", "image")}
        if mask:
            raw = self.raw_images(rgb, depth, pose)
            if mask & 1:
                self.fill["vertex"], self.fill["normal"] = raw["vertex"], raw["normal"]
            if mask & 2:
                self.fill["image"] = raw["image"]
        self.mask = mask

    # -- tracker of one frame
    def _track(self, rgb, pose):
        ol, L, o = self.ol, self.L, self.o
        fill = not dense_enough(o.image("pred_image"))
        V = self.fill["vertex"] if fill else o.image("pred_vertex")
        N = self.fill["normal"] if fill else o.image("pred_normal")
        img = self.fill["image"] if (fill or self.f2f) else o.image("pred_image")
        V, N, img = (np.ascontiguousarray(a) for a in (V, N, img))
        t = L.orc_tracker_create(self.K["w"], self.K["h"], self.K["fx"], self.K["fy"], self.K["cx"], self.K["cy"])
        prev = np.ascontiguousarray(self.prev_rgb, np.uint8)
        L.orc_tracker_init_first_rgb(t, ol.ptr(prev))
        p = np.ascontiguousarray(pose, np.float32).reshape(16).copy()
        L.orc_tracker_init_model(t, ol.ptr(V), ol.ptr(N), ol.ptr(img), ol.ptr(p))
        df = np.ascontiguousarray(o.image("depth_filtered"))
        cur = np.ascontiguousarray(rgb, np.uint8)
        L.orc_tracker_init_frame(t, ol.ptr(df), ol.ptr(cur), 20.0)
        diag = np.zeros(8, np.float32)
        L.orc_tracker_run(t, ol.ptr(p), 10.0, 1, 0, 1, ol.ptr(diag))
        cov = np.zeros(36)
        L.orc_tracker_covariance.argtypes = [C.c_void_p, C.c_void_p]
        L.orc_tracker_covariance(t, ol.ptr(cov))
        lastA = np.frombuffer((C.c_double * 36).from_address(L.orc_tracker_buffer(t, b"lastA", 0)), np.float64).reshape(6, 6).copy()
        L.orc_tracker_destroy(t)
        return p.reshape(4, 4), diag, cov.reshape(6, 6), lastA

    def frame(self, rgb, depth, adopt=None, in_pose=None):
        """One processFrame.  adopt: the recovery pose the fern lookup of this frame returns (taken only while lost, EF/ElasticFusion.cpp:478-484).
        in_pose: the frame takes its pose from the caller: it is not judged (:334, :428-431), fuses unless the map is lost (not restated here: asserted),
        and the tracker's "previous image" stays the last tracked frame's (RGBDOdometry::initRGB is only reached by the tracking branch).
        Returns what the tests compare: pose, status (1 while lost), ok, lost, recovery, count, tick, surfels, fused, err, cov_diag, lastA."""
        o = self.o
        out = dict(ok=True, err=0.0, cov_diag=np.zeros(6), lastA=None, cov=None)
        if o.tick == 1:
            pose = o.process_frame(rgb, depth)
            fused = True
        elif in_pose is not None:
            assert not self.lost
            pose = o.process_frame(rgb, depth, in_pose=in_pose)
            fused = True
        else:
            o.set_frame(rgb, depth)
            pose, diag, cov, lastA = self._track(rgb, o.get_pose())
            ok = True
            if self.reloc:
                ok, self.lost, self.recovery, self.count = gate(diag[0], np.diag(cov), self.lost, self.recovery, self.count)
            out.update(ok=ok, err=float(diag[0]), cov_diag=np.diag(cov).copy(), lastA=lastA, cov=cov)
            fused = ok and not self.lost
            if fused:
                pose = o.process_frame(rgb, depth, in_pose=pose)
            else:
                tick = o.tick
                if self.loop_closure:
                    self.recovery = False                      # :455
                    if adopt is not None and self.lost:        # :478-484
                        pose = np.ascontiguousarray(adopt, np.float32).reshape(4, 4)
                        self.recovery = True
                o.set_pose(pose, tick)
                o.combined_predict(pose, 0 if self.recovery else tick, tick)   # predict(), :729-763
                o.set_pose(pose, tick if self.lost else tick + 1)              # :713-717
        self._take_fill(rgb, depth, pose)
        if in_pose is None:
            self.prev_rgb = np.array(rgb, np.uint8, copy=True)
        out.update(pose=np.array(pose, np.float32).reshape(4, 4), status=1 if self.lost else 0, lost=self.lost, recovery=self.recovery, count=self.count, tick=o.tick,
                   surfels=o.count, fused=fused)
        return out


SCENARIO = dict(w=160, h=120, fx=132.0, fy=132.0, cx=80.0, cy=60.0)
SCENARIO_FRAMES = 24
ADOPT_FRAME = 19


def scenario_stream():
    """synth.make_stream(24, noise=True) at 160x120; the depth of frames 6-17 is zeroed outside rows 48-71 x columns 64-95"""
    from instancefusion_amd import synth

    K = SCENARIO
    st = synth.make_stream(SCENARIO_FRAMES, K["w"], K["h"], K["fx"], K["fy"], K["cx"], K["cy"], noise=True)
    depth = st["depth"].copy()
    for i in range(6, 18):
        keep = depth[i, 48:72, 64:96].copy()
        depth[i] = 0
        depth[i, 48:72, 64:96] = keep
    return dict(rgb=st["rgb"], depth=depth, poses=st["poses"])


_scenario_cache = {}


def scenario_run(ol):
    """The scenario through the driver, once per session, shared and left unchanged by the tests: (stream, per-frame records, maps after frames 15 / 19 / 23,
    ids_after after frame 23, the driver)."""
    if "run" not in _scenario_cache:
        st = scenario_stream()
        d = RelocReference(ol, **SCENARIO)
        recs, maps = [], {}
        for i in range(SCENARIO_FRAMES):
            adopt = st["poses"][ADOPT_FRAME] if i == ADOPT_FRAME else None
            recs.append(d.frame(st["rgb"][i], st["depth"][i], adopt=adopt))
            if i in (15, 19, 23):
                maps[i] = d.o.download()
        ids = d.o.image("ids_after")
        _scenario_cache["run"] = (st, recs, maps, ids, d)
    return _scenario_cache["run"]
