"""What ifx_render_view costs on the bench workload's map (5 M synthetic surfels, as tools/id_rule_cost.py builds it): device outputs, HIP events on the
handle's main stream around the call, warm-up first, the median of the repeats; then the per-kernel times (option kernel_timing) of its three launches.
Two viewports at the tracked pose (640x480, 1280x960) and a close-up (15 cm from the nearest surface on the optical axis, 640x480), where the big-quad
path carries the load; the length of the big-quad list each time.  Beside it, in the same run: the whole-image quad render of the id rule
(ifx_render_ids under option id_rule = 1: k_raster_quad + k_ids_resolve), which reads the same records.

    python tools/view_render_cost.py [surfels] [repeats]"""
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402  (first: libifx.so binds to the HIP runtime torch ships)

import instancefusion_amd as ifx  # noqa: E402
from instancefusion_amd import synth  # noqa: E402

n = int(sys.argv[1]) if len(sys.argv) > 1 else 5_000_000
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 30
W, H = 640, 480
K = dict(fx=528.0, fy=528.0, cx=320.0, cy=240.0)
st = synth.make_stream(2, W, H, noise=True, loop_len=90, **K)
m = synth.make_map(n, st["scene"], st["poses_world"][0], 1000)
pose = np.asarray(st["poses"][0], np.float64).reshape(4, 4)

ef = ifx.ElasticFusion(w=W, h=H, max_surfels=n + 1_500_000, id_rule=ifx.ID_RULE_REFERENCE, **K)
ef.upload(m); ef.set_pose(pose.astype(np.float32), 1000)
L = ef.L
ms, ss = C.c_void_p(), C.c_void_p()
assert L.ifx_stream_handles(ef.handle, C.byref(ms), C.byref(ss)) == 0
main = torch.cuda.ExternalStream(ms.value)
thr = float(ef.cfgd["confidence"])
drawable = (m["col"][:, 1] != -1.0) & (m["pc"][:, 3] > thr)
print(f"view_render_cost: {n} surfels ({int(drawable.sum())} stable with an instance-colour word other than -1), {reps} repeats, median [min .. max] in us")

# the close-up: forward along the optical axis to 15 cm from the nearest stable surface within 8 px of it
Ti = np.linalg.inv(pose)
q = m["pc"][:, :3].astype(np.float64) @ Ti[:3, :3].T + Ti[:3, 3]
with np.errstate(all="ignore"):
    near_axis = (q[:, 2] > 0.2) & (np.hypot(K["fx"] * q[:, 0] / q[:, 2], K["fy"] * q[:, 1] / q[:, 2]) < 8) & drawable
fwd = np.eye(4); fwd[2, 3] = float(q[near_axis, 2].min()) - 0.15
close = pose @ fwd


def timed(call):
    for _ in range(5):
        call()
    ef.sync()
    ev = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(main)
        call()
        b.record(main)
        b.synchronize()
        ev.append(a.elapsed_time(b) * 1e3)
    ev = np.asarray(ev)
    return f"{np.median(ev):8.1f} [{ev.min():8.1f} .. {ev.max():8.1f}]"


def kernels(call, names):
    ef.set_option("kernel_timing", 1); ef.kernel_ms("__reset__")
    for _ in range(10):
        call()
    ef.sync()
    out = ", ".join(f"{nm} {ef.kernel_ms(nm)[0] * 1e3:.1f}" for nm in names)
    ef.set_option("kernel_timing", 0)
    return out


for name, (w, h), T in (("tracked pose", (640, 480), pose), ("tracked pose", (1280, 960), pose), ("close-up", (640, 480), close)):
    s = w / 640.0
    p = ifx.ViewParams()
    mvp = ifx.viewer_mvp(K["fx"] * s, K["fy"] * s, K["cx"] * s, K["cy"] * s, w, h, 0.1, 1000.0, T)
    p.mvp[:] = [float(v) for v in mvp.reshape(16)]
    p.w, p.h, p.threshold, p.color_type, p.unstable, p.draw_window, p.time, p.time_delta = w, h, float("nan"), 4, 0, 0, -1, -1
    p.clear_rgb[:] = [1.0, 1.0, 1.0]
    rgba = torch.empty((h, w, 4), dtype=torch.float32, device="cuda")
    ids = torch.empty((h, w), dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()

    def call():
        assert L.ifx_render_view(ef.handle, C.byref(p), None, None, C.c_void_p(rgba.data_ptr()), C.c_void_p(ids.data_ptr())) == 0

    t = timed(call)
    big = L.ifx_render_view_big_quads(ef.handle)
    drawn = int((ids >= 0).sum())
    print(f"  ifx_render_view {name:12s} {w}x{h}: {t}   big-quad list {big}, {drawn} pixels drawn; kernels (us): {kernels(call, ('view_quad', 'view_big', 'view_resolve'))}")

pose32 = np.ascontiguousarray(pose, np.float32).reshape(16)


def ids_call():
    assert L.ifx_render_ids(ef.handle, pose32.ctypes.data_as(C.c_void_p), 0) == 0


print(f"  ifx_render_ids (id_rule 1) tracked pose {W}x{H}: {timed(ids_call)}   kernels (us): {kernels(ids_call, ('ids_raster_quad', 'ids_resolve'))}")
ef.close()
