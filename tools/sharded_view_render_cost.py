"""What ifx_owner_render_view costs beside ifx_render_view, on the bench workload's map (5 M synthetic surfels, as tools/view_render_cost.py builds it), 640x480
at the tracked pose, colour and ids to device outputs: the same map on an unsharded handle and on a sharded handle at a world of one (n_ranks = -1, the library's
communicator -- two one-rank RCCL collectives), in one process, the two calls ALTERNATING, HIP events on each handle's main stream around its call, warm-up first,
the median of the repeats.  Then the per-kernel times (option kernel_timing) of both calls, the bytes exchanged (ifx_owner_exchange_stats) and the equality of the
two results (an uploaded map: creation number = row = slot).  No run with more than one rank is made here.

    python tools/sharded_view_render_cost.py [surfels] [repeats]"""
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402  (first: libifx.so binds to the HIP runtime torch ships)

import instancefusion_amd as ifx  # noqa: E402
from instancefusion_amd import sharded, synth  # noqa: E402

n = int(sys.argv[1]) if len(sys.argv) > 1 else 5_000_000
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 30
W, H = 640, 480
K = dict(fx=528.0, fy=528.0, cx=320.0, cy=240.0)
st = synth.make_stream(2, W, H, noise=True, loop_len=90, **K)
m = synth.make_map(n, st["scene"], st["poses_world"][0], 1000)
pose = np.asarray(st["poses"][0], np.float32).reshape(4, 4)

one = ifx.ElasticFusion(w=W, h=H, max_surfels=n + 1_500_000, **K)
own = ifx.ElasticFusion(w=W, h=H, max_surfels=n + 1_500_000, n_ranks=-1, rank=0, **K)
osh = sharded.OwnerShardedElasticFusion(own, None, transport="library")
for e in (one, own):
    e.upload(m); e.set_pose(pose, 1000)
assert one.count == own.count == n
L = one.L


def main_stream(e):
    ms = C.c_void_p()
    assert L.ifx_stream_handles(e.handle, C.byref(ms), None) == 0
    return torch.cuda.ExternalStream(ms.value)


p = ifx.view_params(ifx.viewer_mvp(K["fx"], K["fy"], K["cx"], K["cy"], W, H, 0.1, 1000.0, pose), (W, H), color_type=4)
out = {e: (torch.empty((H, W, 4), dtype=torch.float32, device="cuda"), torch.empty((H, W), dtype=torch.int32, device="cuda")) for e in (one, own)}
torch.cuda.synchronize()


def call_one():
    assert L.ifx_render_view(one.handle, C.byref(p), None, None, C.c_void_p(out[one][0].data_ptr()), C.c_void_p(out[one][1].data_ptr())) == 0


def call_own():
    assert L.ifx_owner_render_view(own.handle, C.byref(p), None, None, C.c_void_p(out[own][0].data_ptr()), C.c_void_p(out[own][1].data_ptr())) == 0


def call_own_ids():
    assert L.ifx_owner_render_view(own.handle, C.byref(p), None, None, None, C.c_void_p(out[own][1].data_ptr())) == 0


def alternating(calls):
    """[(handle, call)]: every repeat runs each call once, in turn; -> the device time of each in us"""
    streams = [main_stream(e) for e, _ in calls]
    for _ in range(5):
        for e, c in calls:
            c(); e.sync()
    times = [[] for _ in calls]
    for _ in range(reps):
        for k, (e, c) in enumerate(calls):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(streams[k])
            c()
            b.record(streams[k])
            b.synchronize()
            times[k].append(a.elapsed_time(b) * 1e3)
    return [np.asarray(t) for t in times]


def fmt(t):
    return f"{np.median(t):8.1f} [{t.min():8.1f} .. {t.max():8.1f}]"


def kernels(e, call, names):
    e.set_option("kernel_timing", 1); e.kernel_ms("__reset__")
    for _ in range(10):
        call()
    e.sync()
    ks = [e.kernel_ms(nm)[0] * 1e3 for nm in names]
    e.set_option("kernel_timing", 0)
    return ", ".join(f"{nm} {k:.1f}" for nm, k in zip(names, ks)) + f"; sum {sum(ks):.1f}", sum(ks)


print(f"sharded_view_render_cost: {n} surfels, {W}x{H} at the tracked pose, colour type 4, device outputs, {reps} alternating repeats, median [min .. max] in us")
t_one, t_own, t_ids = alternating([(one, call_one), (own, call_own), (own, call_own_ids)])
print(f"  ifx_render_view        (unsharded)             : {fmt(t_one)}")
print(f"  ifx_owner_render_view  (world of one)          : {fmt(t_own)}   difference of the medians {np.median(t_own) - np.median(t_one):.1f}")
print(f"  ifx_owner_render_view  (world of one, ids only): {fmt(t_ids)}")
k_one, s_one = kernels(one, call_one, ("view_quad", "view_big", "view_resolve"))
k_own, s_own = kernels(own, call_own, ("view_quad_seq", "view_big_seq", "view_own_resolve", "view_own_final"))
print(f"  kernels of ifx_render_view (us)       : {k_one}")
print(f"  kernels of ifx_owner_render_view (us) : {k_own}")
print(f"  outside its kernels (the memset of the list counter, two collectives and the gaps around them): {np.median(t_own) - s_own:.1f} us of the sharded call, "
      f"{np.median(t_one) - s_one:.1f} us of the unsharded one")
osh.exchange_stats(reset=True)
call_own(); own.sync()
print(f"  exchanged per call: {osh.exchange_stats(reset=True)} ({W * H} pixels: 8 B of keys + 16 B of colour each)")
call_own_ids(); own.sync()
print(f"  exchanged per ids-only call: {osh.exchange_stats(reset=True)}")
call_one(); call_own(); one.sync(); own.sync()
same = bool(torch.equal(out[one][1], out[own][1]) and torch.equal(out[one][0].view(torch.int32), out[own][0].view(torch.int32)))
print(f"  results equal (ids, rgba bits): {same}; {int((out[one][1] >= 0).sum())} pixels drawn; big-quad lists {L.ifx_render_view_big_quads(one.handle)} / "
      f"{L.ifx_owner_render_view_big_quads(own.handle)}")
print("  no run with more than one rank has been made: the collectives of a world of one move no data between GPUs")
one.close(); own.close()
sys.exit(0 if same else 1)
