"""What the deferred segmentation costs on a spatially sharded map (ifx_owner_segmentation_snapshot / ifx_owner_process_segmentation_deferred), measured the way
tools/deferred_seg_cost.py measures the unsharded pair: a world-of-one sharded handle (n_ranks = -1, the library's communicator) on the bench workload -- 640x480
frame, 5 M-surfel synthetic map, the frame's canned masks, superpixels on:

  * the snapshot: HIP-event time of k_seg_snapshot<1> (option kernel_timing) and of everything a snapshot enqueues, without and with the frame copy (flags bit 1);
  * k_seg_translate<1> with no compaction since the snapshot, and with one forced ifx_compact in between;
  * the deferred sharded call at lag 0, 8 and 64 frames: wall time from entry to the return behind the call's own synchronisation, next to the ordinary sharded
    call (ifx_owner_process_segmentation, host frame) on the same handle in the same run.

The C entry points are called directly (ctypes), so no Python wrapper work is in the figures.

    python tools/owner_deferred_seg_cost.py [surfels] [repeats per lag]"""
import ctypes as C
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402  (first: libifx.so binds to the HIP runtime torch ships)
import numpy as np  # noqa: E402

import instancefusion_amd as ifx  # noqa: E402
from instancefusion_amd import sharded, synth  # noqa: E402

args = [a for a in sys.argv[1:] if not a.startswith("--")]
n = int(args[0]) if len(args) > 0 else 5_000_000
reps = int(args[1]) if len(args) > 1 else 6
W, H = 640, 480
K = dict(fx=528.0, fy=528.0, cx=320.0, cy=240.0)
NF = 40
st = synth.make_stream(NF, W, H, noise=True, loop_len=90, **K)
m = synth.make_map(n, st["scene"], st["poses_world"][0], 1000)

ef = ifx.ElasticFusion(w=W, h=H, max_surfels=n + 1_500_000, n_ranks=-1, rank=0, **K)
osh = sharded.OwnerShardedElasticFusion(ef, None)
osh.process_frame(st["rgb"][0], st["depth"][0]); ef.upload(m); ef.set_pose(st["poses"][0], 1000); osh.predict()
L = ef.L
pos = [0]


def next_frame():
    """the stream forth and back: consecutive frames are neighbours"""
    pos[0] += 1
    k = pos[0] % (2 * (NF - 1))
    i = k if k < NF else 2 * (NF - 1) - k
    osh.process_frame(st["rgb"][i], st["depth"][i])
    return i


for _ in range(10):
    fi = next_frame()
ef.sync()
frame = [500]
MASKS = {}


def masks_of(i):
    if i not in MASKS:
        mk, cl = synth.canned_masks(st["obj"][i], st["scene"])
        MASKS[i] = (np.ascontiguousarray(mk), np.ascontiguousarray(cl.astype(np.int32)))
    return MASKS[i]


def ordinary(i):
    mk, cl = masks_of(i)
    frame[0] += 3
    t0 = time.perf_counter()
    r = L.ifx_owner_process_segmentation(ef.handle, st["rgb"][i].ctypes.data_as(C.c_void_p), st["depth"][i].ctypes.data_as(C.c_void_p), mk.ctypes.data_as(C.c_void_p),
                                         cl.ctypes.data_as(C.c_void_p), mk.shape[0], frame[0], 2)
    dt = (time.perf_counter() - t0) * 1e6
    assert r == 0, L.ifx_last_error(ef.handle)
    return dt


def deferred(ticket, i):
    mk, cl = masks_of(i)
    frame[0] += 3
    t0 = time.perf_counter()
    r = L.ifx_owner_process_segmentation_deferred(ef.handle, ticket, mk.ctypes.data_as(C.c_void_p), cl.ctypes.data_as(C.c_void_p), mk.shape[0], frame[0], 2)
    dt = (time.perf_counter() - t0) * 1e6
    assert r == 0, L.ifx_last_error(ef.handle)
    return dt


def stats(ticket):
    out = np.zeros(4, np.int32)
    assert L.ifx_segmentation_snapshot_stats(ef.handle, ticket, out.ctypes.data_as(C.c_void_p)) == 0
    return out


def med(a):
    a = np.asarray(a)
    return f"median {np.median(a):7.1f} us  min {a.min():7.1f}  max {a.max():7.1f}  ({a.size} calls)"


for _ in range(4):   # warm-up: allocations, first launches
    ordinary(fi)
print(f"owner_deferred_seg_cost: {W}x{H}, {n} surfels, a world of one on the library's communicator, superpixels on")

ms, ss = C.c_void_p(), C.c_void_p()
assert L.ifx_stream_handles(ef.handle, C.byref(ms), C.byref(ss)) == 0
main = torch.cuda.ExternalStream(ms.value)
for _ in range(3):
    for fl in (0, 2):
        t = L.ifx_owner_segmentation_snapshot(ef.handle, fl); assert t >= 0, L.ifx_last_error(ef.handle); L.ifx_segmentation_snapshot_release(ef.handle, t)
ef.sync()
for fl in (0, 2):
    ev = []
    for _ in range(20):
        next_frame(); ef.sync()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(main)
        t = L.ifx_owner_segmentation_snapshot(ef.handle, fl)
        b.record(main)
        assert t >= 0
        b.synchronize()
        ev.append(a.elapsed_time(b) * 1e3)
        L.ifx_segmentation_snapshot_release(ef.handle, t)
    print(f"  snapshot flags {fl}: everything it enqueues, HIP events on the main stream: {med(ev)}")
ef.set_option("kernel_timing", 1)
ef.kernel_ms("__reset__")
for _ in range(20):
    t = L.ifx_owner_segmentation_snapshot(ef.handle, 0); L.ifx_segmentation_snapshot_release(ef.handle, t)
ef.sync()
avg, c = ef.kernel_ms("seg_snapshot_own")
print(f"  k_seg_snapshot<1> alone (option kernel_timing): {avg * 1e3:.1f} us x {c}")
# translate: nothing compacted since the snapshot / one forced compaction in between
for compact in (0, 1):
    tr = []
    for _ in range(reps):
        fi = next_frame(); next_frame()
        t = L.ifx_owner_segmentation_snapshot(ef.handle, 2)
        slots0 = ef.slots
        if compact:
            ef.compact()
        slots1 = ef.slots
        ef.kernel_ms("__reset__")
        deferred(t, fi)
        ef.sync()
        avg, c = ef.kernel_ms("seg_translate_own")
        tr.append(avg * 1e3)
        s = stats(t)
    print(f"  k_seg_translate<1>, {'one ifx_compact' if compact else 'no compaction'} since the snapshot (slots {slots0} -> {slots1}; last ticket: {s[1]} id pixels, {s[2]} lost): {med(tr)}")
ef.set_option("kernel_timing", 0)

for lag in (0, 8, 64):
    d, o = [], []
    for _ in range(reps):
        fi = next_frame()
        t = L.ifx_owner_segmentation_snapshot(ef.handle, 2)
        for _ in range(lag):
            fj = next_frame()
        d.append(deferred(t, fi))
        s = stats(t)
        fj = next_frame()
        o.append(ordinary(fj))
    print(f"  deferred sharded call at lag {lag:2d} (last ticket: {s[1]} id pixels, {s[2]} lost): {med(d)}")
    print(f"  ordinary sharded call, same schedule (lag {lag:2d}): {med(o)}")
ef.close()
