"""What merging duplicate instances (ifx_merge_instances: the reference's checkLoopClosure, one pass instead of its two) costs on the bench map (5 M-surfel
synthetic map, 640x480): the merge pass, the full label scan behind it and the recolour pass (option kernel_timing) with 1, 8 and 40 pairs, next to clean_table --
the eviction's pass over the same store -- and count_colour measured in the same process on the same votes.  Every surfel carries counters of one to three of the
96 instances (uniformly drawn: which slots a repetition finds registered varies), one in sixteen is a first-frame surfel (-1 in every word).  A repetition uploads
those votes, fills the instance table with calls of 80 rectangles of classes nobody has (the calls that find it full evict: clean_table's samples), uploads the
votes again and merges 1, 8 and 40 of the registered instances into others.  One line of JSON at the end.

    python tools/instance_merge_cost.py [surfels] [repetitions]"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402,F401  (first: libifx.so binds to the HIP runtime torch ships)
import numpy as np  # noqa: E402

import instancefusion_amd as ifx  # noqa: E402
from instancefusion_amd import synth  # noqa: E402

n = int(sys.argv[1]) if len(sys.argv) > 1 else 5_000_000
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 3
W, H = 640, 480
K = dict(fx=528.0, fy=528.0, cx=320.0, cy=240.0)
st = synth.make_stream(12, W, H, noise=True, loop_len=90, **K)
m = synth.make_map(n, st["scene"], st["poses_world"][0], 1000)
rng = np.random.default_rng(26)
votes = np.zeros((n, 48), np.float32)
rows = np.arange(n)
for share in (1.0, 0.3, 0.1):                               # one to three instances per surfel; a word is float((a << 16) + b), exact at these counts
    on = rows[rng.random(n) < share]
    i = rng.integers(0, 96, len(on))
    votes[on, i // 2] += (rng.integers(1, 50, len(on)) * np.where(i % 2 == 0, 65536, 1)).astype(np.float32)
votes[rng.random(n) < 1.0 / 16] = -1.0
m["votes"] = votes


def grid_masks():
    out = np.zeros((80, H, W), np.uint8)
    for c in range(80):
        x0, y0 = (c % 10) * 64 + 4, (c // 10) * 60 + 4
        out[c, y0:y0 + 52, x0:x0 + 56] = 255
    return out


ef = ifx.ElasticFusion(w=W, h=H, max_surfels=n + 1_500_000, **K)
inst = ifx.InstanceFusion(ef)
ef.processFrame(st["rgb"][0], st["depth"][0])
masks = grid_masks()
frame, next_class = [500], [1000]


def restore():
    ef.upload(m); ef.set_pose(st["poses"][0], 1000); ef.combined_predict(st["poses"][0], 1000, 1000)
    ef.processFrame(st["rgb"][1], st["depth"][1])
    ef.sync()


def fill_table():
    """calls of 80 masks of new classes until the table is full: the ones that find it full evict (clean_table, then the full label scan)"""
    for _ in range(3):
        frame[0] += 3
        cls = np.arange(next_class[0], next_class[0] + 80, dtype=np.int32)
        next_class[0] += 80
        inst.ProcessSegmentation(None, None, masks, cls, frame[0])


def kernel_us(names):
    ef.sync()
    return {k: (round(ef.kernel_ms(k)[0] * 1e3, 1), ef.kernel_ms(k)[1]) for k in names}


res = {"surfels": n, "repetitions": reps, "merge": {p: [] for p in (1, 8, 40)}, "clean_table_us": [], "count_colour_us": []}
print(f"instance_merge_cost: {W}x{H}, {n} surfels, {reps} repetitions; kernel times from HIP events (option kernel_timing)")
for rep in range(reps):
    restore()
    ef.set_option("kernel_timing", 1)
    ef.kernel_ms("__reset__")
    fill_table()
    ks = kernel_us(("clean_table", "count_colour"))
    ef.set_option("kernel_timing", 0)
    print(f"  repetition {rep}: filling the table: clean_table {ks['clean_table'][0]} us x {ks['clean_table'][1]}, count_colour {ks['count_colour'][0]} us x {ks['count_colour'][1]}")
    if ks["clean_table"][1]:
        res["clean_table_us"].append(ks["clean_table"][0])
    if ks["count_colour"][1]:
        res["count_colour_us"].append(ks["count_colour"][0])
    restore()
    used = np.nonzero(inst.getInstanceTable() != -1)[0].tolist()
    assert len(used) >= 60, len(used)
    froms, targets = used[:49], used[49:]
    at = 0
    ef.set_option("kernel_timing", 1)
    for p in (1, 8, 40):
        pairs = [(froms[at + k], targets[k % len(targets)]) for k in range(p)]
        at += p
        ef.kernel_ms("__reset__")
        inst.merge_instances(pairs, resolve=False)
        ks = kernel_us(("merge_votes", "count_colour", "merge_recolour"))
        assert ks["merge_votes"][1] == 1, ks
        print(f"  repetition {rep}: {p:2d} pairs: merge_votes {ks['merge_votes'][0]:8.1f} us  count_colour {ks['count_colour'][0]:8.1f} us  merge_recolour {ks['merge_recolour'][0]:7.1f} us")
        res["merge"][p].append([ks["merge_votes"][0], ks["count_colour"][0], ks["merge_recolour"][0]])
    ef.set_option("kernel_timing", 0)
ct = res["clean_table_us"]
if ct:
    spread = (max(ct) - min(ct)) / np.median(ct)
    print(f"clean_table: median {np.median(ct):.1f} us over {len(ct)} repetitions, spread (max - min) / median {100 * spread:.1f} %")
    for p in (1, 8, 40):
        mv = [x[0] for x in res["merge"][p]]
        print(f"merge_votes, {p:2d} pairs: median {np.median(mv):.1f} us = {np.median(mv) / np.median(ct):.2f} x clean_table (min {min(mv):.1f}, max {max(mv):.1f})")
ef.close()
print(json.dumps(res))
