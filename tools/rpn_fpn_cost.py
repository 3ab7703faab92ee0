"""What the RPN's proposal stage over an FPN costs on the GPU (ifx_rpn_proposals_fpn: one memset and nine launches whatever the number of levels) beside the
formulation it replaces, on the same inputs and the same build: one ElasticFusion.rpn_proposals call per level (each reads its count back), then torch.cat twice,
torch.topk and two gathers for select_over_all_levels (maskrcnn_benchmark/modeling/rpn/inference.py:123-179) -- the loop RpnPostProcessor.forward ran before.
Workload: the pyramid of an 800 x 1344 image, A = 3, five levels of 200 x 336, 100 x 168, 50 x 84, 25 x 42 and 13 x 21 cells, random logits and codes, the
anchors of the released FPN configuration (sizes 32 .. 512, aspect ratios 0.5 / 1 / 2, strides 4 .. 64), pre = post = F = 1000, threshold 0.7, min_size 0.
Per figure: HIP-event time of the whole call on its stream and the host time until the call returns; the paths are run alternately, `rounds` rounds of `calls`
calls each, and the median of every round and the median of those medians are printed.  The results of the two paths are compared first.  Then the kernels of one
call of each path (HIP events around every launch).

    python tools/rpn_fpn_cost.py [calls] [rounds]"""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402  (first: libifx.so binds to the HIP runtime torch ships)
import numpy as np  # noqa: E402

import instancefusion_amd as ifx  # noqa: E402

calls = int(sys.argv[1]) if len(sys.argv) > 1 else 30
rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 5
ef = ifx.ElasticFusion(w=640, h=480, fx=528.0, fy=528.0, cx=320.0, cy=240.0, max_surfels=100000)
rng = np.random.default_rng(1)
IMAGE = (1344, 800)
CELLS = [(200, 336), (100, 168), (50, 84), (25, 42), (13, 21)]
PRE = POST = FPN_POST = 1000
THR, MIN_SIZE = 0.7, 0


def level_anchors(H, W, stride, size, ratios=(0.5, 1.0, 2.0)):
    """the anchor generator of the released configuration for one level: [H W A, 4], row (y W + x) A + a"""
    ctr = 0.5 * (stride - 1)
    ws = np.round(np.sqrt(stride * stride / np.asarray(ratios)))
    hs = np.round(ws * np.asarray(ratios))
    ws, hs = ws * (size / stride), hs * (size / stride)
    base = np.stack([ctr - 0.5 * (ws - 1), ctr - 0.5 * (hs - 1), ctr + 0.5 * (ws - 1), ctr + 0.5 * (hs - 1)], axis=1)
    ys, xs = np.mgrid[0:H, 0:W]
    shift = np.stack([xs, ys, xs, ys], axis=-1).reshape(H * W, 1, 4) * stride
    return (shift + base[None]).reshape(-1, 4).astype(np.float32)


def timed(fn, reps):
    """HIP-event time of fn() on the current stream and the host time until it returns: medians in us"""
    dev, host = [], []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        t0 = time.perf_counter()
        fn()
        t1 = time.perf_counter()
        b.record()
        b.synchronize()
        dev.append(a.elapsed_time(b) * 1e3); host.append((t1 - t0) * 1e6)
    return float(np.median(dev)), float(np.median(host))


def per_level_loop(obj, reg, anc):
    """RpnPostProcessor.forward's loop for one image as it was before ifx_rpn_proposals_fpn"""
    boxes, scores = [], []
    for o, r, a in zip(obj, reg, anc):
        b, s, _ = ef.rpn_proposals(o, r, a, IMAGE, PRE, POST, THR, MIN_SIZE)      # the host waits here for the count
        boxes.append(b)
        scores.append(s)
    boxes, scores = torch.cat(boxes), torch.cat(scores)
    _, top = torch.topk(scores, min(FPN_POST, int(scores.numel())), dim=0, sorted=True)
    return boxes[top], scores[top]


print(f"rpn_fpn_cost: {torch.cuda.get_device_name(0)}, {rounds} alternating rounds of {calls} calls, medians")
obj = [torch.from_numpy((rng.standard_normal((3, H, W)) * 2).astype(np.float32)).cuda() for H, W in CELLS]
reg = [torch.from_numpy((rng.standard_normal((12, H, W)) * 0.5).astype(np.float32)).cuda() for H, W in CELLS]
anc = [torch.from_numpy(level_anchors(H, W, 4 << l, 32 << l)).cuda() for l, (H, W) in enumerate(CELLS)]
padded = lambda: ef.rpn_proposals_fpn(obj, reg, anc, IMAGE, PRE, POST, THR, MIN_SIZE, FPN_POST, padded=True)
cut = lambda: ef.rpn_proposals_fpn(obj, reg, anc, IMAGE, PRE, POST, THR, MIN_SIZE, FPN_POST)
loop = lambda: per_level_loop(obj, reg, anc)
b1, s1, lv, _, cnt, per_level = padded()
b2, s2 = loop()
torch.cuda.synchronize()
c = int(cnt.item())
print(f"  {sum(3 * H * W for H, W in CELLS)} anchors in {len(CELLS)} levels; proposals per level {per_level.tolist()}, {c} selected, per level "
      f"{torch.bincount(lv[:c].long(), minlength=len(CELLS)).tolist()}; scores equal to the loop's: {bool(torch.equal(s1[:c], s2))}; boxes equal: "
      f"{bool(torch.equal(b1[:c], b2))} (the loop's topk does not define the order among equal scores: {c - int(torch.unique(s2).numel())} repeated)")
for _ in range(3):
    padded(); cut(); loop()
torch.cuda.synchronize()
res = {"padded": [], "cut": [], "loop": []}
for _ in range(rounds):
    res["padded"].append(timed(padded, calls))
    res["cut"].append(timed(cut, calls))
    res["loop"].append(timed(loop, calls))
for name, key, syncs in (("ifx_rpn_proposals_fpn, padded=True      ", "padded", 0), ("ifx_rpn_proposals_fpn, cut to the count ", "cut", 1),
                         ("per-level loop + cat + topk (the parent)", "loop", len(CELLS))):
    dev, host = [v[0] for v in res[key]], [v[1] for v in res[key]]
    print(f"    {name}: stream {np.median(dev):8.1f} us {[round(v, 1) for v in dev]};  the call returns after {np.median(host):8.1f} us {[round(v, 1) for v in host]};  "
          f"host synchronisations per call: {syncs}")
ef.set_option("kernel_timing", 1)
nsel = sum(3 * H * W > 8192 for H, W in CELLS)                                     # the levels that run the radix select
L = len(CELLS)
# (name, launches per call): the number behind "x" below is how many launches' events the library had collected, not a number of calls
for title, fn, names in (("one call", padded, (("rpn_fpn_hist", 3), ("rpn_fpn_count", 1), ("rpn_fpn_compact", 1), ("rpn_fpn_sort_decode", 1), ("rpn_fpn_mask", 1),
                                               ("rpn_fpn_reduce", 1), ("rpn_fpn_merge", 1))),
                         ("the loop", loop, (("rpn_hist", 3 * nsel), ("rpn_count", nsel), ("rpn_compact", nsel), ("rpn_sort_decode", L), ("rpn_mask", L), ("rpn_reduce", L)))):
    ef.kernel_ms("__reset__")
    for _ in range(calls):
        fn()
    ef.sync(); torch.cuda.synchronize()
    total, launches = 0.0, 0
    print(f"    kernels of {title} (HIP events around every launch, average per launch):")
    for n, per_call in names:
        avg, k = ef.kernel_ms(n)
        print(f"      {n:20s} {avg * 1e3:8.1f} us x {k:4d}   {per_call:2d} per call: {avg * 1e3 * per_call:8.1f} us")
        total += avg * 1e3 * per_call
        launches += per_call
    print(f"      {'sum':20s} {total:8.1f} us in {launches} launches per call" + (f" (and torch's sigmoid x {L}, cat x 2, topk, gather x 2)" if fn is loop else " (and one sigmoid)"))
ef.set_option("kernel_timing", 0)
ef.close()
