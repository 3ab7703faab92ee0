#!/usr/bin/env python3
"""What one 64-candidate step of k_raster_view's pixel loop spans on the bench map (CPU only, numpy; no kernel involved).

    python tools/walk_step_stats.py [surfels]

The bench map (synth.make_map(5 M, ...), random order) at the first pose, ids_step = 10: every surfel that the walk would draw gets its pixel box by the
kernel's rules restated in f32 numpy (surfel_geo / surfel_id_box / the lattice rule of k_raster_view), the boxes are put in list order -- the window list in slot
order, then the stable slots outside the window -- and cut into waves of 64 entries.  Printed: the distribution of box areas, of candidates per wave, and of the
number of boxes that START inside a 64-candidate step (what the owner lookup replaced paid per box; a box also pays in the step it ends in).
Approximations, stated: list membership is "in front of the camera and within reach of the image" (the scan keeps a margin and ages its lists over several
frames); entries the walk culls sit in the list as empty boxes and are counted as such; the map is the uploaded one, not the map after the warm-up frames."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from instancefusion_amd import synth  # noqa: E402

f32 = np.float32
n = int(sys.argv[1]) if len(sys.argv) > 1 else 5_000_000
W, H, fx, fy, cx, cy = 640, 480, f32(528), f32(528), f32(320), f32(240)
TICK, DELTA, CONF, MAXD, STEP, SPRITE = 1000, 200, f32(10), f32(20), 10, f32(512)
st = synth.make_stream(2, W, H, noise=True, loop_len=90, fx=528.0, fy=528.0, cx=320.0, cy=240.0)
m = synth.make_map(n, st["scene"], st["poses_world"][0], TICK, seed=synth.SEED + 7)
T = np.linalg.inv(st["poses"][0].astype(np.float64)).astype(f32)
q = m["pc"][:, :3] @ T[:3, :3].T + T[:3, 3]
nn = m["nr"][:, :3] @ T[:3, :3].T
nn /= np.maximum(np.linalg.norm(nn, axis=1, keepdims=True), f32(1e-20))
r, conf, last = m["nr"][:, 3], m["pc"][:, 3], m["tm"][:, 1]
reach = r.max() * f32(1.41421356 * 1.001)
z = q[:, 2]
with np.errstate(all="ignore"):
    u, v = fx * q[:, 0] / z + cx, fy * q[:, 1] / z + cy
    marg = reach * (fx + np.abs(u - cx)) / np.maximum(z - reach, f32(1e-3)) + 2
    near = (z > 0) & ~((u + marg < 0) | (v + marg < 0) | (u - marg > W) | (v - marg > H))
    window = ~((TICK - last) > DELTA)
    listed_a = near & window
    listed_i = near & ~window & (conf >= CONF)
    order = np.concatenate([np.nonzero(listed_a)[0], np.nonzero(listed_i)[0]])
    na = int(listed_a.sum())
    q, nn, r, conf, last, z, u, v = (a[order] for a in (q, nn, r, conf, last, z, u, v))
    in_a = np.arange(order.size) < na
    # disc_extent
    x1 = np.stack([nn[:, 1] - nn[:, 2], -nn[:, 0], nn[:, 0]], 1)
    x1 = x1 / np.linalg.norm(x1, axis=1, keepdims=True) * (r * f32(1.41421356))[:, None]
    y1 = np.cross(nn, x1)
    pts = np.stack([q + x1, q + y1, q - y1, q - x1], 1)
    pu, pv = fx * pts[:, :, 0] / pts[:, :, 2] + cx, fy * pts[:, :, 1] / pts[:, :, 2] + cy
    xs0, xs1, ys0, ys1, minz = pu.min(1), pu.max(1), pv.min(1), pv.max(1), pts[:, :, 2].min(1)
    alive = ~(conf < CONF)
    f_ids = alive & (conf > CONF) & (z / MAXD > f32(0.01))
    f_spl = alive & in_a & ~(z > MAXD) & (u >= 0) & (u <= W) & (v >= 0) & (v <= H)
    s = np.clip(np.maximum(np.abs(xs1 - xs0), np.abs(ys1 - ys0)), 1, SPRITE)
    clampx, clampy = (lambda a: np.clip(a, 0, W - 1).astype(np.int64)), (lambda a: np.clip(a, 0, H - 1).astype(np.int64))
    sx0, sx1 = clampx(np.ceil(u - s * f32(0.5) - f32(0.5))), clampx(np.floor(u + s * f32(0.5) - f32(0.5)))
    sy0, sy1 = clampy(np.ceil(v - s * f32(0.5) - f32(0.5))), clampy(np.floor(v + s * f32(0.5) - f32(0.5)))
    do_s = f_spl & np.isfinite(s)
    do_i = f_ids & (minz > 0) & ~((xs1 - xs0 > SPRITE) | (ys1 - ys0 > SPRITE) | (xs1 < 0) | (ys1 < 0) | (xs0 > W) | (ys0 > H))
    ix0, ix1 = clampx(np.ceil(xs0 - f32(0.5))), clampx(np.floor(xs1 - f32(0.5)))
    iy0, iy1 = clampy(np.ceil(ys0 - f32(0.5))), clampy(np.floor(ys1 - f32(0.5)))
lx0, lx1, ly0, ly1 = (ix0 + STEP - 1) // STEP * STEP, ix1 // STEP * STEP, (iy0 + STEP - 1) // STEP * STEP, iy1 // STEP * STEP
do_i &= (lx0 <= lx1) & (ly0 <= ly1)
lattice = do_i & ~do_s
x0 = np.where(do_s & do_i, np.minimum(sx0, lx0), np.where(do_s, sx0, lx0)); x1_ = np.where(do_s & do_i, np.maximum(sx1, lx1), np.where(do_s, sx1, lx1))
y0 = np.where(do_s & do_i, np.minimum(sy0, ly0), np.where(do_s, sy0, ly0)); y1_ = np.where(do_s & do_i, np.maximum(sy1, ly1), np.where(do_s, sy1, ly1))
nx = np.where(lattice, (x1_ - x0) // STEP + 1, x1_ - x0 + 1); ny = np.where(lattice, (y1_ - y0) // STEP + 1, y1_ - y0 + 1)
area = np.where((do_s | do_i) & (x1_ >= x0) & (y1_ >= y0), nx * ny, 0)


def dist(a, name, pcs=(10, 50, 90, 99)):
    a = np.asarray(a)
    print(f"  {name}: n {a.size}  mean {a.mean():.2f}  " + "  ".join(f"p{p} {np.percentile(a, p):.0f}" for p in pcs) + f"  max {a.max()}")


print(f"map {n} surfels; listed: window {na}, stable outside the window {order.size - na}; drawn (area > 0) {int((area > 0).sum())}: splat+ids or splat {int(do_s.sum())}, "
      f"id-only lattice records {int((lattice & (area > 0)).sum())}")
dist(area[area > 0], "box area, all drawn entries")
dist(area[(area > 0) & ~lattice], "box area, splat entries")
dist(area[(area > 0) & lattice], "box area, id-only lattice records")
pad = (-area.size) % 64
waves = np.concatenate([area, np.zeros(pad, np.int64)]).reshape(-1, 64)
tot = waves.sum(1)
dist(tot[tot > 0], "candidates per wave of 64 entries")
dist(-(-tot[tot > 0] // 64), "steps per wave")
excl = np.cumsum(waves, 1) - waves
starts = []
for wv, ex, t in zip(waves[tot > 0], excl[tot > 0], tot[tot > 0]):
    starts.append(np.bincount((ex[wv > 0] // 64), minlength=-(-t // 64)))
starts = np.concatenate(starts)
dist(starts, "boxes that start inside a step")
print(f"  steps {starts.size}, box starts {int(starts.sum())}: {starts.sum() / starts.size:.2f} a step; a box pays the old search in the step it starts and (unless it is the same) the step it ends in")
