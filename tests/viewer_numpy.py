"""The reference viewer's surfel pass (draw_global_surface.vert / .geom / .frag and draw_global_ID.*, GlobalModel::renderPointCloud / renderGlobalID)
as a screen-space quad rule under an arbitrary 4x4 MVP, restated in f32 numpy.

This is the CPU statement of ifx_render_view (ifx_map.hip view_setup / view_key / view_colour): every f32 operation below is the one the HIP code
performs, in the same order and without FMA contraction, so that the GPU tests can ask for array equality.  The fixed-point machinery -- the 1/256 px
snap, the exact int64 edge functions, the top-left rule, the strip's triangles, 24-bit depth with GL_LESS, ties to the lower index -- is
quad_ids_numpy's, imported.  The rule:

  per surfel   drawn unless the instance-colour word is -1.0 (draw_global_surface.vert:44), and only if confidence > threshold or `unstable`
               (a slot with a negative confidence is a tombstone of the store and is never drawn; the reference's map has none);
               corners centre +x, +y, -y, -x with x = normalize(n.y - n.z, -n.x, n.x) * r * 1.41421356, y = cross(n, x); each through
               clip = MVP . (corner, 1) summed left to right; a surfel with a corner whose clip.w is not > 0 and finite is NOT drawn, nor one whose
               window x or y leaves the guard band (GL would clip such a quad and draw the visible part: the one stated deviation);
               xw = (clip.x / clip.w * 0.5 + 0.5) * W, yw likewise with H, zw = clip.z / clip.w * 0.5 + 0.5; xw, yw snapped to 1/256 px
  per pixel    coverage from the fixed-point edge functions; la, lb, lc the affine barycentrics; texcoord perspective-correct,
               u = (la ua / wa + lb ub / wb + lc uc / wc) / (la / wa + lb / wb + lc / wc); zw affine (GL interpolates depth in window space);
               discarded where u^2 + v^2 > 1 or zw is outside [0, 1] (the depth clip: it stands in for near and far clipping)
  depth        zw + radius for a surfel with confidence <= threshold (draw_global_surface.frag:35-42), clamped to [0, 1], rint(d * 16777215);
               a fragment at 16777215 is not drawn (GL_LESS against the cleared depth buffer); key = depth24 << 32 | slot, the minimum wins
  outputs      ids int32 [H, W]: the winner's slot, -1 where nothing was drawn; rgba f32 [H, W, 4]: the winner's base colour (per surfel, not
               interpolated), alpha 1; the clear colour with alpha 0 where nothing was drawn.  Output row r is GL window row H - 1 - r."""
import numpy as np

import quad_ids_numpy as Q
from instancefusion_amd import viewer_mvp  # noqa: F401  (the reference's camera: Pangolin's ProjectionMatrix times the inverse pose)

f32 = np.float32
SUB, GUARD = Q.SUB, Q.GUARD
EMPTY = np.iinfo(np.uint64).max


def _decode(c):
    """decodeColor of color.glsl: the bytes of int(c)"""
    with np.errstate(all="ignore"):
        v = np.asarray(c, f32).astype(np.int32)
    return [((v >> s) & 0xFF).astype(f32) / f32(255.0) for s in (16, 8, 0)]


def _max0(a):
    return np.where(a > f32(0), a, f32(0)).astype(f32)


def view_colour(nr, col, tm, color_type, draw_window, time, time_delta):
    """Per surfel: the base colour of draw_global_surface.geom:50-88, (n, 3) f32."""
    nr, col, tm = np.asarray(nr, f32), np.asarray(col, f32), np.asarray(tm, f32)
    with np.errstate(all="ignore"):
        d = np.abs((nr[:, 0] + nr[:, 1]) + nr[:, 2])
        grey = f32(0.5) * d + f32(0.1)
        if color_type == 1:
            c = [nr[:, 0], nr[:, 1], nr[:, 2]]
        elif color_type == 2:
            c = _decode(col[:, 0])
        elif color_type == 3:
            ft = f32(time)
            ratio = (f32(2.0) * (tm[:, 0] - f32(1.0))) / (ft - f32(1.0))
            cx = _max0(f32(1.0) - ratio)
            cy = _max0(ratio - f32(1.0))
            cz = (f32(1.0) - cx) - cy
            s = d + f32(0.1)
            c = [cx * s, cy * s, cz * s]
        elif color_type == 4:
            c = _decode(col[:, 1])
        else:
            c = [grey, grey, grey]
        dim = ((f32(time) - tm[:, 1]) > f32(time_delta)) if draw_window else np.zeros(nr.shape[0], bool)
        out = np.zeros((nr.shape[0], 3), f32)
        for k in range(3):
            ck = np.where(dim, c[k] * f32(0.25), c[k]).astype(f32)
            out[:, k] = ck * f32(0.6) + grey * f32(0.4)
    return out


def view_setup(pc, nr, col, mvp, w, h, threshold, unstable):
    """Per surfel: drawn?, snapped corners (int64 1/256 px, (n, 4)), zw and 1/w of the corners, the pixel box clipped to the viewport."""
    pc, nr, col = np.asarray(pc, f32), np.asarray(nr, f32), np.asarray(col, f32)
    M = np.ascontiguousarray(mvp, f32).reshape(16)
    n = pc.shape[0]
    with np.errstate(all="ignore"):
        ok = ~(col[:, 1] == f32(-1.0)) & (pc[:, 3] >= f32(0))
        ok &= (pc[:, 3] > f32(threshold)) | bool(unstable)
        ax, ay, az = nr[:, 1] - nr[:, 2], -nr[:, 0], nr[:, 0]
        rn = f32(1.0) / np.sqrt((ax * ax + ay * ay) + az * az)
        s = nr[:, 3]
        ax, ay, az = ((ax * rn) * s) * f32(1.41421356), ((ay * rn) * s) * f32(1.41421356), ((az * rn) * s) * f32(1.41421356)
        bx, by, bz = nr[:, 1] * az - nr[:, 2] * ay, nr[:, 2] * ax - nr[:, 0] * az, nr[:, 0] * ay - nr[:, 1] * ax
        px, py, pz = pc[:, 0], pc[:, 1], pc[:, 2]
        corners = [(px + ax, py + ay, pz + az), (px + bx, py + by, pz + bz), (px - bx, py - by, pz - bz), (px - ax, py - ay, pz - az)]
        X = np.zeros((n, 4), np.int64)
        Y = np.zeros((n, 4), np.int64)
        Zw = np.zeros((n, 4), f32)
        Iw = np.zeros((n, 4), f32)
        wok = np.ones(n, bool)
        for k, (qx, qy, qz) in enumerate(corners):
            cxx = ((M[0] * qx + M[1] * qy) + M[2] * qz) + M[3]
            cyy = ((M[4] * qx + M[5] * qy) + M[6] * qz) + M[7]
            czz = ((M[8] * qx + M[9] * qy) + M[10] * qz) + M[11]
            cww = ((M[12] * qx + M[13] * qy) + M[14] * qz) + M[15]
            wgood = (cww > f32(0)) & (cww < f32(np.inf))
            wok &= wgood
            xw = ((cxx / cww) * f32(0.5) + f32(0.5)) * f32(w)
            yw = ((cyy / cww) * f32(0.5) + f32(0.5)) * f32(h)
            zw = (czz / cww) * f32(0.5) + f32(0.5)
            fin = wgood & (np.abs(xw) <= GUARD) & (np.abs(yw) <= GUARD) & (np.abs(zw) < f32(np.inf))
            ok &= fin
            X[:, k] = np.rint(np.where(fin, xw, f32(0)) * f32(SUB)).astype(np.int64)
            Y[:, k] = np.rint(np.where(fin, yw, f32(0)) * f32(SUB)).astype(np.int64)
            Zw[:, k] = np.where(fin, zw, f32(0))
            Iw[:, k] = np.where(fin, f32(1.0) / cww, f32(0))
    x0 = np.maximum(-((-(X.min(1) - SUB // 2)) // SUB), 0)
    x1 = np.minimum((X.max(1) - SUB // 2) // SUB, w - 1)
    y0 = np.maximum(-((-(Y.min(1) - SUB // 2)) // SUB), 0)
    y1 = np.minimum((Y.max(1) - SUB // 2) // SUB, h - 1)
    ok &= (x0 <= x1) & (y0 <= y1)
    return ok, X, Y, Zw, Iw, (x0, x1, y0, y1), wok


def view_keys(X, Y, Zw, Iw, push, sx, sy):
    """Per (surfel, pixel) pair: the best key of the two triangles (depth24 << 32), or all-ones where neither draws.  push: (m,) f32 added to zw
    (the radius of an unstable surfel, 0 otherwise)."""
    m = sx.shape[0]
    best = np.full(m, EMPTY, np.uint64)
    for (ia, ib, ic) in Q.TRIS:
        ax, ay, bx, by, cx, cy = X[:, ia], Y[:, ia], X[:, ib], Y[:, ib], X[:, ic], Y[:, ic]
        za, zb, zc = Zw[:, ia], Zw[:, ib], Zw[:, ic]
        qa, qb, qc = Iw[:, ia], Iw[:, ib], Iw[:, ic]
        ua, va, ub, vb, uc, vc = (np.full(m, Q.TEX[i, j], f32) for i in (ia, ib, ic) for j in (0, 1))
        A = Q._edge(ax, ay, bx, by, cx, cy)
        flip = A < 0                       # clockwise: b <-> c
        bx, cx = np.where(flip, cx, bx), np.where(flip, bx, cx)
        by, cy = np.where(flip, cy, by), np.where(flip, by, cy)
        zb, zc = np.where(flip, zc, zb), np.where(flip, zb, zc)
        qb, qc = np.where(flip, qc, qb), np.where(flip, qb, qc)
        ub, uc = np.where(flip, uc, ub), np.where(flip, ub, uc)
        vb, vc = np.where(flip, vc, vb), np.where(flip, vb, vc)
        A = np.abs(A)
        w0, w1, w2 = Q._edge(bx, by, cx, cy, sx, sy), Q._edge(cx, cy, ax, ay, sx, sy), Q._edge(ax, ay, bx, by, sx, sy)
        inside = (A > 0) & ((w0 > 0) | ((w0 == 0) & Q._owns(bx, by, cx, cy))) & ((w1 > 0) | ((w1 == 0) & Q._owns(cx, cy, ax, ay))) \
            & ((w2 > 0) | ((w2 == 0) & Q._owns(ax, ay, bx, by)))
        with np.errstate(all="ignore"):
            fA = A.astype(f32)
            la, lb, lc = w0.astype(f32) / fA, w1.astype(f32) / fA, w2.astype(f32) / fA
            pa, pb, pc_ = la * qa, lb * qb, lc * qc
            den = (pa + pb) + pc_
            u = ((pa * ua + pb * ub) + pc_ * uc) / den
            v = ((pa * va + pb * vb) + pc_ * vc) / den
            z = (la * za + lb * zb) + lc * zc
            keep = inside & ~((u * u + v * v) > f32(1.0)) & (z >= f32(0.0)) & (z <= f32(1.0))
            d = z + push
            d = np.minimum(np.maximum(d, f32(0.0)), f32(1.0))
            d24 = np.rint(d * f32(16777215.0))
            keep &= d24 < f32(16777215.0)        # GL_LESS against the cleared buffer: a fragment at depth 1 is not drawn
        key = np.where(keep, d24, 0).astype(np.uint64) << np.uint64(32)
        best = np.where(keep & (key < best), key, best)
    return best


def render_view(m, mvp, w, h, threshold, color_type=0, unstable=0, draw_window=0, time=1, time_delta=200, clear_rgb=(1.0, 1.0, 1.0), chunk=1 << 21, info=None):
    """m: dict with pc (n, 4), nr (n, 4), col (n, 2), tm (n, 2).  Returns (rgba (h, w, 4) f32, ids (h, w) int32), top row first.
    info: a dict that receives `w_skipped` (surfels the w > 0 rule alone removed) and `big` (drawn quads whose box holds more than 256 pixels)."""
    pc, nr, col, tm = (np.asarray(m[k], f32) for k in ("pc", "nr", "col", "tm"))
    ok, X, Y, Zw, Iw, (x0, x1, y0, y1), wok = view_setup(pc, nr, col, mvp, w, h, threshold, unstable)
    idx = np.nonzero(ok)[0]
    keys = np.full(w * h, EMPTY, np.uint64)
    bw = (x1 - x0 + 1)[idx]
    cnt = bw * (y1 - y0 + 1)[idx]
    if info is not None:
        with np.errstate(all="ignore"):
            cand = ~(col[:, 1] == f32(-1.0)) & (pc[:, 3] >= f32(0)) & ((pc[:, 3] > f32(threshold)) | bool(unstable))
        info["w_skipped"] = int((cand & ~wok).sum())
        info["big"] = int((cnt > 256).sum())
    starts = np.concatenate([[0], np.cumsum(cnt)])
    with np.errstate(all="ignore"):
        push_all = np.where(pc[:, 3] <= f32(threshold), nr[:, 3], f32(0)).astype(f32)
    s = 0
    while s < idx.size:
        e = int(np.searchsorted(starts, starts[s] + chunk, side="right")) - 1
        e = min(max(e, s + 1), idx.size)
        sel = idx[s:e]
        c = cnt[s:e]
        rep = np.repeat(np.arange(e - s), c)
        off = np.arange(rep.size) - np.repeat(starts[s:e] - starts[s], c)
        bws = bw[s:e][rep]
        px = x0[sel][rep] + off % bws
        py = y0[sel][rep] + off // bws
        surf = sel[rep]
        k = view_keys(X[surf], Y[surf], Zw[surf], Iw[surf], push_all[surf], px * SUB + SUB // 2, py * SUB + SUB // 2)
        drawn = k != EMPTY
        np.minimum.at(keys, (py * w + px)[drawn], k[drawn] | surf[drawn].astype(np.uint64))
        s = e
    keys = keys.reshape(h, w)[::-1]                       # output row r is GL window row h - 1 - r
    hit = keys != EMPTY
    ids = np.where(hit, keys & np.uint64(0xFFFFFFFF), 0).astype(np.int64)
    ids = np.where(hit, ids, -1).astype(np.int32)
    rgba = np.zeros((h, w, 4), f32)
    rgba[..., :3] = np.asarray(clear_rgb, f32)
    if hit.any():
        win = ids[hit]
        rgba[hit, :3] = view_colour(nr[win], col[win], tm[win], color_type, draw_window, time, time_delta)
        rgba[hit, 3] = f32(1.0)
    return rgba, ids
