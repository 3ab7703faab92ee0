"""The reference's surfel-id render (surfel_ids.vert / .geom / .frag, instance_surfel_ids.vert) as a screen-space quad rule, restated in f32 numpy.

This is the CPU statement of option "id_rule" = 1 (ifx_map.hip quad_setup / quad_key): every f32 operation below is the one the HIP code performs, in
the same order and without FMA contraction, so that the GPU tests can ask for array equality.  The rule:

  per surfel   culls of surfel_ids.vert / .geom (confidence > threshold, z / maxDepth > 0.01 at the centre; INSTANCECOMPARE also skips a surfel whose
               twelve vote vec4 are all equal, instance_surfel_ids.vert:44-53); the four corners of surfel_ids.geom -- centre +x, +y, -y, -x with
               x = normalize(n.y - n.z, -n.x, n.x) * r * 1.41421356 and y = cross(n, x), in the WORLD frame -- projected as project_point does
               (window coordinates through NDC, w = 1, z_ndc = z / maxDepth) and snapped to 1/256 px (llvmpipe's sub-pixel precision)
  per pixel    the strip's two triangles (v0 v1 v2) and (v2 v1 v3) sampled at the pixel centre with exact fixed-point edge functions and a top-left
               rule (y up: an edge owns its zero line when it runs downwards, or horizontally to the left), texcoord and z_ndc interpolated affinely
               from f32 barycentrics, discarded where dot(texcoord, texcoord) > 1 or z_ndc is outside [-1, 1] (GL's depth clip)
  depth        24-bit unorm: rint((z_ndc * 0.5 + 0.5) * (2^24 - 1)), GL_LESS; ties go to the lower index (the surfel drawn first)

The image holds the slot index of the winner, 0 for "no surfel" and for the lowest live slot (the reference's surfel 0)."""
import numpy as np

f32 = np.float32
SUB = 256                    # sub-pixel steps per pixel
GUARD = f32(65536.0)         # quads with a corner farther out than this (window coordinates) are not drawn (a corner behind the camera)


def pose_inverse(pose):
    """ifx_dev.h pose_inverse in f32: R^T, -(R^T t) summed left to right."""
    p = np.ascontiguousarray(pose, f32).reshape(16)
    o = np.zeros(16, f32)
    for i in range(3):
        for j in range(3):
            o[i * 4 + j] = p[j * 4 + i]
    for i in range(3):
        o[i * 4 + 3] = -((o[i * 4] * p[3] + o[i * 4 + 1] * p[7]) + o[i * 4 + 2] * p[11])
    o[15] = f32(1.0)
    return o


def _xf(T, x, y, z):
    return (((T[0] * x + T[1] * y) + T[2] * z) + T[3], ((T[4] * x + T[5] * y) + T[6] * z) + T[7], ((T[8] * x + T[9] * y) + T[10] * z) + T[11])


def _window(T, x, y, z, K, w, h, max_depth):
    """project_point of surfel_ids.geom, then the viewport transform: window x, y and z_ndc"""
    fx, fy, cx, cy = (f32(v) for v in K)
    X, Y, Z = _xf(T, x, y, z)
    hw, hh = f32(w) * f32(0.5), f32(h) * f32(0.5)
    xl = (((fx * X) / Z + cx) - hw) / hw
    yl = (((fy * Y) / Z + cy) - hh) / hh
    return xl * hw + hw, yl * hh + hh, Z / f32(max_depth)


def quad_setup(pc, nr, pose, K, w, h, max_depth, conf, votes=None):
    """Per surfel: drawn?, snapped corners (int64 1/256 px, shape (n, 4)), z_ndc of the corners, pixel box."""
    pc = np.asarray(pc, f32)
    nr = np.asarray(nr, f32)
    n = pc.shape[0]
    T = pose_inverse(pose)
    with np.errstate(all="ignore"):
        ok = pc[:, 3] > f32(conf)
        if votes is not None:      # INSTANCECOMPARE: all twelve vote vec4 equal to the first -> vertexId = -1
            v = np.asarray(votes, f32).reshape(n, 12, 4)
            ok &= ~np.all(v[:, 1:, :] == v[:, :1, :], axis=(1, 2))
        _, _, zc = _window(T, pc[:, 0], pc[:, 1], pc[:, 2], K, w, h, max_depth)
        ok &= zc > f32(0.01)
        # x = normalize(vec3(n.y - n.z, -n.x, n.x)) * r * 1.41421356, y = cross(n, x)
        ax, ay, az = nr[:, 1] - nr[:, 2], -nr[:, 0], nr[:, 0]
        rn = f32(1.0) / np.sqrt((ax * ax + ay * ay) + az * az)
        s = nr[:, 3]
        ax, ay, az = ((ax * rn) * s) * f32(1.41421356), ((ay * rn) * s) * f32(1.41421356), ((az * rn) * s) * f32(1.41421356)
        bx, by, bz = nr[:, 1] * az - nr[:, 2] * ay, nr[:, 2] * ax - nr[:, 0] * az, nr[:, 0] * ay - nr[:, 1] * ax
        px, py, pz = pc[:, 0], pc[:, 1], pc[:, 2]
        corners = [(px + ax, py + ay, pz + az), (px + bx, py + by, pz + bz), (px - bx, py - by, pz - bz), (px - ax, py - ay, pz - az)]
        X = np.zeros((n, 4), np.int64)
        Y = np.zeros((n, 4), np.int64)
        Zn = np.zeros((n, 4), f32)
        for k, (qx, qy, qz) in enumerate(corners):
            xw, yw, zn = _window(T, qx, qy, qz, K, w, h, max_depth)
            fin = np.isfinite(xw) & np.isfinite(yw) & np.isfinite(zn) & (np.abs(xw) <= GUARD) & (np.abs(yw) <= GUARD)
            ok &= fin
            xw = np.where(fin, xw, f32(0))
            yw = np.where(fin, yw, f32(0))
            X[:, k] = np.rint(xw * f32(SUB)).astype(np.int64)
            Y[:, k] = np.rint(yw * f32(SUB)).astype(np.int64)
            Zn[:, k] = np.where(fin, zn, f32(0))
    # pixels whose centre (p * 256 + 128) lies inside the snapped bounding box
    x0 = np.maximum(-((-(X.min(1) - SUB // 2)) // SUB), 0)
    x1 = np.minimum((X.max(1) - SUB // 2) // SUB, w - 1)
    y0 = np.maximum(-((-(Y.min(1) - SUB // 2)) // SUB), 0)
    y1 = np.minimum((Y.max(1) - SUB // 2) // SUB, h - 1)
    ok &= (x0 <= x1) & (y0 <= y1)
    return ok, X, Y, Zn, (x0, x1, y0, y1)


TRIS = ((0, 1, 2), (2, 1, 3))                                              # the strip's two triangles
TEX = np.array([(-1, -1), (1, -1), (-1, 1), (1, 1)], np.float32)          # texcoord of v0..v3


def _edge(ax, ay, bx, by, px, py):
    return (bx - ax) * (py - ay) - (by - ay) * (px - ax)


def _owns(ax, ay, bx, by):
    dx, dy = bx - ax, by - ay
    return (dy < 0) | ((dy == 0) & (dx < 0))


def quad_keys(X, Y, Zn, sx, sy):
    """Per (surfel, pixel) pair: the best key of the two triangles (depth24 << 32 before the id is added), or all-ones where neither draws.
    X, Y, Zn: (m, 4) corners of the pair's surfel; sx, sy: (m,) fixed-point pixel centres."""
    m = sx.shape[0]
    best = np.full(m, np.iinfo(np.uint64).max, np.uint64)
    for (ia, ib, ic) in TRIS:
        ax, ay, bx, by, cx, cy = X[:, ia], Y[:, ia], X[:, ib], Y[:, ib], X[:, ic], Y[:, ic]
        za, zb, zc = Zn[:, ia], Zn[:, ib], Zn[:, ic]
        ua, va, ub, vb, uc, vc = TEX[ia, 0], TEX[ia, 1], TEX[ib, 0], TEX[ib, 1], TEX[ic, 0], TEX[ic, 1]
        A = _edge(ax, ay, bx, by, cx, cy)
        flip = A < 0                       # clockwise: b <-> c
        bx, cx = np.where(flip, cx, bx), np.where(flip, bx, cx)
        by, cy = np.where(flip, cy, by), np.where(flip, by, cy)
        zb, zc = np.where(flip, zc, zb), np.where(flip, zb, zc)
        ub, uc = np.where(flip, uc, ub), np.where(flip, ub, uc)
        vb, vc = np.where(flip, vc, vb), np.where(flip, vb, vc)
        A = np.abs(A)
        w0, w1, w2 = _edge(bx, by, cx, cy, sx, sy), _edge(cx, cy, ax, ay, sx, sy), _edge(ax, ay, bx, by, sx, sy)
        inside = (A > 0) & ((w0 > 0) | ((w0 == 0) & _owns(bx, by, cx, cy))) & ((w1 > 0) | ((w1 == 0) & _owns(cx, cy, ax, ay))) \
            & ((w2 > 0) | ((w2 == 0) & _owns(ax, ay, bx, by)))
        with np.errstate(all="ignore"):
            fA = A.astype(f32)
            la, lb, lc = w0.astype(f32) / fA, w1.astype(f32) / fA, w2.astype(f32) / fA
            u = (la * f32(ua) + lb * f32(ub)) + lc * f32(uc)
            v = (la * f32(va) + lb * f32(vb)) + lc * f32(vc)
            z = (la * za + lb * zb) + lc * zc
            keep = inside & ~((u * u + v * v) > f32(1.0)) & (z >= f32(-1.0)) & (z <= f32(1.0))
            d24 = np.rint((z * f32(0.5) + f32(0.5)) * f32(16777215.0))
        key = np.where(keep, d24, 0).astype(np.uint64) << np.uint64(32)
        best = np.where(keep & (key < best), key, best)
    return best


def render_ids(pc, nr, pose, K, w, h, max_depth=20.0, conf=10.0, votes=None, first_live=None, step=1, chunk=1 << 21):
    """The id image (h, w) int32; votes given: INSTANCECOMPARE.  first_live: the slot named 0 (default: the first slot that is alive, tm.y > -1e9 is
    not known here -- the caller passes it; None = slot 0).  step > 1: only the pixels of that lattice are drawn (the others stay 0)."""
    ok, X, Y, Zn, (x0, x1, y0, y1) = quad_setup(pc, nr, pose, K, w, h, max_depth, conf, votes)
    idx = np.nonzero(ok)[0]
    keys = np.full(w * h, np.iinfo(np.uint64).max, np.uint64)
    fl = 0 if first_live is None else int(first_live)
    if step > 1:                            # the lattice points inside the box
        x0 = -((-x0) // step) * step; y0 = -((-y0) // step) * step
        x1 = (x1 // step) * step; y1 = (y1 // step) * step
        good = (x0 <= x1) & (y0 <= y1) & ok
        idx = np.nonzero(good)[0]
    bw = ((x1 - x0) // step + 1)[idx]
    bh = ((y1 - y0) // step + 1)[idx]
    cnt = bw * bh
    starts = np.concatenate([[0], np.cumsum(cnt)])
    # chunks of whole surfels, each expanded to its (surfel, pixel) pairs
    s = 0
    while s < idx.size:
        e = int(np.searchsorted(starts, starts[s] + chunk, side="right")) - 1
        e = max(e, s + 1)
        e = min(e, idx.size)
        sel = idx[s:e]
        c = cnt[s:e]
        rep = np.repeat(np.arange(e - s), c)
        off = np.arange(rep.size) - np.repeat(starts[s:e] - starts[s], c)
        bws = bw[s:e][rep]
        px = x0[sel][rep] + (off % bws) * step
        py = y0[sel][rep] + (off // bws) * step
        surf = sel[rep]
        k = quad_keys(X[surf], Y[surf], Zn[surf], px * SUB + SUB // 2, py * SUB + SUB // 2)
        drawn = k != np.iinfo(np.uint64).max
        ids = surf[drawn].astype(np.uint64)
        ids[ids == np.uint64(fl)] = 0
        np.minimum.at(keys, (py * w + px)[drawn], k[drawn] | ids)
        s = e
    out = np.where(keys == np.iinfo(np.uint64).max, 0, keys & np.uint64(0xFFFFFFFF)).astype(np.int32)
    return out.reshape(h, w)
