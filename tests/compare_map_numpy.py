"""The mask rule of the compare map (option compare_map 2; include/ifx_c_api.h, ifx_mask_compare_map) written down twice in numpy, for the tests:
tables_literal -- the reference's loops as they stand (maskCompareMapKernel, IF/Core/InstanceFusionCuda.cu:826-881: per pixel, per mask, per instance, 3 x 3 flags);
tables -- dilate, then count.  decide -- the decision loop (IF/Core/InstanceFusion.cpp:834-861).  presence -- instanceProjectMap > 0 of
getProjectInstanceListKernel (:781-807) from an id image and packed vote words, decoded by the oracle's orc_vote_decode."""
import ctypes as C

import numpy as np

NI = 96


def decode_words(votes):
    """[n, 48] float32 vote words -> [n, 96] int32 counters through the oracle's orc_vote_decode (word w: instance 2w in the high half, 2w + 1 in the low one)"""
    import oracle_lib as ol

    L = ol.lib()
    f = np.ascontiguousarray(votes, np.float32)
    flat = f.reshape(-1)
    out = np.zeros((flat.size, 2), np.int32)
    cache = {}
    a, b = C.c_int(0), C.c_int(0)
    for k, (word, key) in enumerate(zip(flat.tolist(), flat.view(np.uint32).tolist())):
        if key not in cache:
            L.orc_vote_decode(C.c_float(word), C.byref(a), C.byref(b))
            cache[key] = (a.value, b.value)
        out[k] = cache[key]
    return out.reshape(f.shape[0], 2 * f.shape[1])


def presence(ids, votes, count=None):
    """[96, H, W] bool: pixel p names a surfel of the map (0 < id < count) whose counter i is > 0"""
    n = votes.shape[0] if count is None else count
    cnt = decode_words(votes)
    has = (ids > 0) & (ids < n)
    safe = np.where(has, ids, 0)
    return np.moveaxis((cnt[safe] > 0) & has[..., None], -1, 0)


def surfel_boxes_degenerate(masks, ids, votes, count=None):
    """The box rule's degenerate-box test, which the mask rule keeps: the mask's box over its pixels that carry a surfel whose counter 0 is not -1
    (computeProjectBoundingBoxKernel, :909-952) has max <= min in x or in y (no such pixel: degenerate)."""
    n = votes.shape[0] if count is None else count
    has = (ids > 0) & (ids < n)
    first = decode_words(votes[:, :1])[:, 0]
    has &= first[np.where(has, ids, 0)] != -1
    out = np.zeros(len(masks), bool)
    for m, mk in enumerate(masks):
        ys, xs = np.nonzero((mk > 0) & has)
        out[m] = len(xs) == 0 or xs.max() <= xs.min() or ys.max() <= ys.min()
    return out


def dilate(a):
    """3 x 3 dilation of [..., H, W] bool; neighbours outside the image are skipped"""
    H, W = a.shape[-2:]
    p = np.zeros(a.shape[:-2] + (H + 2, W + 2), bool)
    p[..., 1:-1, 1:-1] = a
    out = np.zeros_like(a, dtype=bool)
    for dy in range(3):
        for dx in range(3):
            out |= p[..., dy:dy + H, dx:dx + W]
    return out


def tables(masks, pres, mask_cls, inst_cls):
    """(I, U, A_M, A_I): dilate, then count; pairs whose classes differ (unused slots, class -1, included) stay 0"""
    pres = np.asarray(pres, bool)
    P = pres.shape[-2] * pres.shape[-1]
    Md = dilate(np.asarray(masks).reshape((-1,) + pres.shape[-2:]) > 0).reshape(len(masks), P).astype(np.int64)
    Id = dilate(pres).reshape(NI, P).astype(np.int64)
    AM, AI = Md.sum(1), Id.sum(1)
    I = Md @ Id.T
    U = AM[:, None] + AI[None, :] - I
    same = (np.asarray(inst_cls)[None, :] != -1) & (np.asarray(mask_cls)[:, None] == np.asarray(inst_cls)[None, :])
    return np.where(same, I, 0).astype(np.int32), np.where(same, U, 0).astype(np.int32), AM.astype(np.int32), AI.astype(np.int32)


def tables_literal(masks, pres, mask_cls, inst_cls):
    """(I, U) as maskCompareMapKernel counts them: one pixel at a time, the 3 x 3 flags of every mask and instance, then the pairs of equal class"""
    nm = len(masks)
    H, W = pres.shape[-2:]
    I, U = np.zeros((nm, NI), np.int32), np.zeros((nm, NI), np.int32)
    for y in range(H):
        for x in range(W):
            mflag, iflag = [False] * nm, [False] * NI
            for dy in (-1, 0, 1):
                for dx in (-1, 0, 1):
                    yy, xx = y + dy, x + dx
                    if yy < 0 or yy >= H or xx < 0 or xx >= W:
                        continue
                    for m in range(nm):
                        if masks[m][yy, xx] > 0:
                            mflag[m] = True
                    for i in np.nonzero(pres[:, yy, xx])[0]:
                        iflag[i] = True
            for m in range(nm):
                for i in range(NI):
                    if inst_cls[i] == -1 or inst_cls[i] != mask_cls[m]:
                        continue
                    if mflag[m] and iflag[i]:
                        I[m, i] += 1
                    if mflag[m] or iflag[i]:
                        U[m, i] += 1
    return I, U


def decide(I, U, mask_cls, inst_cls, unavailable=None):
    """best[m]: ascending instances of the mask's class, iou = f32(I) / f32(U), a candidate iff > 0.5, replaces the best iff > the best so far, and `if best > 0`"""
    nm = len(mask_cls)
    best = np.full(nm, -1, np.int32)
    for m in range(nm):
        if unavailable is not None and unavailable[m]:
            continue
        b, biou = -1, np.float32(0)
        for i in range(NI):
            if inst_cls[i] == -1 or inst_cls[i] != mask_cls[m]:
                continue
            with np.errstate(divide="ignore", invalid="ignore"):
                iou = np.float32(I[m, i]) / np.float32(U[m, i])
            if iou > np.float32(0.5) and iou > biou:
                b, biou = i, iou
        if b > 0:
            best[m] = b
    return best


def box_rule(masks, ids, votes, mask_cls, inst_cls, unavailable=None, count=None):
    """The default rule for comparison (computeCompareMap, IF/Core/InstanceFusion.cpp:595-651): box IoU > 0.5 between the mask's box and the box of the instance's
    projected arg-max pixels, the same class, the LAST instance over the threshold wins, instance 0 never matches.  best[m] or -1."""
    n = votes.shape[0] if count is None else count
    H, W = ids.shape
    cnt = decode_words(votes)
    has = (ids > 0) & (ids < n)
    c = cnt[np.where(has, ids, 0)]
    has &= c[..., 0] != -1
    pos = np.where(c > 0, c, 0)
    arg = np.where(has & (pos.max(-1) > 0), pos.argmax(-1), -1)

    def box(sel):
        ys, xs = np.nonzero(sel)
        return (W + 1, -1, H + 1, -1) if len(xs) == 0 else (xs.min(), xs.max(), ys.min(), ys.max())

    best = np.full(len(masks), -1, np.int32)
    for m, mk in enumerate(masks):
        x0, x1, y0, y1 = box((mk > 0) & has)
        if x1 <= x0 or y1 <= y0 or (unavailable is not None and unavailable[m]):
            continue
        b = -1
        for i in range(NI):
            if inst_cls[i] == -1 or inst_cls[i] != mask_cls[m]:
                continue
            a0, a1, b0, b1 = box(arg == i)
            if a1 <= a0 or b1 <= b0:
                continue
            iw, ih = np.float32(min(a1, x1) - max(a0, x0)), np.float32(min(b1, y1) - max(b0, y0))
            if iw <= 0 or ih <= 0:
                continue
            I = iw * ih
            U = np.float32((a1 - a0) * (b1 - b0) + (x1 - x0) * (y1 - y0)) - I
            if I / U > np.float32(0.5):
                b = i
        if b > 0:
            best[m] = b
    return best
