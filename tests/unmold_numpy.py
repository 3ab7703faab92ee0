"""The rule of ifx_unmold_detections in numpy (include/ifx_c_api.h, k_unmold_select / k_unmold_paste): MaskRCNN.unmold_detections (deps/mask_rcnn/model.py:2285-2344)
and utils.unmold_mask (deps/mask_rcnn/utils.py:490-507) behind scipy.misc.imresize -- bytescale, Pillow's 8-bit bilinear resampling (detector_input_numpy.resize),
the threshold, the paste.  Every cast is written out, so the statement does not depend on the promotion rules of the installed numpy.  No torch, no Pillow."""
import numpy as np

import detector_input_numpy as di

COORD_LIMIT = float(1 << 24)


def box_scale(window, W, H):
    """model.py:2314-2316 in Python's f64: min(H / (wy2 - wy1), W / (wx2 - wx1))"""
    wy1, wx1, wy2, wx2 = (int(v) for v in window)
    return min(H / (wy2 - wy1), W / (wx2 - wx1))


def count_rows(det):
    """step 1 (model.py:2304-2305): the first row whose class id is 0 (-0 too), else all of them"""
    z = np.nonzero(det[:, 4] == np.float32(0.0))[0]
    return int(z[0]) if len(z) else int(det.shape[0])


def row_box(d, window, scale):
    """steps 2 and 8 of one row: (y1, x1, y2, x2) as Python ints, or None when a coordinate is not finite or beyond +-2^24 (before or after the scale)"""
    shift = (int(window[0]), int(window[1]), int(window[0]), int(window[1]))
    out = []
    for k in range(4):
        x = float(np.float32(d[k]))
        if not np.isfinite(x) or abs(x) > COORD_LIMIT:
            return None
        v = (x - float(shift[k])) * scale                      # (f32 - int64 -> f64, model.py:2322)
        if not abs(v) <= COORD_LIMIT:
            return None
        out.append(int(v))                                     # astype(int32): toward zero
    return tuple(out)


def bytescale(m, reading="f32"):
    """step 4 on a finite float32 [M, M]: scipy.misc.bytescale(m) with cmin = m.min(), cmax = m.max(), low = 0, high = 255.  reading 'f32': as numpy evaluated it
    before NEP 50 (the f64 scalar 255 / cscale does not widen the f32 array); 'f64': the array widened to f64 by the scalar."""
    m = np.asarray(m, np.float32)
    cmin, cmax = np.float32(m.min()), np.float32(m.max())
    cs = np.float32(cmax - cmin)
    if cs == 0:
        cs = np.float32(1.0)
    if reading == "f32":
        s = np.float32(255.0 / float(cs))
        v = (m - cmin).astype(np.float32) * s
        assert v.dtype == np.float32
        v = np.minimum(np.maximum(v, np.float32(0.0)), np.float32(255.0)) + np.float32(0.5)
        assert v.dtype == np.float32
    else:
        v = (m - cmin).astype(np.float32).astype(np.float64) * (255.0 / float(cs))
        v = np.minimum(np.maximum(v, 0.0), 255.0) + 0.5
    return v.astype(np.uint8)                                  # (0.5 .. 255.5: toward zero)


def resize_bytes(b, w, h):
    """step 5: Pillow's Image.resize((w, h), BILINEAR) of uint8 [M, M]"""
    return di.resize(np.ascontiguousarray(b)[:, :, None], int(w), int(h))[:, :, 0]


def mask_defined(m):
    """step 8: every sample finite, and both the range cs = f32(cmax - cmin) and the factor s = f32(255.0 / f64(cs)) finite in f32"""
    m = np.asarray(m, np.float32)
    if not np.isfinite(m).all():
        return False
    with np.errstate(over="ignore"):
        cs = np.float32(m.max()) - np.float32(m.min())
        return bool(np.isfinite(cs)) and bool(np.isfinite(np.float32(255.0 / float(cs if cs != 0 else 1.0))))


def unmold_mask(m, box, W, H, reading="f32"):
    """steps 4 to 8 of one surviving row: uint8 [H, W] of 0 / 1.  box None (no defined coordinates) or not within the image, or m None (no channel): empty"""
    out = np.zeros((H, W), np.uint8)
    if box is None or m is None:
        return out
    y1, x1, y2, x2 = box
    if not (0 <= y1 < y2 <= H and 0 <= x1 < x2 <= W) or not mask_defined(m):
        return out
    r = resize_bytes(bytescale(m, reading), x2 - x1, y2 - y1)
    out[y1:y2, x1:x2] = (r >= 128).astype(np.uint8)            # f32(b) / 255.0f >= 0.5f, exactly from 128 on
    return out


def unmold_detections(det, masks, window, W, H, layout="nhwc", class_map=None, reading="f32"):
    """The whole rule.  det: float32 [R, 6]; masks: float32 [R, M, M, C] ('nhwc') or [R, C, M, M] ('nchw'); window: 4 ints.  Returns the padded outputs
    (masks [R, H, W] uint8, class ids [R] int32, boxes [R, 4] int32, scores [R] float32, rows [R] int32, kept)."""
    det = np.asarray(det, np.float32).reshape(-1, 6)
    R = det.shape[0]
    C = masks.shape[3] if layout == "nhwc" else masks.shape[1]
    o_m = np.zeros((R, H, W), np.uint8)
    o_c = np.full(R, -1, np.int32)
    o_b = np.zeros((R, 4), np.int32)
    o_s = np.zeros(R, np.float32)
    o_r = np.full(R, -1, np.int32)
    scale = box_scale(window, W, H)
    k = 0
    for r in range(count_rows(det)):
        box = row_box(det[r], window, scale)
        if box is not None and (box[2] - box[0]) * (box[3] - box[1]) <= 0:      # step 3 (Python ints: no overflow)
            continue
        cid = det[r, 4]
        valid = bool(cid >= np.float32(1.0)) and bool(cid < np.float32(C))     # (NaN: neither)
        c = int(cid) if valid else 0
        m = None
        if valid:
            m = masks[r, :, :, c] if layout == "nhwc" else masks[r, c]
        o_m[k] = unmold_mask(m, box, W, H, reading)
        o_c[k] = (int(class_map[c]) if class_map is not None else c) if valid else 0
        o_b[k] = box if box is not None else (0, 0, 0, 0)
        o_s[k] = det[r, 5]
        o_r[k] = r
        k += 1
    return o_m, o_c, o_b, o_s, o_r, k
