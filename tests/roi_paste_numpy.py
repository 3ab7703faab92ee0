"""The ROI paste of ifx_process_segmentation_rois as a CPU statement: maskrcnn-benchmark's Masker (paste_mask_in_image with expand_masks / expand_boxes,
maskrcnn_benchmark/modeling/roi_heads/mask_head/inference.py:91-154) restated in float32, one rounding per operation and no fused multiply-add, followed by the
bridge's two steps (binarise to 0/255, stable sort by area, descending) and the overlap clean.  The kernels k_roi_area / k_roi_gather follow this operation order;
tests/test_roi_paste_cpu.py holds it against the reference's own masks (tests/golden/roi_paste_ref.npz)."""
import os

import numpy as np

F = np.float32
HALF = F(0.5)
COORD_LIMIT = F(16777216.0)   # 2^24: a box coordinate beyond it (or a non-finite one) gives an empty mask -- the reference raises there
BAND = 2.0 ** -22             # |v - threshold| <= BAND: a tie the reference's vectorised kernel (which contracts to FMA) may decide the other way


def roi_record(box, M, W, H):
    """Steps 1-7: (b0, b1, X0, X1, Y0, Y1, sx, sy) of a box (x0, y0, x1, y1) for an M x M ROI in a W x H image, or None for an empty mask."""
    b = np.asarray(box, F).reshape(4)
    if not np.all(np.isfinite(b)) or np.any(np.abs(b) > COORD_LIMIT):
        return None
    S = M + 2
    scale = F(float(S) / M)
    wh = (b[2] - b[0]) * HALF
    hh = (b[3] - b[1]) * HALF
    xc = (b[2] + b[0]) * HALF
    yc = (b[3] + b[1]) * HALF
    wh = wh * scale
    hh = hh * scale
    e = np.trunc(np.array([xc - wh, yc - hh, xc + wh, yc + hh], F)).astype(np.int64)   # (every term is an f32; |e| < 2^26)
    b0, b1, b2, b3 = (int(t) for t in e)
    w = max(b2 - b0 + 1, 1)
    h = max(b3 - b1 + 1, 1)
    sx = F(S) / F(w)
    sy = F(S) / F(h)
    X0, X1 = max(b0, 0), min(b2 + 1, W)
    Y0, Y1 = max(b1, 0), min(b3 + 1, H)
    if X1 <= X0 or Y1 <= Y0:
        return None
    return b0, b1, X0, X1, Y0, Y1, sx, sy


def _axis(s, lo, hi, b, S):
    """Step 8 for the pixels lo .. hi - 1 of one axis: (i0, i1, l0, l1)"""
    d = (np.arange(lo, hi, dtype=np.int64) - b).astype(F)
    r = np.maximum(s * (d + HALF) - HALF, F(0))
    i0 = np.minimum(r.astype(np.int64), S - 1)
    i1 = np.minimum(i0 + 1, S - 1)
    l1 = r - i0.astype(F)
    l0 = F(1) - l1
    return i0, i1, l0, l1


def paste_values(roi, box, W, H):
    """Steps 1-9: ((X0, X1, Y0, Y1), v) with v the interpolated f32 values of the clip rectangle, or (None, None) for an empty mask."""
    roi = np.asarray(roi, F)
    M = roi.shape[-1]
    roi = roi.reshape(M, M)
    rec = roi_record(box, M, W, H)
    if rec is None:
        return None, None
    b0, b1, X0, X1, Y0, Y1, sx, sy = rec
    S = M + 2
    pm = np.zeros((S, S), F)
    pm[1:-1, 1:-1] = roi
    xi0, xi1, xl0, xl1 = _axis(sx, X0, X1, b0, S)
    yi0, yi1, yl0, yl1 = _axis(sy, Y0, Y1, b1, S)
    with np.errstate(invalid="ignore", over="ignore"):
        top = xl0[None, :] * pm[yi0][:, xi0] + xl1[None, :] * pm[yi0][:, xi1]
        bot = xl0[None, :] * pm[yi1][:, xi0] + xl1[None, :] * pm[yi1][:, xi1]
        v = yl0[:, None] * top + yl1[:, None] * bot
    assert v.dtype == F
    return (X0, X1, Y0, Y1), v


def paste_roi(roi, box, W, H, thr, with_band=False):
    """Steps 1-10: the H x W mask (0 / 255) of one ROI; with_band: also the pixels whose value lies within BAND of the threshold."""
    out = np.zeros((H, W), np.uint8)
    band = np.zeros((H, W), bool)
    rect, v = paste_values(roi, box, W, H)
    if rect is not None:
        X0, X1, Y0, Y1 = rect
        with np.errstate(invalid="ignore"):
            out[Y0:Y1, X0:X1] = np.where(v > F(thr), 255, 0)   # NaN compares false: outside
            band[Y0:Y1, X0:X1] = np.abs(v.astype(np.float64) - float(F(thr))) <= BAND
    return (out, band) if with_band else out


def paste_rois(rois, boxes, class_ids, W, H, thr):
    """What the ingestion leaves: (ori [n,H,W] 0/255 in the bridge's order, the overlap-cleaned masks, order [n] input indices, class ids in that order)."""
    n = len(boxes)
    pasted = [paste_roi(rois[i], boxes[i], W, H, thr) for i in range(n)]
    area = [int((m != 0).sum()) for m in pasted]
    order = sorted(range(n), key=lambda i: -area[i])   # stable: ties keep their input order
    ori = np.stack([pasted[i] for i in order]) if n else np.zeros((0, H, W), np.uint8)
    clean = ori.copy()
    flag = np.zeros((H, W), bool)
    for s in range(n - 1, -1, -1):   # maskCleanOverlap: a pixel stays in the last mask of the order that holds it
        clean[s][flag] = 0
        flag |= ori[s] != 0
    return ori, clean, np.asarray(order, np.int32), np.asarray([class_ids[i] for i in order], np.int32)


def load_fixture():
    """The cases of tests/golden/roi_paste_ref.npz: dicts of W, H, M, thr, box (f32[4]), roi (f32[M,M] = f32(q) / f32(255)), ref (bool[H,W], the reference's mask)."""
    d = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "roi_paste_ref.npz"))
    cases, qo, bo = [], 0, 0
    for i in range(len(d["w"])):
        W, H, M = int(d["w"][i]), int(d["h"][i]), int(d["m"][i])
        q = d["roi_q"][qo:qo + M * M].reshape(M, M); qo += M * M
        nb = (W * H + 7) // 8
        ref = np.unpackbits(d["ref_bits"][bo:bo + nb])[:W * H].reshape(H, W).astype(bool); bo += nb
        cases.append(dict(W=W, H=H, M=M, thr=float(d["thr"][i]), box=d["boxes"][i].astype(np.float32), roi=q.astype(np.float32) / np.float32(255), ref=ref))
    assert qo == len(d["roi_q"]) and bo == len(d["ref_bits"])
    return cases


def rois_from_masks(masks, M=28):
    """What a mask head would have produced for image-sized masks (n x H x W, non-zero = inside): the tight box of each mask (x0, y0, x1, y1: its first and last
    column and row) and the M x M area average of its crop, float32.  An empty mask gives a zero box and zero probabilities."""
    def avg(n_out, n_in):
        e = np.linspace(0.0, n_in, n_out + 1)
        j = np.arange(n_in)
        return np.clip(np.minimum(e[1:, None], j[None, :] + 1.0) - np.maximum(e[:-1, None], j[None, :]), 0.0, None) / (e[1:] - e[:-1])[:, None]

    rois = np.zeros((len(masks), M, M), F)
    boxes = np.zeros((len(masks), 4), F)
    for i, m in enumerate(masks):
        ys, xs = np.nonzero(m)
        if not len(ys):
            continue
        x0, x1, y0, y1 = xs.min(), xs.max(), ys.min(), ys.max()
        crop = (m[y0:y1 + 1, x0:x1 + 1] != 0).astype(np.float64)
        rois[i] = (avg(M, crop.shape[0]) @ crop @ avg(M, crop.shape[1]).T).astype(F)
        boxes[i] = (x0, y0, x1, y1)
    return rois, boxes
