"""Multi-level ROI pooling in numpy, as include/ifx_c_api.h states it (ifx_fpn_roi_align; k_fpn_roi_align in csrc/ifx_detector.hip): maskrcnn-benchmark's FPN
Pooler (maskrcnn_benchmark/modeling/poolers.py:11-121) -- LevelMapper's level per ROI, then ROIAlign on that level's map.  The pooling itself is
detector_ops_numpy.roi_align_forward.  Held against the reference's own Pooler.forward and LevelMapper by tests/test_fpn_pooler_cpu.py through
tests/golden/fpn_pooler_ref.npz.

The level of an ROI, every operation rounded to f32 and none fused: area = (x1 - x0 + 1) * (y1 - y0 + 1); s = sqrt(area); v = s / s0 + eps;
L = log2(v) in f64, rounded once to f32; t = f32(lvl0 + L); level = clamp(floor(t), k_min, k_max) - k_min.  A NaN t (a negative or NaN area, a negative v) is no
level, -1: the ROI's outputs are zeros.  On the device the level is the number of thresholds T_1 .. T_{levels-1} that v reaches (level_thresholds below)."""
import numpy as np

import detector_ops_numpy as dn

F = np.float32


def ladder(scales):
    """(k_min, k_max) of scales[l] == 2^-(k_min + l), k_min >= 0; None for any other list"""
    scales = [F(s) for s in scales]
    if not 1 <= len(scales) <= 8:
        return None
    for k in range(0, 127):
        if scales[0] == F(2.0 ** -k):
            break
    else:
        return None
    if k + len(scales) - 1 > 126 or any(s != F(2.0 ** -(k + l)) for l, s in enumerate(scales)):
        return None
    return k, k + len(scales) - 1


def rule_value(v, canonical_level=4):
    """floor(f32(lvl0 + f32(log2(v)))) of f32 v, as f32: NaN for a NaN or negative v, -inf for 0"""
    v = np.asarray(v, F)
    with np.errstate(invalid="ignore", divide="ignore"):
        L = np.log2(v.astype(np.float64)).astype(F)
        t = F(canonical_level) + L
    assert t.dtype == F
    return np.floor(t)


def level_of_v(v, k_min, k_max, canonical_level=4):
    """the level index of v (int32), -1 for no level"""
    f = rule_value(v, canonical_level)
    with np.errstate(invalid="ignore"):
        lev = np.clip(f, F(k_min), F(k_max)) - F(k_min)
    return np.where(np.isnan(f), -1, np.nan_to_num(lev, nan=0.0)).astype(np.int32)


def v_of_rois(rois, canonical_scale=224, eps=1e-6):
    """v = sqrt(area) / s0 + eps of n x 5 ROIs (f32)"""
    r = np.ascontiguousarray(rois, F).reshape(-1, 5)
    one = F(1)
    with np.errstate(invalid="ignore", over="ignore"):
        area = (r[:, 3] - r[:, 1] + one) * (r[:, 4] - r[:, 2] + one)
        s = np.sqrt(area)
        v = s / F(canonical_scale) + F(eps)
    assert v.dtype == F
    return v


def levels(rois, k_min, k_max, canonical_scale=224, canonical_level=4, eps=1e-6):
    return level_of_v(v_of_rois(rois, canonical_scale, eps), k_min, k_max, canonical_level)


def level_thresholds(k_min, k_max, canonical_level=4):
    """T_j, j = 1 .. k_max - k_min: the smallest f32 v >= 0 whose rule value reaches k_min + j, by bisection over the bit patterns 0 .. +inf (the value is
    monotone in v).  With them the level of a v >= 0 is the number of j with v >= T_j."""
    out = []
    for j in range(1, k_max - k_min + 1):
        lo, hi = 0, 0x7F800000                       # the rule value of 0 is -inf, that of +inf is +inf
        while hi - lo > 1:
            mid = (lo + hi) // 2
            if rule_value(np.asarray([mid], np.uint32).view(F), canonical_level)[0] >= k_min + j:
                hi = mid
            else:
                lo = mid
        out.append(hi)
    return np.asarray(out, np.uint32).view(F)


def level_by_thresholds(v, thresholds):
    """what the device does with the thresholds: -1 unless v >= 0, else the number of thresholds reached"""
    v = np.asarray(v, F)
    with np.errstate(invalid="ignore"):
        lev = (v[..., None] >= np.asarray(thresholds, F)).sum(axis=-1).astype(np.int32)
        return np.where(v >= 0, lev, -1).astype(np.int32)


def fpn_roi_align(features, rois, scales, pooled_h, pooled_w, sampling_ratio, canonical_scale=224, canonical_level=4, eps=1e-6):
    """features: a list of [B,C,H_l,W_l] f32; rois [n,5] f32 -> (out [n,C,pooled_h,pooled_w] f32, levels [n] int32)"""
    k = ladder(scales)
    assert k is not None and len(features) == len(scales)
    rois = np.ascontiguousarray(rois, F).reshape(-1, 5)
    n, C = rois.shape[0], features[0].shape[1]
    if len(features) == 1:                           # no mapping at all (poolers.py:101-102)
        return dn.roi_align_forward(features[0], rois, F(scales[0]), pooled_h, pooled_w, sampling_ratio), np.zeros(n, np.int32)
    lev = levels(rois, k[0], k[1], canonical_scale, canonical_level, eps)
    out = np.zeros((n, C, pooled_h, pooled_w), F)
    for l, (f, s) in enumerate(zip(features, scales)):
        idx = np.nonzero(lev == l)[0]
        if idx.size:
            out[idx] = dn.roi_align_forward(f, rois[idx], F(s), pooled_h, pooled_w, sampling_ratio)
    return out, lev
