"""The rule of ifx_molded_input_size / ifx_detector_input_molded in numpy (include/ifx_c_api.h): MaskRCNN.mold_inputs (deps/mask_rcnn/model.py:2247-2283) =
utils.resize_image (deps/mask_rcnn/utils.py:384-432) with padding + mold_image (model.py:2524-2529).  Python's own arithmetic for the size rule, Pillow's 8-bit
bilinear resampling from detector_input_numpy, every cast of the float tail written out.  No torch, no Pillow."""
import numpy as np

import detector_input_numpy as di

MEAN_PIXEL = (123.7, 116.8, 103.9)


def molded_size(w, h, min_dim, max_dim):
    """(nw, nh, S, S, top, left, top + nh, left + nw), or None where the library refuses (an empty or too large image, a resize scale above 8)"""
    if w < 1 or h < 1 or max_dim < 1:
        return None
    scale = 1
    if min_dim > 0:
        scale = max(1, min_dim / min(h, w))                    # utils.py:411: scale up but not down
    if round(max(h, w) * scale) > max_dim:                     # utils.py:415 (Python 3's round: half to even)
        scale = max_dim / max(h, w)
    nh, nw = (round(h * scale), round(w * scale)) if scale != 1 else (h, w)
    if not (1 <= nh <= max_dim and 1 <= nw <= max_dim):
        return None
    if h / nh > di.MAX_SCALE or w / nw > di.MAX_SCALE:
        return None
    top, left = (max_dim - nh) // 2, (max_dim - nw) // 2
    return nw, nh, max_dim, max_dim, top, left, top + nh, left + nw


def molded_input(img, min_dim=800, max_dim=1024, mean=MEAN_PIXEL, channels_last=True):
    """the whole rule on a uint8 [h, w, 3] image: (float32 [S, S, 3] or [3, S, S], window (y1, x1, y2, x2)).  mold_image: f32 array - f64 array -> f64, cast to
    f32 by Keras: f32(f64(b) - mean[c]); the padding is byte 0 before the subtraction."""
    h, w, _ = img.shape
    nw, nh, S, _, top, left, bottom, right = molded_size(w, h, min_dim, max_dim)
    padded = np.zeros((S, S, 3), np.uint8)
    padded[top:bottom, left:right] = di.resize(img, nw, nh)
    out = (padded.astype(np.float64) - np.asarray(mean, np.float64).reshape(1, 1, 3)).astype(np.float32)
    if not channels_last:
        out = np.ascontiguousarray(out.transpose(2, 0, 1))
    return out, (top, left, bottom, right)
