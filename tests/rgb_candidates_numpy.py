"""numpy statement of the pose-independent part of the photometric residual's gate (RGBResidual, EF/Cuda/reduce.cu:739-863; residual_body in
instancefusion_amd/csrc/ifx_track.hip): which pixels of a pyramid level can ever yield a photometric correspondence, whatever the pose.

  * inside the 16-pixel border (and the two narrower margins the kernel also states: j < w - 5, i < h - 1),
  * all 16 pixels of the 4x4 block rows i-2 .. i+1, columns j-2 .. j+1 of the frame's intensity image non-zero,
  * squared Sobel magnitude gx*gx + gy*gy, as a float, at least minGrad(level)^2 / sobelScale^2.

The frame side builds this set once per frame (option rgb_cand, the frame slot's candidate list); the list is unordered, so it is compared sorted."""
from __future__ import annotations

import numpy as np

MIN_GRAD = (5.0, 3.0, 1.0)      # RGBDOdometry's minimumGradientMagnitudes, finest level first
SOBEL_SCALE = 1.0 / 8.0
CAND_DTYPE = np.dtype([("pixel", np.uint32), ("gx", np.int16), ("gy", np.int16)])


def min_scale(level: int) -> np.float32:
    return np.float32(MIN_GRAD[level] ** 2 / SOBEL_SCALE ** 2)


def gate_mask(next_img: np.ndarray, didx: np.ndarray, didy: np.ndarray, level: int) -> np.ndarray:
    """Boolean image of the pixels that pass.  next_img: (h, w) uint8, didx / didy: (h, w) int16, all of one pyramid level."""
    h, w = next_img.shape
    i, j = np.mgrid[0:h, 0:w]
    ok = (i >= 16) & (i < h - 16) & (j >= 16) & (j < w - 16) & (j < w - 5) & (i < h - 1)
    nz = next_img != 0
    block = np.ones((h, w), bool)
    for a in range(-2, 2):
        for b in range(-2, 2):
            block &= np.roll(nz, (-a, -b), axis=(0, 1))   # [i, j] <- nz[i + a, j + b]; the wrap-around only reaches pixels outside the border
    gx, gy = didx.astype(np.int32), didy.astype(np.int32)
    m2 = (gx * gx + gy * gy).astype(np.float32)
    return ok & block & (m2 >= min_scale(level))


def gate_entries(next_img: np.ndarray, didx: np.ndarray, didy: np.ndarray, level: int) -> np.ndarray:
    """The candidate entries {pixel index, gx, gy} of the level, sorted by pixel."""
    m = gate_mask(next_img, didx, didy, level)
    pix = np.flatnonzero(m)
    out = np.zeros(pix.shape[0], CAND_DTYPE)
    out["pixel"] = pix
    out["gx"] = didx.reshape(-1)[pix]
    out["gy"] = didy.reshape(-1)[pix]
    return out


def sorted_entries(entries: np.ndarray) -> np.ndarray:
    return np.sort(entries, order="pixel")
