#!/usr/bin/env python3
"""Writes tests/golden/unmold_cases.npz: inputs and recorded results of the reference's own utils.unmold_mask and utils.resize_image
(deps/mask_rcnn/utils.py:490-507, 384-432), executed as they lie.  CPU only; needs the reference tree, numpy and Pillow:

    python tools/make_golden_unmold.py <reference tree>

utils.py is loaded by path.  Its imports of tensorflow and skimage, which the two functions never touch, are met by empty stand-in modules.  scipy.misc.imresize,
which left scipy long ago, is defined here as what it was: bytescale (cmin, cmax the array's own, low 0, high 255; uint8 passes unchanged), Image.frombytes, PIL's
resize with BILINEAR, back to an array.  bytescale is written with every cast spelled out in the reading numpy had when the reference was written (float /
np.float32 gave a float64 scalar, and a float64 scalar did not widen a float32 array); the other reading (the scalar widens the array to f64) is evaluated beside it
and the number of bytes on which the two differ over the cases is recorded in the fixture (`bytescale_f64_differs`), for information.

The fixture holds arrays only: masks, boxes and the bit-packed results of unmold_mask; for resize_image the image sizes, dims, windows, scales, a CRC-32 of the padded
image and a 64 x 64 crop of it (the images themselves are made by `pattern_image`, which the tests import from here)."""
import importlib.util
import os
import sys
import types
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "unmold_cases.npz")
IMAGE_W, IMAGE_H = 160, 120
F64_DIFFERS = [0]


def pattern_image(w, h):
    """a deterministic uint8 [h, w, 3] image with structure at every scale"""
    y, x = np.mgrid[0:h, 0:w].astype(np.int64)
    return np.stack([(x * 7 + y * 13 + c * 29 + (x * y) % 251 + ((x // 16 + y // 16) % 2) * 90) & 255 for c in range(3)], axis=-1).astype(np.uint8)


def bytescale(data):
    if data.dtype == np.uint8:
        return data
    data = np.asarray(data)
    cmin, cmax = data.min(), data.max()
    cscale = cmax - cmin
    if cscale == 0:
        cscale = 1
    scale = np.float64(255.0) / np.float64(cscale)
    if data.dtype == np.float32:
        d = (data - np.float32(cmin)).astype(np.float32)
        narrow = ((d * np.float32(scale)).astype(np.float32).clip(np.float32(0), np.float32(255)) + np.float32(0.5)).astype(np.uint8)
        wide = ((d.astype(np.float64) * scale).clip(0.0, 255.0) + 0.5).astype(np.uint8)
        F64_DIFFERS[0] += int((narrow != wide).sum())
        return narrow
    return (((data - cmin) * scale).clip(0, 255) + 0.5).astype(np.uint8)


def imresize(arr, size, interp="bilinear", mode=None):
    from PIL import Image

    assert interp == "bilinear" and mode is None
    b = np.ascontiguousarray(bytescale(np.asarray(arr)))
    if b.ndim == 2:
        im = Image.frombytes("L", (b.shape[1], b.shape[0]), b.tobytes())
    else:
        im = Image.frombytes("RGB", (b.shape[1], b.shape[0]), b.tobytes())
    return np.array(im.resize((int(size[1]), int(size[0])), resample=Image.BILINEAR))


def load_utils(tree):
    import scipy

    for name in ("tensorflow", "skimage", "skimage.color", "skimage.io"):
        sys.modules.setdefault(name, types.ModuleType(name))
    misc = types.ModuleType("scipy.misc")
    misc.imresize = imresize
    sys.modules["scipy.misc"] = misc
    scipy.misc = misc
    spec = importlib.util.spec_from_file_location("ref_mask_rcnn_utils", os.path.join(tree, "deps", "mask_rcnn", "utils.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def smooth_mask(rng, M):
    y, x = np.mgrid[0:M, 0:M].astype(np.float64) / max(M - 1, 1)
    cx, cy = rng.uniform(0.3, 0.7, 2)
    p = 1.0 / (1.0 + np.exp((np.hypot(x - cx, y - cy) - rng.uniform(0.2, 0.6)) * rng.uniform(4, 20)))
    return (p * rng.uniform(0.5, 1.0) + rng.uniform(0.0, 0.05) * rng.random((M, M))).astype(np.float32)


def unmold_cases(rng):
    """(mask, box) pairs: boxes of one pixel, 1 x wide, tall x 1, exactly M, upscaling, downscaling, at the image's edges; a constant mask; a lone maximum"""
    W, H, M = IMAGE_W, IMAGE_H, 28
    cases = []
    for box in [(5, 7, 6, 8), (0, 0, 1, 1), (H - 1, W - 1, H, W), (10, 3, 11, 150), (2, 40, 118, 41), (0, 0, 28, 28), (50, 60, 78, 88), (92, 132, 120, 160),
                (0, 0, H, W), (0, 0, 28, W), (0, 0, H, 28), (30, 30, 33, 37), (30, 30, 44, 44), (30, 30, 57, 59), (0, 100, 90, 160), (60, 0, 120, 90),
                (10, 10, 38, 100), (10, 10, 100, 38), (7, 9, 9, 11), (1, 1, 119, 159)]:
        cases.append((smooth_mask(rng, M), box))
    cases.append((np.full((M, M), 0.7, np.float32), (20, 20, 60, 70)))                     # cs == 0: every byte 0
    cases.append((np.zeros((M, M), np.float32), (20, 20, 60, 70)))
    lone = np.zeros((M, M), np.float32); lone[13, 17] = 1.0
    cases.append((lone, (20, 20, 90, 110)))
    cases.append((lone, (20, 20, 30, 30)))
    cases.append(((smooth_mask(rng, M) - 0.5).astype(np.float32), (15, 25, 75, 95)))      # negative samples: the stretch moves them
    cases.append(((smooth_mask(rng, M) * 1e-3).astype(np.float32), (15, 25, 75, 95)))     # all below 0.5: the stretch still fills the box's core
    while len(cases) < 40:
        y1, x1 = int(rng.integers(0, H - 1)), int(rng.integers(0, W - 1))
        cases.append((rng.random((M, M)).astype(np.float32) if len(cases) % 2 else smooth_mask(rng, M),
                      (y1, x1, int(rng.integers(y1 + 1, H + 1)), int(rng.integers(x1 + 1, W + 1)))))
    return cases


def crop_of(img, window):
    cy, cx = max(window[0] - 8, 0), max(window[1] - 8, 0)
    c = np.zeros((64, 64, 3), np.uint8)
    part = img[cy:cy + 64, cx:cx + 64]
    c[:part.shape[0], :part.shape[1]] = part
    return c


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    if len(args) != 1:
        sys.exit(__doc__)
    utils = load_utils(args[0])
    rng = np.random.default_rng(20260)
    out = {}
    cases = unmold_cases(rng)
    out["image_size"] = np.array([IMAGE_W, IMAGE_H], np.int32)
    out["masks"] = np.stack([m for m, _ in cases])
    out["boxes"] = np.array([b for _, b in cases], np.int32)
    full = [utils.unmold_mask(m, np.array(b, np.int32), (IMAGE_H, IMAGE_W, 3)) for m, b in cases]
    assert all(f.dtype == np.uint8 and f.shape == (IMAGE_H, IMAGE_W) and f.max() <= 1 for f in full)
    out["unmolded_bits"] = np.packbits(np.stack(full).reshape(len(cases), -1), axis=1)
    out["bytescale_f64_differs"] = np.array([F64_DIFFERS[0]], np.int64)

    # resize_image: the sizes alone on a grid (zero images), then the bytes of pattern images
    grid, grid_ref = [], []
    for (w, h) in [(640, 480), (480, 640), (160, 120), (120, 160), (100, 76), (64, 64), (33, 200), (1, 1), (300, 7)]:
        for (mn, mx) in [(800, 1024), (512, 512), (128, 128), (200, 256), (0, 160), (0, 640), (100, 101), (90, 94), (75, 77)]:
            try:
                img, window, scale, _ = utils.resize_image(np.zeros((h, w, 3), np.uint8), min_dim=mn, max_dim=mx, padding=True)
            except Exception:
                continue                                   # (a negative pad: the image does not fit max_dim)
            grid.append((w, h, mn, mx))
            grid_ref.append((img.shape[1], img.shape[0]) + tuple(int(v) for v in window))
    out["size_cases"] = np.array(grid, np.int32)
    out["size_ref"] = np.array(grid_ref, np.int32)             # S, S, wy1, wx1, wy2, wx2
    inputs, ref, crops = [], [], []
    for (w, h, mn, mx) in [(640, 480, 512, 512), (640, 480, 800, 1024), (160, 120, 128, 128), (160, 120, 200, 256), (160, 120, 0, 160), (120, 160, 200, 256)]:
        img, window, scale, _ = utils.resize_image(pattern_image(w, h), min_dim=mn, max_dim=mx, padding=True)
        assert img.dtype == np.uint8 and img.shape == (mx, mx, 3)
        inputs.append((w, h, mn, mx))
        ref.append(tuple(int(v) for v in window) + (zlib.crc32(np.ascontiguousarray(img).tobytes()),))
        crops.append(crop_of(img, window))
        print(f"resize_image {w}x{h} ({mn},{mx}): window {tuple(window)}, scale {scale}")
    out["input_cases"] = np.array(inputs, np.int32)
    out["input_ref"] = np.array(ref, np.int64)                 # wy1, wx1, wy2, wx2, crc32 of the padded bytes
    out["input_crops"] = np.stack(crops)
    np.savez_compressed(OUT, **out)
    print(f"{OUT}: {len(cases)} unmold cases, {len(grid)} sizes, {len(inputs)} inputs, {os.path.getsize(OUT)} bytes; "
          f"bytescale readings differ on {F64_DIFFERS[0]} bytes")


if __name__ == "__main__":
    main()
