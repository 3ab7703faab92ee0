#!/usr/bin/env python3
"""Writes tests/golden/roi_paste_ref.npz: ROI masks and boxes with the image-sized masks that maskrcnn-benchmark's own paste_mask_in_image makes of them.

    python tools/make_golden_roi_paste.py /path/to/maskrcnn_benchmark/modeling/roi_heads/mask_head/inference.py

The three functions (expand_boxes, expand_masks, paste_mask_in_image) are taken from that file BY PATH AT RUN TIME -- their ast nodes, executed with
interpolate = torch.nn.functional.interpolate -- and run on CPU torch; none of their text is in this repository.  The file holds, per case, the image size, M,
the threshold, the box, the ROI probabilities as bytes q (the ROI is float32(q) / float32(255): smooth, and never exactly a threshold) and the reference's mask,
bit-packed.  Before writing, the float32 restatement (tests/roi_paste_numpy.py) is held against the masks with the conditions of tests/test_roi_paste_cpu.py."""
import ast
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
OUT = os.path.join(ROOT, "tests", "golden", "roi_paste_ref.npz")
SIZES = ((160, 120), (320, 240))
MS = (7, 14, 28, 29, 56)
THRESHOLDS = (0.5, 0.25, 0.7)


def load_reference(path):
    import torch

    with open(path) as f:
        tree = ast.parse(f.read())
    want = ("expand_boxes", "expand_masks", "paste_mask_in_image")
    nodes = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name in want]
    assert sorted(n.name for n in nodes) == sorted(want), [n.name for n in nodes]
    ns = {"torch": torch, "interpolate": torch.nn.functional.interpolate}
    exec(compile(ast.Module(body=nodes, type_ignores=[]), path, "exec"), ns)
    return ns["paste_mask_in_image"]


def smooth_roi(rng, M):
    """A blob of probabilities with a few waves on it, quantised to bytes."""
    y, x = np.mgrid[0:M, 0:M].astype(np.float64) / max(M - 1, 1)
    cx, cy = rng.uniform(0.3, 0.7, 2)
    rad = rng.uniform(0.25, 0.6)
    p = 1.0 / (1.0 + np.exp((np.hypot(x - cx, y - cy) - rad) * rng.uniform(6, 20)))
    for _ in range(3):
        fx, fy = rng.uniform(-9, 9, 2)
        p += rng.uniform(0.03, 0.15) * np.cos(fx * x + fy * y + rng.uniform(0, 6.28))
    return np.clip(np.rint(p * 255.0), 0, 255).astype(np.uint8)


def boxes_for(rng, W, H, k):
    """The box shapes of one (size, M, threshold) combination, already clipped to the image as the detector's clip_to_image leaves them (x in [0, W-1], y in
    [0, H-1]); k rotates which special shapes a combination gets, every shape appearing for every size and M."""
    def rnd():
        x0, x1 = np.sort(rng.uniform(0, W - 1, 2)); y0, y1 = np.sort(rng.uniform(0, H - 1, 2))
        return [x0, y0, x1, y1]

    ix, iy = int(rng.integers(2, W - 40)), int(rng.integers(2, H - 40))
    special = [
        [ix + 0.3, iy + 0.4, ix + 0.6, iy + 0.9],                                  # sub-pixel
        [ix, iy, ix + 1, iy + 1],                                                   # 1 px, integer corners
        [ix + 0.5, iy + 0.5, ix + 2.5, iy + 3.5],                                   # 2-3 px, half-integer corners
        [ix + 0.2, iy, ix + 3.1, iy + 1.7],                                         # 1-3 px
        [0, 0, W - 1, H - 1],                                                       # the whole image: the expansion leaves it on every side
        [0, iy, rng.uniform(5, W / 2), iy + rng.uniform(5, 30)],                    # touching the left border
        [rng.uniform(W / 2, W - 6), iy, W - 1, iy + rng.uniform(5, 30)],            # the right
        [ix, 0, ix + rng.uniform(5, 30), rng.uniform(5, H / 2)],                    # the top
        [ix, rng.uniform(H / 2, H - 6), ix + rng.uniform(5, 30), H - 1],            # the bottom
        [ix, iy, ix + int(rng.integers(4, 38)), iy + int(rng.integers(4, 38))],     # integer corners
        [ix + 0.5, iy + 0.5, ix + int(rng.integers(4, 38)) + 0.5, iy + int(rng.integers(4, 38)) + 0.5],   # half-integer corners
        [0, 0, rng.uniform(3, 40), rng.uniform(3, 40)],                             # a corner of the image
    ]
    pick = [special[(k * 5 + j) % len(special)] for j in range(5)]
    return np.asarray(pick + [rnd() for _ in range(3)], np.float32)


def main():
    import torch

    import roi_paste_numpy as rp

    if len(sys.argv) != 2:
        sys.exit(__doc__)
    paste = load_reference(sys.argv[1])
    rng = np.random.default_rng(20261017)
    torch.set_num_threads(1)
    W_, H_, M_, T_, B_, Q_, R_ = [], [], [], [], [], [], []
    box_px = band_px = differ_outside = differ_band = 0
    k = 0
    for (W, H) in SIZES:
        for M in MS:
            for thr in THRESHOLDS:
                for box in boxes_for(rng, W, H, k):
                    q = smooth_roi(rng, M)
                    roi = q.astype(np.float32) / np.float32(255)
                    ref = paste(torch.from_numpy(roi), torch.from_numpy(box), H, W, thresh=thr).numpy() != 0
                    mine, band = rp.paste_roi(roi, box, W, H, thr, with_band=True)
                    rect, _ = rp.paste_values(roi, box, W, H)
                    assert rect is not None
                    box_px += (rect[1] - rect[0]) * (rect[3] - rect[2])
                    band_px += int(band.sum())
                    diff = (mine != 0) != ref
                    differ_outside += int((diff & ~band).sum())
                    differ_band += int((diff & band).sum())
                    W_.append(W); H_.append(H); M_.append(M); T_.append(thr); B_.append(box); Q_.append(q.reshape(-1)); R_.append(np.packbits(ref.reshape(-1)))
                k += 1
    print(f"{len(W_)} cases, {box_px} box pixels, {band_px} within 2^-22 of the threshold, {differ_band} of those differ, {differ_outside} differ outside the band")
    assert differ_outside == 0
    assert band_px * 100000 <= box_px
    np.savez_compressed(OUT, w=np.asarray(W_, np.int32), h=np.asarray(H_, np.int32), m=np.asarray(M_, np.int32), thr=np.asarray(T_, np.float32),
                        boxes=np.stack(B_), roi_q=np.concatenate(Q_), ref_bits=np.concatenate(R_))
    print(f"{OUT}: {os.path.getsize(OUT)} bytes")
    assert os.path.getsize(OUT) < 1000000


if __name__ == "__main__":
    main()
