#!/usr/bin/env python3
"""Writes tests/golden/detector_ops_ref.npz: what maskrcnn-benchmark's own CPU operators give on small inputs.

    python tools/make_golden_detector_ops.py /path/to/maskrcnn_benchmark

csrc/cpu/nms_cpu.cpp and csrc/cpu/ROIAlign_cpu.cpp are compiled FROM THEIR FILES, unmodified, as a throw-away torch extension (torch.utils.cpp_extension.load with
its build directory in a temporary directory outside the repository): nothing compiled is kept and none of their text is in this repository.  Against the installed
torch they need a stand-in "cpu/vision.h" on the include path -- the lines below, this tool's own -- and a module definition in a second file.
The file holds inputs and outputs only.  ROIAlign: scales 1/16 .. 1, pooled 1x1 / 2x3 / 7x7 / 14x14, sampling ratios 0 .. 3, ROIs partly and wholly outside,
malformed (reversed) ROIs, height or width 1, channels 1 / 3 / 5, feature maps up to 17 x 13, finite values.  NMS: n = 1 .. 300, thresholds 0.3 / 0.5 / 0.7,
distinct scores (the reference's sort is not stable) and NO pair whose IoU equals the threshold, the one place where nms_cpu.cpp (>=) and nms.cu (>) part: such
pairs are counted with the numpy statement, a case that has one is drawn again, and the count (0) is stored.
Before writing, the numpy statement (tests/detector_ops_numpy.py) is held against every stored figure."""
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
OUT = os.path.join(ROOT, "tests", "golden", "detector_ops_ref.npz")

VISION_H = """#pragma once
#include <torch/extension.h>
#define AT_ASSERTM TORCH_CHECK
namespace detail { inline at::ScalarType scalar_type(const at::DeprecatedTypeProperties& t) { return t.scalarType(); } }
at::Tensor ROIAlign_forward_cpu(const at::Tensor& input, const at::Tensor& rois, const float spatial_scale, const int pooled_height, const int pooled_width, const int sampling_ratio);
at::Tensor nms_cpu(const at::Tensor& dets, const at::Tensor& scores, const float threshold);
"""
MODULE_CPP = """#include "cpu/vision.h"
PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) { m.def("nms", &nms_cpu); m.def("roi_align_forward", &ROIAlign_forward_cpu); }
"""

POOLED = ((1, 1), (2, 3), (7, 7), (14, 14))
SCALES = (1.0 / 16, 1.0 / 8, 0.25, 0.5, 1.0)
ROI_CASES = 40
NMS_CASES = 60


def load_reference(pkg, tmp):
    from torch.utils.cpp_extension import load

    inc = os.path.join(tmp, "include")
    os.makedirs(os.path.join(inc, "cpu"))
    os.makedirs(os.path.join(tmp, "build"))
    with open(os.path.join(inc, "cpu", "vision.h"), "w") as f:
        f.write(VISION_H)
    mod = os.path.join(tmp, "module.cpp")
    with open(mod, "w") as f:
        f.write(MODULE_CPP)
    src = [os.path.join(pkg, "csrc", "cpu", "nms_cpu.cpp"), os.path.join(pkg, "csrc", "cpu", "ROIAlign_cpu.cpp"), mod]
    return load(name="detector_ops_ref", sources=src, extra_include_paths=[inc], extra_cflags=["-O2", "-ffp-contract=off", "-w"],
                build_directory=os.path.join(tmp, "build"), verbose=False)


def roi_case(rng, k):
    """one ROIAlign case: (input [B,C,H,W], rois [n,5], scale, ph, pw, ratio)"""
    ph, pw = POOLED[k % 4]
    ratio = (k // 4) % 4
    scale = SCALES[k % 5]
    C = (1, 3, 5)[k % 3]
    B = 1 + k % 2
    H, W = int(rng.integers(2, 18)), int(rng.integers(2, 14))
    if k % 10 == 7:
        H = 1
    if k % 10 == 9:
        W = 1
    inp = rng.standard_normal((B, C, H, W)).astype(np.float32)
    n = 6 if ph * pw > 49 else 12
    iw, ih = W / scale, H / scale                       # the image the ROIs live in
    x0 = rng.uniform(-0.3 * iw, 1.1 * iw, n)
    y0 = rng.uniform(-0.3 * ih, 1.1 * ih, n)
    x1 = x0 + rng.uniform(0, 0.9 * iw, n)
    y1 = y0 + rng.uniform(0, 0.9 * ih, n)
    rois = np.stack([rng.integers(0, B, n).astype(np.float64), x0, y0, x1, y1], axis=1).astype(np.float32)
    rois[1, 1:] = (-3 * iw, -3 * ih, -2 * iw, -2 * ih)  # wholly outside
    rois[2, 1:] = (2 * iw, 2 * ih, 3 * iw, 3 * ih)
    rois[3, 1:] = rois[3, [3, 4, 1, 2]]                 # malformed: reversed
    rois[4, 1:] = (0, 0, iw, ih)                        # the whole map
    if ratio == 0 and ph * pw > 49:                     # (an adaptive grid on 14 x 14 bins: keep the ROIs near the map)
        rois[:, 1:] = np.clip(rois[:, 1:], -iw, 2 * iw)
    return inp, rois, np.float32(scale), ph, pw, ratio


def nms_case(rng, k, dn):
    n = (1, 2, 3, 63, 64, 65, 128, 129, 200, 300)[k % 10] if k < 20 else int(rng.integers(1, 301))
    thr = (0.3, 0.5, 0.7)[k % 3]
    while True:
        c = rng.uniform(0, 60, (n, 2))
        wh = rng.uniform(4, 40, (n, 2))
        boxes = np.concatenate([c, c + wh], axis=1).astype(np.float32)      # not rounded: integer boxes do meet 0.5 exactly
        scores = rng.permutation(n).astype(np.float32) / np.float32(n) + np.float32(0.001)
        assert np.unique(scores).size == n
        if dn.pairs_at_threshold(boxes, thr) == 0:
            return boxes, scores, np.float32(thr)


def main():
    import torch

    import detector_ops_numpy as dn

    if len(sys.argv) != 2:
        sys.exit(__doc__)
    rng = np.random.default_rng(20261018)
    data = {}
    with tempfile.TemporaryDirectory() as tmp:
        assert not os.path.abspath(tmp).startswith(ROOT + os.sep)
        ref = load_reference(sys.argv[1], tmp)
        outputs = 0
        for k in range(ROI_CASES):
            inp, rois, scale, ph, pw, ratio = roi_case(rng, k)
            out = ref.roi_align_forward(torch.from_numpy(inp), torch.from_numpy(rois), float(scale), ph, pw, ratio).numpy()
            assert np.isfinite(out).all()
            mine = dn.roi_align_forward(inp, rois, scale, ph, pw, ratio)
            diff = int((mine.view(np.uint32) != out.view(np.uint32)).sum())
            assert mine.shape == out.shape and diff == 0, (k, diff, out.size)
            outputs += out.size
            data[f"roi{k}_input"], data[f"roi{k}_rois"], data[f"roi{k}_out"] = inp, rois, out
            data[f"roi{k}_par"] = np.asarray([scale, ph, pw, ratio], np.float64)
        kept = 0
        for k in range(NMS_CASES):
            boxes, scores, thr = nms_case(rng, k, dn)
            keep = ref.nms(torch.from_numpy(boxes), torch.from_numpy(scores), float(thr)).numpy().astype(np.int64)
            mine = dn.nms(boxes, scores, thr)
            assert np.array_equal(mine, keep), (k, mine, keep)
            kept += keep.size
            data[f"nms{k}_boxes"], data[f"nms{k}_scores"], data[f"nms{k}_keep"] = boxes, scores, keep
            data[f"nms{k}_par"] = np.asarray([thr, dn.pairs_at_threshold(boxes, thr)], np.float64)
    data["counts"] = np.asarray([ROI_CASES, NMS_CASES], np.int32)
    print(f"{ROI_CASES} ROIAlign cases with {outputs} outputs, {NMS_CASES} NMS cases with {kept} kept boxes: the statement equals every one")
    np.savez_compressed(OUT, **data)
    print(f"{OUT}: {os.path.getsize(OUT)} bytes")
    assert os.path.getsize(OUT) < 600000


if __name__ == "__main__":
    main()
