#!/usr/bin/env python3
"""Writes tests/golden/detector_input_ref.npz: what maskrcnn-benchmark's input transform makes of small frames, piece by piece.

    python tools/make_golden_detector_input.py /path/to/maskrcnn_benchmark

Sizes: Resize.get_size of data/transforms/transforms.py and the padded shape of to_image_list of structures/image_list.py, both taken from those files BY PATH AT
RUN TIME -- their ast nodes, executed here -- none of their text is in this repository.  Resized bytes: the installed Pillow, Image.resize((ow, oh), BILINEAR), what
torchvision's Resize does to the PIL image ToPILImage hands it.  Float tail: CPU torch ops as demo/predictor.py:142-157 and transforms.py:86-90 chain them
(torchvision is not needed: to_tensor of a uint8 image is .float().div(255), normalize is .sub_(mean[:, None, None]).div_(std[:, None, None]) on float32 tensors,
torchvision/transforms/functional.py), on all 256 byte values per flag combination and for two mean / std sets.
Before writing, the numpy statement (tests/detector_input_numpy.py) is held against every stored figure: all of them equal."""
import ast
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
OUT = os.path.join(ROOT, "tests", "golden", "detector_input_ref.npz")

# the source images: (width, height, kind)
IMAGES = ((160, 120, "random"), (160, 120, "gradient"), (120, 160, "random"), (64, 48, "random"), (70, 50, "random"), (20, 12, "random"))
# resized through the size rule: (image, min_size, max_size or 0, size_divisible)
RULE_CASES = ((0, 160, 0, 32), (0, 56, 0, 0), (0, 40, 0, 32), (0, 16, 0, 0), (0, 15, 0, 0), (0, 120, 0, 32), (0, 100, 120, 32), (1, 100, 120, 0), (1, 56, 0, 32),
              (2, 56, 0, 32), (2, 90, 0, 32), (3, 56, 0, 32), (3, 48, 0, 0), (4, 64, 0, 32), (5, 32, 0, 0))
# resized to a free size (one axis only, both axes unequally): (image, ow, oh)
FREE_CASES = ((0, 160, 150), (0, 100, 120), (3, 64, 20), (3, 30, 48), (1, 213, 120))
MEAN_STD = (((102.9801, 115.9465, 122.7717), (1.0, 1.0, 1.0)), ((0.485, 0.456, 0.406), (0.229, 0.224, 0.225)))


def load_reference(pkg):
    import random

    import torch

    def nodes_of(path, want, kinds):
        with open(path) as f:
            tree = ast.parse(f.read())
        nodes = [n for n in tree.body if isinstance(n, kinds) and n.name in want]
        assert sorted(n.name for n in nodes) == sorted(want), (path, [n.name for n in nodes])
        return ast.Module(body=nodes, type_ignores=[])

    tpath = os.path.join(pkg, "data", "transforms", "transforms.py")
    ns_t = {"random": random}
    exec(compile(nodes_of(tpath, ("Resize",), (ast.ClassDef,)), tpath, "exec"), ns_t)   # (its __call__ names torchvision: never called)
    ipath = os.path.join(pkg, "structures", "image_list.py")
    ns_i = {"torch": torch}
    exec(compile(nodes_of(ipath, ("ImageList", "to_image_list"), (ast.ClassDef, ast.FunctionDef)), ipath, "exec"), ns_i)

    def get_size(w, h, min_size, max_size):
        oh, ow = ns_t["Resize"](min_size, max_size if max_size > 0 else None).get_size((w, h))
        return int(ow), int(oh)

    def padded(ow, oh, d):
        t = ns_i["to_image_list"](torch.ones(3, oh, ow), d).tensors
        assert t.shape[0] == 1 and t.shape[1] == 3
        assert float(t[0, :, :oh, :ow].min()) == 1.0 and float(t.sum()) == 3.0 * oh * ow    # zero-filled behind the image
        return int(t.shape[3]), int(t.shape[2])

    return get_size, padded


def make_image(rng, w, h, kind):
    if kind == "random":
        return rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    g = np.add.outer(np.arange(h) * 3, np.arange(w) * 2)
    return np.stack([g % 256, (g * 2 + 40) % 256, 255 - g % 256], axis=2).astype(np.uint8)


def size_cases():
    """(w, h, min_size, max_size or 0, size_divisible): about two hundred, among them the rows of the table in include/ifx_c_api.h's neighbourhood, both exact halves
    of the max_size branch (90 * 120 / 160 = 67.5 -> 68, 94 * 120 / 160 = 70.5 -> 70) and frames that keep their size"""
    out = [(640, 480, 512, 0, 32), (640, 480, 800, 0, 32), (160, 120, 100, 120, 0), (160, 120, 100, 90, 32), (160, 120, 100, 94, 0), (120, 160, 100, 90, 32),
           (120, 160, 100, 94, 32), (640, 480, 800, 1333, 32), (1280, 720, 800, 1333, 32), (640, 480, 480, 0, 32), (480, 640, 480, 0, 0), (100, 100, 100, 0, 7)]
    rng = np.random.default_rng(7)
    while len(out) < 200:
        w, h = (int(v) for v in rng.integers(64, 700, 2))
        mn = int(rng.integers(40, 900))
        mx = 0 if rng.random() < 0.4 else int(rng.integers(mn // 2 + 1, 2 * mn + 2))
        out.append((w, h, mn, mx, int(rng.choice((0, 1, 7, 32, 64)))))
    return np.asarray(out, np.int32)


def tail_reference(ramp, mean, std, scale_255, swap_rb):
    import torch

    x = torch.from_numpy(ramp.copy())[:, None, :].float().div(255)      # ToTensor on a [1, 256] image of three channels
    if scale_255 and swap_rb:
        x = x[[2, 1, 0]] * 255                                           # transforms.py:86-90
    elif scale_255:
        x = x * 255                                                      # predictor.py:143
    elif swap_rb:
        x = x[[2, 1, 0]]                                                 # predictor.py:145
    m = torch.as_tensor(mean, dtype=torch.float32)
    s = torch.as_tensor(std, dtype=torch.float32)
    x = x.clone()
    x.sub_(m[:, None, None]).div_(s[:, None, None])                      # Normalize
    return x[:, 0, :].numpy()


def main():
    from PIL import Image

    import detector_input_numpy as dn

    if len(sys.argv) != 2:
        sys.exit(__doc__)
    get_size, padded = load_reference(sys.argv[1])
    rng = np.random.default_rng(20261018)
    images = [make_image(rng, w, h, kind) for (w, h, kind) in IMAGES]
    # sizes
    sc = size_cases()
    sref = []
    for (w, h, mn, mx, d) in sc.tolist():
        ow, oh = get_size(w, h, mn, mx)
        sref.append((ow, oh) + padded(ow, oh, d))
        assert dn.input_size(w, h, mn, mx, d) == sref[-1], ((w, h, mn, mx, d), sref[-1])
    # resized bytes
    cases, resized = [], []
    samples = 0
    for (i, mn, mx, d) in RULE_CASES:
        h, w, _ = images[i].shape
        ow, oh = get_size(w, h, mn, mx)
        cases.append((i, mn, mx, d, ow, oh) + padded(ow, oh, d))
    for (i, ow, oh) in FREE_CASES:
        cases.append((i, 0, 0, 0, ow, oh, ow, oh))
    for c in cases:
        i, ow, oh = c[0], c[4], c[5]
        ref = np.asarray(Image.fromarray(images[i]).resize((ow, oh), Image.BILINEAR))
        assert ref.shape == (oh, ow, 3) and ref.dtype == np.uint8
        assert np.array_equal(dn.resize(images[i], ow, oh), ref), c
        resized.append(ref.reshape(-1))
        samples += ref.size
    # float tail
    ramp = np.stack([np.arange(256), (np.arange(256) + 85) % 256, (np.arange(256) * 7 + 3) % 256]).astype(np.uint8)
    tail = np.zeros((4, len(MEAN_STD), 3, 256), np.float32)
    for flags in range(4):
        for k, (mean, std) in enumerate(MEAN_STD):
            tail[flags, k] = tail_reference(ramp, mean, std, bool(flags & 2), bool(flags & 1))
            mine = dn.float_tail(ramp, mean, std, bool(flags & 2), bool(flags & 1))
            assert np.array_equal(tail[flags, k].view(np.uint32), mine.view(np.uint32)), (flags, k)
    print(f"{len(sc)} sizes, {len(cases)} resized images with {samples} samples, {tail.size} tail values: the statement equals every one")
    np.savez_compressed(OUT, img_shape=np.asarray([im.shape[:2] for im in images], np.int32), img_bytes=np.concatenate([im.reshape(-1) for im in images]),
                        size_cases=sc, size_ref=np.asarray(sref, np.int32), cases=np.asarray(cases, np.int32), resized=np.concatenate(resized), ramp=ramp,
                        mean_std=np.asarray(MEAN_STD, np.float64), tail=tail)
    print(f"{OUT}: {os.path.getsize(OUT)} bytes")
    assert os.path.getsize(OUT) < 1000000


if __name__ == "__main__":
    main()
