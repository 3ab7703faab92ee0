"""The detector-input rule in numpy (include/ifx_c_api.h, instancefusion_amd/host/ifx_detector_prep.hpp, k_detector_input): the size rule of maskrcnn-benchmark's
Resize, Pillow's 8-bit bilinear resampling, the float tail of ToTensor / x255 / flip / Normalize and to_image_list's zero padding.  No torch, no Pillow: what the
tests compare the library, the golden file and the installed Pillow with."""
import math

import numpy as np

PRECISION_BITS = 22
MAX_SCALE = 8
DEFAULT_MEAN = (102.9801, 115.9465, 122.7717)


def get_size(w, h, min_size, max_size=None):
    """(ow, oh): Resize.get_size (maskrcnn_benchmark/data/transforms/transforms.py:35-55) in Python's own arithmetic; max_size None or <= 0: none"""
    size = int(min_size)
    if max_size is not None and max_size > 0:
        mn, mx = float(min(w, h)), float(max(w, h))
        if mx / mn * size > max_size:
            size = int(round(max_size * mn / mx))      # Python 3: half to even
    if (w <= h and w == size) or (h <= w and h == size):
        return w, h
    if w < h:
        return size, int(size * h / w)
    return int(size * w / h), size


def input_size(w, h, min_size, max_size=None, size_divisible=0):
    """(ow, oh, W', H'): the resized size and the size padded as to_image_list pads (structures/image_list.py:54-61)"""
    ow, oh = get_size(w, h, min_size, max_size)
    d = int(size_divisible)
    if d > 0:
        return ow, oh, int(math.ceil(ow / d) * d), int(math.ceil(oh / d) * d)
    return ow, oh, ow, oh


def resize_taps(in_size, out_size):
    """Pillow's taps of one axis: first [out], count [out], coeff [out, ksize] (int64; zero behind count)"""
    scale = in_size / out_size
    fs = max(scale, 1.0)
    support = fs
    ksize = int(math.ceil(support)) * 2 + 1
    ss = 1.0 / fs
    first, count = np.zeros(out_size, np.int64), np.zeros(out_size, np.int64)
    coeff = np.zeros((out_size, ksize), np.int64)
    for xx in range(out_size):
        center = (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        n = min(int(center + support + 0.5), in_size) - xmin
        w = []
        for x in range(n):
            a = abs((x + xmin - center + 0.5) * ss)
            w.append(1.0 - a if a < 1.0 else 0.0)
        ww = 0.0
        for v in w:
            ww += v
        for x in range(n):
            v = (w[x] / ww if ww != 0.0 else w[x]) * (1 << PRECISION_BITS)
            coeff[xx, x] = int(-0.5 + v) if v < 0 else int(0.5 + v)
        first[xx], count[xx] = xmin, n
    return first, count, coeff


def resample_axis1(img, out_size):
    """one pass along axis 1 of a uint8 [A, in, C] image: clip8(((1 << 21) + sum v * k) >> 22)"""
    first, count, coeff = resize_taps(img.shape[1], out_size)
    src = img.astype(np.int64)
    out = np.zeros((img.shape[0], out_size, img.shape[2]), np.uint8)
    for xx in range(out_size):
        f, n = int(first[xx]), int(count[xx])
        acc = (1 << (PRECISION_BITS - 1)) + np.tensordot(src[:, f:f + n, :], coeff[xx, :n], axes=([1], [0]))
        out[:, xx, :] = np.clip(acc >> PRECISION_BITS, 0, 255)
    return out


def resize(img, ow, oh, force_passes=False):
    """Pillow's Image.resize((ow, oh), BILINEAR) of a uint8 [h, w, 3] image: horizontal pass, then vertical, each skipped when its axis keeps its size
    (force_passes: executed all the same -- the identity taps give the same bytes)"""
    h, w, _ = img.shape
    t = img
    if ow != w or force_passes:
        t = resample_axis1(t, ow)
    if oh != h or force_passes:
        t = resample_axis1(t.transpose(1, 0, 2), oh).transpose(1, 0, 2)
    return np.ascontiguousarray(t)


def float_tail(planar_u8, mean, std, scale_255, swap_rb):
    """uint8 [3, ...] (source channel order) -> float32 [3, ...]: f32(byte) / 255, x 255 if scale_255, output channel c from source channel 2 - c if swap_rb,
    (t - mean[c]) / std[c]; every operation rounded to f32"""
    t = planar_u8.astype(np.float32) / np.float32(255.0)
    if scale_255:
        t = t * np.float32(255.0)
    if swap_rb:
        t = t[::-1]
    shape = (3,) + (1,) * (t.ndim - 1)
    m = np.asarray(mean, np.float32).reshape(shape)
    s = np.asarray(std, np.float32).reshape(shape)
    out = (t - m) / s
    assert out.dtype == np.float32
    return out


def detector_input(img, min_size=800, max_size=None, size_divisible=0, mean=DEFAULT_MEAN, std=(1.0, 1.0, 1.0), to_bgr255=True, swap_rb=False):
    """the whole rule on a uint8 [h, w, 3] image: (float32 [1, 3, H', W'], (oh, ow))"""
    h, w, _ = img.shape
    ow, oh, Wp, Hp = input_size(w, h, min_size, max_size, size_divisible)
    small = resize(img, ow, oh)
    out = np.zeros((1, 3, Hp, Wp), np.float32)
    out[0, :, :oh, :ow] = float_tail(small.transpose(2, 0, 1), mean, std, to_bgr255, swap_rb)
    return out, (oh, ow)
