"""The detector-input rule without a GPU: the numpy statement (tests/detector_input_numpy.py) against the golden file made from maskrcnn-benchmark's own size
functions, the installed Pillow and CPU torch (tools/make_golden_detector_input.py) -- every size, every resized byte, every tail value bit-equal; against a live
Pillow where there is one; and the library's two host-only entries and the stand-alone check of their header against the statement."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import detector_input_numpy as dn
from conftest import ROOT

GOLDEN = os.path.join(ROOT, "tests", "golden", "detector_input_ref.npz")


@pytest.fixture(scope="module")
def golden():
    g = dict(np.load(GOLDEN))
    images, at = [], 0
    for (h, w) in g["img_shape"].tolist():
        images.append(g["img_bytes"][at:at + h * w * 3].reshape(h, w, 3))
        at += h * w * 3
    assert at == g["img_bytes"].size
    g["images"] = images
    return g


def test_sizes_equal_the_golden(golden):
    """all 200 (w, h, min_size, max_size, size_divisible): the resized and the padded size, among them both exact halves of the max_size branch"""
    sc, ref = golden["size_cases"].tolist(), golden["size_ref"].tolist()
    assert len(sc) >= 200
    assert [dn.input_size(*c) for c in sc] == [tuple(r) for r in ref]
    assert dn.input_size(640, 480, 512, None, 32) == (682, 512, 704, 512)
    assert dn.input_size(640, 480, 800, None, 32) == (1066, 800, 1088, 800)
    assert dn.get_size(160, 120, 100, 120) == (120, 90)
    assert dn.get_size(160, 120, 100, 90) == (90, 68) and dn.get_size(160, 120, 100, 94) == (93, 70)      # 67.5 -> 68, 70.5 -> 70: half to even


def test_resized_bytes_equal_the_golden(golden):
    """every byte of the 20 resized images (upscale, scale 3, 7.5 and exactly 8, identity, portrait, max_size, one axis only): 100 % of the samples"""
    at = samples = 0
    for c in golden["cases"].tolist():
        i, mn, mx, d, ow, oh, Wp, Hp = c
        img = golden["images"][i]
        if mn:
            assert dn.input_size(img.shape[1], img.shape[0], mn, mx, d) == (ow, oh, Wp, Hp), c
        ref = golden["resized"][at:at + ow * oh * 3].reshape(oh, ow, 3)
        at += ref.size
        got = dn.resize(img, ow, oh)
        assert got.dtype == np.uint8 and np.array_equal(got, ref), (c, int((got != ref).sum()))
        samples += ref.size
    assert at == golden["resized"].size and samples > 500000


def test_a_skipped_pass_equals_an_executed_identity_pass(golden):
    """taps of an axis that keeps its size are (2^22, 0): executing the pass gives the bytes that skipping it gives"""
    img = golden["images"][0]
    h, w, _ = img.shape
    first, count, coeff = dn.resize_taps(w, w)
    assert np.array_equal(first, np.arange(w)) and np.array_equal(coeff[:, 0], np.full(w, 1 << 22)) and not coeff[:, 1:].any()
    for (ow, oh) in ((w, h), (w, 90), (100, h)):
        assert np.array_equal(dn.resize(img, ow, oh), dn.resize(img, ow, oh, force_passes=True))


def test_tail_equals_the_golden(golden):
    """all 256 bytes x 3 channels x 4 flag combinations x 2 mean / std sets, bit for bit against CPU torch's ToTensor / x255 / flip / Normalize chain"""
    ramp, tail, ms = golden["ramp"], golden["tail"], golden["mean_std"]
    for flags in range(4):
        for k in range(ms.shape[0]):
            got = dn.float_tail(ramp, ms[k, 0], ms[k, 1], bool(flags & 2), bool(flags & 1))
            assert got.dtype == np.float32 and np.array_equal(got.view(np.uint32), tail[flags, k].view(np.uint32)), (flags, k)
    # multiplying by the reciprocal is NOT the rule: it differs for many of the bytes
    b = np.arange(256, dtype=np.float32)
    assert int((b / np.float32(255) != b * (np.float32(1) / np.float32(255))).sum()) > 100


def test_whole_rule_pads_with_zeros(golden):
    img = golden["images"][4]                                     # 70 x 50 -> 89 x 64 inside 96 x 64
    out, (oh, ow) = dn.detector_input(img, min_size=64, size_divisible=32, swap_rb=True)
    assert out.shape == (1, 3, 64, 96) and (oh, ow) == (64, 89)
    assert not out[0, :, :, ow:].any() and out[0, :, :, :ow].all()
    small = dn.resize(img, ow, oh)
    assert out[0, 0, 5, 7] == np.float32(np.float32(small[5, 7, 2]) / np.float32(255) * np.float32(255)) - np.float32(102.9801)


def test_live_pillow_sweep():
    """the statement against the installed Pillow, among others 640x480 -> 682x512 and -> 1066x800: every byte"""
    pytest.importorskip("PIL")
    from PIL import Image

    rng = np.random.default_rng(11)
    total = 0
    for (w, h, ow, oh) in ((640, 480, 682, 512), (640, 480, 1066, 800), (160, 120, 213, 160), (160, 120, 53, 40), (160, 120, 20, 15), (120, 160, 56, 74),
                           (160, 120, 160, 90), (160, 120, 100, 120), (160, 120, 160, 120), (64, 48, 9, 7), (33, 17, 70, 50)):
        for kind in range(2):
            if kind == 0:
                img = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
            else:
                g = np.add.outer(np.arange(h) * 3, np.arange(w) * 2)
                img = np.stack([g % 256, (g * 2 + 40) % 256, 255 - g % 256], axis=2).astype(np.uint8)
            ref = np.asarray(Image.fromarray(img).resize((ow, oh), Image.BILINEAR))
            got = dn.resize(img, ow, oh)
            assert np.array_equal(got, ref), (w, h, ow, oh, kind, int((got != ref).sum()))
            total += ref.size
    assert total > 7000000


def _lib():
    import instancefusion_amd as ifx

    return ifx, ifx.lib()      # (loads without a GPU, as test_abi has it)


def test_library_sizes_equal_the_statement(golden):
    """ifx_detector_input_size through ctypes: the golden's 200 combinations, the worked values, and what it refuses"""
    ifx, L = _lib()
    for c, ref in zip(golden["size_cases"].tolist(), golden["size_ref"].tolist()):
        w, h, mn, mx, d = c
        assert ifx.detector_input_size(w, h, mn, mx, d) == tuple(ref) == dn.input_size(w, h, mn, mx, d), c
    assert ifx.detector_input_size(640, 480, 512, None, 32) == (682, 512, 704, 512)
    assert ifx.detector_input_size(160, 120, 100, 90, 0) == (90, 68, 90, 68)
    assert ifx.detector_input_size(160, 120, 100, 94, 0) == (93, 70, 93, 70)
    assert ifx.detector_input_size(120, 160, 100, 94, 32) == (70, 93, 96, 96)
    out = np.zeros(4, np.int32)
    for kw in (dict(min_size=0), dict(size_divisible=-1), dict(std=(1.0, 0.0, 1.0))):
        p = ifx.detector_prep(**{"min_size": 100, **kw})
        assert L.ifx_detector_input_size(64, 48, C.byref(p), out.ctypes.data) == -1, kw
    p = ifx.detector_prep(min_size=100)
    p.flags = 4
    assert L.ifx_detector_input_size(64, 48, C.byref(p), out.ctypes.data) == -1
    p.flags = 3
    assert L.ifx_detector_input_size(64, 48, None, out.ctypes.data) == -1 and L.ifx_detector_input_size(64, 48, C.byref(p), None) == -1
    assert L.ifx_detector_input_size(0, 48, C.byref(p), out.ctypes.data) == -1
    assert L.ifx_detector_input_size(64, 48, C.byref(p), out.ctypes.data) == 0 and tuple(out) == (133, 100, 133, 100)


def test_library_taps_equal_the_statement(golden):
    """ifx_detector_resize_taps through ctypes: every axis pair of the golden and the two of the worked values"""
    ifx, L = _lib()
    pairs = {(640, 682), (480, 512), (640, 1066), (480, 800), (1, 1), (1, 16), (160, 20), (17, 1)}
    for c in golden["cases"].tolist():
        h, w, _ = golden["images"][c[0]].shape
        pairs.add((w, c[4])); pairs.add((h, c[5]))
    for (a, b) in sorted(pairs):
        first, count, coeff = dn.resize_taps(a, b)
        f2, c2, k2 = ifx.detector_resize_taps(a, b)
        assert k2.shape == coeff.shape, (a, b)
        assert np.array_equal(first, f2) and np.array_equal(count, c2) and np.array_equal(coeff, k2), (a, b)
    z = np.zeros(64, np.int32)
    assert L.ifx_detector_resize_taps(160, 20, z.ctypes.data, z.ctypes.data, z.ctypes.data, 16) == -1      # 17 taps do not fit 16
    assert L.ifx_detector_resize_taps(0, 20, z.ctypes.data, z.ctypes.data, z.ctypes.data, 17) == -1
    assert L.ifx_detector_resize_taps(8, 8, None, z.ctypes.data, z.ctypes.data, 17) == -1
    assert not z.any()


def test_stand_alone_check_under_sanitizers(tmp_path):
    """tests/cpp/detector_prep_check.cpp over ifx_detector_prep.hpp with g++ -fsanitize=address,undefined: tap tables at in = 1, out = 1, scale 8 and scale 1/16
    in exactly-sized buffers (a program of its own: nothing sanitised is loaded into Python)"""
    exe = str(tmp_path / "detector_prep_check")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "include"),
                    "-I", os.path.join(ROOT, "instancefusion_amd", "host"), os.path.join(ROOT, "tests", "cpp", "detector_prep_check.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    lines = r.stdout.splitlines()
    assert lines[-1] == "ok", r.stdout[-2000:]
    taps = {tuple(int(v) for v in ln.split()[1:3]): [int(v) for v in ln.split()[3:]] for ln in lines if ln.startswith("taps ")}
    assert taps[(1, 1)] == [3, 1, 0, 1] and taps[(1, 16)] == [3, 1, 0, 1]
    assert taps[(160, 20)][0] == 17 and taps[(161, 20)][0] == 19 and taps[(10, 160)] == [3, 2, 0, 10] and taps[(640, 1)][:2] == [1281, 640]
    for (a, b), v in taps.items():
        first, count, coeff = dn.resize_taps(a, b)
        assert v == [coeff.shape[1], int(count.max()), int(first.min()), int((first + count).max())], (a, b)
