"""The default detector's rule without a GPU: the numpy statements (tests/unmold_numpy.py, tests/molded_input_numpy.py) against the fixture recorded from the
reference's own utils.unmold_mask / utils.resize_image (tools/make_golden_unmold.py) -- every pixel, no tie band: the rule is integer from the resize on --, against
the installed Pillow, against a plain numpy evaluation of model.py:2314-2333 on adversarial rows; the host-only ifx_molded_input_size through ctypes; and the
stand-alone check of its header."""
import ctypes as C
import os
import subprocess
import zlib

import numpy as np
import pytest

import detector_input_numpy as di
import molded_input_numpy as mi
import unmold_numpy as un
from conftest import ROOT

GOLDEN = os.path.join(ROOT, "tests", "golden", "unmold_cases.npz")


@pytest.fixture(scope="module")
def golden():
    return dict(np.load(GOLDEN))


def _pattern_image(w, h):
    """tools/make_golden_unmold.py's pattern_image"""
    y, x = np.mgrid[0:h, 0:w].astype(np.int64)
    return np.stack([(x * 7 + y * 13 + c * 29 + (x * y) % 251 + ((x // 16 + y // 16) % 2) * 90) & 255 for c in range(3)], axis=-1).astype(np.uint8)


def test_unmold_mask_equals_the_reference(golden):
    """all 40 cases of utils.unmold_mask, every pixel: one-pixel boxes, 1 x wide, tall x 1, exactly M, both scale directions, the image's edges, a constant mask,
    a lone maximum"""
    W, H = (int(v) for v in golden["image_size"])
    masks, boxes = golden["masks"], golden["boxes"]
    ref = np.unpackbits(golden["unmolded_bits"], axis=1)[:, :H * W].reshape(-1, H, W)
    assert len(masks) >= 40
    for i, (m, b) in enumerate(zip(masks, boxes)):
        got = un.unmold_mask(m, tuple(int(v) for v in b), W, H)
        assert np.array_equal(got, ref[i]), (i, b.tolist(), int((got != ref[i]).sum()))
    assert ref[20].sum() == 0 and ref[21].sum() == 0          # cs == 0: bytes of 0, nothing inside
    assert 0 < ref[22].sum() < 70 * 90                        # the lone maximum is stretched to 255 and spreads
    assert ref[25].sum() > 0                                  # samples all below 0.5: the stretch, not the probability, decides


def test_resampler_equals_pillow():
    """the statement's resize against executed Pillow for M in {1, 2, 27, 28, 64} and every width 1 .. 160 (heights cycle over 1 .. 120)"""
    Image = pytest.importorskip("PIL.Image")
    rng = np.random.default_rng(5)
    for M in (1, 2, 27, 28, 64):
        b = rng.integers(0, 256, (M, M), dtype=np.uint8)
        for w in range(1, 161):
            h = (w * 7) % 120 + 1
            ref = np.array(Image.frombytes("L", (M, M), b.tobytes()).resize((w, h), 2))
            assert np.array_equal(un.resize_bytes(b, w, h), ref), (M, w, h)


def _numpy_boxes(det, window, W, H):
    """model.py:2304-2333 as numpy evaluates it: (boxes int32 [k, 4], the surviving rows)"""
    z = np.where(det[:, 4] == 0)[0]
    N = z[0] if z.shape[0] > 0 else det.shape[0]
    scale = min(H / (window[2] - window[0]), W / (window[3] - window[1]))
    shifts = np.array([window[0], window[1], window[0], window[1]])
    boxes = np.multiply(det[:N, :4] - shifts, np.array([scale] * 4)).astype(np.int32)
    ex = np.where((boxes[:, 2] - boxes[:, 0]) * (boxes[:, 3] - boxes[:, 1]) <= 0)[0]
    return np.delete(boxes, ex, axis=0), np.delete(np.arange(N), ex)


def adversarial_rows():
    """rows for steps 1 to 3 at 160 x 120 behind the window (16, 0, 112, 128), scale 1.25: a zero class in the middle, zero and negative extents, both extents
    negative, coordinates that truncate toward zero from both sides"""
    d = [
        (16.0, 0.0, 112.0, 128.0, 3, 0.9),          # the whole image
        (20.0, 8.0, 20.0, 60.0, 1, 0.8),            # zero height: excluded
        (20.0, 8.0, 60.0, 8.0, 1, 0.8),             # zero width: excluded
        (60.0, 8.0, 20.0, 60.0, 2, 0.8),            # negative height: excluded
        (60.0, 60.0, 20.0, 8.0, 2, 0.7),            # both negative: survives step 3, no paste
        (16.7, 0.7, 17.5, 1.5, 4, 0.6),             # 0.875 -> 0 and 1.875 -> 1
        (15.3, -0.7, 17.0, 1.0, 4, 0.6),            # -0.875 -> 0 from below: truncation, not floor
        (15.0, -1.0, 40.0, 40.0, 5, 0.5),           # -1.25 -> -1: survives, outside the image
        (16.0, 0.0, 113.0, 129.0, 5, 0.5),          # one pixel beyond the far edges
        (30.5, 40.6, 30.9, 41.3, 6, 0.4),           # h = 0 after truncation
        (0.0, 0.0, 0.0, 0.0, 0, 0.0),               # the first zero class: N = 10
        (16.0, 0.0, 112.0, 128.0, 3, 0.9),
    ]
    return np.array(d, np.float32)


def test_steps_1_to_3_equal_numpy():
    det = adversarial_rows()
    window, W, H = (16, 0, 112, 128), 160, 120
    masks = np.random.default_rng(3).random((len(det), 4, 4, 8)).astype(np.float32)
    _, cls, boxes, scores, rows, kept = un.unmold_detections(det, masks, window, W, H)
    ref_boxes, ref_rows = _numpy_boxes(det, window, W, H)
    assert kept == len(ref_rows) == 6
    assert np.array_equal(boxes[:kept], ref_boxes) and np.array_equal(rows[:kept], ref_rows)
    assert rows[:kept].tolist() == [0, 4, 5, 6, 7, 8]
    assert boxes[2].tolist() == [0, 0, 1, 1] and boxes[3].tolist() == [0, 0, 1, 1] and boxes[4].tolist() == [-1, -1, 30, 50]
    assert np.array_equal(cls[:kept], det[ref_rows, 4].astype(np.int32)) and np.array_equal(scores[:kept], det[ref_rows, 5])
    assert (boxes[kept:] == 0).all() and (cls[kept:] == -1).all() and (rows[kept:] == -1).all()
    det2 = det.copy(); det2[10, 4] = 2.0                       # no zero class: N = R; row 10's own box is empty, row 11 joins
    assert un.unmold_detections(det2, masks, window, W, H)[5] == 7
    det2[3, 4] = -0.0
    assert un.count_rows(det2) == 3


def test_molded_input_equals_the_reference(golden):
    """utils.resize_image's windows and bytes: the issue's two 640 x 480 cases and four small ones, by CRC-32 of the padded image and a 64 x 64 crop"""
    cases, ref, crops = golden["input_cases"].tolist(), golden["input_ref"].tolist(), golden["input_crops"]
    assert (640, 480, 512, 512) in [tuple(c) for c in cases] and (640, 480, 800, 1024) in [tuple(c) for c in cases]
    for (w, h, mn, mx), r, crop in zip(cases, ref, crops):
        out, window = mi.molded_input(_pattern_image(w, h), mn, mx, mean=(0.0, 0.0, 0.0))
        assert window == tuple(r[:4]), (w, h, mn, mx)
        b = out.astype(np.uint8)
        assert np.array_equal(b.astype(np.float32), out)
        assert zlib.crc32(np.ascontiguousarray(b).tobytes()) == r[4], (w, h, mn, mx)
        cy, cx = max(window[0] - 8, 0), max(window[1] - 8, 0)
        part = b[cy:cy + 64, cx:cx + 64]
        assert np.array_equal(part, crop[:part.shape[0], :part.shape[1]])
    assert tuple(ref[0][:4]) == (64, 0, 448, 512) and tuple(ref[1][:4]) == (128, 0, 896, 1024)
    out, _ = mi.molded_input(_pattern_image(160, 120), 128, 128)
    assert out.dtype == np.float32 and out[0, 0].tolist() == [np.float32(-123.7), np.float32(-116.8), np.float32(-103.9)]


def test_molded_input_size_through_ctypes(golden):
    """the host-only ifx_molded_input_size (no GPU) against the fixture's windows, and against the statement on a grid of sizes and dims, refusals included"""
    import instancefusion_amd as ifx

    L = ifx.lib()
    o = np.zeros(8, np.int32)
    n_ref = 0
    for (w, h, mn, mx), r in zip(golden["size_cases"].tolist(), golden["size_ref"].tolist()):
        want = mi.molded_size(w, h, mn, mx)
        rc = L.ifx_molded_input_size(w, h, mn, mx, o.ctypes.data)
        if want is None:                                      # (a resize scale above 8: the library's own cap)
            assert rc == -1 and max(h, w) / mx > 8, (w, h, mn, mx)
            continue
        assert rc == 0 and tuple(o) == want, (w, h, mn, mx, o.tolist(), want)
        assert [o[2], o[3]] == r[:2] and o[4:].tolist() == r[2:], (w, h, mn, mx)
        n_ref += 1
    assert n_ref >= 60
    for w in (1, 2, 3, 63, 64, 100, 159, 160, 161, 640):
        for h in (1, 5, 76, 119, 120, 121, 480):
            for mn, mx in ((0, 160), (128, 128), (200, 256), (800, 1024), (64, 65), (1, 1), (7, 1000), (90, 94)):
                want = mi.molded_size(w, h, mn, mx)
                rc = L.ifx_molded_input_size(w, h, mn, mx, o.ctypes.data)
                assert (rc == -1) if want is None else (rc == 0 and tuple(o) == want), (w, h, mn, mx, rc, o.tolist(), want)
    assert ifx.molded_input_size(640, 480, 800, 1024) == (1024, 768, 1024, 1024, 128, 0, 896, 1024)
    assert ifx.molded_input_size(160, 120, 90, 94) == (94, 70, 94, 94, 12, 0, 82, 94)                      # 70.5 -> 70: half to even
    for bad in ((0, 120, 128, 128), (160, 0, 128, 128), (160, 120, 128, 0), (160, 120, 0, 19), (1000, 100, 0, 100)):
        assert L.ifx_molded_input_size(*bad, o.ctypes.data) == -1, bad
    assert L.ifx_molded_input_size(160, 120, 128, 128, None) == -1
    with pytest.raises(ifx.IfxError):
        ifx.molded_input_size(160, 120, 0, 19)


def test_stand_alone_check_under_sanitizers(tmp_path):
    """tests/cpp/molded_prep_check.cpp over ifx_detector_prep.hpp with g++ -fsanitize=address,undefined: the size rule at its corners and the tap tables of
    28 -> 1 .. 160 in exactly-sized buffers (a program of its own: nothing sanitised is loaded into Python); its tap sums equal the statement's"""
    exe = str(tmp_path / "molded_prep_check")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "include"),
                    "-I", os.path.join(ROOT, "instancefusion_amd", "host"), os.path.join(ROOT, "tests", "cpp", "molded_prep_check.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    lines = r.stdout.splitlines()
    assert lines[-1] == "ok", r.stdout[-2000:]
    sums = {tuple(int(v) for v in ln.split()[1:3]): [int(v) for v in ln.split()[3:]] for ln in lines if ln.startswith("taps ")}
    assert len(sums) == 5 * 160
    for (a, b), v in sums.items():
        first, count, coeff = di.resize_taps(a, b)
        assert int(count.max()) <= a                              # what the paste kernel's LDS rows rely on: never more than M taps
        assert v == [int(count.max()), int((first * 3 + count).sum()), int((coeff * np.arange(1, coeff.shape[1] + 1)).sum() % 1000003)], (a, b)
