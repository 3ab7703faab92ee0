"""The record of the sharded call's device forms, restated in numpy (tests/owner_seg_record_numpy.py): its layout, and the ingest from the bit form against
mask_bridge_numpy's ingest of the unpacked tensors.  All comparisons are equalities."""
import numpy as np
import pytest

import mask_bridge_numpy as mb
import owner_seg_record_numpy as rec

SHAPES = [(240, 320), (244, 324), (4, 12)]   # P = 76 800; two with P % 32 == 16


def _masks(dtype, n, shape, seed):
    """n masks of `dtype` with two of equal area (stable order), one all empty, and -- float32 -- a NaN and a value equal to the threshold inside the first"""
    rng = np.random.default_rng(seed)
    H, W = shape
    m = np.zeros((n, H, W), np.float32)
    for i in range(n):
        y0, x0 = int(rng.integers(0, H // 2)), int(rng.integers(0, W // 2))
        m[i, y0:y0 + 1 + int(rng.integers(1, H // 2)), x0:x0 + 1 + int(rng.integers(1, W // 2))] = rng.uniform(0.51, 1.0)
    if n >= 3:
        m[1] = 0
        m[1, 0:2, 0:3] = 0.9
        m[2] = 0
        m[2, 1:3, 2:5] = 0.8          # the area of mask 1, overlapping it
    if n >= 4:
        m[3] = 0                      # all empty
    if dtype == np.float32:
        if n:
            m[0, 0, 0] = np.nan
            m[0, 0, 1] = 0.5          # equal to the threshold: outside
        return m
    if dtype == np.bool_:
        return m > 0.5
    return np.where(m > 0.5, rng.integers(1, 256, m.shape), 0).astype(np.uint8)


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("dtype", [np.uint8, np.bool_, np.float32])
@pytest.mark.parametrize("n,max_n", [(0, 4), (1, 1), (1, 8), (3, 8), (5, 5), (8, 8)])
def test_bit_ingest_equals_bridge(shape, dtype, n, max_n):
    masks = _masks(dtype, n, shape, 7 * n + max_n)
    cls = np.arange(10, 10 + n, dtype=np.int32)[::-1].copy()
    r = rec.record_image(masks, cls, max_n, 0.5)
    P = shape[0] * shape[1]
    assert r.dtype == np.int32 and r.shape == (rec.record_words(1, max_n, 0, P),)
    assert rec.parse_header(r) == (1, n, 0, P, max_n)
    got = rec.ingest_bits(r, shape)
    want = mb.bridge_masks(masks, cls, 0.5)
    for g, w, name in zip(got, want, ("ori", "clean", "order", "class ids")):
        assert g.dtype == w.dtype and np.array_equal(g, w), name
    if n >= 3:
        o = list(got[2])
        assert o.index(1) < o.index(2), "equal areas keep their input order"
    if n >= 4:
        assert got[2][-1] == 3 and not got[0][-1].any(), "the empty mask comes last"


def test_bit_order_and_padding():
    m = np.zeros((2, 4, 12), np.uint8)          # P = 48: one whole word and half a word per mask
    m[0].reshape(-1)[[0, 31, 32, 47]] = 1
    m[1].reshape(-1)[[5]] = 200
    b = rec.pack_bits(m)
    assert b.dtype == np.uint32 and b.shape == (2, 2)
    assert b[0, 0] == (1 | 1 << 31) and b[0, 1] == (1 | 1 << 15) and b[1, 0] == 1 << 5 and b[1, 1] == 0
    f = np.full((1, 4, 12), np.nan, np.float32)
    f.reshape(-1)[3] = 0.5
    f.reshape(-1)[4] = np.nextafter(np.float32(0.5), np.float32(1))
    assert rec.pack_bits(f, 0.5).tolist() == [[1 << 4, 0]]


def test_rois_record_layout():
    rng = np.random.default_rng(3)
    rm = rng.random((3, 1, 5, 5), dtype=np.float32)
    bx = rng.random((3, 4), dtype=np.float32) * 100
    r = rec.record_rois(rm, bx, [7, 8, 9], 4, 48)
    assert r.shape == (rec.record_words(2, 4, 5, 48),) and r.size == 8 + 4 + 16 + 100
    assert rec.parse_header(r) == (2, 3, 5, 48, 4)
    assert r[8:12].tolist() == [7, 8, 9, 0]
    assert np.array_equal(r[12:24].view(np.float32).reshape(3, 4), bx) and not r[24:28].any()
    assert np.array_equal(r[28:103].view(np.float32).reshape(3, 5, 5), rm[:, 0]) and not r[103:].any()
