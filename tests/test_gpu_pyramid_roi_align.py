"""ifx_pyramid_roi_align on the device (PyramidROIAlign.call of the Keras Mask R-CNN): outputs and levels equal to the numpy statement (tests/keras_layers_numpy.py)
bit for bit, compared as uint32, on maps of 16^2, 8^2, 4^2 and 2^2: both layouts; the scalar path (C = 1, 3; C = 8 behind a pointer that is not 16-byte aligned)
and the 16-byte path (C = 4, 256); pools 7 x 7, 14 x 14, 1 x 1, 3 x 5; boxes with sqrt(area) at the three thresholds and one f32 step to either side; the zero
row, boxes outside, ending at 1.0, reaching beyond it, flipped, NaN; n = 1 and 1000; two images with distinct maps; every row in one level; a NULL levels pointer;
a prefilled out= between guard bands; the refusals."""
import ctypes as C

import numpy as np
import pytest

import keras_layers_gpu as kg
import keras_layers_numpy as kl
from keras_layers_gpu import F, cuda

pytestmark = pytest.mark.gpu

SIZES = (16, 8, 4, 2)
SPECIAL = np.asarray([[0, 0, 0, 0],                    # the zero-padded row: level 2, every bin the top-left texel
                      [1.5, 1.5, 1.8, 1.9],            # wholly outside: zeros
                      [0.5, 0.25, 1.0, 1.0],           # ends exactly at 1.0: in_y == H - 1, floor == ceil
                      [0.5, 0.5, 1.25, 1.125],         # reaches beyond 1.0: a zero band
                      [-0.25, -0.125, 0.5, 0.5],       # starts in front of 0: a zero band at the other end
                      [0.9, 0.1, 0.1, 0.9],            # flipped in y
                      [0.2, 0.8, 0.7, 0.3],            # flipped in x
                      [np.nan, 0, 1, 1], [0, 0, 1, np.nan], [0.1, 0.1, np.inf, 0.5]], F)


@pytest.fixture(scope="module")
def ifx():
    import instancefusion_amd as m

    m.lib()
    return m


@pytest.fixture(scope="module")
def ef(ifx):
    e = ifx.ElasticFusion(**kg.Q, max_surfels=100000)
    yield e
    e.close()


def _maps(seed, B, Cn):
    rng = np.random.default_rng(seed)
    return [rng.standard_normal((B, s, s, Cn)).astype(F) for s in SIZES]


def _boxes(seed, B, n, special=True):
    """random boxes inside the unit square over a wide range of sizes (image 512 x 512: all four levels), the special ones in front"""
    rng = np.random.default_rng(seed)
    side = np.exp(rng.uniform(np.log(0.02), np.log(0.98), (B, n, 2)))
    side[:, : n // 6] = rng.uniform(0.65, 0.98, (B, n // 6, 2))
    p = rng.uniform(0, 1, (B, n, 2)) * (1 - side)
    b = np.concatenate([p, p + side], axis=2).astype(F)
    if special and n >= len(SPECIAL):
        b[:, :len(SPECIAL)] = SPECIAL
    return b


def _run(ef, maps, boxes, image, pool, layout, levels=True, misalign=False):
    """the Python method on guarded buffers: (out in NHWC order on the host, levels or None)"""
    import torch

    B, n = boxes.shape[:2]
    Cn = maps[0].shape[3]
    feats = []
    for m in maps:
        a = m if layout == "nhwc" else np.ascontiguousarray(m.transpose(0, 3, 1, 2))
        if misalign:                                    # the same floats one float behind a 16-byte boundary
            t = torch.empty(a.size + 1, device="cuda")
            t[1:] = cuda(a).reshape(-1)
            feats.append(t[1:].view(a.shape))
            assert feats[-1].data_ptr() % 16 == 4 and feats[-1].is_contiguous()
        else:
            feats.append(cuda(a))
    ph, pw = pool
    shape = (B, n, ph, pw, Cn) if layout == "nhwc" else (B, n, Cn, ph, pw)
    buf = torch.full((2 * kg.GUARD + int(np.prod(shape)),), -7.5, device="cuda")
    out = buf[kg.GUARD:buf.numel() - kg.GUARD].view(shape)
    lbuf = torch.full((2 * kg.GUARD + B * n,), -77, dtype=torch.int32, device="cuda")
    lv = lbuf[kg.GUARD:lbuf.numel() - kg.GUARD].view(B, n)
    r = ef.pyramid_roi_align(feats, cuda(boxes), image, pool, layout=layout, out=out, levels_out=lv if levels else None)
    torch.cuda.synchronize()
    assert r is out
    got = kg.payload(buf, -7.5).reshape(shape)
    if layout == "nchw":
        got = got.transpose(0, 1, 3, 4, 2)
    glv = kg.payload(lbuf, -77).reshape(B, n)
    if not levels:
        assert (glv == -77).all()
    return got, glv if levels else None


def _check(ef, maps, boxes, image, pool, layout, **kw):
    got, glv = _run(ef, maps, boxes, image, pool, layout, **kw)
    ref, rlv = kl.pyramid_roi_align(maps, boxes, image, pool)
    if glv is not None:
        assert np.array_equal(glv, rlv), int((glv != rlv).sum())
    bad = kg.bits(got) != kg.bits(ref)
    assert not bad.any(), (int(bad.sum()), np.argwhere(bad)[:4].tolist())
    return ref, rlv


@pytest.mark.parametrize("layout", ["nhwc", "nchw"])
@pytest.mark.parametrize("Cn", [1, 3, 4, 256])
def test_channels_and_layouts(ef, Cn, layout):
    """C = 1, 3: the scalar path; 4, 256: the 16-byte path (NHWC); 46 boxes over all four levels with the special rows"""
    ref, lv = _check(ef, _maps(Cn, 1, Cn), _boxes(Cn + 1, 1, 46), (512, 512), (7, 7), layout)
    assert set(np.unique(lv)) == {2, 3, 4, 5}
    assert lv[0, 0] == 2 and (ref[0, 0] == _maps(Cn, 1, Cn)[0][0, 0, 0]).all()                # the zero row
    assert (ref[0, 1] == 0).all() and (ref[0, 7] == 0).all() and (ref[0, 3][-1] == 0).all() and (ref[0, 4][0] == 0).all() and (ref[0, 3][0] != 0).any()


@pytest.mark.parametrize("layout", ["nhwc", "nchw"])
@pytest.mark.parametrize("pool", [(14, 14), (1, 1), (3, 5)])
def test_pool_shapes(ef, pool, layout):
    _check(ef, _maps(7, 1, 4), _boxes(8, 1, 40), (512, 512), pool, layout)
    _check(ef, _maps(9, 1, 3), _boxes(10, 1, 40), (512, 512), pool, layout)


def test_divisible_channels_behind_an_unaligned_pointer(ef):
    """C = 8 with every map 4 bytes behind a 16-byte boundary: the scalar path on a divisible C"""
    maps, boxes = _maps(11, 1, 8), _boxes(12, 1, 46)
    _check(ef, maps, boxes, (512, 512), (7, 7), "nhwc", misalign=True)
    _check(ef, maps, boxes, (512, 512), (7, 7), "nhwc")


def _area_with_root(s):
    a = F(np.float64(s) * np.float64(s))
    for cand in (a, np.nextafter(a, F(0)), np.nextafter(a, F(9))):
        if np.sqrt(F(cand)) == s:
            return F(cand)
    raise AssertionError(s)


@pytest.mark.parametrize("image", [(64, 64), (512, 512), (1024, 800)])
def test_levels_at_the_thresholds(ifx, ef, image):
    """sqrt(area) one f32 step below, at and one step above T0, T1, T2: levels 2 2 3, 3 4 4, 4 4 5 (half to even); image 64 x 64: the boxes reach beyond 1.0"""
    T = ifx.pyramid_level_thresholds(*image)
    assert np.array_equal(T.view(np.uint32), kl.level_thresholds(*image).view(np.uint32))
    rows = []
    for t in T:
        for s in (np.nextafter(t, F(0)), t, np.nextafter(t, F(9))):
            rows.append([0, 0, 1, _area_with_root(s)])
    boxes = np.asarray(rows, F)[None]
    ref, lv = _check(ef, _maps(13, 1, 4), boxes, image, (7, 7), "nhwc")
    assert lv[0].tolist() == [2, 2, 3, 3, 4, 4, 4, 4, 5]


@pytest.mark.parametrize("n", [1, 1000])
def test_one_row_and_a_thousand(ef, n):
    _check(ef, _maps(14, 1, 4), _boxes(15 + n, 1, n), (512, 512), (7, 7), "nhwc")
    _check(ef, _maps(14, 1, 4), _boxes(15 + n, 1, n), (512, 512), (7, 7), "nchw")


@pytest.mark.parametrize("layout", ["nhwc", "nchw"])
def test_two_images_with_distinct_maps(ef, layout):
    maps = _maps(16, 2, 4)
    boxes = _boxes(17, 2, 30)
    boxes[1] = boxes[0]                                 # the same boxes: the rows differ because the maps do
    ref, _ = _check(ef, maps, boxes, (512, 512), (7, 7), layout)
    assert not np.array_equal(ref[0, 12], ref[1, 12])


def test_every_row_in_one_level_and_null_levels(ef):
    """image 64 x 64: every box inside the unit square is level 2, the other three maps have no rows; and without a levels pointer"""
    maps, boxes = _maps(18, 1, 4), _boxes(19, 1, 60, special=False)
    _, lv = _check(ef, maps, boxes, (64, 64), (7, 7), "nhwc")
    assert (lv == 2).all()
    _check(ef, maps, boxes, (512, 512), (7, 7), "nhwc", levels=False)
    big = np.tile(np.asarray([[0.05, 0.1, 0.95, 0.9]], F), (1, 20, 1))
    _, lv = _check(ef, maps, big, (512, 512), (14, 14), "nchw")
    assert (lv == 5).all()


def test_python_argument_checks_and_refusals(ifx, ef):
    import torch

    maps = [cuda(m) for m in _maps(20, 1, 4)]
    boxes = cuda(_boxes(21, 1, 12))
    assert tuple(ef.pyramid_roi_align(maps, boxes[0], (512, 512), (7, 7)).shape) == (12, 7, 7, 4)       # [n,4] boxes with one image
    assert tuple(ef.pyramid_roi_align(maps, boxes[:, :0], (512, 512), (7, 7)).shape) == (1, 0, 7, 7, 4)
    with pytest.raises(ValueError):
        ef.pyramid_roi_align(maps[:3], boxes, (512, 512), (7, 7))
    with pytest.raises(ValueError):
        ef.pyramid_roi_align(maps, boxes, (512, 512), (7, 7), layout="hwc")
    with pytest.raises(TypeError):
        ef.pyramid_roi_align(maps, boxes.double(), (512, 512), (7, 7))
    with pytest.raises(ValueError):
        ef.pyramid_roi_align(maps, boxes.expand(2, 12, 4).contiguous(), (512, 512), (7, 7))
    with pytest.raises(ValueError):
        ef.pyramid_roi_align(maps[:3] + [maps[3][..., :2].contiguous()], boxes, (512, 512), (7, 7))
    with pytest.raises(ValueError):
        ef.pyramid_roi_align(maps, boxes, (512, 512), (7, 7), out=torch.empty((1, 12, 7, 7, 3), device="cuda"))
    with pytest.raises(ValueError):
        ef.pyramid_roi_align(maps, boxes, (512, 512), (7, 7), levels_out=torch.empty((1, 11), dtype=torch.int32, device="cuda"))
    with pytest.raises(ValueError):
        ef.pyramid_roi_align(maps, boxes.transpose(1, 2), (512, 512), (7, 7))
    for kw in (dict(image=(0, 512)), dict(image=(512, -1)), dict(pool=(0, 7)), dict(pool=(7, 129))):
        with pytest.raises(ifx.IfxError, match="ifx_pyramid_roi_align"):
            ef.pyramid_roi_align(maps, boxes, kw.get("image", (512, 512)), kw.get("pool", (7, 7)))
    out = torch.full((12 * 49 * 4,), -7.5, device="cuda")
    ptrs = (C.c_void_p * 4)(*[m.data_ptr() for m in maps])
    hs = (C.c_int32 * 4)(*SIZES)
    nul = (C.c_void_p * 4)(maps[0].data_ptr(), None, maps[2].data_ptr(), maps[3].data_ptr())
    bad_h = (C.c_int32 * 4)(16, 8, 0, 2)
    pb, po = C.c_void_p(boxes.data_ptr()), C.c_void_p(out.data_ptr())

    def call(f=ptrs, h=hs, w=hs, B=1, Cn=4, layout=1, b=pb, n=12, o=po):
        return ef.L.ifx_pyramid_roi_align(ef.handle, f, h, w, B, Cn, layout, b, n, 512, 512, 7, 7, o, None, None)

    for kw in (dict(f=None), dict(f=nul), dict(h=None), dict(w=None), dict(h=bad_h), dict(B=0), dict(Cn=0), dict(layout=2), dict(layout=-1), dict(b=None), dict(n=0),
               dict(n=-1), dict(o=None)):
        assert call(**kw) == kg.E_INVALID, kw
        assert ef.L.ifx_last_error(ef.handle).startswith(b"ifx_pyramid_roi_align: "), kw
    torch.cuda.synchronize()
    assert (out == -7.5).all()                          # nothing was enqueued
    assert call() == 0                                  # NULL stream: the handle's main stream
    torch.cuda.synchronize()
    ref, _ = kl.pyramid_roi_align(_maps(20, 1, 4), _boxes(21, 1, 12), (512, 512), (7, 7))
    assert np.array_equal(kg.bits(out.cpu().numpy().reshape(ref.shape)), kg.bits(ref))
