"""Multi-level ROI pooling on the device (ifx_fpn_roi_align, one launch): equal to the numpy statement (tests/fpn_pooler_numpy.py, itself held against
maskrcnn-benchmark's Pooler and LevelMapper in test_fpn_pooler_cpu.py) -- every pooled output in its bits, every level index exactly -- on the golden cases, on a
four-level pyramid, at the level edges and at the edge sizes; rows of no level; the streams; every refusal, which leaves the handle usable; ifx.pooler against the
reference's per-level loop over roi_align_forward; and a map that does not notice."""
import ctypes as C
import os

import numpy as np
import pytest

import fpn_pooler_numpy as fp
from conftest import ROOT

pytestmark = pytest.mark.gpu

E_INVALID = -1
F = np.float32
Q = dict(w=160, h=120, fx=132.0, fy=132.0, cx=80.0, cy=60.0)
GOLDEN = os.path.join(ROOT, "tests", "golden", "fpn_pooler_ref.npz")
SCALES4 = [0.25, 0.125, 0.0625, 0.03125]
SIZES4 = [(24, 32), (12, 16), (6, 8), (3, 4)]            # the pyramid of a 96 x 128 image


@pytest.fixture(scope="module")
def ifx():
    import instancefusion_amd as m

    m.lib()
    return m


@pytest.fixture(scope="module")
def ef(ifx):
    """a handle that never sees a frame: the call needs none"""
    e = ifx.ElasticFusion(**Q, max_surfels=100000)
    yield e
    e.close()


@pytest.fixture(scope="module")
def golden():
    return dict(np.load(GOLDEN))


@pytest.fixture(scope="module")
def pyramid():
    """four separate maps, B = 2, C = 65 (one full run of 64 channels and one channel more), and 40 ROIs over every level"""
    rng = np.random.default_rng(31)
    feats = [rng.standard_normal((2, 65, h, w)).astype(F) for h, w in SIZES4]
    return feats, _rois(rng, 40, 2, 128, 96)


def _cuda(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _bits_equal(got, ref):
    return got.shape == ref.shape and got.dtype == ref.dtype == F and np.array_equal(got.view(np.uint32), ref.view(np.uint32))


def _rois(rng, n, B, iw, ih, lo=3.0, hi=10.5):
    """n ROIs around an iw x ih image with sides of 2^lo .. 2^hi pixels (every level of the released ladder and beyond both ends), some leaving the image"""
    side = 2.0 ** (lo + (hi - lo) * rng.permutation((np.arange(n) + rng.uniform(0, 1, n)) / n))      # one in every n-th of the range
    w, h = side * rng.uniform(0.7, 1.4, n), side / rng.uniform(0.7, 1.4, n)
    cx, cy = rng.uniform(-0.1 * iw, 1.1 * iw, n), rng.uniform(-0.1 * ih, 1.1 * ih, n)
    return np.stack([rng.integers(0, B, n).astype(np.float64), cx - w / 2, cy - h / 2, cx + w / 2, cy + h / 2], axis=1).astype(F)


def _step(x, k):
    """the f32 k steps above (below) x > 0"""
    return (np.asarray(x, F).view(np.uint32).astype(np.int64) + k).astype(np.uint32).view(F)


def _area_with_root(s):
    """an f32 a with sqrt(a) == s, per entry"""
    a = (s.astype(np.float64) ** 2).astype(F)
    for k in (-1, 1, -2, 2):
        c = _step(a, k)
        a = np.where((np.sqrt(a) != s) & (np.sqrt(c) == s), c, a)
    assert (np.sqrt(a) == s).all()
    return a


def _boxes_of_area(a):
    """ROIs of image 0 with (x1 - x0 + 1) * (y1 - y0 + 1) == a in f32, 1 <= a < 2^24: x0 = 1, x1 = a and one row (a - 1 and (a - 1) + 1 are exact there)"""
    assert ((a >= 1) & (a < 2 ** 24)).all()
    z = np.zeros_like(a)
    return np.stack([z, z + F(1), z, a, z], axis=1).astype(F)


def _run(ef, feats, rois, scales, ph, pw, ratio, **kw):
    """the call with levels_out: (out, levels) as numpy"""
    import torch

    rois = np.ascontiguousarray(rois, F).reshape(-1, 5)
    lev = torch.full((rois.shape[0],), -9, dtype=torch.int32, device="cuda")
    out = ef.fpn_roi_align([_cuda(f) for f in feats], _cuda(rois), scales, ph, pw, ratio, levels_out=lev, **kw)
    return out.cpu().numpy(), lev.cpu().numpy()


def _check(ef, feats, rois, scales, ph, pw, ratio, **kw):
    got, lev = _run(ef, feats, rois, scales, ph, pw, ratio, **kw)
    ref, ref_lev = fp.fpn_roi_align(feats, rois, scales, ph, pw, ratio, **kw)
    assert np.array_equal(lev, ref_lev), (lev, ref_lev)
    assert _bits_equal(got, ref), (got.shape, int((got.view(np.uint32) != ref.view(np.uint32)).sum()))
    return got, lev


def test_golden_cases(ef, golden):
    cases = int(golden["counts"][0])
    assert cases == 26
    for k in range(cases):
        scales = [float(s) for s in golden[f"pool{k}_scales"]]
        feats = [golden[f"pool{k}_feat{l}"] for l in range(len(scales))]
        res, ratio = (int(v) for v in golden[f"pool{k}_par"])
        got, lev = _run(ef, feats, golden[f"pool{k}_rois"], scales, res, res, ratio)
        assert np.array_equal(lev, golden[f"pool{k}_levels"]), k
        assert _bits_equal(got, golden[f"pool{k}_out"]), k


@pytest.mark.parametrize("res,ratio", [(7, 2), (14, 2), (7, 0)])
def test_four_level_pyramid(ef, pyramid, res, ratio):
    """ratio 0: the adaptive grid, so the work of an ROI differs with its level"""
    feats, rois = pyramid
    got, lev = _check(ef, feats, rois, SCALES4, res, res, ratio)
    assert got.shape == (40, 65, res, res) and set(lev.tolist()) == {0, 1, 2, 3} and np.isfinite(got).all()


def test_non_square_output_and_other_mapper_constants(ef, pyramid):
    feats, rois = pyramid
    _check(ef, feats, rois[:12], SCALES4, 2, 3, 1)
    _, lev = _check(ef, feats, rois[:12], SCALES4, 3, 2, 2, canonical_scale=56, canonical_level=3, eps=0.0)
    assert not np.array_equal(lev, fp.levels(rois[:12], 2, 5))


def test_level_edges(ifx, ef, golden):
    """the golden edge boxes: sqrt(area) at 56 .. 896 and one step either side, v within a few steps of each edge -- the levels are the reference's own"""
    rng = np.random.default_rng(32)
    feats = [rng.standard_normal((1, 2, h, w)).astype(F) for h, w in SIZES4]
    rois, ref_lev = golden["edge_rois"], golden["edge_levels"]
    with np.errstate(invalid="ignore"):
        finite = np.isfinite(rois).all(axis=1)
    assert (~finite).sum() == 4 and finite[:-7].all()
    got, lev = _check(ef, feats, rois[finite], SCALES4, 2, 2, 2)
    assert np.array_equal(lev, ref_lev[finite])
    # with the four non-finite boxes: two of a NaN area (no level), two of an infinite area (the last level; what is pooled there is not part of the statement)
    got, lev = _run(ef, feats, rois, SCALES4, 2, 2, 2)
    assert np.array_equal(lev, ref_lev)
    assert lev[~finite].tolist() == [3, 3, -1, -1] and not got[lev < 0].any()
    # the thresholds themselves and one step either side: canonical_scale 16 and eps 0 make v = sqrt(area) / 16, an exact division, for areas a box can carry
    k_min, T = ifx.fpn_level_thresholds(SCALES4)
    assert k_min == 2 and T.size == 3
    v = np.concatenate([_step(T, d) for d in (-1, 0, 1)])
    boxes = _boxes_of_area(_area_with_root(v * F(16)))
    assert np.array_equal(fp.v_of_rois(boxes, 16, 0.0).view(np.uint32), v.view(np.uint32))
    _, lev = _check(ef, feats, boxes, SCALES4, 1, 1, 1, canonical_scale=16, eps=0.0)
    assert lev.tolist() == [0, 1, 2, 1, 2, 3, 1, 2, 3]      # one step below T_j: level j - 1; at T_j and above: level j


def test_all_rois_in_one_level_and_a_level_without_rois(ef, pyramid):
    feats, _ = pyramid
    rng = np.random.default_rng(33)
    small = _rois(rng, 9, 2, 128, 96, lo=2.0, hi=6.0)                                 # all below 112: level 0
    _, lev = _check(ef, feats, small, SCALES4, 7, 7, 2)
    assert not lev.any()
    big = _rois(rng, 9, 2, 128, 96, lo=10.2, hi=11.0)                                  # all above 896: level 3
    _, lev = _check(ef, feats, big, SCALES4, 7, 7, 2)
    assert (lev == 3).all()
    both = np.concatenate([small[:4], big[:4], _rois(rng, 4, 2, 128, 96, lo=8.1, hi=8.6)])   # levels 0, 3 and 2: none in level 1
    _, lev = _check(ef, feats, both, SCALES4, 7, 7, 2)
    assert set(lev.tolist()) == {0, 2, 3}


def test_rows_of_no_level_read_nothing(ef, pyramid):
    """NaN-area and non-finite ROIs and a batch index out of range give rows of zeros; maps full of NaNs show that nothing was read for them"""
    _, base = pyramid
    poisoned = [np.full((2, 65, h, w), np.nan, F) for h, w in SIZES4]
    nan, inf = np.nan, np.inf
    rois = np.asarray([[0, 30, 10, 10, 40],               # a negative area
                       [1, nan, 0, 10, 10], [0, 0, nan, 10, 10], [1, 0, 0, nan, 10], [0, 0, 0, 10, nan],
                       [0, inf, 0, inf, 10], [1, 0, -inf, 10, -inf], [0, -inf, -inf, inf, -inf],
                       [2, 0, 0, 50, 50], [-1, 0, 0, 50, 50], [nan, 0, 0, 50, 50], [inf, 0, 0, 300, 300], [-0.5, 0, 0, 50, 50]], F)
    got, lev = _run(ef, poisoned, rois, SCALES4, 7, 7, 2)
    ref_lev = fp.levels(rois, 2, 5)
    assert np.array_equal(lev, ref_lev) and lev[:8].tolist() == [-1] * 8 and (lev[8:] >= 0).all()
    assert not got[:12].any() and not np.signbit(got[:12]).any()                      # +0 everywhere
    assert np.isnan(got[12]).all()                                                     # (int)-0.5 is image 0: this row did read the maps
    feats, _ = pyramid
    mixed = np.concatenate([base[:6], rois[:12], base[6:10]])
    got, lev = _check(ef, feats, mixed, SCALES4, 7, 7, 2)
    assert not got[6:18].any() and got[:6].any() and got[18:].any()


@pytest.mark.parametrize("n", [0, 1])
def test_roi_counts(ef, pyramid, n):
    feats, rois = pyramid
    got, lev = _check(ef, feats, rois[:n], SCALES4, 7, 7, 2)
    assert got.shape == (n, 65, 7, 7) and lev.shape == (n,)


def test_one_level_is_roi_align_forward(ef, pyramid):
    """no mapping at all: NaN-area ROIs are pooled as ifx_roi_align_forward pools them, the levels are 0"""
    feats, rois = pyramid
    rois = np.concatenate([rois[:10], np.asarray([[0, 30, 10, 10, 40], [1, 5, 5, 4, 4], [2, 0, 0, 9, 9]], F)])
    for l in (0, 2):
        got, lev = _check(ef, feats[l:l + 1], rois, SCALES4[l:l + 1], 7, 7, 2)
        plain = ef.roi_align_forward(_cuda(feats[l]), _cuda(rois), SCALES4[l], 7, 7, 2).cpu().numpy()
        assert _bits_equal(got, plain) and not lev.any() and got[10].any() and not got[12].any()


def test_eight_levels_with_one_by_one_top_maps(ef):
    rng = np.random.default_rng(34)
    scales = [2.0 ** -k for k in range(8)]
    feats = [rng.standard_normal((1, 3, max(1, 20 >> k), max(1, 28 >> k))).astype(F) for k in range(8)]
    assert feats[5].shape[2:] == (1, 1) and feats[7].shape[2:] == (1, 1)
    rois = _rois(rng, 40, 1, 28, 20, lo=0.0, hi=12.0)
    _, lev = _check(ef, feats, rois, scales, 2, 2, 2)
    assert set(lev.tolist()) == set(range(8))
    _check(ef, feats, rois, scales, 2, 2, 2, canonical_level=7)


def test_prefilled_out_guard_bands_and_streams(ef, pyramid):
    """out= inside a larger pre-filled buffer: every row is written (zeros where the rule says zeros), the floats on both sides keep their values; the call on a
    side stream is ordered on that stream alone"""
    import torch

    feats, rois = pyramid
    rois = rois[:14].copy()
    rois[3, 1:] = (30, 10, 10, 40)
    rois[9, 0] = 5
    ref, ref_lev = fp.fpn_roi_align(feats, rois, SCALES4, 7, 7, 2)
    guard = 4096
    buf = torch.full((2 * guard + ref.size,), -7.5, device="cuda")
    out = buf[guard:guard + ref.size].view(ref.shape)
    lev_buf = torch.full((rois.shape[0] + 16,), -9, dtype=torch.int32, device="cuda")
    d_feats, d_rois = [_cuda(f) for f in feats], _cuda(rois)
    ret = ef.fpn_roi_align(d_feats, d_rois, SCALES4, 7, 7, 2, out=out, levels_out=lev_buf[8:8 + rois.shape[0]])
    assert ret is out
    host = buf.cpu().numpy()
    assert (host[:guard] == -7.5).all() and (host[guard + ref.size:] == -7.5).all()
    got = host[guard:guard + ref.size].reshape(ref.shape)
    assert _bits_equal(got, ref) and not got[3].any() and not got[9].any()
    lev = lev_buf.cpu().numpy()
    assert (lev[:8] == -9).all() and (lev[8 + rois.shape[0]:] == -9).all() and np.array_equal(lev[8:8 + rois.shape[0]], ref_lev)
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        a = ef.fpn_roi_align(d_feats, d_rois, SCALES4, 7, 7, 2)                       # the current stream
    b = ef.fpn_roi_align(d_feats, d_rois, SCALES4, 7, 7, 2, stream=side)              # named
    side.synchronize()
    assert _bits_equal(a.cpu().numpy(), ref) and _bits_equal(b.cpu().numpy(), ref)


def test_refusals_leave_the_handle_usable(ifx, ef):
    import torch

    L = ifx.lib()
    maps = [torch.zeros(1, 2, 4, 4, device="cuda"), torch.zeros(1, 2, 2, 2, device="cuda")]
    rois, out = torch.zeros(3, 5, device="cuda"), torch.full((3, 2, 2, 2), -3.0, device="cuda")
    lev = torch.full((3,), -9, dtype=torch.int32, device="cuda")

    def call(ptrs=(maps[0].data_ptr(), maps[1].data_ptr()), heights=(4, 2), widths=(4, 2), scales=(0.5, 0.25), levels=2, batch=1, channels=2, d_rois=rois.data_ptr(), n=3,
             s0=224.0, lvl0=4, eps=1e-6, ph=2, pw=2, ratio=2, d_out=out.data_ptr(), d_lev=lev.data_ptr(), null=()):
        nl = len(ptrs)
        a = dict(p=(C.c_void_p * nl)(*ptrs), h=(C.c_int32 * nl)(*heights), w=(C.c_int32 * nl)(*widths), s=(C.c_float * nl)(*scales))
        for k in null:
            a[k] = None
        return L.ifx_fpn_roi_align(ef.handle, a["p"], a["h"], a["w"], a["s"], levels, batch, channels, d_rois, n, s0, lvl0, eps, ph, pw, ratio, d_out, d_lev, None)

    nine = dict(ptrs=(maps[0].data_ptr(),) * 9, heights=(4,) * 9, widths=(4,) * 9, scales=tuple(2.0 ** -k for k in range(9)), levels=9)
    bad = [dict(null=("p",)), dict(null=("h",)), dict(null=("w",)), dict(null=("s",)), dict(ptrs=(maps[0].data_ptr(), None)), dict(d_rois=None), dict(d_out=None),
           dict(levels=0), dict(levels=-1), nine, dict(n=-1), dict(batch=0), dict(channels=0), dict(heights=(4, 0)), dict(widths=(0, 2)), dict(ph=0), dict(pw=0),
           dict(ratio=-1), dict(scales=(0.5, 0.5)), dict(scales=(0.5, 0.125)), dict(scales=(0.25, 0.5)), dict(scales=(0.3, 0.15)), dict(scales=(2.0, 1.0)),
           dict(scales=(0.0, 0.0)), dict(scales=(float("nan"), 0.25)), dict(scales=(-0.5, -0.25)), dict(scales=(2.0 ** -126, 2.0 ** -127)),
           dict(s0=0.0), dict(s0=-224.0), dict(s0=float("nan")), dict(s0=float("inf")), dict(eps=float("nan")), dict(eps=float("inf")), dict(eps=float("-inf")),
           dict(channels=64 * 3, n=2 ** 30), dict(ph=4097, pw=4097), dict(heights=(65536, 2), widths=(32768, 2))]
    for kw in bad:
        assert call(**kw) == E_INVALID, kw
        assert b"ifx_fpn_roi_align" in L.ifx_last_error(ef.handle)
    torch.cuda.synchronize()
    assert bool((out == -3.0).all()) and bool((lev == -9).all())                       # nothing was enqueued
    assert call(n=0, d_rois=None, d_out=None, d_lev=None) == 0                          # n == 0 succeeds and writes nothing
    torch.cuda.synchronize()
    assert bool((out == -3.0).all())
    assert call(d_lev=None) == 0                                                        # the levels are optional
    assert call() == 0
    assert call(eps=-1.0) == 0                                                          # a v below 0: no level, zeros
    torch.cuda.synchronize()
    assert bool((out == 0).all()) and lev.tolist() == [-1, -1, -1]
    assert call(levels=1) == 0                                                          # one level of a two-entry table
    torch.cuda.synchronize()
    assert lev.tolist() == [0, 0, 0]


def test_python_argument_checks(ifx, ef):
    import torch

    maps = [torch.zeros(1, 2, 4, 4, device="cuda"), torch.zeros(1, 2, 2, 2, device="cuda")]
    rois = torch.zeros(3, 5, device="cuda")
    good = dict(features=maps, rois=rois, scales=[0.5, 0.25], pooled_h=2, pooled_w=2, sampling_ratio=2)
    for kw in (dict(features=[maps[0], maps[1].half()]), dict(features=[maps[0].double(), maps[1]]), dict(rois=rois.half()), dict(features=[maps[0], maps[1].cpu().numpy()]),
               dict(out=torch.zeros(3, 2, 2, 2, device="cuda", dtype=torch.float16)), dict(levels_out=torch.zeros(3, dtype=torch.int64, device="cuda")),
               dict(levels_out=torch.zeros(3, device="cuda"))):
        with pytest.raises(TypeError):
            ef.fpn_roi_align(**{**good, **kw})
    for kw in (dict(features=[]), dict(features=[maps[0], maps[1].cpu()]), dict(rois=rois.cpu()), dict(features=[maps[0], maps[1][0]]),
               dict(features=[maps[0], torch.zeros(1, 3, 2, 2, device="cuda")]), dict(features=[maps[0], torch.zeros(2, 2, 2, 2, device="cuda")]),
               dict(features=[maps[0].transpose(2, 3)[:, :, :, :3], maps[1]]), dict(rois=torch.zeros(3, 4, device="cuda")), dict(rois=torch.zeros(5, 3, device="cuda").t()),
               dict(scales=[0.5]), dict(scales=[0.5, 0.25, 0.125]), dict(out=torch.zeros(3, 2, 2, 3, device="cuda")), dict(out=torch.zeros(3, 2, 2, 2)),
               dict(levels_out=torch.zeros(4, dtype=torch.int32, device="cuda")), dict(levels_out=torch.zeros(3, dtype=torch.int32))):
        with pytest.raises(ValueError):
            ef.fpn_roi_align(**{**good, **kw})
    with pytest.raises(ifx.IfxError, match="scales"):
        ef.fpn_roi_align(**{**good, "scales": [0.5, 0.3]})
    assert tuple(ef.fpn_roi_align(**good).shape) == (3, 2, 2, 2)                        # and the handle goes on


class _Boxes:
    """a stand-in for maskrcnn-benchmark's BoxList: what Pooler asks of it"""
    def __init__(self, bbox):
        self.bbox = bbox

    def __len__(self):
        return int(self.bbox.shape[0])

    def area(self):
        b = self.bbox
        return (b[:, 2] - b[:, 0] + 1) * (b[:, 3] - b[:, 1] + 1)


def _reference_loop(ef, x, boxes, scales, res, ratio, levels):
    """Pooler.forward (poolers.py:91-121) line for line over ef.roi_align_forward, the levels given (LevelMapper's arithmetic on the device is not the rule's)"""
    import torch

    concat = torch.cat([b.bbox for b in boxes], dim=0)
    ids = torch.cat([torch.full((len(b), 1), i, dtype=concat.dtype, device=concat.device) for i, b in enumerate(boxes)], dim=0)
    rois = torch.cat([ids, concat], dim=1)
    if len(scales) == 1:
        return ef.roi_align_forward(x[0], rois, scales[0], res, res, ratio)
    result = torch.zeros((len(rois), x[0].shape[1], res, res), dtype=x[0].dtype, device=x[0].device)
    for level, (per_level_feature, scale) in enumerate(zip(x, scales)):
        idx_in_level = torch.nonzero(levels == level).squeeze(1)
        rois_per_level = rois[idx_in_level]
        result[idx_in_level] = ef.roi_align_forward(per_level_feature, rois_per_level.contiguous(), scale, res, res, ratio)
    return result


def test_pooler_module_against_the_reference_loop(ifx, ef, pyramid):
    import torch

    feats, rois = pyramid
    x = [_cuda(f) for f in feats]
    per_image = [rois[rois[:, 0] == i, 1:] for i in range(2)]
    boxes = [_Boxes(_cuda(b)) for b in per_image]
    levels = _cuda(fp.levels(np.concatenate([np.concatenate([np.full((len(b), 1), i, F), b], axis=1) for i, b in enumerate(per_image)]), 2, 5))
    for res, ratio in ((7, 2), (14, 2)):
        mod = ifx.pooler(ef, (res, res), SCALES4, ratio)
        assert isinstance(mod, torch.nn.Module)
        got = mod(x, boxes)
        assert torch.equal(got, _reference_loop(ef, x, boxes, SCALES4, res, ratio, levels))
    one = ifx.pooler(ef, 7, SCALES4[1:2], 2)
    assert torch.equal(one(x[1:2], boxes), _reference_loop(ef, x[1:2], boxes, SCALES4[1:2], 7, 2, None))
    sliced = [t.transpose(2, 3).contiguous().transpose(2, 3) for t in x]              # maps that are not contiguous: the module makes them so
    assert torch.equal(ifx.pooler(ef, 7, SCALES4, 2)(sliced, boxes), ifx.pooler(ef, 7, SCALES4, 2)(x, boxes))


def test_the_map_does_not_notice(ifx, pyramid):
    """two handles through the same three frames; on one of them the call runs (null stream, side stream) between the last frame and
    process_segmentation_rois: labels, instance table and map are those of the other"""
    import torch

    from instancefusion_amd import synth

    st = synth.make_stream(3, Q["w"], Q["h"], Q["fx"], Q["fy"], Q["cx"], Q["cy"], noise=True)
    M = 28
    y, x = np.mgrid[0:M, 0:M]
    roi_masks = np.stack([(np.hypot(x - 13.5, y - 13.5) < r).astype(F) * 0.9 for r in (9, 11, 13)])
    seg_boxes = np.asarray([[20, 15, 80, 70], [70, 40, 140, 110], [30, 60, 90, 115]], F)
    cls = np.asarray([3, 7, 11], np.int32)
    feats, rois = pyramid
    feats, rois = [f[:, :8] for f in feats], rois[:12]
    results = []
    for with_call in (False, True):
        e = ifx.ElasticFusion(**Q, max_surfels=200000)
        inst = ifx.InstanceFusion(e)
        for i in range(3):
            e.processFrame(st["rgb"][i], st["depth"][i])
        if with_call:
            side = torch.cuda.Stream()
            d_feats, d_rois = [_cuda(f) for f in feats], _cuda(rois)
            r1 = e.fpn_roi_align(d_feats, d_rois, SCALES4, 7, 7, 2)
            torch.cuda.synchronize()
            r2 = e.fpn_roi_align(d_feats, d_rois, SCALES4, 7, 7, 2, stream=side)
            side.synchronize()
            ref, _ = fp.fpn_roi_align(feats, rois, SCALES4, 7, 7, 2)
            assert _bits_equal(r1.cpu().numpy(), ref) and torch.equal(r1, r2)
        inst.process_segmentation_rois(_cuda(roi_masks), _cuda(seg_boxes), _cuda(cls), 2)
        results.append((inst.labels(), np.asarray(inst.getInstanceTable()), e.download()))
        e.close()
    (la, ta, ma), (lb, tb, mb) = results
    assert la.size > 0 and np.array_equal(la, lb)
    assert np.array_equal(ta, tb)
    for k in ma:
        assert np.array_equal(ma[k], mb[k]), k
