"""The proposal stage and the box decoding on the device (ifx_rpn_proposals / ifx_box_decode): equal to the numpy statement (tests/rpn_proposals_numpy.py, itself held
against maskrcnn-benchmark's Python in test_rpn_proposals_cpu.py) bit for bit -- boxes, logits, indices, count, and the padding behind the count -- on the golden
cases, at the sizes where the kernels change path (n <= 8192: one sort; above: the radix select), on the directed cases; guard bands, streams, NULL outputs, every
refusal, the Python checks, the module that stands in for RPNPostProcessor, and a map that does not notice.  (A NaN box coordinate, which only ifx_box_decode can
return, is compared as a NaN: its payload is not part of the rule.)"""
import ctypes as C
import os

import numpy as np
import pytest

import rpn_proposals_cases as rc
import rpn_proposals_numpy as rp
from conftest import ROOT

pytestmark = pytest.mark.gpu

E_INVALID = -1
F = np.float32
Q = dict(w=160, h=120, fx=132.0, fy=132.0, cx=80.0, cy=60.0)
GOLDEN = os.path.join(ROOT, "tests", "golden", "rpn_proposals_ref.npz")
GUARD = 64


@pytest.fixture(scope="module")
def ifx():
    import instancefusion_amd as m

    m.lib()
    return m


@pytest.fixture(scope="module")
def ef(ifx):
    """a handle that never sees a frame: the calls need none"""
    e = ifx.ElasticFusion(**Q, max_surfels=100000)
    yield e
    e.close()


@pytest.fixture(scope="module")
def golden():
    return dict(np.load(GOLDEN))


@pytest.fixture(scope="module")
def directed():
    return rc.directed()


def _cuda(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def _params(ifx, img, pre, post, thr, min_size, weights=(1, 1, 1, 1), xform_clip=0.0):
    p = ifx.RpnParams()
    p.pre_nms_top_n, p.post_nms_top_n, p.nms_thresh, p.min_size = int(pre), int(post), float(thr), float(min_size)
    p.weights[:] = [float(v) for v in weights]
    p.xform_clip = xform_clip
    p.image_w, p.image_h = int(img[0]), int(img[1])
    return p


def _raw(ifx, ef, d_obj, d_reg, d_anc, img, pre, post, thr, min_size, weights=(1, 1, 1, 1), stream=None, logits=True, index=True):
    """ifx_rpn_proposals itself, every output inside guard bands: returns the torch buffers (read them with _read once the stream is done)"""
    import torch

    A, H, W = (int(v) for v in d_obj.shape)
    bufs = [torch.full((2 * GUARD + 4 * post,), -7.5, device="cuda"), torch.full((2 * GUARD + post,), -7.5, device="cuda"),
            torch.full((2 * GUARD + post,), -77, dtype=torch.int64, device="cuda"), torch.full((2 * GUARD + 1,), -77, dtype=torch.int32, device="cuda")]
    ptr = [C.c_void_p(b.data_ptr() + GUARD * b.element_size()) for b in bufs]
    if stream is not None:
        stream.wait_stream(torch.cuda.current_stream())                                # (the fills above are on the current stream)
    p = _params(ifx, img, pre, post, thr, min_size, weights)
    r = ef.L.ifx_rpn_proposals(ef.handle, C.c_void_p(d_obj.data_ptr()), C.c_void_p(d_reg.data_ptr()), C.c_void_p(d_anc.data_ptr()), A, H, W, C.byref(p), ptr[0],
                               ptr[1] if logits else None, ptr[2] if index else None, ptr[3], C.c_void_p(stream.cuda_stream) if stream is not None else None)
    assert r == 0, ef.L.ifx_last_error(ef.handle)
    return bufs


def _read(bufs, post):
    """(boxes [post,4], logits [post], index [post], count) out of _raw's buffers; the guard bands must be as they were"""
    host = [b.cpu().numpy() for b in bufs]
    for h, fill in zip(host, (-7.5, -7.5, -77, -77)):
        assert (h[:GUARD] == fill).all() and (h[-GUARD:] == fill).all()
    return host[0][GUARD:-GUARD].reshape(post, 4), host[1][GUARD:-GUARD], host[2][GUARD:-GUARD], int(host[3][GUARD])


def _equal(got, ref, post):
    """the device's padded outputs against the statement's result, bit for bit"""
    boxes, logits, index, count = got
    pb, pl, pi, c = rp.padded(ref, post)
    assert count == c, (count, c)
    assert np.array_equal(index, pi), int((index != pi).sum())
    assert np.array_equal(_bits(boxes), _bits(pb)), int((_bits(boxes) != _bits(pb)).sum())
    assert np.array_equal(_bits(logits), _bits(pl))


def _check(ifx, ef, obj, reg, anc, img, pre, post, thr, min_size, weights=(1, 1, 1, 1)):
    import torch

    bufs = _raw(ifx, ef, _cuda(obj), _cuda(reg), _cuda(anc), img, pre, post, thr, min_size, weights)
    torch.cuda.synchronize()
    ref = rp.rpn_proposals(obj, reg, anc, img, pre, post, thr, min_size, weights)
    _equal(_read(bufs, post), ref, post)
    return ref


# ------------------------------------------------------------------------------------------------------------------------------------------------ proposals

def test_golden_cases(ifx, ef, golden):
    for k in range(int(golden["counts"][0])):
        iw, ih, pre, post, thr, min_size = golden[f"rpn{k}_par"][:6]
        ref = _check(ifx, ef, golden[f"rpn{k}_objectness"], golden[f"rpn{k}_regression"], golden[f"rpn{k}_anchors"], (int(iw), int(ih)), int(pre), int(post), thr, min_size)
        assert np.array_equal(ref[2], golden[f"rpn{k}_index"])


# n = A H W on both sides of 8192 (the select is skipped up to it), the reference's level (38 x 50 x 15) and an FPN level 0 (200 x 336 x 3)
SIZES = [((1, 1, 1), 1), ((7, 3, 3), 1000), ((1, 8, 8), 8192), ((5, 1, 13), 1), ((5, 10, 20), 1000), ((5, 10, 20), 6000), ((2, 64, 64), 8192), ((2, 64, 64), 6000),
         ((3, 1, 2731), 8192), ((3, 1, 2731), 1), ((3, 1, 2731), 1000), ((15, 38, 50), 6000), ((15, 38, 50), 1), ((15, 38, 50), 8192), ((3, 200, 336), 1000),
         ((3, 200, 336), 8192)]


@pytest.mark.parametrize("shape,pre", SIZES)
def test_sizes(ifx, ef, shape, pre):
    A, H, W = shape
    assert A * H * W in (1, 63, 64, 65, 1000, 8192, 8193, 28500, 201600)
    obj, reg, anc, img = rc.level(A * H * W + pre, A, H, W)
    post = 200 if pre == 6000 else 1000
    ref = _check(ifx, ef, obj, reg, anc, img, pre, post, 0.7, 0)
    assert ref[2].size == min(post, ref[2].size) and (pre < 1000 or A * H * W < 1000 or ref[2].size >= 100)


def test_directed_cases(ifx, ef, directed):
    for name, (obj, reg, anc, img, pre, post, thr, min_size) in directed.items():
        ref = _check(ifx, ef, obj, reg, anc, img, pre, post, thr, min_size)
        assert (ref[2].size == 0) == (name == "all_removed"), name


def test_thousands_tie_at_the_boundary(ifx, ef):
    """the reference's level with the logits quantised to 8 values: the radix select's boundary key is shared by thousands, the lowest indices win"""
    obj, reg, anc, img = rc.level(5, 15, 38, 50)
    q = np.clip(np.round(obj), -4, 3).astype(F)
    assert np.unique(q).size == 8
    logits, _ = rp.flatten(q, reg)
    for pre in (6000, 1, 8192):
        ref = _check(ifx, ef, q, reg, anc, img, pre, 300, 0.7, 0)
        last = np.sort(logits)[::-1][pre - 1]
        assert (logits == last).sum() > 2000 and (logits > last).sum() < pre
    q[:] = 1.5                                                                         # all equal: the first 6000 anchors
    _check(ifx, ef, q, reg, anc, img, 6000, 300, 0.7, 0)
    q[:] = np.nan
    q.reshape(-1)[::5] = 1.5                                                           # 5700 numbers: the boundary inside the NaNs
    _check(ifx, ef, q, reg, anc, img, 8192, 300, 2.0, 0)
    _check(ifx, ef, np.full_like(q, np.nan), reg, anc, img, 100, 100, 2.0, 0)


def test_weights_min_size_and_thresholds(ifx, ef):
    obj, reg, anc, img = rc.level(6, 3, 20, 30)
    _check(ifx, ef, obj, reg * 4, anc, img, 1000, 100, 0.5, 8, weights=(10, 10, 5, 5))
    assert _check(ifx, ef, obj, reg, anc, img, 1800, 64, 0.3, 0)[2].size == 64
    assert _check(ifx, ef, obj, reg, anc, img, 500, 500, float("inf"), 16)[2].size < 500          # nothing suppressed: the filter alone
    assert _check(ifx, ef, obj, reg, anc, img, 500, 500, -1.0, 0)[2].size == 1                     # every IoU is > -1: the best box alone


def test_python_call_padded_and_cut(ifx, ef):
    import torch

    obj, reg, anc, img = rc.level(7, 15, 12, 17)
    ref = rp.rpn_proposals(obj, reg, anc, img, 2000, 900, 0.3, 0)
    d = (_cuda(obj), _cuda(reg), _cuda(anc))
    boxes, score, index = ef.rpn_proposals(*d, img, 2000, 900, 0.3, 0)
    c = ref[2].size
    assert 0 < c < 900 and boxes.shape == (c, 4) and score.shape == (c,) and index.dtype == torch.int64
    assert np.array_equal(_bits(boxes.cpu().numpy()), _bits(ref[0])) and np.array_equal(index.cpu().numpy(), ref[2])
    assert torch.equal(score, torch.sigmoid(_cuda(ref[1])))
    pb, ps, pi, count = ef.rpn_proposals(d[0][None], d[1][None], d[2], img, 2000, 900, 0.3, 0, padded=True)      # [1,A,H,W] too
    assert pb.shape == (900, 4) and ps.shape == (900,) and pi.shape == (900,) and count.dtype == torch.int32 and int(count.item()) == c
    assert torch.equal(pb[:c], boxes) and torch.equal(ps[:c], score) and torch.equal(pi[:c], index)
    assert not pb[c:].any() and bool((ps[c:] == 0.5).all()) and bool((pi[c:] == -1).all())           # sigmoid(0) behind the count
    b2, s2, i2 = ef.rpn_proposals(*d, img, pre_nms_top_n=2000, post_nms_top_n=900, nms_thresh=0.3)                    # defaults: min_size 0, weights (1, 1, 1, 1)
    assert torch.equal(b2, boxes) and torch.equal(i2, index)


def test_two_streams_back_to_back(ifx, ef):
    """calls on two streams with nothing in between share the handle's scratch: each waits for the one before on the device"""
    import torch

    cases = []
    for seed, (A, H, W), pre in ((8, (15, 38, 50), 6000), (9, (3, 30, 40), 3000), (10, (15, 38, 50), 2000), (11, (1, 9, 9), 50)):
        obj, reg, anc, img = rc.level(seed, A, H, W)
        cases.append(((_cuda(obj), _cuda(reg), _cuda(anc)), img, pre, rp.rpn_proposals(obj, reg, anc, img, pre, 200, 0.7, 0)))
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    torch.cuda.synchronize()
    outs = [_raw(ifx, ef, *d, img, pre, 200, 0.7, 0, stream=(s1, s2)[i % 2]) for i, (d, img, pre, _) in enumerate(cases)]
    outs.append(_raw(ifx, ef, *cases[0][0], cases[0][1], cases[0][2], 200, 0.7, 0))                   # and the null stream
    torch.cuda.synchronize()
    for bufs, (_, _, _, ref) in zip(outs, cases + cases[:1]):
        _equal(_read(bufs, 200), ref, 200)


def test_null_logits_and_index(ifx, ef):
    import torch

    obj, reg, anc, img = rc.level(12, 3, 9, 11)
    ref = rp.rpn_proposals(obj, reg, anc, img, 200, 40, 0.7, 0)
    d = (_cuda(obj), _cuda(reg), _cuda(anc))
    for logits, index in ((False, True), (True, False), (False, False)):
        bufs = _raw(ifx, ef, *d, img, 200, 40, 0.7, 0, logits=logits, index=index)
        torch.cuda.synchronize()
        boxes, lg, idx, count = _read(bufs, 40)
        pb, pl, pi, c = rp.padded(ref, 40)
        assert count == c and np.array_equal(_bits(boxes), _bits(pb))
        assert np.array_equal(_bits(lg), _bits(pl)) if logits else (lg == -7.5).all()
        assert np.array_equal(idx, pi) if index else (idx == -77).all()


# ----------------------------------------------------------------------------------------------------------------------------------------------- box_decode

def _decode_equal(got, ref):
    nan = np.isnan(ref)
    assert got.shape == ref.shape and np.array_equal(np.isnan(got), nan)
    assert np.array_equal(_bits(got)[~nan], _bits(ref)[~nan]), int((_bits(got)[~nan] != _bits(ref)[~nan]).sum())


@pytest.mark.parametrize("n", [0, 1, 65, 1000])
@pytest.mark.parametrize("k", [1, 81])
def test_box_decode_sizes(ef, n, k):
    rng = np.random.default_rng(100 * n + k)
    weights = (10, 10, 5, 5) if k == 81 else (1, 1, 1, 1)
    c0 = rng.uniform(0, 500, (n, 2))
    boxes = np.concatenate([c0, c0 + rng.uniform(2, 300, (n, 2))], axis=1).astype(F).reshape(n, 4)
    codes = rng.standard_normal((n, k, 4)) * 0.7
    codes[..., 2:][rng.random((n, k, 2)) < 0.1] = 7.0                                  # above the clip
    codes[..., 3][rng.random((n, k)) < 0.02] = -300.0                                  # EXP's lower clamp
    codes = (codes * np.asarray(weights)).reshape(n, 4 * k).astype(F)
    if n > 1:
        codes[1, 0], codes[1, -1], boxes[n // 2, 2] = np.nan, np.nan, np.nan
        codes[2 % n, 2] = np.inf
    d_codes, d_boxes = _cuda(codes), _cuda(boxes)
    _decode_equal(ef.box_decode(d_codes, d_boxes, weights).cpu().numpy(), rp.box_decode(codes, boxes, weights))
    _decode_equal(ef.box_decode(d_codes, d_boxes, weights, clip_to=(333, 217)).cpu().numpy(), rp.box_decode(codes, boxes, weights, clip_to=(333, 217)))


def test_box_decode_golden_out_and_stream(ef, golden):
    import torch

    for k in range(int(golden["counts"][1])):
        codes, boxes, weights = golden[f"dec{k}_codes"], golden[f"dec{k}_boxes"], golden[f"dec{k}_weights"]
        _decode_equal(ef.box_decode(_cuda(codes), _cuda(boxes), tuple(weights)).cpu().numpy(), rp.box_decode(codes, boxes, weights))
    codes, boxes = golden["dec2_codes"], golden["dec2_boxes"]
    ref = rp.box_decode(codes, boxes, golden["dec2_weights"])
    buf = torch.full((2 * GUARD + ref.size,), -7.5, device="cuda")
    out = buf[GUARD:GUARD + ref.size].view(ref.shape)
    side = torch.cuda.Stream()
    d_codes, d_boxes = _cuda(codes), _cuda(boxes)
    torch.cuda.synchronize()
    assert ef.box_decode(d_codes, d_boxes, tuple(golden["dec2_weights"]), out=out, stream=side) is out
    side.synchronize()
    host = buf.cpu().numpy()
    assert (host[:GUARD] == -7.5).all() and (host[-GUARD:] == -7.5).all()
    _decode_equal(host[GUARD:-GUARD].reshape(ref.shape), ref)


# ----------------------------------------------------------------------------------------------------------------------------------------------- interfaces

def test_refusals_leave_the_handle_usable(ifx, ef):
    import torch

    L = ifx.lib()
    obj, reg, anc, img = rc.level(13, 3, 4, 5)
    d_obj, d_reg, d_anc = _cuda(obj), _cuda(reg), _cuda(anc)
    boxes, logits = torch.full((10, 4), -7.5, device="cuda"), torch.zeros(10, device="cuda")
    index, count = torch.zeros(10, dtype=torch.int64, device="cuda"), torch.full((1,), -9, dtype=torch.int32, device="cuda")
    P = lambda t: C.c_void_p(t.data_ptr())

    def call(o=P(d_obj), r=P(d_reg), a=P(d_anc), A=3, H=4, W=5, par=True, b=P(boxes), c=P(count), **kw):
        args = dict(img=img, pre=50, post=10, thr=0.7, min_size=0.0)
        args.update(kw)
        p = _params(ifx, **args)
        return L.ifx_rpn_proposals(ef.handle, o, r, a, A, H, W, C.byref(p) if par else None, b, P(logits), P(index), c, None)

    nan, inf = float("nan"), float("inf")
    bad = [dict(o=None), dict(r=None), dict(a=None), dict(b=None), dict(c=None), dict(par=False), dict(A=-1), dict(H=-1), dict(W=-1), dict(A=4096, H=4096, W=2),
           dict(pre=0), dict(pre=8193), dict(post=0), dict(post=8193), dict(thr=nan), dict(weights=(1, 0, 1, 1)), dict(weights=(1, 1, nan, 1)), dict(weights=(inf, 1, 1, 1)),
           dict(img=(0, 10)), dict(img=(10, 0))]
    for kw in bad:
        assert call(**kw) == E_INVALID, kw
        assert b"ifx_rpn_proposals" in L.ifx_last_error(ef.handle)
    torch.cuda.synchronize()
    assert int(count.item()) == -9 and bool((boxes == -7.5).all())                     # nothing was enqueued
    assert call(A=0, o=None, r=None, a=None) == 0                                      # no anchors: count 0 and the padding
    torch.cuda.synchronize()
    assert int(count.item()) == 0 and not boxes.any() and bool((index == -1).all())
    assert call(xform_clip=nan) == 0 and call(thr=inf) == 0 and call() == 0
    torch.cuda.synchronize()
    ref = rp.rpn_proposals(obj, reg, anc, img, 50, 10, 0.7, 0)
    assert int(count.item()) == ref[2].size and np.array_equal(_bits(boxes.cpu().numpy()[:ref[2].size]), _bits(ref[0]))
    codes, bx, out = torch.zeros(3, 8, device="cuda"), torch.zeros(3, 4, device="cuda"), torch.full((3, 8), -7.5, device="cuda")

    def dec(c=P(codes), b=P(bx), n=3, k=2, w=(1, 1, 1, 1), cw=0, ch=0, o=P(out)):
        return L.ifx_box_decode(ef.handle, c, b, n, k, C.byref((C.c_float * 4)(*w)) if w else None, 0.0, cw, ch, o, None)

    for kw in (dict(c=None), dict(b=None), dict(o=None), dict(w=None), dict(n=-1), dict(k=0), dict(n=1 << 20, k=1 << 12), dict(w=(0, 1, 1, 1)), dict(w=(1, 1, 1, nan)),
               dict(cw=5), dict(ch=5), dict(cw=-1, ch=-1)):
        assert dec(**kw) == E_INVALID, kw
        assert b"ifx_box_decode" in L.ifx_last_error(ef.handle)
    torch.cuda.synchronize()
    assert bool((out == -7.5).all())
    assert dec(n=0, c=None, b=None, o=None) == 0 and dec() == 0 and dec(cw=5, ch=5) == 0
    torch.cuda.synchronize()
    assert not bool((out == -7.5).any())


def test_python_argument_checks(ifx, ef):
    import torch

    obj, reg, anc = torch.zeros(3, 4, 5, device="cuda"), torch.zeros(12, 4, 5, device="cuda"), torch.zeros(60, 4, device="cuda")
    good = dict(objectness=obj, box_regression=reg, anchors=anc, image_size=(80, 64))
    for kw in (dict(objectness=obj.half()), dict(box_regression=reg.double()), dict(anchors=anc.int()), dict(objectness=obj.cpu().numpy())):
        with pytest.raises(TypeError):
            ef.rpn_proposals(**{**good, **kw})
    for kw in (dict(objectness=obj.cpu()), dict(box_regression=reg.cpu()), dict(anchors=anc.cpu()), dict(objectness=obj[0]), dict(objectness=torch.zeros(2, 3, 4, 5, device="cuda")),
               dict(box_regression=torch.zeros(11, 4, 5, device="cuda")), dict(anchors=torch.zeros(59, 4, device="cuda")), dict(anchors=torch.zeros(60, 5, device="cuda")),
               dict(objectness=torch.zeros(3, 5, 4, device="cuda").transpose(1, 2)), dict(anchors=torch.zeros(4, 60, device="cuda").t())):
        with pytest.raises(ValueError):
            ef.rpn_proposals(**{**good, **kw})
    with pytest.raises(ifx.IfxError):
        ef.rpn_proposals(**good, pre_nms_top_n=8193)
    with pytest.raises(ifx.IfxError):
        ef.rpn_proposals(**good, weights=(1, 1, 0, 1))
    assert ef.rpn_proposals(**good)[0].shape[1] == 4                                  # and the handle goes on
    codes, boxes = torch.zeros(5, 8, device="cuda"), torch.zeros(5, 4, device="cuda")
    for kw in (dict(codes=codes.half()), dict(boxes=boxes.double()), dict(out=torch.zeros(5, 8, device="cuda", dtype=torch.float16))):
        with pytest.raises(TypeError):
            ef.box_decode(**{**dict(codes=codes, boxes=boxes), **kw})
    for kw in (dict(codes=codes.cpu()), dict(boxes=boxes.cpu()), dict(codes=torch.zeros(5, 7, device="cuda")), dict(codes=torch.zeros(4, 8, device="cuda")),
               dict(boxes=torch.zeros(5, 5, device="cuda")), dict(codes=torch.zeros(8, 5, device="cuda").t()), dict(out=torch.zeros(5, 4, device="cuda")),
               dict(out=torch.zeros(5, 8))):
        with pytest.raises(ValueError):
            ef.box_decode(**{**dict(codes=codes, boxes=boxes), **kw})
    with pytest.raises(ifx.IfxError):
        ef.box_decode(codes, boxes, clip_to=(5, 0))
    assert ef.box_decode(codes, boxes).shape == (5, 8)


class _BoxList:
    """the least of maskrcnn-benchmark's BoxList that the module needs"""
    def __init__(self, bbox, size, mode="xyxy"):
        self.bbox, self.size, self.mode, self.fields = bbox, size, mode, {}

    def add_field(self, name, value):
        self.fields[name] = value

    def get_field(self, name):
        return self.fields[name]


def test_rpn_post_processor_one_level_and_two(ifx, ef):
    import torch

    l0 = [rc.level(20 + i, 3, 12, 16) for i in range(2)]                              # two images, level 0
    l1 = [rc.level(30 + i, 3, 6, 8, stride=32) for i in range(2)]                     # level 1
    size = l0[0][3]
    one = ifx.rpn_post_processor(ef, 300, 40, 0.7, 0).eval()
    anchors = [[_BoxList(_cuda(l0[i][2]), size)] for i in range(2)]
    objectness = [_cuda(np.stack([l0[0][0], l0[1][0]]))]
    regression = [_cuda(np.stack([l0[0][1], l0[1][1]]))]
    res = one(anchors, objectness, regression)
    assert len(res) == 2
    for i, r in enumerate(res):
        b, s, _ = ef.rpn_proposals(_cuda(l0[i][0]), _cuda(l0[i][1]), _cuda(l0[i][2]), size, 300, 40, 0.7, 0)
        assert type(r) is _BoxList and r.size == size and r.mode == "xyxy" and torch.equal(r.bbox, b) and torch.equal(r.get_field("objectness"), s)
        assert np.array_equal(_bits(b.cpu().numpy()), _bits(rp.rpn_proposals(l0[i][0], l0[i][1], l0[i][2], size, 300, 40, 0.7, 0)[0]))
    two = ifx.rpn_post_processor(ef, 300, 40, 0.7, 0, fpn_post_nms_top_n=50).eval()
    anchors = [[_BoxList(_cuda(l0[i][2]), size), _BoxList(_cuda(l1[i][2]), size)] for i in range(2)]
    objectness.append(_cuda(np.stack([l1[0][0], l1[1][0]])))
    regression.append(_cuda(np.stack([l1[0][1], l1[1][1]])))
    res = two(anchors, objectness, regression, targets=None)
    for i, r in enumerate(res):
        parts = [rp.rpn_proposals(lv[i][0], lv[i][1], lv[i][2], size, 300, 40, 0.7, 0) for lv in (l0, l1)]
        boxes = np.concatenate([p[0] for p in parts])
        score = torch.sigmoid(_cuda(np.concatenate([p[1] for p in parts])))
        assert score.numel() > 50 and torch.unique(score).numel() == score.numel()   # (distinct: the top-k's order is determined)
        top = torch.topk(score, 50, dim=0, sorted=True)[1]
        assert torch.equal(r.get_field("objectness"), score[top])
        assert np.array_equal(_bits(r.bbox.cpu().numpy()), _bits(boxes[top.cpu().numpy()]))
    with pytest.raises(RuntimeError, match="inference only"):
        two.train()(anchors, objectness, regression)


def test_the_map_does_not_notice(ifx):
    """two handles through the same three frames; on one of them both calls run (null stream, side stream) between the second frame and the third: the third
    frame's pose and the map's count are those of the other"""
    import torch

    from instancefusion_amd import synth

    st = synth.make_stream(3, Q["w"], Q["h"], Q["fx"], Q["fy"], Q["cx"], Q["cy"], noise=True)
    obj, reg, anc, img = rc.level(40, 15, 38, 50)
    ref = rp.rpn_proposals(obj, reg, anc, img, 6000, 200, 0.7, 0)
    results = []
    for with_calls in (False, True):
        e = ifx.ElasticFusion(**Q, max_surfels=200000)
        for i in range(2):
            e.processFrame(st["rgb"][i], st["depth"][i])
        if with_calls:
            side = torch.cuda.Stream()
            d = (_cuda(obj), _cuda(reg), _cuda(anc))
            torch.cuda.synchronize()
            a = e.rpn_proposals(*d, img, 6000, 200, 0.7, 0)
            b = e.rpn_proposals(*d, img, 6000, 200, 0.7, 0, stream=side)
            dec = e.box_decode(d[1].reshape(-1, 4)[:anc.shape[0]].contiguous(), d[2], stream=side)
            side.synchronize()
            assert np.array_equal(a[2].cpu().numpy(), ref[2]) and torch.equal(a[0], b[0]) and np.array_equal(_bits(a[0].cpu().numpy()), _bits(ref[0]))
            assert dec.shape == (anc.shape[0], 4)
        pose = e.processFrame(st["rgb"][2], st["depth"][2])
        results.append((np.asarray(pose).copy(), e.count, e.download()))
        e.close()
    (pa, ca, ma), (pb, cb, mb) = results
    assert np.array_equal(pa, pb) and ca == cb and ca > 0
    for k in ma:
        assert np.array_equal(ma[k], mb[k]), k
