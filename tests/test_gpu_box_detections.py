"""The box head's post-processing on the device (ifx_box_detections): equal to the numpy statement (tests/box_detections_numpy.py, itself held against
maskrcnn-benchmark's Python in test_box_detections_cpu.py) bit for bit -- boxes, scores, labels, indices, count, stats, and the padding behind the count -- on the
golden cases, at the sizes where the kernels change path, at the cap of 8192 candidates and above it, at the limit with and without ties, at the suppression's
extremes; guard bands, streams that share the scratch with ifx_nms and ifx_rpn_proposals, NULL outputs, every refusal, the Python checks, the module that stands in
for PostProcessor, and a map that does not notice."""
import ctypes as C
import os

import numpy as np
import pytest

import box_detections_cases as bc
import box_detections_numpy as bd
import rpn_proposals_cases as rc
import rpn_proposals_numpy as rp
from conftest import ROOT
from detector_ops_numpy import nms as nms_numpy

pytestmark = pytest.mark.gpu

E_INVALID = -1
F = np.float32
Q = dict(w=160, h=120, fx=132.0, fy=132.0, cx=80.0, cy=60.0)
GOLDEN = os.path.join(ROOT, "tests", "golden", "box_detections_ref.npz")
GUARD = 64
FILL = (-7.5, -7.5, -77, -77, -77, -77)


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


def _cuda(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def _params(ifx, img, st, nms, M, max_out, weights=bc.WEIGHTS, xform_clip=0.0):
    p = ifx.BoxDetParams()
    p.score_thresh, p.nms, p.detections_per_img, p.max_out = float(st), float(nms), int(M), int(max_out)
    p.weights[:] = [float(v) for v in weights]
    p.xform_clip = xform_clip
    p.image_w, p.image_h = int(img[0]), int(img[1])
    return p


def _raw(ifx, ef, d, img, st, nms, M, max_out, weights=bc.WEIGHTS, stream=None, present=(True, True, True, True)):
    """ifx_box_detections itself, every output inside guard bands: returns the torch buffers (read them with _read once the stream is done).
    present: scores, labels, index, stats -- False passes NULL"""
    import torch

    d_logits, d_reg, d_prop = d
    R, Cn = (int(v) for v in d_logits.shape)
    bufs = [torch.full((2 * GUARD + 4 * max_out,), FILL[0], device="cuda"), torch.full((2 * GUARD + max_out,), FILL[1], device="cuda"),
            torch.full((2 * GUARD + max_out,), FILL[2], dtype=torch.int64, device="cuda"), torch.full((2 * GUARD + max_out,), FILL[3], dtype=torch.int64, device="cuda"),
            torch.full((2 * GUARD + 1,), FILL[4], dtype=torch.int32, device="cuda"), torch.full((2 * GUARD + 2,), FILL[5], dtype=torch.int32, device="cuda")]
    ptr = [C.c_void_p(b.data_ptr() + GUARD * b.element_size()) for b in bufs]
    if stream is not None:
        stream.wait_stream(torch.cuda.current_stream())                                # (the fills above are on the current stream)
    p = _params(ifx, img, st, nms, M, max_out, weights)
    r = ef.L.ifx_box_detections(ef.handle, C.c_void_p(d_logits.data_ptr()), C.c_void_p(d_reg.data_ptr()), C.c_void_p(d_prop.data_ptr()), R, Cn, int(d_reg.shape[1]) // 4,
                                C.byref(p), ptr[0], ptr[1] if present[0] else None, ptr[2] if present[1] else None, ptr[3] if present[2] else None, ptr[4],
                                ptr[5] if present[3] else None, C.c_void_p(stream.cuda_stream) if stream is not None else None)
    assert r == 0, ef.L.ifx_last_error(ef.handle)
    return bufs


def _read(bufs, max_out):
    """(boxes [max_out,4], scores, labels, index, count, stats [2]) out of _raw's buffers; the guard bands must be as they were"""
    host = [b.cpu().numpy() for b in bufs]
    for h, fill in zip(host, FILL):
        assert (h[:GUARD] == fill).all() and (h[-GUARD:] == fill).all()
    return host[0][GUARD:-GUARD].reshape(max_out, 4), host[1][GUARD:-GUARD], host[2][GUARD:-GUARD], host[3][GUARD:-GUARD], int(host[4][GUARD]), host[5][GUARD:-GUARD]


def _equal(got, ref, max_out, present=(True, True, True, True)):
    """the device's padded outputs against the statement's result, bit for bit; an output that was NULL must be untouched"""
    boxes, scores, labels, index, count, stats = got
    pb, ps, pl, pi, c, st = bd.padded(ref, max_out)
    assert count == c, (count, c)
    assert np.array_equal(_bits(boxes), _bits(pb)), int((_bits(boxes) != _bits(pb)).sum())
    assert np.array_equal(_bits(scores), _bits(ps)) if present[0] else (scores == FILL[1]).all()
    assert np.array_equal(labels, pl) if present[1] else (labels == FILL[2]).all()
    assert np.array_equal(index, pi) if present[2] else (index == FILL[3]).all()
    assert np.array_equal(stats, st) if present[3] else (stats == FILL[5]).all()


def _check(ifx, ef, case, st=0.05, nms=0.5, M=100, max_out=None, weights=bc.WEIGHTS):
    import torch

    logits, reg, prop, img = case
    max_out = max_out if max_out is not None else (M if M > 0 else 8192)
    bufs = _raw(ifx, ef, (_cuda(logits), _cuda(reg), _cuda(prop)), img, st, nms, M, max_out, weights)
    torch.cuda.synchronize()
    ref = bd.box_detections(logits, reg, prop, img, st, nms, M, weights)
    _equal(_read(bufs, max_out), ref, max_out)
    return ref


# ------------------------------------------------------------------------------------------------------------------------------------------------ the rule

def test_golden_cases(ifx, ef, golden):
    for k in range(int(golden["counts"][0])):
        iw, ih, st, nms, M, K, Dk = golden[f"det{k}_par"]
        ref = _check(ifx, ef, (golden[f"det{k}_logits"], golden[f"det{k}_regression"], golden[f"det{k}_proposals"], (int(iw), int(ih))), st, nms, int(M),
                     max_out=int(M) if M > 0 else 1024, weights=tuple(golden[f"det{k}_weights"]))
        assert np.array_equal(ref[2], golden[f"det{k}_labels"]) and np.array_equal(ref[3], golden[f"det{k}_index"]) and ref[4:] == (int(K), int(Dk))


# (R, C, K): one row, one wave's worth of rows and one more, more than one softmax block, the reference's 1000 x 81, and 4 x 2049 plane positions, which cross a
# compaction chunk of 2048; K on 0, 1, 63, 64, 65 (the pair mask's tile) and a few thousand
SIZES = [(0, 81, 0), (1, 2, 0), (1, 2, 1), (1, 81, 1), (1, 81, 12), (63, 3, 63), (64, 3, 64), (65, 3, 65), (64, 3, 0), (65, 3, 1), (300, 81, 3000), (1000, 81, 6000),
         (2049, 5, 4100), (2049, 5, 65)]


@pytest.mark.parametrize("R,Cn,K", SIZES)
def test_sizes(ifx, ef, R, Cn, K):
    case = bc.with_k(1000 * R + K, R, Cn, K)
    ref = _check(ifx, ef, case, M=0, max_out=8192)
    assert ref[4] == K and (K == 0 or 0 < ref[5] <= K)
    _check(ifx, ef, case, M=100)


def test_random_heads_and_weights(ifx, ef):
    assert _check(ifx, ef, bc.head(1, 300, 81, scale=2.5))[4] > 300
    assert _check(ifx, ef, bc.head(2, 777, 3, scale=1.0), st=0.3, nms=0.3, M=5)[5] > 5
    assert _check(ifx, ef, bc.head(3, 129, 1024, scale=4.0), M=0, max_out=4096)[4] > 100                 # the widest row
    _check(ifx, ef, bc.head(4, 200, 7, weights=(1, 1, 1, 1)), weights=(1, 1, 1, 1), M=0, max_out=2048)
    logits, reg, prop, img = bc.head(5, 50, 6, scale=1.0)
    logits[3, 2], logits[7, 0], logits[11, :], logits[13, 5], logits[48, 1] = np.nan, np.inf, -np.inf, -np.inf, np.nan      # rows that yield nothing; a plain 0
    ref = _check(ifx, ef, (logits, reg, prop, img), M=0, max_out=512)
    assert not np.isin(ref[3], [3, 7, 11, 48]).any() and 13 in ref[3]
    assert _check(ifx, ef, (np.full((40, 4), np.nan, F), reg[:40, :16], prop[:40], img))[4] == 0


def test_the_cap(ifx, ef):
    """K = 8192 exactly runs; K = 8194 writes the padding, count -1 and stats {8194, 0}; the cut form raises; the next call is correct"""
    import torch

    ref = _check(ifx, ef, bc.at_the_cap(4096), M=100)
    assert ref[4] == 8192 and ref[0].shape[0] >= 100
    over = bc.at_the_cap(4097)
    ref = _check(ifx, ef, over, M=100)
    assert ref[4:] == (8194, 0)
    d = tuple(_cuda(a) for a in over[:3])
    with pytest.raises(ifx.IfxError, match="8194.*8192"):
        ef.box_detections(*d, over[3])
    b, s, l, i, count, stats = ef.box_detections(*d, over[3], padded=True)
    torch.cuda.synchronize()
    assert int(count.item()) == -1 and stats.tolist() == [8194, 0] and not b.any() and bool((l == -1).all())
    assert len(ef.box_detections(*d, over[3], score_thresh=0.5)[0]) == 0                                   # met by raising score_thresh
    _check(ifx, ef, bc.head(6, 100, 9))


def test_the_limit(ifx, ef):
    case = bc.head(11, 400, 5, scale=1.0)
    Dk = _check(ifx, ef, case, M=0, max_out=2048)[5]
    assert 20 < Dk < 2048
    for M in (Dk - 1, Dk, Dk + 1, Dk // 2, 1):
        ref = _check(ifx, ef, case, M=M)
        assert ref[0].shape[0] == min(M, Dk) and ref[5] == Dk                                             # (distinct scores: the limit is met exactly)
    rng = np.random.default_rng(12)                                                                       # quantised logits: many kept scores tie at t
    R = 600
    logits = np.zeros((R, 3), F)
    logits[:, 1] = rng.integers(0, 3, R).astype(F)
    reg, prop = np.zeros((R, 12), F), (np.arange(R, dtype=F)[:, None] * 40 + np.asarray([0, 0, 20, 20], F)).astype(F)
    tied = (logits, reg, prop, (30000, 100))
    free = bd.box_detections(*tied, 0.3, 0.5, 0)
    top = int((free[1] == free[1].max()).sum())
    for M in (1, top, top + 1):
        ref = _check(ifx, ef, tied, st=0.3, M=M)                                                          # max_out = M: a count above it leaves exactly M rows
        assert ref[0].shape[0] == (top if M <= top else int((free[1] >= np.unique(free[1])[-2]).sum())) and (M == top or ref[0].shape[0] > M)
        _check(ifx, ef, tied, st=0.3, M=M, max_out=2048)


def test_suppression_extremes_and_classes_apart(ifx, ef):
    case = bc.head(13, 150, 6, scale=1.0)
    ref = _check(ifx, ef, case, nms=-1.0, M=0, max_out=1024)                                              # every IoU is > -1: the best box of each class alone
    assert ref[5] == 5 and ref[2].tolist() == [1, 2, 3, 4, 5]
    ref = _check(ifx, ef, case, nms=float("inf"), M=0, max_out=1024)
    assert ref[5] == ref[4] > 100
    logits, reg, prop, img = bc.head(14, 20, 3, creg=1)                                                   # one code for both classes: identical boxes in two classes
    logits[:] = np.asarray([0, 1, 1.5], F)
    prop = (np.arange(20, dtype=F)[:, None] * 60 + np.asarray([0, 0, 30, 30], F)).astype(F)
    reg = np.zeros_like(reg)
    ref = _check(ifx, ef, (logits, reg, prop, (2000, 100)), M=0, max_out=64)
    assert ref[4] == 40 and ref[5] == 40 and np.array_equal(ref[0][:20], ref[0][20:])                     # neither suppresses the other
    same = np.tile(prop[:1], (20, 1))
    assert _check(ifx, ef, (logits, reg, same, (2000, 100)), M=0, max_out=64)[5] == 2     # and within a class one is left


def test_cls_agnostic(ifx, ef):
    case = bc.head(15, 333, 9, creg=1)
    ref = _check(ifx, ef, case)
    assert ref[0].shape[0] >= 100
    tiled = (case[0], np.tile(case[1], (1, 9)), case[2], case[3])
    assert np.array_equal(_check(ifx, ef, tiled)[0], ref[0])


def test_null_optional_outputs(ifx, ef):
    import torch

    logits, reg, prop, img = bc.head(16, 120, 5)
    ref = bd.box_detections(logits, reg, prop, img, 0.05, 0.5, 30)
    d = (_cuda(logits), _cuda(reg), _cuda(prop))
    T = True
    for present in ((False, T, T, T), (T, False, T, T), (T, T, False, T), (T, T, T, False), (False, False, False, False)):
        bufs = _raw(ifx, ef, d, img, 0.05, 0.5, 30, 40, present=present)
        torch.cuda.synchronize()
        _equal(_read(bufs, 40), ref, 40, present)


def test_two_streams_and_the_shared_scratch(ifx, ef):
    """calls on two streams and the null stream with nothing in between, an ifx_nms and an ifx_rpn_proposals call among them: the handle's one buffer is laid out
    anew by each user and each call waits for the one before on the device"""
    import torch

    cases = []
    for seed, (R, Cn) in ((20, (1000, 81)), (21, (300, 3)), (22, (64, 81)), (23, (1500, 4))):
        c = bc.head(seed, R, Cn)
        cases.append((tuple(_cuda(a) for a in c[:3]), c[3], bd.box_detections(*c, 0.05, 0.5, 100)))
    obj, reg, anc, img = rc.level(24, 15, 38, 50)
    d_rpn, rpn_ref = (_cuda(obj), _cuda(reg), _cuda(anc)), rp.rpn_proposals(obj, reg, anc, img, 6000, 200, 0.7, 0)
    rng = np.random.default_rng(25)
    nb, ns = bc.proposals(rng, 700), rng.random(700).astype(F)
    d_nb, d_ns = _cuda(nb), _cuda(ns)
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    torch.cuda.synchronize()
    outs = []
    for i, (d, im, _) in enumerate(cases):
        outs.append(_raw(ifx, ef, d, im, 0.05, 0.5, 100, 100, stream=(s1, s2)[i % 2]))
        if i == 0:
            keep, count = ef.nms(d_nb, d_ns, 0.5, stream=s2, padded=True)
        if i == 2:
            rpn = ef.rpn_proposals(*d_rpn, img, 6000, 200, 0.7, 0, padded=True, stream=s1)
    outs.append(_raw(ifx, ef, cases[0][0], cases[0][1], 0.05, 0.5, 100, 100))                           # and the null stream
    torch.cuda.synchronize()
    for bufs, (_, _, ref) in zip(outs, cases + cases[:1]):
        _equal(_read(bufs, 100), ref, 100)
    kept = nms_numpy(nb, ns, 0.5)
    assert int(count.item()) == kept.size and np.array_equal(keep.cpu().numpy()[:kept.size], kept)
    assert int(rpn[3].item()) == rpn_ref[2].size and np.array_equal(rpn[2].cpu().numpy()[:rpn_ref[2].size], rpn_ref[2])


# ----------------------------------------------------------------------------------------------------------------------------------------------- interfaces

def test_refusals_leave_the_handle_usable(ifx, ef):
    import torch

    L = ifx.lib()
    logits, reg, prop, img = bc.head(30, 20, 3)
    d_logits, d_reg, d_prop = _cuda(logits), _cuda(reg), _cuda(prop)
    boxes, scores = torch.full((10, 4), -7.5, device="cuda"), torch.full((10,), -7.5, device="cuda")
    labels, index = torch.full((10,), -77, dtype=torch.int64, device="cuda"), torch.full((10,), -77, dtype=torch.int64, device="cuda")
    count, stats = torch.full((1,), -9, dtype=torch.int32, device="cuda"), torch.full((2,), -9, dtype=torch.int32, device="cuda")
    P = lambda t: C.c_void_p(t.data_ptr())

    def call(lg=P(d_logits), rg=P(d_reg), pr=P(d_prop), R=20, Cn=3, Creg=3, par=True, b=P(boxes), c=P(count), **kw):
        args = dict(img=img, st=0.05, nms=0.5, M=10, max_out=10)
        args.update(kw)
        p = _params(ifx, **args)
        return L.ifx_box_detections(ef.handle, lg, rg, pr, R, Cn, Creg, C.byref(p) if par else None, b, P(scores), P(labels), P(index), c, P(stats), None)

    nan, inf = float("nan"), float("inf")
    bad = [dict(par=False), dict(b=None), dict(c=None), dict(lg=None), dict(rg=None), dict(pr=None), dict(R=-1), dict(Cn=1, Creg=1), dict(Cn=1025, Creg=1025),
           dict(R=1 << 15, Cn=1024, Creg=1024), dict(Creg=2), dict(Creg=0), dict(max_out=0), dict(max_out=8193, M=0), dict(M=11), dict(st=nan), dict(nms=nan),
           dict(weights=(10, 0, 5, 5)), dict(weights=(10, 10, nan, 5)), dict(weights=(inf, 10, 5, 5)), dict(img=(0, 10)), dict(img=(10, 0))]
    for kw in bad:
        assert call(**kw) == E_INVALID, kw
        assert b"ifx_box_detections" in L.ifx_last_error(ef.handle)
    torch.cuda.synchronize()
    assert int(count.item()) == -9 and bool((boxes == -7.5).all()) and bool((scores == -7.5).all()) and bool((labels == -77).all()) and bool((index == -77).all())
    assert stats.tolist() == [-9, -9]                                                  # nothing was enqueued
    assert call(R=0, lg=None, rg=None, pr=None) == 0                                   # no rows: count 0, stats {0, 0} and the padding
    torch.cuda.synchronize()
    assert int(count.item()) == 0 and stats.tolist() == [0, 0] and not boxes.any() and not scores.any() and bool((labels == -1).all()) and bool((index == -1).all())
    assert call(xform_clip=nan) == 0 and call(nms=inf) == 0 and call(st=-inf) == 0 and call(M=-3) == 0 and call() == 0
    torch.cuda.synchronize()
    ref = bd.box_detections(logits, reg, prop, img, 0.05, 0.5, 10)
    pb, ps, pl, pi, c, st = bd.padded(ref, 10)
    assert int(count.item()) == c and np.array_equal(_bits(boxes.cpu().numpy()), _bits(pb)) and np.array_equal(labels.cpu().numpy(), pl)
    assert np.array_equal(index.cpu().numpy(), pi) and np.array_equal(stats.cpu().numpy(), st)


def test_python_call_cut_padded_and_argument_checks(ifx, ef):
    import torch

    logits, reg, prop, img = bc.head(31, 500, 81, scale=2.5)
    ref = bd.box_detections(logits, reg, prop, img)
    d = (_cuda(logits), _cuda(reg), _cuda(prop))
    boxes, scores, labels, index = ef.box_detections(*d, img)
    c = ref[0].shape[0]
    assert c == 100 and boxes.shape == (c, 4) and labels.dtype == torch.int64 and index.dtype == torch.int64
    assert np.array_equal(_bits(boxes.cpu().numpy()), _bits(ref[0])) and np.array_equal(_bits(scores.cpu().numpy()), _bits(ref[1]))
    assert np.array_equal(labels.cpu().numpy(), ref[2]) and np.array_equal(index.cpu().numpy(), ref[3])
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    pb, ps, pl, pi, count, stats = ef.box_detections(*d, img, max_out=150, padded=True, stream=side)
    side.synchronize()
    assert pb.shape == (150, 4) and ps.shape == (150,) and count.dtype == torch.int32 and int(count.item()) == c and stats.tolist() == [ref[4], ref[5]]
    assert torch.equal(pb[:c], boxes) and torch.equal(ps[:c], scores) and torch.equal(pl[:c], labels) and torch.equal(pi[:c], index)
    assert not pb[c:].any() and not ps[c:].any() and bool((pl[c:] == -1).all()) and bool((pi[c:] == -1).all())
    free = bd.box_detections(logits, reg, prop, img, 0.05, 0.5, 0)
    got = ef.box_detections(*d, img, detections_per_img=0)                             # max_out defaults to 8192
    assert got[0].shape[0] == free[0].shape[0] > 100 and np.array_equal(got[3].cpu().numpy(), free[3])
    e0 = ef.box_detections(d[0][:0], d[1][:0], d[2][:0], img)
    assert e0[0].shape == (0, 4) and e0[2].numel() == 0
    good = dict(class_logits=d[0], box_regression=d[1], proposals=d[2], image_size=img)
    for kw in (dict(class_logits=d[0].half()), dict(box_regression=d[1].double()), dict(proposals=d[2].int()), dict(class_logits=logits)):
        with pytest.raises(TypeError):
            ef.box_detections(**{**good, **kw})
    for kw in (dict(class_logits=d[0].cpu()), dict(box_regression=d[1].cpu()), dict(proposals=d[2].cpu()), dict(class_logits=d[0][0]), dict(class_logits=d[0][:-1]),
               dict(box_regression=d[1][:, :8]), dict(proposals=torch.zeros(500, 5, device="cuda")), dict(proposals=d[2][:-1]),
               dict(class_logits=torch.zeros(81, 500, device="cuda").t()), dict(proposals=torch.zeros(4, 500, device="cuda").t())):
        with pytest.raises(ValueError):
            ef.box_detections(**{**good, **kw})
    for kw in (dict(max_out=8193), dict(max_out=50), dict(weights=(10, 10, 0, 5)), dict(score_thresh=float("nan")), dict(image_size=(0, 5))):
        with pytest.raises(ifx.IfxError, match="ifx_box_detections"):
            ef.box_detections(**{**good, **kw})
    assert torch.equal(ef.box_detections(**good)[0], boxes)                            # and the handle goes on


class _BoxList:
    """the least of maskrcnn-benchmark's BoxList that the module needs"""
    def __init__(self, bbox, size, mode="xyxy"):
        self.bbox, self.size, self.mode, self.fields = bbox, size, mode, {}

    def __len__(self):
        return self.bbox.shape[0]

    def add_field(self, name, value):
        self.fields[name] = value

    def get_field(self, name):
        return self.fields[name]


def test_box_post_processor_two_images(ifx, ef):
    import torch

    heads = [bc.head(40, 230, 9), bc.head(41, 77, 9)]
    sizes = [(333, 217), (300, 200)]
    logits, reg = _cuda(np.concatenate([h[0] for h in heads])), _cuda(np.concatenate([h[1] for h in heads]))
    boxes = [_BoxList(_cuda(h[2]), s) for h, s in zip(heads, sizes)]
    pp = ifx.box_post_processor(ef, 0.05, 0.5, 20).eval()
    res = pp((logits, reg), boxes)
    assert len(res) == 2
    for h, s, r in zip(heads, sizes, res):
        b, sc, l, _ = ef.box_detections(_cuda(h[0]), _cuda(h[1]), _cuda(h[2]), s, 0.05, 0.5, 20)
        ref = bd.box_detections(h[0], h[1], h[2], s, 0.05, 0.5, 20)
        assert type(r) is _BoxList and r.size == s and r.mode == "xyxy" and set(r.fields) == {"scores", "labels"} and r.get_field("labels").dtype == torch.int64
        assert torch.equal(r.bbox, b) and torch.equal(r.get_field("scores"), sc) and torch.equal(r.get_field("labels"), l)
        assert len(r) == 20 and np.array_equal(_bits(b.cpu().numpy()), _bits(ref[0])) and np.array_equal(l.cpu().numpy(), ref[2])
    ag = ifx.box_post_processor(ef, 0.05, 0.5, 20, cls_agnostic_bbox_reg=True).eval()                    # the last four columns are every class's code
    res = ag((logits, reg), boxes)
    for h, s, r in zip(heads, sizes, res):
        ref = bd.box_detections(h[0], h[1][:, -4:], h[2], s, 0.05, 0.5, 20)
        assert np.array_equal(_bits(r.bbox.cpu().numpy()), _bits(ref[0])) and np.array_equal(r.get_field("labels").cpu().numpy(), ref[2])
    with pytest.raises(RuntimeError, match="inference only"):
        pp.train()((logits, reg), boxes)


def test_the_map_does_not_notice(ifx):
    """two handles through the same three frames; on one of them the call runs (null stream, side stream) between the second frame and the third: the third
    frame's pose and the map's count are those of the other"""
    import torch

    from instancefusion_amd import synth

    st = synth.make_stream(3, Q["w"], Q["h"], Q["fx"], Q["fy"], Q["cx"], Q["cy"], noise=True)
    logits, reg, prop, img = bc.head(50, 1000, 81, scale=2.5)
    ref = bd.box_detections(logits, reg, prop, img)
    results = []
    for with_calls in (False, True):
        e = ifx.ElasticFusion(**Q, max_surfels=200000)
        for i in range(2):
            e.processFrame(st["rgb"][i], st["depth"][i])
        if with_calls:
            side = torch.cuda.Stream()
            d = (_cuda(logits), _cuda(reg), _cuda(prop))
            torch.cuda.synchronize()
            a = e.box_detections(*d, img)
            b = e.box_detections(*d, img, stream=side)
            side.synchronize()
            assert np.array_equal(a[3].cpu().numpy(), ref[3]) and torch.equal(a[0], b[0]) and np.array_equal(_bits(a[0].cpu().numpy()), _bits(ref[0]))
        pose = e.processFrame(st["rgb"][2], st["depth"][2])
        results.append((np.asarray(pose).copy(), e.count, e.download()))
        e.close()
    (pa, ca, ma), (pb, cb, mb) = results
    assert np.array_equal(pa, pb) and ca == cb and ca > 0
    for k in ma:
        assert np.array_equal(ma[k], mb[k]), k
