"""The proposal stage over the levels of an FPN on the device (ifx_rpn_proposals_fpn): equal to the numpy statement (tests/rpn_fpn_numpy.py, itself held against
maskrcnn-benchmark's RPNPostProcessor.forward in test_rpn_fpn_cpu.py) bit for bit -- boxes, logits, levels, indices, the padding behind the count, the count and
the levels' counts -- on the golden cases and at the smallest shapes at which each mechanism of the level-batched kernels is exercised: levels that only sort,
one or two levels that run the radix select beside levels that do not, ties at both cuts, one level, eight levels, empty levels; guard bands, a scratch that is
reused and regrown, streams, NULL outputs, every refusal, the Python checks, the module that stands in for RPNPostProcessor, and a map that does not notice."""
import ctypes as C

import numpy as np
import pytest

import rpn_fpn_cases as fc
import rpn_fpn_numpy as rf
import rpn_proposals_cases as rc
import rpn_proposals_numpy as rp

pytestmark = pytest.mark.gpu

E_INVALID = -1
F = np.float32
Q = dict(w=160, h=120, fx=132.0, fy=132.0, cx=80.0, cy=60.0)
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


def _cuda(a):
    import torch

    return torch.from_numpy(np.array(a, order="C")).cuda()                              # (a copy: the shared references are read-only)


def _dev(levels):
    return [tuple(_cuda(a) for a in lv) for lv in levels]


def _bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def _params(ifx, img, pre, post, thr, min_size, weights=(1, 1, 1, 1), xform_clip=0.0):
    p = ifx.RpnParams()
    p.pre_nms_top_n, p.post_nms_top_n, p.nms_thresh, p.min_size = int(pre), int(post), float(thr), float(min_size)
    p.weights[:] = [float(v) for v in weights]
    p.xform_clip = xform_clip
    p.image_w, p.image_h = int(img[0]), int(img[1])
    return p


def _table(ifx, d_levels):
    lv = (ifx.RpnLevel * max(len(d_levels), 1))()
    for l, (o, r, a) in enumerate(d_levels):
        lv[l].objectness, lv[l].regression, lv[l].anchors = o.data_ptr() or None, r.data_ptr() or None, a.data_ptr() or None
        lv[l].A, lv[l].H, lv[l].W = (int(v) for v in o.shape)
    return lv


FILLS = (-7.5, -7.5, -77, -77, -77, -77)


def _raw(ifx, ef, d_levels, img, pre, post, thr, min_size, Fn, stream=None, use=(True, True, True, True)):
    """ifx_rpn_proposals_fpn itself, every output inside guard bands: returns the torch buffers (read them with _read once the stream is done).
    use: whether d_logits, d_level, d_index, d_level_counts are given"""
    import torch

    L = len(d_levels)
    bufs = [torch.full((2 * GUARD + 4 * Fn,), -7.5, device="cuda"), torch.full((2 * GUARD + Fn,), -7.5, device="cuda"),
            torch.full((2 * GUARD + Fn,), -77, dtype=torch.int32, device="cuda"), torch.full((2 * GUARD + Fn,), -77, dtype=torch.int64, device="cuda"),
            torch.full((2 * GUARD + 1,), -77, dtype=torch.int32, device="cuda"), torch.full((2 * GUARD + L,), -77, dtype=torch.int32, device="cuda")]
    ptr = [C.c_void_p(b.data_ptr() + GUARD * b.element_size()) for b in bufs]
    if stream is not None:
        stream.wait_stream(torch.cuda.current_stream())                                # (the fills above are on the current stream)
    p = _params(ifx, img, pre, post, thr, min_size)
    r = ef.L.ifx_rpn_proposals_fpn(ef.handle, _table(ifx, d_levels), L, C.byref(p), Fn, ptr[0], ptr[1] if use[0] else None, ptr[2] if use[1] else None,
                                   ptr[3] if use[2] else None, ptr[4], ptr[5] if use[3] else None, C.c_void_p(stream.cuda_stream) if stream is not None else None)
    assert r == 0, ef.L.ifx_last_error(ef.handle)
    return bufs


def _read(bufs, Fn):
    """(boxes [F,4], logits [F], level [F], index [F], count, level_counts [L]) out of _raw's buffers; the guard bands must be as they were"""
    host = [b.cpu().numpy() for b in bufs]
    for h, fill in zip(host, FILLS):
        assert (h[:GUARD] == fill).all() and (h[-GUARD:] == fill).all()
    return host[0][GUARD:-GUARD].reshape(Fn, 4), host[1][GUARD:-GUARD], host[2][GUARD:-GUARD], host[3][GUARD:-GUARD], int(host[4][GUARD]), host[5][GUARD:-GUARD]


def _equal(got, ref, Fn):
    """the device's padded outputs against the statement's result, bit for bit"""
    boxes, logits, level, index, count, level_counts = got
    pb, pl, pv, pi, c, lc = rf.padded(ref, Fn)
    assert count == c, (count, c)
    assert np.array_equal(level_counts, lc), (level_counts, lc)
    assert np.array_equal(level, pv), int((level != pv).sum())
    assert np.array_equal(index, pi), int((index != pi).sum())
    assert np.array_equal(_bits(boxes), _bits(pb)), int((_bits(boxes) != _bits(pb)).sum())
    assert np.array_equal(_bits(logits), _bits(pl))


def _check(ifx, ef, name, levels, img, pre, post, thr, min_size, Fn):
    import torch

    bufs = _raw(ifx, ef, _dev(levels), img, pre, post, thr, min_size, Fn)
    torch.cuda.synchronize()
    ref = fc.statement(name, levels, img, pre, post, thr, min_size, Fn)
    _equal(_read(bufs, Fn), ref, Fn)
    return ref


# ------------------------------------------------------------------------------------------------------------------------------------------------ the kernels

def test_golden_cases(ifx, ef):
    g = fc.golden()
    for k in range(int(g["counts"][0])):
        levels, img, pre, post, thr, min_size, Fn = fc.golden_case(k)
        ref = _check(ifx, ef, f"golden{k}", levels, img, pre, post, thr, min_size, Fn)
        assert np.array_equal(ref[2], g[f"fpn{k}_level"]) and np.array_equal(ref[3], g[f"fpn{k}_index"])


def test_levels_that_only_sort(ifx, ef):
    levels, img = fc.pyramid(100, [(3, 12, 16), (3, 6, 8), (3, 3, 4), (3, 2, 2), (3, 1, 1)])
    ref = _check(ifx, ef, "sort_only", levels, img, 300, 40, 0.7, 0, 50)
    assert ref[0].shape[0] == 50 and ref[4][0] == 40 and len(set(ref[2].tolist())) >= 3


@pytest.mark.parametrize("first", [True, False])
def test_one_selecting_level_among_small_ones(ifx, ef, first):
    """8736 > 8192 anchors: that level runs the radix select; the blocks of the other levels' rows of the same launches must leave it untouched"""
    shapes = [(3, 56, 52), (3, 6, 8), (1, 1, 1)]
    levels, img = fc.pyramid(110, shapes)
    if not first:
        levels = levels[::-1]
    ref = _check(ifx, ef, f"one_select_{first}", levels, img, 1000, 200, 0.7, 0, 300)
    assert levels[0 if first else 2][0].size == 8736 and ref[4][0 if first else 2] == 200 and ref[4][2 if first else 0] == 1


def test_two_selecting_levels_with_different_block_counts(ifx, ef):
    """5 and 8 blocks of 2048 keys: histograms, state or per-block counts shared between levels, or a grid sized by the wrong level, show here"""
    for shapes in ([(3, 64, 48), (3, 60, 80)], [(3, 60, 80), (3, 6, 8), (3, 64, 48)]):
        assert sorted(-(-A * H * W // 2048) for A, H, W in shapes if A * H * W > 8192) == [5, 8]
        levels, img = fc.pyramid(120, shapes)
        ref = _check(ifx, ef, f"two_select_{len(shapes)}", levels, img, 1000, 300, 0.7, 0, 500)
        assert ref[0].shape[0] == 500 and (ref[4] > 0).all()


def test_ties_at_both_cuts(ifx, ef):
    """thousands of equal logits span the pre_nms_top_n boundary of a selecting level (the lowest anchor indices win), and equal logits of two levels span the
    cut at F (the lower level, then the lower row, wins); threshold 2: nothing is suppressed, the selections themselves come out"""
    levels, img = fc.pyramid(130, [(3, 56, 52), (3, 12, 16)])
    levels = [(np.clip(np.round(o), -4, 6).astype(F), r, a) for o, r, a in levels]
    lg = rp.flatten(levels[0][0], levels[0][1])[0]
    last = np.sort(lg)[::-1][999]
    assert (lg == last).sum() > 1000 and (lg > last).sum() < 1000
    full = fc.statement("ties_full", levels, img, 1000, 400, 2.0, 0, 8192)
    cut = [i + 1 for i in range(full[1].size - 1) if full[1][i] == full[1][i + 1] and full[2][i] != full[2][i + 1]]
    assert cut and full[4].tolist() == [400, 400]
    for Fn in (cut[0], cut[-1], cut[0] + 1):
        ref = _check(ifx, ef, f"ties_{Fn}", levels, img, 1000, 400, 2.0, 0, Fn)
        assert np.array_equal(ref[2], full[2][:Fn]) and np.array_equal(ref[3], full[3][:Fn])
    flat = [(np.full_like(o, 0.25), r, a) for o, r, a in levels]                       # every logit equal: level 0's first anchors alone
    ref = _check(ifx, ef, "ties_flat", flat, img, 1000, 400, 2.0, 0, 300)
    assert (ref[2] == 0).all() and np.array_equal(ref[3], np.arange(300))
    nans = [(np.full_like(levels[0][0], np.nan), levels[0][1], levels[0][2]), levels[1]]     # a level of NaN logits lies behind the numbers of the next one
    ref = _check(ifx, ef, "ties_nan", nans, img, 1000, 400, 2.0, 0, 600)
    assert (ref[2][:400] == 1).all() and (ref[2][400:] == 0).all() and np.array_equal(ref[3][400:], np.arange(200))


def test_one_level_is_the_single_level_call(ifx, ef):
    import torch

    for seed, shape, pre in ((140, (3, 9, 11), 200), (141, (3, 56, 52), 1000)):
        obj, reg, anc, img = rc.level(seed, *shape)
        ref = _check(ifx, ef, f"one_level_{seed}", [(obj, reg, anc)], img, pre, 60, 0.7, 0, 60)
        assert (ref[2] == 0).all() and ref[4].tolist() == [ref[0].shape[0]]
        b, s, i, n = ef.rpn_proposals(_cuda(obj), _cuda(reg), _cuda(anc), img, pre, 60, 0.7, 0, padded=True)
        fb, fs, fl, fi, fn, _ = ef.rpn_proposals_fpn([_cuda(obj)], [_cuda(reg)], [_cuda(anc)], img, pre, 60, 0.7, 0, padded=True)
        assert torch.equal(b, fb) and torch.equal(s, fs) and torch.equal(i, fi) and torch.equal(n, fn)


def test_eight_tiny_levels_and_empty_ones(ifx, ef):
    import torch

    levels, img = fc.pyramid(150, [(3, 5, 6), (3, 3, 3), (1, 2, 2), (3, 1, 2), (1, 1, 1), (3, 1, 1), (2, 1, 1), (1, 1, 1)])
    ref = _check(ifx, ef, "eight", levels, img, 50, 20, 0.7, 0, 30)
    assert ref[4].size == 8 and (ref[4] > 0).all()
    levels, img = fc.pyramid(160, [(3, 8, 9), (3, 0, 5), (3, 2, 3)])                 # H = 0 in the middle
    ref = _check(ifx, ef, "empty_middle", levels, img, 100, 30, 0.7, 0, 40)
    assert ref[4][1] == 0 and ref[4][0] > 0 and ref[4][2] > 0 and 1 not in ref[2]
    levels, img = fc.pyramid(170, [(3, 0, 5), (1, 4, 0), (0, 3, 3)])                 # all levels empty: count 0 and the padding only
    ref = _check(ifx, ef, "all_empty", levels, img, 100, 30, 0.7, 0, 40)
    assert ref[0].shape[0] == 0 and not ref[4].any()
    d = _dev(levels)
    b, s, v, i = ef.rpn_proposals_fpn([x[0] for x in d], [x[1] for x in d], [x[2] for x in d], img, 100, 30)
    assert b.shape == (0, 4) and s.numel() == 0 and v.dtype == torch.int32 and i.dtype == torch.int64


def test_a_full_level_beside_a_nearly_empty_one(ifx, ef):
    """c_l == post_nms_top_n in one level, c_l < 5 in another; F below, at and above T"""
    levels, img = fc.pyramid(180, [(3, 12, 16), (3, 6, 8), (3, 1, 1)])
    full = fc.statement("quota_full", levels, img, 300, 25, 0.7, 0, 8192)
    T = int(full[4].sum())
    assert full[4][0] == 25 and 0 < full[4][2] < 5
    for Fn in (T - 9, T, T + 9):
        ref = _check(ifx, ef, f"quota_{Fn}", levels, img, 300, 25, 0.7, 0, Fn)
        assert ref[0].shape[0] == min(Fn, T)


def test_a_b_a_on_one_handle(ifx, ef):
    """three calls with different level sets: the first and the third result are identical in every bit (the zeroed words are zeroed by each call; the scratch
    grows for B and is carved anew for A)"""
    import torch

    a_levels, a_img = fc.pyramid(190, [(3, 64, 48), (3, 6, 8)])
    b_levels, b_img = fc.pyramid(191, [(3, 6, 8), (3, 60, 80), (3, 56, 52), (1, 3, 3)])
    da, db = _dev(a_levels), _dev(b_levels)
    one = _raw(ifx, ef, da, a_img, 1000, 100, 0.7, 0, 150)
    two = _raw(ifx, ef, db, b_img, 2000, 200, 0.7, 0, 333)
    three = _raw(ifx, ef, da, a_img, 1000, 100, 0.7, 0, 150)
    torch.cuda.synchronize()
    for x, y in zip(one, three):
        assert torch.equal(x, y)
    _equal(_read(one, 150), fc.statement("aba_a", a_levels, a_img, 1000, 100, 0.7, 0, 150), 150)
    _equal(_read(two, 333), fc.statement("aba_b", b_levels, b_img, 2000, 200, 0.7, 0, 333), 333)


def test_two_streams_back_to_back(ifx, ef):
    """calls on two streams with nothing in between share the handle's scratch: each waits for the one before on the device"""
    import torch

    cases = []
    for i, shapes in enumerate(([(3, 64, 48), (3, 6, 8)], [(3, 12, 16), (3, 6, 8), (3, 3, 4)], [(3, 6, 8), (3, 56, 52)], [(1, 9, 9)])):
        levels, img = fc.pyramid(200 + 10 * i, shapes)
        cases.append((_dev(levels), img, fc.statement(f"streams{i}", levels, img, 1000, 100, 0.7, 0, 120)))
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    torch.cuda.synchronize()
    outs = [_raw(ifx, ef, d, img, 1000, 100, 0.7, 0, 120, stream=(s1, s2)[i % 2]) for i, (d, img, _) in enumerate(cases)]
    outs.append(_raw(ifx, ef, cases[0][0], cases[0][1], 1000, 100, 0.7, 0, 120))                     # and the null stream
    torch.cuda.synchronize()
    for bufs, (_, _, ref) in zip(outs, cases + cases[:1]):
        _equal(_read(bufs, 120), ref, 120)


def test_null_outputs(ifx, ef):
    import torch

    levels, img = fc.pyramid(240, [(3, 9, 11), (3, 5, 6)])
    ref = fc.statement("null_outputs", levels, img, 200, 40, 0.7, 0, 90)
    pb, pl, pv, pi, c, lc = rf.padded(ref, 90)
    assert c < 90
    d = _dev(levels)
    for use in ((False, True, True, True), (True, False, True, True), (True, True, False, True), (True, True, True, False), (False, False, False, False)):
        bufs = _raw(ifx, ef, d, img, 200, 40, 0.7, 0, 90, use=use)
        torch.cuda.synchronize()
        boxes, lg, level, idx, count, counts = _read(bufs, 90)
        assert count == c and np.array_equal(_bits(boxes), _bits(pb))
        assert np.array_equal(_bits(lg), _bits(pl)) if use[0] else (lg == -7.5).all()
        assert np.array_equal(level, pv) if use[1] else (level == -77).all()
        assert np.array_equal(idx, pi) if use[2] else (idx == -77).all()
        assert np.array_equal(counts, lc) if use[3] else (counts == -77).all()


# ----------------------------------------------------------------------------------------------------------------------------------------------- interfaces

def test_refusals_leave_the_handle_usable(ifx, ef):
    import torch

    L = ifx.lib()
    levels, img = fc.pyramid(250, [(3, 4, 5), (3, 2, 3)])
    d = _dev(levels)
    boxes, logits, level = torch.full((10, 4), -7.5, device="cuda"), torch.zeros(10, device="cuda"), torch.zeros(10, dtype=torch.int32, device="cuda")
    index, count = torch.zeros(10, dtype=torch.int64, device="cuda"), torch.full((1,), -9, dtype=torch.int32, device="cuda")
    counts = torch.full((8,), -9, dtype=torch.int32, device="cuda")
    P = lambda t: C.c_void_p(t.data_ptr())

    def call(n_levels=2, Fn=10, tab=True, par=True, b=P(boxes), c=P(count), edit=None, **kw):
        args = dict(img=img, pre=50, post=10, thr=0.7, min_size=0.0)
        args.update(kw)
        p = _params(ifx, **args)
        lv = (ifx.RpnLevel * 9)()
        for l, e in enumerate(_table(ifx, d)):
            lv[l] = e
        for l in range(2, 9):
            lv[l] = lv[1]
        if edit:
            setattr(lv[edit[0]], edit[1], edit[2])
        return L.ifx_rpn_proposals_fpn(ef.handle, lv if tab else None, n_levels, C.byref(p) if par else None, Fn, b, P(logits), P(level), P(index), c, P(counts), None)

    nan, inf = float("nan"), float("inf")
    bad = [dict(n_levels=0), dict(n_levels=9), dict(n_levels=-1), dict(Fn=0), dict(Fn=8193), dict(tab=False), dict(par=False), dict(b=None), dict(c=None),
           dict(edit=(0, "objectness", None)), dict(edit=(1, "regression", None)), dict(edit=(1, "anchors", None)), dict(edit=(0, "A", -1)), dict(edit=(1, "H", -1)),
           dict(edit=(1, "W", -1)), dict(edit=(1, "A", 4096 * 4096 * 2)), dict(edit=(1, "H", 1 << 23)),
           dict(pre=0), dict(pre=8193), dict(post=0), dict(post=8193), dict(thr=nan), dict(weights=(1, 0, 1, 1)), dict(weights=(1, 1, nan, 1)), dict(weights=(inf, 1, 1, 1)),
           dict(img=(0, 10)), dict(img=(10, 0))]
    for kw in bad:
        assert call(**kw) == E_INVALID, kw
        assert b"ifx_rpn_proposals_fpn" in L.ifx_last_error(ef.handle)
    torch.cuda.synchronize()
    assert int(count.item()) == -9 and bool((boxes == -7.5).all()) and bool((counts == -9).all())     # nothing was enqueued
    assert call(edit=(1, "H", 0)) == 0                                                 # a level without anchors: its pointers are not looked at
    assert call(n_levels=8) == 0 and call(xform_clip=nan) == 0 and call(thr=inf) == 0 and call() == 0
    torch.cuda.synchronize()
    ref = rf.rpn_proposals_fpn(levels, img, 50, 10, 0.7, 0, 10)
    assert int(count.item()) == 10 and np.array_equal(_bits(boxes.cpu().numpy()), _bits(ref[0])) and np.array_equal(level.cpu().numpy(), ref[2])
    assert np.array_equal(counts.cpu().numpy()[:2], ref[4])


def test_python_argument_checks(ifx, ef):
    import torch

    obj = [torch.zeros(3, 4, 5, device="cuda"), torch.zeros(3, 2, 3, device="cuda")]
    reg = [torch.zeros(12, 4, 5, device="cuda"), torch.zeros(12, 2, 3, device="cuda")]
    anc = [torch.zeros(60, 4, device="cuda"), torch.zeros(18, 4, device="cuda")]
    good = dict(objectness=obj, box_regression=reg, anchors=anc, image_size=(80, 64))
    sub = lambda lst, t: [lst[0], t]
    for kw in (dict(objectness=sub(obj, obj[1].half())), dict(box_regression=sub(reg, reg[1].double())), dict(anchors=sub(anc, anc[1].int())),
               dict(objectness=sub(obj, obj[1].cpu().numpy()))):
        with pytest.raises(TypeError):
            ef.rpn_proposals_fpn(**{**good, **kw})
    for kw in (dict(objectness=sub(obj, obj[1].cpu())), dict(box_regression=sub(reg, reg[1].cpu())), dict(anchors=sub(anc, anc[1].cpu())), dict(objectness=obj[:1]),
               dict(box_regression=reg + reg[:1]), dict(anchors=anc[:1]), dict(objectness=[], box_regression=[], anchors=[]), dict(objectness=sub(obj, obj[1][0])),
               dict(objectness=sub(obj, torch.zeros(2, 3, 2, 3, device="cuda"))), dict(box_regression=sub(reg, torch.zeros(11, 2, 3, device="cuda"))),
               dict(anchors=sub(anc, torch.zeros(17, 4, device="cuda"))), dict(anchors=sub(anc, torch.zeros(18, 5, device="cuda"))),
               dict(objectness=sub(obj, torch.zeros(3, 3, 2, device="cuda").transpose(1, 2))), dict(anchors=sub(anc, torch.zeros(4, 18, device="cuda").t()))):
        with pytest.raises(ValueError):
            ef.rpn_proposals_fpn(**{**good, **kw})
    with pytest.raises(ifx.IfxError):
        ef.rpn_proposals_fpn(**good, pre_nms_top_n=8193)
    with pytest.raises(ifx.IfxError):
        ef.rpn_proposals_fpn(**good, fpn_post_nms_top_n=0)
    with pytest.raises(ifx.IfxError):
        ef.rpn_proposals_fpn(obj * 5, reg * 5, anc * 5, (80, 64))                       # ten levels
    assert ef.rpn_proposals_fpn(**good)[0].shape[1] == 4                              # and the handle goes on


def test_python_call_padded_and_cut(ifx, ef):
    import torch

    levels, img = fc.pyramid(260, [(3, 12, 17), (3, 6, 9), (3, 3, 5)])
    ref = fc.statement("python_call", levels, img, 400, 60, 0.3, 0, 200)
    d = _dev(levels)
    o, r, a = [x[0] for x in d], [x[1] for x in d], [x[2] for x in d]
    boxes, score, level, index = ef.rpn_proposals_fpn(o, r, a, img, 400, 60, 0.3, 0, 200)
    c = ref[0].shape[0]
    assert 0 < c < 200 and boxes.shape == (c, 4) and score.shape == (c,) and level.dtype == torch.int32 and index.dtype == torch.int64
    assert np.array_equal(_bits(boxes.cpu().numpy()), _bits(ref[0])) and np.array_equal(level.cpu().numpy(), ref[2]) and np.array_equal(index.cpu().numpy(), ref[3])
    assert torch.equal(score, torch.sigmoid(_cuda(ref[1])))
    pb, ps, pv, pi, count, counts = ef.rpn_proposals_fpn([x[None] for x in o], [x[None] for x in r], a, img, 400, 60, 0.3, 0, 200, padded=True)      # [1,A,H,W] too
    assert pb.shape == (200, 4) and ps.shape == (200,) and pv.shape == (200,) and pi.shape == (200,) and int(count.item()) == c
    assert count.dtype == torch.int32 and np.array_equal(counts.cpu().numpy(), ref[4])
    assert torch.equal(pb[:c], boxes) and torch.equal(ps[:c], score) and torch.equal(pv[:c], level) and torch.equal(pi[:c], index)
    assert not pb[c:].any() and bool((ps[c:] == 0.5).all()) and bool((pv[c:] == -1).all()) and bool((pi[c:] == -1).all())      # sigmoid(0) behind the count
    b2, _, v2, i2 = ef.rpn_proposals_fpn(o, r, a, img, pre_nms_top_n=400, post_nms_top_n=60, nms_thresh=0.3)          # fpn_post_nms_top_n None: post_nms_top_n
    assert b2.shape[0] == 60 and torch.equal(b2, boxes[:60]) and torch.equal(v2, level[:60]) and torch.equal(i2, index[:60])


class _BoxList:
    """the least of maskrcnn-benchmark's BoxList that the module needs"""
    def __init__(self, bbox, size, mode="xyxy"):
        self.bbox, self.size, self.mode, self.fields = bbox, size, mode, {}

    def add_field(self, name, value):
        self.fields[name] = value

    def get_field(self, name):
        return self.fields[name]


def test_rpn_post_processor_three_levels_two_images(ifx, ef):
    import torch

    shapes = [(3, 12, 16), (3, 6, 8), (3, 3, 4)]
    images = [fc.pyramid(270 + 10 * i, shapes) for i in range(2)]
    size = images[0][1]
    mod = ifx.rpn_post_processor(ef, 300, 40, 0.7, 0, fpn_post_nms_top_n=70).eval()
    anchors = [[_BoxList(_cuda(lv[2]), size) for lv in levels] for levels, _ in images]
    objectness = [_cuda(np.stack([images[i][0][l][0] for i in range(2)])) for l in range(3)]
    regression = [_cuda(np.stack([images[i][0][l][1] for i in range(2)])) for l in range(3)]
    res = mod(anchors, objectness, regression, targets=None)
    assert len(res) == 2
    for i, r in enumerate(res):
        ref = fc.statement(f"module{i}", images[i][0], size, 300, 40, 0.7, 0, 70)
        assert ref[0].shape[0] == 70
        assert type(r) is _BoxList and r.size == size and r.mode == "xyxy" and set(r.fields) == {"objectness"}
        assert np.array_equal(_bits(r.bbox.cpu().numpy()), _bits(ref[0])) and torch.equal(r.get_field("objectness"), torch.sigmoid(_cuda(ref[1])))
    with pytest.raises(RuntimeError, match="inference only"):
        mod.train()(anchors, objectness, regression)


def test_the_map_does_not_notice(ifx):
    """two handles through the same three frames; on one of them the call runs (null stream, side stream) between the second frame and the third: the third
    frame's pose and the map's count are those of the other"""
    import torch

    from instancefusion_amd import synth

    st = synth.make_stream(3, Q["w"], Q["h"], Q["fx"], Q["fy"], Q["cx"], Q["cy"], noise=True)
    levels, img = fc.pyramid(290, [(3, 56, 52), (3, 12, 16), (3, 3, 4)])
    ref = fc.statement("map", levels, img, 1000, 200, 0.7, 0, 300)
    results = []
    for with_calls in (False, True):
        e = ifx.ElasticFusion(**Q, max_surfels=200000)
        for i in range(2):
            e.processFrame(st["rgb"][i], st["depth"][i])
        if with_calls:
            side = torch.cuda.Stream()
            d = _dev(levels)
            args = ([x[0] for x in d], [x[1] for x in d], [x[2] for x in d], img, 1000, 200, 0.7, 0, 300)
            torch.cuda.synchronize()
            a = e.rpn_proposals_fpn(*args)
            b = e.rpn_proposals_fpn(*args, stream=side)
            side.synchronize()
            assert np.array_equal(a[3].cpu().numpy(), ref[3]) and np.array_equal(a[2].cpu().numpy(), ref[2]) and torch.equal(a[0], b[0])
            assert np.array_equal(_bits(a[0].cpu().numpy()), _bits(ref[0]))
        pose = e.processFrame(st["rgb"][2], st["depth"][2])
        results.append((np.asarray(pose).copy(), e.count, e.download()))
        e.close()
    (pa, ca, ma), (pb, cb, mb) = results
    assert np.array_equal(pa, pb) and ca == cb and ca > 0
    for k in ma:
        assert np.array_equal(ma[k], mb[k]), k
