"""ifx_keras_proposals on the device (ProposalLayer.call of the Keras Mask R-CNN): equal to the numpy statement (tests/keras_layers_numpy.py) bit for bit -- boxes,
indices, count and the padding behind the count, compared as uint32 -- at the sizes where the selection changes path (n <= 8192: one sort; above: the radix select
with the score's stride), at the reference's size, on directed cases (ties at the K-th place, NaN and -0 scores, the proposal count reached inside a 64-box block
and at its end, everything and nothing suppressed, boxes clipped to zero area, deltas that overflow EXP); guard bands, a NULL index, streams that share the scratch
with ifx_nms and ifx_rpn_proposals, every refusal, the Python method.  Every case's background column is larger than its foreground column: the stride check."""
import ctypes as C

import numpy as np
import pytest

import keras_layers_gpu as kg
import keras_layers_numpy as kl
from keras_layers_gpu import F, cuda

pytestmark = pytest.mark.gpu

IMG = (1024, 1024)


@pytest.fixture(scope="module")
def ifx():
    import instancefusion_amd as m

    m.lib()
    return m


@pytest.fixture(scope="module")
def ef(ifx):
    """a handle that never sees a frame: the calls need none"""
    e = ifx.ElasticFusion(**kg.Q, max_surfels=100000)
    yield e
    e.close()


def _check(ifx, ef, case, pre, count, thr, image=IMG, index=True):
    import torch

    probs, bbox, anc = case
    bufs = kg.raw_proposals(ifx, ef, cuda(probs), cuda(bbox), cuda(anc), image, pre, count, thr, index=index)
    torch.cuda.synchronize()
    ref = kl.keras_proposals(probs, bbox, anc, image, pre, count, thr)
    boxes, idx, c = kg.read_proposals(bufs, count)
    if not index:
        assert (idx == -77).all()
    kg.proposals_equal((boxes, idx if index else None, c), ref, count)
    return ref


@pytest.mark.parametrize("n,pre,count", [(50, 6000, 100), (8192, 6000, 300), (8193, 6000, 300), (65472, 6000, 1000)])
def test_sizes(ifx, ef, n, pre, count):
    """everything selected and fewer survivors than proposal_count (zero rows, -1 indices); the selection's two paths; the reference's configuration"""
    ref = _check(ifx, ef, kg.proposal_case(n, n), pre, count, 0.7)
    assert 0 < ref[0].shape[0] < count if n == 50 else ref[0].shape[0] == count         # (n == 50: fewer survivors than rows; else the walk stops at the count)


@pytest.mark.parametrize("n,pre", [(500, 100), (9000, 100), (20000, 6000)])
def test_equal_scores_straddle_the_kth_place(ifx, ef, n, pre):
    """eight distinct scores: the K-th place lies inside a run of equal ones, of which the lower indices win (tf.nn.top_k)"""
    case = kg.proposal_case(n + 1, n, quantise=8)
    ref = _check(ifx, ef, case, pre, 200, 0.7)
    order = np.lexsort((np.arange(n), -case[0][:, 1]))[:pre]
    assert (case[0][np.setdiff1d(np.arange(n), order), 1] == case[0][order[-1], 1]).any()      # an equal score was left out
    assert set(ref[1]) <= set(order)


@pytest.mark.parametrize("n,pre", [(50, 50), (8200, 8192)])
def test_nan_and_negative_zero_scores(ifx, ef, n, pre):
    """a NaN lies behind every number, -0 equals +0 (the lower index first); with 20 NaNs and 8 places too few the NaNs of the lowest indices are selected"""
    probs, bbox, anc = kg.proposal_case(7 * n, n)
    rng = np.random.default_rng(n)
    probs[:, 1] -= F(0.5)                                                   # negative numbers too
    where = rng.choice(n, 30, replace=False)
    probs[where[:20], 1] = np.nan
    probs[where[20:25], 1] = F(-0.0)
    probs[where[25:], 1] = F(0.0)
    ref = _check(ifx, ef, (probs, bbox, anc), pre, min(n, 8192), 1.5)       # nothing is suppressed: the output is the selection in its order
    assert ref[1].size == pre
    zeros = [i for i in ref[1] if probs[i, 1] == 0]
    assert zeros == sorted(where[20:].tolist())
    nans = [i for i in ref[1] if np.isnan(probs[i, 1])]
    assert nans == sorted(where[:20].tolist())[:len(nans)] and ref[1][-len(nans):].tolist() == nans and len(nans) == (20 if n == 50 else 12)


def _grid_case(n, size=8.0, pitch=16.0, per_row=32):
    """n disjoint anchors on a grid, zero deltas, descending scores: nothing is suppressed"""
    k = np.arange(n)
    y, x = (k // per_row) * pitch, (k % per_row) * pitch
    anc = np.stack([y, x, y + size, x + size], axis=1).astype(F)
    fg = (1.0 - k / (2.0 * n)).astype(F)
    return np.stack([fg + F(2), fg], axis=1).astype(F), np.zeros((n, 4), F), anc


@pytest.mark.parametrize("count", [64, 70, 128, 300, 400])
def test_nothing_suppressed_and_the_count_inside_a_block_and_at_its_end(ifx, ef, count):
    """300 disjoint boxes: proposal_count reached exactly at the end of a 64-box block (64, 128), inside one (70), by the last box (300), never (400)"""
    ref = _check(ifx, ef, _grid_case(300), 6000, count, 0.7)
    assert ref[1].tolist() == list(range(min(count, 300)))


def test_everything_suppressed_by_one_box(ifx, ef):
    probs, bbox, anc = _grid_case(700)
    anc[:] = np.asarray([100, 100, 300, 260], F)
    anc[1:, 2] += np.linspace(0, 3, 699).astype(F)                          # near copies: IoU above 0.98 with the first
    ref = _check(ifx, ef, (probs, bbox, anc), 6000, 100, 0.7)
    assert ref[1].tolist() == [0]


def test_boxes_clipped_to_zero_area_are_all_kept(ifx, ef):
    """anchors wholly outside the image clip to lines and points on its border: area 0, IoU 0, nothing suppresses anything"""
    probs, bbox, anc = _grid_case(200)
    anc[:, [0, 2]] -= F(5000)
    anc[100:] = anc[0]                                                      # a hundred identical ones among them
    ref = _check(ifx, ef, (probs, bbox, anc), 6000, 150, 0.7)
    assert ref[1].tolist() == list(range(150)) and (ref[0][:, 0] == 0).all() and (ref[0][:, 2] == 0).all()


def test_deltas_that_overflow_exp(ifx, ef):
    """log-scale deltas of +-600 (times 0.2: beyond EXP's clamps): infinite and zero sizes, NaN corners that stay NaN through clip and division"""
    probs, bbox, anc = kg.proposal_case(3, 600)
    bbox[::3, 2] = F(600)
    bbox[1::3, 3] = F(-600)
    bbox[5::7, 2:] = F(600)
    ref = _check(ifx, ef, (probs, bbox, anc), 6000, 300, 0.7)
    assert np.isnan(ref[0]).any()


def test_null_index(ifx, ef):
    _check(ifx, ef, kg.proposal_case(11, 3000), 1000, 100, 0.7, index=False)


def test_streams_share_the_scratch_with_nms_and_rpn_proposals(ifx, ef):
    """calls on a side stream back to back with ifx_nms and ifx_rpn_proposals on another, nothing in between: each waits on the device for the scratch's last user"""
    import torch

    import rpn_proposals_cases as rc
    import rpn_proposals_numpy as rp
    from detector_ops_numpy import nms

    cases = [kg.proposal_case(21, 9000), kg.proposal_case(22, 700), kg.proposal_case(23, 20000)]
    refs = [kl.keras_proposals(*c, IMG, 6000, 200, 0.7) for c in cases]
    dev = [tuple(cuda(a) for a in c) for c in cases]
    obj, reg, anc, img = rc.level(8, 15, 38, 50)
    rref = rp.rpn_proposals(obj, reg, anc, img, 6000, 200, 0.7, 0)
    d_rpn = (cuda(obj), cuda(reg), cuda(anc))
    rng = np.random.default_rng(4)
    c0 = rng.uniform(0, 300, (3000, 2))
    nb = np.concatenate([c0, c0 + rng.uniform(5, 80, (3000, 2))], axis=1).astype(F)
    ns = rng.random(3000).astype(F)
    d_nb, d_ns = cuda(nb), cuda(ns)
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    torch.cuda.synchronize()
    out = []
    out.append(kg.raw_proposals(ifx, ef, *dev[0], IMG, 6000, 200, 0.7, stream=s1))
    keep = ef.nms(d_nb, d_ns, 0.5, stream=s2, padded=True)
    out.append(kg.raw_proposals(ifx, ef, *dev[1], IMG, 6000, 200, 0.7, stream=s1))
    rpn = ef.rpn_proposals(*d_rpn, img, 6000, 200, 0.7, 0, padded=True, stream=s2)
    out.append(kg.raw_proposals(ifx, ef, *dev[2], IMG, 6000, 200, 0.7, stream=s1))
    out.append(kg.raw_proposals(ifx, ef, *dev[0], IMG, 6000, 200, 0.7))                  # NULL: the handle's main stream
    torch.cuda.synchronize()
    for bufs, ref in zip(out, refs + refs[:1]):
        kg.proposals_equal(kg.read_proposals(bufs, 200), ref, 200)
    k = keep[0].cpu().numpy()[:int(keep[1].item())]
    assert np.array_equal(k, nms(nb, ns, 0.5))
    c = int(rpn[3].item())
    assert c == rref[0].shape[0] and np.array_equal(rpn[2].cpu().numpy()[:c], rref[2])


def test_python_method_padded_cut_batched_and_out(ifx, ef):
    import torch

    case = kg.proposal_case(31, 5000)
    ref = kl.keras_proposals(*case, IMG, 6000, 400, 0.7)
    d = tuple(cuda(a) for a in case)
    boxes, index = ef.keras_proposals(*d, IMG, proposal_count=400)
    kg.same_floats(boxes.cpu().numpy(), ref[0])
    assert np.array_equal(index.cpu().numpy(), ref[1])
    buf = torch.full((2 * kg.GUARD + 1600,), -7.5, device="cuda")
    out = buf[kg.GUARD:-kg.GUARD].view(400, 4)
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    pb, pi, count = ef.keras_proposals(*d, IMG, proposal_count=400, out=out, padded=True, stream=side)
    side.synchronize()
    assert pb is out
    kg.proposals_equal((kg.payload(buf, -7.5).reshape(400, 4), pi.cpu().numpy(), int(count.item())), ref, 400)
    case2 = kg.proposal_case(32, 5000)
    ref2 = kl.keras_proposals(case2[0], case2[1], case[2], IMG, 6000, 400, 0.7)
    bb, bi, bc = ef.keras_proposals(cuda(np.stack([case[0], case2[0]])), cuda(np.stack([case[1], case2[1]])), d[2], IMG, proposal_count=400)
    assert tuple(bb.shape) == (2, 400, 4) and tuple(bi.shape) == (2, 400) and tuple(bc.shape) == (2,)
    for k, r in enumerate((ref, ref2)):
        kg.proposals_equal((bb[k].cpu().numpy(), bi[k].cpu().numpy(), int(bc[k].item())), r, 400)
    with pytest.raises(TypeError):
        ef.keras_proposals(d[0].double(), d[1], d[2], IMG)
    with pytest.raises(ValueError):
        ef.keras_proposals(d[0], d[1][:-1], d[2], IMG)
    with pytest.raises(ValueError):
        ef.keras_proposals(d[0], d[1], d[2].t(), IMG)
    with pytest.raises(ValueError):
        ef.keras_proposals(d[0], d[1], d[2], IMG, out=torch.empty((3, 4), device="cuda"))
    with pytest.raises(ValueError):
        ef.keras_proposals(d[0].cpu(), d[1], d[2], IMG)
    with pytest.raises(ifx.IfxError):
        ef.keras_proposals(d[0], d[1], d[2], IMG, proposal_count=9000)


def test_refusals_leave_the_handle_usable(ifx, ef):
    import torch

    case = kg.proposal_case(41, 300)
    d = [cuda(a) for a in case]
    ptr = [C.c_void_p(t.data_ptr()) for t in d]
    out, idx, cnt = torch.full((400,), -7.5, device="cuda"), torch.full((100,), -77, dtype=torch.int64, device="cuda"), torch.full((1,), -77, dtype=torch.int32, device="cuda")
    po, pi, pc = (C.c_void_p(t.data_ptr()) for t in (out, idx, cnt))
    good = dict(pre=6000, count=100, thr=0.7, image=IMG, n=300)

    def call(probs=ptr[0], bbox=ptr[1], anc=ptr[2], o=po, c=pc, params=True, **kw):
        a = dict(good, **kw)
        p = kg.proposal_params(ifx, a["image"], a["pre"], a["count"], a["thr"])
        return ef.L.ifx_keras_proposals(ef.handle, probs, bbox, anc, a["n"], C.byref(p) if params else None, o, pi, c, None)

    bad = [dict(pre=0), dict(pre=8193), dict(count=0), dict(count=8193), dict(n=0), dict(n=-5), dict(n=1 << 24), dict(image=(0, 64)), dict(image=(64, -1)),
           dict(probs=None), dict(bbox=None), dict(anc=None), dict(o=None), dict(c=None), dict(params=False)]
    for kw in bad:
        assert call(**kw) == kg.E_INVALID, kw
        assert ef.L.ifx_last_error(ef.handle).startswith(b"ifx_keras_proposals: "), kw
    torch.cuda.synchronize()
    assert (out == -7.5).all() and (idx == -77).all() and (cnt == -77).all()          # nothing was enqueued
    assert call() == 0
    torch.cuda.synchronize()
    ref = kl.keras_proposals(*case, IMG, 6000, 100, 0.7)
    kg.proposals_equal((out.cpu().numpy().reshape(100, 4), idx.cpu().numpy(), int(cnt.item())), ref, 100)
