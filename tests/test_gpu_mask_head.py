"""The mask head's logits to the map's votes on the GPU (ifx_mask_head_select / ifx_process_segmentation_detections / ifx_process_segmentation_deferred_detections):
the stage array-equal to the numpy statement (tests/mask_head_numpy.py) over the rule's edges (tests/mask_head_cases.py) and over the shapes at which the kernels
take another path; the full and the deferred call bit for bit against the ROI entries fed the statement's stage outputs, on twins; the producer stream; the
capacity; the refusals; mask_post_processor."""
import ctypes as C

import numpy as np
import pytest

import mask_head_cases as mc
import mask_head_numpy as mh
import roi_paste_numpy as rp
from conftest import SMALL

pytestmark = pytest.mark.gpu

F = np.float32
MAP_KEYS = ("pc", "nr", "col", "tm", "ic", "votes")
TINY = dict(w=160, h=120, fx=132.0, fy=132.0, cx=80.0, cy=60.0)
IN_SIZE = (640, 480)          # the network's input for the full calls: twice the 320 x 240 frame, so that a box shifted by whole frame pixels stays one (the
                              # stage tests run the inexact and the unequal ratios)


@pytest.fixture(scope="module")
def ifx():
    import instancefusion_amd as m

    m.lib()
    return m


@pytest.fixture(scope="module")
def ef(ifx):
    """One handle for the stage tests (no frame is processed on it)."""
    e = ifx.ElasticFusion(**TINY, max_surfels=100000)
    yield e
    e.close()


def _misaligned(t):
    """The same values in a contiguous tensor that starts one element past an aligned address."""
    import torch

    buf = torch.zeros(t.numel() + 1, dtype=t.dtype, device=t.device)
    v = buf[1:].view(t.shape)
    v.copy_(t)
    assert t.numel() == 0 or v.data_ptr() % 16 != 0
    return v


def _equal_f32(got, want, what):
    """array-equal, bit for bit outside the NaNs (which must sit in the same places)"""
    assert got.dtype == want.dtype == F and got.shape == want.shape, what
    gn, wn = np.isnan(got), np.isnan(want)
    assert np.array_equal(gn, wn), (what, "NaN places")
    same = np.where(gn, np.uint32(0), got.view(np.uint32)) == np.where(wn, np.uint32(0), want.view(np.uint32))
    assert same.all(), (what, np.argwhere(~same)[:5])


def _device(c, misaligned=False):
    """the tensors of a case on the device: (logits, boxes, scores, labels, count or None, class map or None)"""
    import torch

    up = lambda a: (_misaligned(torch.from_numpy(np.ascontiguousarray(a)).cuda()) if misaligned else torch.from_numpy(np.ascontiguousarray(a)).cuda())
    cnt = None if c["count"] is None else up(np.asarray([c["count"]], np.int32))
    cmap = None if c["class_map"] is None else up(c["class_map"])
    return up(c["logits"]), up(c["boxes"]), up(c["scores"]), up(c["labels"]), cnt, cmap


def _check_stage(ef, c, what, misaligned=False, logits_dev=None):
    """padded=True against the padded statement, every output; then the cut form"""
    x, b, s, l, cnt, cmap = _device(dict(c, logits=c["logits"] if logits_dev is None else np.zeros(0, F)), misaligned)
    if logits_dev is not None:
        x = logits_dev
    R = int(c["logits"].shape[0])
    want = mh.padded(mh.mask_head_select(**c), R)
    kw = dict(score_thresh=c["score_thresh"], sort_by_score=c["sort_by_score"], count=cnt, class_map=cmap)
    got = ef.mask_head_select(x, b, s, l, c["in_size"], c["out_size"], padded=True, **kw)
    assert len(got) == 5
    got = [g.cpu().numpy() for g in got]
    _equal_f32(got[0], want[0], (what, "masks"))
    _equal_f32(got[1], want[1], (what, "boxes"))
    for g, w, name in zip(got[2:], want[2:], ("class ids", "rows", "kept")):
        assert g.dtype == w.dtype and np.array_equal(g, w), (what, name, g[:8], w[:8])
    k = int(want[4][0])
    cut = [g.cpu().numpy() for g in ef.mask_head_select(x, b, s, l, c["in_size"], c["out_size"], **kw)]
    assert len(cut) == 4 and all(len(g) == k for g in cut), what
    _equal_f32(cut[0], want[0][:k], (what, "cut masks"))
    _equal_f32(cut[1], want[1][:k], (what, "cut boxes"))
    assert np.array_equal(cut[2], want[2][:k]) and np.array_equal(cut[3], want[3][:k]), what
    return k


@pytest.mark.parametrize("R,Cn,M", [(64, 5, 7), (63, 2, 28), (65, 81, 29), (12, 1, 64), (1024, 2, 1)])
def test_stage_edges_equal_the_statement(ef, R, Cn, M):
    """The case list -- count 0 / R / above R / negative, NaN and +-inf scores, score == thresh, thresh -inf, labels -1 and C, all and none kept, logits +-200,
    +-inf and NaN, the class map -- at five shapes, the last of them with tensors one element past 16-byte alignment."""
    import torch

    cases = mc.edge_cases(R, Cn, M, seed=R + M)
    shared = cases[0][1]["logits"]
    shared_dev = torch.from_numpy(shared).cuda()
    kept = []
    for name, c in cases:
        kept.append(_check_stage(ef, c, name, logits_dev=shared_dev if c["logits"] is shared else None))
    assert max(kept) == R and min(kept) == 0
    for name, c in cases[::4]:
        _check_stage(ef, c, name + ", misaligned", misaligned=True)


def test_stage_many_equal_scores(ef):
    """R = 1024 with three score values: the sort network's full width, ties by ascending row"""
    c = mc.many_equal_scores()
    k = _check_stage(ef, c, "R = 1024")
    assert 600 < k < 1024
    _check_stage(ef, dict(c, sort_by_score=False), "R = 1024, no sort", misaligned=True)
    _check_stage(ef, dict(c, scores=np.full(1024, F(0.9))), "R = 1024, every row kept")


@pytest.mark.parametrize("M", [1, 28, 29, 64])
def test_stage_shapes_equal_the_statement(ef, M):
    """C in {1, 2, 81} x R in {0, 1, 63, 64, 65, 1024} at this M, sorted and unsorted.  The logits are made on the device (up to 1.4 GB at M = 64); the statement
    gets each kept row's own channel, gathered there by stock indexing."""
    import torch

    g = torch.Generator(device="cuda")
    g.manual_seed(1000 + M)
    for Cn in (1, 2, 81):
        for R in (0, 1, 63, 64, 65, 1024):
            c = mc.head(7 * R + Cn, R, Cn, 1)
            x = torch.randn((R, Cn, M, M), generator=g, device="cuda") * 5.0
            dev = [torch.from_numpy(c[n]).cuda() for n in ("boxes", "scores", "labels")]
            for sort in (True, False):
                rows = mh.kept_rows(c["scores"], c["labels"], Cn, 0.7, sort)
                own = x[torch.from_numpy(rows.astype(np.int64)).cuda(), torch.from_numpy(c["labels"][rows]).cuda()].cpu().numpy().reshape(len(rows), M, M)
                want = mh.padded(mh.stage_outputs(own, c["boxes"], c["labels"], rows, c["in_size"], c["out_size"]), R)
                got = [t.cpu().numpy() for t in ef.mask_head_select(x, *dev, c["in_size"], c["out_size"], sort_by_score=sort, padded=True)]
                what = (M, Cn, R, sort)
                _equal_f32(got[0], want[0], what)
                _equal_f32(got[1], want[1], what)
                assert np.array_equal(got[2], want[2]) and np.array_equal(got[3], want[3]) and np.array_equal(got[4], want[4]), what
            del x


def test_count_straight_from_box_detections(ef):
    """box_detections(padded=True) -> mask_head_select with its boxes, scores, labels and count tensors as they are: no read-back in between."""
    import torch

    import box_detections_cases as bc
    import box_detections_numpy as bd

    R, Cn, M = 64, 5, 14
    logits, reg, prop, img = bc.head(31, R, Cn, scale=2.5)
    d = [torch.from_numpy(a).cuda() for a in (logits, reg, prop)]
    b, s, l, _, count, _ = ef.box_detections(*d, img, 0.05, 0.5, 40, bc.WEIGHTS, max_out=R, padded=True)        # 40 detections in 64 rows
    x = (np.random.default_rng(32).standard_normal((R, Cn, M, M)) * 4).astype(F)
    for thr, sort in ((0.3, True), (-float("inf"), False)):
        got = [t.cpu().numpy() for t in ef.mask_head_select(torch.from_numpy(x).cuda(), b, s, l, img, (160, 120), score_thresh=thr, sort_by_score=sort, count=count,
                                                            padded=True)]
        n = int(count.item())
        ref = bd.padded(bd.box_detections(logits, reg, prop, img, 0.05, 0.5, 40, bc.WEIGHTS), R)
        assert n == int(ref[4]) and 0 < n < R
        hb, hs, hl = b.cpu().numpy(), s.cpu().numpy(), l.cpu().numpy()
        assert np.array_equal(hb, ref[0]) and np.array_equal(hl, ref[2])
        want = mh.padded(mh.mask_head_select(x, hb, hs, hl, img, (160, 120), thr, sort, count=n), R)
        _equal_f32(got[0], want[0], thr)
        _equal_f32(got[1], want[1], thr)
        assert np.array_equal(got[2], want[2]) and np.array_equal(got[3], want[3]) and np.array_equal(got[4], want[4])
        assert 0 < int(want[4][0]) <= n


# ---- the full calls against the ROI entries on twins

def _prepared(a):
    m = a.download()
    m["pc"][:, 3] = 20.0
    return m


def _twins(ifx, st, n_frames=8, clear_votes=False):
    """test_gpu_seg_rois._twins: two handles on the same labelled-ready map (every surfel stable after frame 3)"""
    a = ifx.ElasticFusion(**SMALL, max_surfels=400000)
    b = ifx.ElasticFusion(**SMALL, max_surfels=400000)
    for i in range(n_frames):
        pa = a.processFrame(st["rgb"][i], st["depth"][i]); pb = b.processFrame(st["rgb"][i], st["depth"][i])
        assert np.array_equal(pa, pb)
        if i == 3:
            m = _prepared(a)
            if clear_votes:
                m["votes"][:] = 0.0
            for e in (a, b):
                e.upload(m); e.set_pose(pa, a.tick)
    return a, b, ifx.InstanceFusion(a), ifx.InstanceFusion(b)


def _same(ia, ib, what):
    assert np.array_equal(ia.getInstanceTable(), ib.getInstanceTable()), what
    assert np.array_equal(ia.getLoopClosureInstanceTable(), ib.getLoopClosureInstanceTable()), what
    assert np.array_equal(ia.labels(), ib.labels()), what


def _same_maps(a, b):
    ma, mb = a.download(), b.download()
    for k in MAP_KEYS:
        assert np.array_equal(ma[k], mb[k]), k


CLASS_MAP = np.asarray([11, 23, 37, 41, 59], np.int32)


def _head_case(st, i, rng, tie_pair=False):
    """The canned masks of frame i as a detector's two heads would hand them over: logits [R,5,28,28] with logit = log(p / (1 - p)) (clipped to +-12) of the masks'
    ROI form in the label's channel and noise in the other four, boxes in IN_SIZE coordinates, scores above 0.7, a few rows below it, the rows shuffled; tie_pair:
    the largest mask that keeps 16 pixels from every border twice, the copy shifted by eight frame pixels (the same ROI in a box of the same size: the same
    area), the LOWER score first in the input, and the two labels given to no other row.  Returns the case and the statement's stage outputs."""
    from instancefusion_amd import synth

    W, H = SMALL["w"], SMALL["h"]
    masks, _ = synth.canned_masks(st["obj"][i], st["scene"])
    rois, boxes = rp.rois_from_masks(masks)
    n = len(masks)
    scores = (0.72 + 0.27 * rng.permutation(n) / max(n, 1)).astype(F)
    if tie_pair:
        inside = [j for j in range(n) if boxes[j][0] >= 16 and boxes[j][1] >= 16 and boxes[j][2] + 8 <= W - 17 and boxes[j][3] <= H - 17]
        j = inside[0]
        keep = [j] + [q for q in range(n) if q != j]
        rois, boxes, scores = rois[keep], boxes[keep], scores[keep]
        rois = np.concatenate([rois[:1], rois])
        boxes = np.concatenate([boxes[:1] + F(8) * np.asarray([1, 0, 1, 0], F), boxes])
        scores = np.concatenate([[F(0.75)], scores])
        scores[1] = F(0.97)
        n += 1
    low = 3
    rois = np.concatenate([rois, rng.uniform(0.2, 0.9, (low, 28, 28)).astype(F)])
    boxes = np.concatenate([boxes, np.asarray([[30, 20, 200, 150], [5, 5, 60, 90], [100, 100, 300, 230]], F)])
    scores = np.concatenate([scores, np.asarray([0.69, 0.7, 0.05], F)])
    R = n + low
    p = np.clip(rois.astype(np.float64), 1e-9, 1 - 1e-9)
    own = np.clip(np.log(p / (1 - p)), -12, 12).astype(F)
    labels = rng.integers(0, 5, R).astype(np.int64)
    if tie_pair:
        labels = 2 * rng.integers(0, 3, R).astype(np.int64)
        labels[0], labels[1] = 1, 3                                      # two class ids of their own: the overlap clean's winner shows in the votes
    logits = (rng.standard_normal((R, 5, 28, 28)) * 3).astype(F)
    logits[np.arange(R), labels] = own
    boxes_in = (boxes.astype(np.float64) * np.asarray([IN_SIZE[0] / W, IN_SIZE[1] / H] * 2)).astype(F)
    perm = np.arange(R) if tie_pair else rng.permutation(R)
    c = dict(logits=logits[perm], boxes=boxes_in[perm], scores=scores[perm], labels=labels[perm], in_size=IN_SIZE, out_size=(W, H), score_thresh=0.7,
             sort_by_score=True, count=None, class_map=CLASS_MAP)
    stage = mh.mask_head_select(**c)
    assert len(stage[3]) == n
    return c, stage


def _call(inst, c, frame, ticket=None, stream=None, **kw):
    import torch

    t = [torch.from_numpy(c[k]).cuda() for k in ("logits", "boxes", "scores", "labels")]
    cmap = torch.from_numpy(c["class_map"]).cuda()
    if ticket is None:
        return inst.process_segmentation_detections(*t, c["in_size"], frame, c["score_thresh"], class_map=cmap, stream=stream, **kw)
    return inst.process_segmentation_deferred_detections(ticket, *t, c["in_size"], frame, c["score_thresh"], class_map=cmap, stream=stream, **kw)


def _rois_call(inst, stage, frame, ticket=None, **kw):
    import torch

    masks, boxes, cls, _ = stage
    if ticket is None:
        return inst.process_segmentation_rois(torch.from_numpy(masks).cuda(), torch.from_numpy(boxes).cuda(), cls, frame, **kw)
    return inst.process_segmentation_deferred_rois(ticket, torch.from_numpy(masks).cuda(), torch.from_numpy(boxes).cuda(), cls, frame, **kw)


def test_full_call_equals_the_roi_entry_on_the_stage_outputs(ifx, small_stream):
    """Twins at frames 4..7, superpixels on and off, one call with the kNN smoothing: logits, boxes, scores and labels on one, the ROI entry fed the statement's
    stage outputs on the other.  Frame 7 carries two detections of equal area and different score, the lower score first in the input: they reach the map in score
    order, and the overlap clean shows it."""
    import torch

    st = small_stream
    rng = np.random.default_rng(41)
    a = ifx.ElasticFusion(**SMALL, max_surfels=400000)
    b = ifx.ElasticFusion(**SMALL, max_surfels=400000)
    ia, ib = ifx.InstanceFusion(a), ifx.InstanceFusion(b)
    for i in range(8):
        pa = a.processFrame(st["rgb"][i], st["depth"][i]); pb = b.processFrame(st["rgb"][i], st["depth"][i])
        assert np.array_equal(pa, pb)
        if i == 3:
            m = _prepared(a)
            for e in (a, b):
                e.upload(m); e.set_pose(pa, a.tick)
        if i >= 4:
            c, stage = _head_case(st, i, rng, tie_pair=(i == 7))
            kw = dict(isflann=(i == 6), superpixels=(i != 5))
            kept = _call(ia, c, 100 + 3 * i, **kw)
            assert kept == len(stage[3])
            _rois_call(ib, stage, 100 + 3 * i, **kw)
            _same(ia, ib, i)
            if i == 7:
                W, H = SMALL["w"], SMALL["h"]
                rows = stage[3].tolist()
                assert rows.index(1) < rows.index(0)                                   # the higher score first, although it is the later row
                unsorted = mh.mask_head_select(**dict(c, sort_by_score=False))
                ori_s, clean_s, order_s, cls_s = rp.paste_rois(stage[0], stage[1], stage[2], W, H, 0.5)
                ori_u, clean_u, order_u, cls_u = rp.paste_rois(unsorted[0], unsorted[1], unsorted[2], W, H, 0.5)
                j1, j0 = cls_s.tolist().index(int(CLASS_MAP[3])), cls_s.tolist().index(int(CLASS_MAP[1]))
                assert (ori_s[j1] != 0).sum() == (ori_s[j0] != 0).sum() > 400 and j0 == j1 + 1      # equal areas: the stable area sort keeps the score order
                both = (ori_s[j1] != 0) & (ori_s[j0] != 0) & ~(ori_s[j0 + 1:] != 0).any(axis=0)      # (what no smaller mask behind the two takes)
                assert both.sum() > 100 and not clean_s[j1][both].any() and clean_s[j0][both].all()  # the later of the order keeps the overlap: the lower score
                k1, k0 = cls_u.tolist().index(int(CLASS_MAP[3])), cls_u.tolist().index(int(CLASS_MAP[1]))
                assert k1 == k0 + 1 and clean_u[k1][both].all()                                      # (the input order would have given it to the other one)
                got = ia.paste_roi_masks(torch.from_numpy(stage[0]).cuda(), torch.from_numpy(stage[1]).cuda(), stage[2])
                assert np.array_equal(got[1], clean_s) and np.array_equal(got[3], cls_s)
    assert (ia.labels() >= 0).sum() > 100
    assert (ia.getInstanceTable() >= 0).sum() >= 2
    _same_maps(a, b)
    assert np.array_equal(ia.renderProjectMap(), ib.renderProjectMap())
    a.close(); b.close()


def test_deferred_detections(ifx, small_stream):
    """Lag 0: snapshot + deferred call equals the ordinary call.  Lag 4 with the camera moving: equals the deferred ROI entry fed the statement's stage outputs."""
    st = small_stream
    rng = np.random.default_rng(42)
    a, b, ia, ib = _twins(ifx, st, 5, clear_votes=True)
    for k, sp in enumerate((True, False)):
        c, stage = _head_case(st, 4, rng)
        t = ia.snapshot(superpixels=sp)
        assert _call(ia, c, 100 + 3 * k, ticket=t, superpixels=sp) == len(stage[3])
        assert ia.snapshot_stats(t)["in_use"] == 0          # a successful call releases its ticket
        assert _call(ib, c, 100 + 3 * k, superpixels=sp) == len(stage[3])
        _same(ia, ib, ("lag 0", sp))
    assert (ia.getInstanceTable() >= 0).sum() >= 1
    _same_maps(a, b)
    pose5 = None
    for i in range(5, 10):
        pa = a.processFrame(st["rgb"][i], st["depth"][i]); pb = b.processFrame(st["rgb"][i], st["depth"][i])
        assert np.array_equal(pa, pb)
        if i == 5:
            pose5 = pa.copy()
            ta, tb = ia.snapshot(superpixels=True), ib.snapshot(superpixels=True)
    assert not np.array_equal(pose5, pa)                       # the camera moved
    c, stage = _head_case(st, 5, rng)
    _call(ia, c, 200, ticket=ta, superpixels=True)
    _rois_call(ib, stage, 200, ticket=tb, superpixels=True)
    _same(ia, ib, "lag 4")
    assert (ia.labels() >= 0).sum() > 100
    _same_maps(a, b)
    a.close(); b.close()


def test_inputs_written_on_a_producer_stream(ifx, small_stream):
    """Logits, boxes, scores and labels written into zeroed tensors on a side stream behind several milliseconds of other work there; the call gets that stream and
    no host synchronisation: the stage runs on that stream, behind the writes (a call that does not wait reads zeros: scores of 0 keep nothing)."""
    import torch

    st = small_stream
    a, b, ia, ib = _twins(ifx, st)
    c, stage = _head_case(st, 7, np.random.default_rng(43))
    src = [torch.from_numpy(c[k]).cuda() for k in ("logits", "boxes", "scores", "labels")]
    dst = [torch.zeros_like(t) for t in src]
    cmap = torch.from_numpy(c["class_map"]).cuda()
    x = torch.randn(4096, 4096, device="cuda") / 64.0
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        y = x
        for _ in range(8):
            y = y @ x
        one = (y[0, 0] == y[0, 0]).to(torch.float32)           # (depends on the chain's result; 1 unless the chain produced NaN)
        for d_, s_ in zip(dst[:3], src[:3]):
            d_.copy_(s_ * one)
        dst[3].copy_(src[3] * one.to(torch.int64))
    kept = ia.process_segmentation_detections(*dst, c["in_size"], 100, c["score_thresh"], class_map=cmap, superpixels=True, stream=s)
    _rois_call(ib, stage, 100, superpixels=True)
    torch.cuda.synchronize()
    assert all(torch.equal(d_, s_) for d_, s_ in zip(dst, src))
    assert kept == len(stage[3]) > 0
    assert (ib.getInstanceTable() >= 0).sum() >= 1
    _same(ia, ib, "producer stream")
    _same_maps(a, b)
    a.close(); b.close()


def test_capacity_and_refusals_leave_the_handle_usable(ifx, small_stream):
    """kept = 257 -> IFX_E_CAPACITY and nothing applied; a sharded handle -> IFX_E_STATE for the two process entries while the stage entry runs there; M, C, R
    outside their ranges, NULL inputs with R > 0, NULL outputs, a NaN score_thresh, sizes < 1 -> IFX_E_INVALID; TypeError / ValueError in Python.  After the
    refusals a valid call on the same handle still equals its twin."""
    import torch

    st = small_stream
    L = ifx.lib()
    c, stage = _head_case(st, 7, np.random.default_rng(44))
    d_x, d_b, d_s, d_l = [torch.from_numpy(c[k]).cuda() for k in ("logits", "boxes", "scores", "labels")]
    R = int(d_x.shape[0])
    o_m, o_b = torch.zeros((R, 28, 28), device="cuda"), torch.zeros((R, 4), device="cuda")
    o_c, o_r, o_k = torch.zeros(R, dtype=torch.int32, device="cuda"), torch.zeros(R, dtype=torch.int32, device="cuda"), torch.full((1,), -7, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    P = lambda t: C.c_void_p(t.data_ptr())

    def params(thresh=0.7, in_w=IN_SIZE[0], in_h=IN_SIZE[1], out_w=SMALL["w"], out_h=SMALL["h"], sort=1):
        p = ifx.MaskHeadParams()
        p.score_thresh, p.in_w, p.in_h, p.out_w, p.out_h, p.sort_by_score = thresh, in_w, in_h, out_w, out_h, sort
        return p

    e = ifx.ElasticFusion(**SMALL, max_surfels=100000, n_ranks=-1, rank=0)
    try:
        p = params()
        out_kept = C.c_int32(-5)
        r = L.ifx_process_segmentation_detections(e.handle, P(d_x), P(d_b), P(d_s), P(d_l), None, None, R, 5, 28, C.byref(p), 0.5, 100, 0, None, C.byref(out_kept))
        assert r == -4 and b"sharded" in L.ifx_last_error(e.handle)
        assert L.ifx_process_segmentation_deferred_detections(e.handle, 0, P(d_x), P(d_b), P(d_s), P(d_l), None, None, R, 5, 28, C.byref(p), 0.5, 100, 0, None, None) == -4
        with pytest.raises(ifx.IfxError, match=r"\(-4\)"):
            ifx.InstanceFusion(e).process_segmentation_detections(d_x, d_b, d_s, d_l, IN_SIZE, 100)
        # the stage entry is allowed on a sharded handle
        assert L.ifx_mask_head_select(e.handle, P(d_x), P(d_b), P(d_s), P(d_l), None, None, R, 5, 28, C.byref(p), P(o_m), P(o_b), P(o_c), P(o_r), P(o_k), None) == 0
        torch.cuda.synchronize()
        want = mh.padded(mh.mask_head_select(**dict(c, class_map=None)), R)
        _equal_f32(o_m.cpu().numpy(), want[0], "sharded handle")
        _equal_f32(o_b.cpu().numpy(), want[1], "sharded handle")
        assert np.array_equal(o_r.cpu().numpy(), want[3]) and int(o_k.item()) == int(want[4][0])
        assert L.ifx_mask_head_select(e.handle, None, None, None, None, None, None, 0, 5, 28, C.byref(p), None, None, None, None, P(o_k), None) == 0      # R == 0: kept = 0
        torch.cuda.synchronize()
        assert int(o_k.item()) == 0
    finally:
        e.close()

    a, b, ia, ib = _twins(ifx, st)
    frame = 100

    def valid_call(what):
        nonlocal frame
        assert _call(ia, c, frame, superpixels=True) == len(stage[3])
        _rois_call(ib, stage, frame, superpixels=True)
        _same(ia, ib, what)
        frame += 3

    # capacity: 257 rows above the threshold
    n = 257
    big = mc.head(9, n, 1, 2)
    big_t = [torch.from_numpy(big[k]).cuda() for k in ("logits", "boxes", "scores", "labels")]
    big_t[2] = torch.full((n,), 0.9, device="cuda")
    out_kept = C.c_int32(-5)
    p = params()
    r = L.ifx_process_segmentation_detections(a.handle, P(big_t[0]), P(big_t[1]), P(big_t[2]), P(big_t[3]), None, None, n, 1, 2, C.byref(p), 0.5, frame, 2, None, C.byref(out_kept))
    assert r == -3 and out_kept.value == 257 and b"256" in L.ifx_last_error(a.handle)
    with pytest.raises(ifx.IfxError, match=r"\(-3\)"):
        ia.process_segmentation_detections(*big_t, IN_SIZE, frame)
    t = ia.snapshot()
    assert L.ifx_process_segmentation_deferred_detections(a.handle, t, P(big_t[0]), P(big_t[1]), P(big_t[2]), P(big_t[3]), None, None, n, 1, 2, C.byref(p), 0.5, frame, 0,
                                                          None, None) == -3
    assert ia.snapshot_stats(t)["in_use"] == 1                 # a failed call keeps its ticket
    ia.release_snapshot(t)
    valid_call("capacity")

    nan = float("nan")
    refusals = [
        ("M = 0", dict(M=0)), ("M = 65", dict(M=65)), ("C = 0", dict(Cn=0)), ("C = 1025", dict(Cn=1025)), ("R < 0", dict(R=-1)), ("R = 1025", dict(R=1025)),
        ("null logits", dict(x=None)), ("null boxes", dict(b=None)), ("null scores", dict(s=None)), ("null labels", dict(l=None)),
        ("NaN score_thresh", dict(p=params(thresh=nan))), ("in_w = 0", dict(p=params(in_w=0))), ("in_h < 0", dict(p=params(in_h=-3))), ("null params", dict(p=None)),
    ]
    for what, kw in refusals:
        q = dict(x=P(d_x), b=P(d_b), s=P(d_s), l=P(d_l), R=R, Cn=5, M=28, p=params())
        q.update(kw)
        pp = None if q["p"] is None else C.byref(q["p"])
        lead = (q["x"], q["b"], q["s"], q["l"], None, None, q["R"], q["Cn"], q["M"], pp)
        assert L.ifx_mask_head_select(a.handle, *lead, P(o_m), P(o_b), P(o_c), P(o_r), P(o_k), None) == -1, what
        assert L.ifx_process_segmentation_detections(a.handle, *lead, 0.5, frame, 2, None, None) == -1, what
        t = ia.snapshot()
        assert L.ifx_process_segmentation_deferred_detections(a.handle, t, *lead, 0.5, frame, 0, None, None) == -1, what
        ia.release_snapshot(t)
    for what, pp_, outs in (("out_w = 0", params(out_w=0), (P(o_m), P(o_b), P(o_c), P(o_r), P(o_k))), ("out_h = 0", params(out_h=0), (P(o_m), P(o_b), P(o_c), P(o_r), P(o_k))),
                            ("null kept", params(), (P(o_m), P(o_b), P(o_c), P(o_r), None)), ("null masks", params(), (None, P(o_b), P(o_c), P(o_r), P(o_k))),
                            ("null class ids", params(), (P(o_m), P(o_b), None, P(o_r), P(o_k)))):
        assert L.ifx_mask_head_select(a.handle, P(d_x), P(d_b), P(d_s), P(d_l), None, None, R, 5, 28, C.byref(pp_), *outs, None) == -1, what
    assert L.ifx_process_segmentation_deferred_detections(a.handle, 12345, P(d_x), P(d_b), P(d_s), P(d_l), None, None, R, 5, 28, C.byref(params()), 0.5, frame, 0, None, None) == -1
    valid_call("refusals")
    o_k.fill_(-7)
    assert L.ifx_mask_head_select(a.handle, P(d_x), P(d_b), P(d_s), P(d_l), None, None, R, 5, 28, C.byref(params()), P(o_m), P(o_b), P(o_c), None, P(o_k), None) == 0   # NULL d_rows
    torch.cuda.synchronize()
    want = mh.padded(mh.mask_head_select(**dict(c, class_map=None)), R)
    _equal_f32(o_m.cpu().numpy(), want[0], "NULL d_rows")
    assert np.array_equal(o_c.cpu().numpy(), want[2]) and int(o_k.item()) == int(want[4][0])

    ea = a
    sel = lambda **k: ea.mask_head_select(k.get("x", d_x), k.get("b", d_b), k.get("s", d_s), k.get("l", d_l), k.get("in_size", IN_SIZE), k.get("out_size", (320, 240)),
                                          **{n_: v for n_, v in k.items() if n_ in ("score_thresh", "count", "class_map")})
    with pytest.raises(ValueError):
        sel(x=torch.from_numpy(c["logits"]))                                    # CPU tensor
    with pytest.raises(ValueError):
        sel(x=d_x[:, :, :, :-1])                                                # not square (and not contiguous)
    with pytest.raises(ValueError):
        sel(x=d_x[0])                                                           # [C,M,M]
    with pytest.raises(ValueError):
        sel(x=torch.zeros((R, 5, 65, 65), device="cuda"))                       # M = 65
    with pytest.raises(ValueError):
        sel(b=d_b[:, :3].contiguous())
    with pytest.raises(ValueError):
        sel(s=d_s[:-1])
    with pytest.raises(ValueError):
        sel(l=d_l[:-1])
    with pytest.raises(ValueError):
        sel(class_map=torch.zeros(4, dtype=torch.int32, device="cuda"))
    with pytest.raises(ValueError):
        sel(count=torch.zeros(2, dtype=torch.int32, device="cuda"))
    with pytest.raises(ValueError):
        sel(score_thresh=nan)
    with pytest.raises(ValueError):
        sel(in_size=(0, 600))
    with pytest.raises(ValueError):
        ia.process_segmentation_detections(d_x, d_b, d_s[:-1], d_l, IN_SIZE, frame)
    with pytest.raises(TypeError):
        sel(x=d_x.to(torch.float16))
    with pytest.raises(TypeError):
        sel(l=d_l.to(torch.int32))
    with pytest.raises(TypeError):
        sel(s=d_s.to(torch.float64))
    with pytest.raises(TypeError):
        sel(count=torch.zeros(1, dtype=torch.int64, device="cuda"))
    with pytest.raises(TypeError):
        sel(class_map=torch.zeros(5, dtype=torch.int64, device="cuda"))
    with pytest.raises(TypeError):
        sel(x=c["logits"])                                                      # not a tensor
    with pytest.raises(TypeError):
        ia.process_segmentation_deferred_detections(0, d_x, d_b.to(torch.float64), d_s, d_l, IN_SIZE, frame)
    valid_call("python")
    assert (ib.getInstanceTable() >= 0).sum() >= 2
    _same_maps(a, b)
    a.close(); b.close()


class _Boxes:
    """A duck-typed box list: what mask_post_processor needs of maskrcnn-benchmark's BoxList"""
    def __init__(self, bbox, size, mode="xyxy"):
        self.bbox, self.size, self.mode, self.extra = bbox, size, mode, {}

    def add_field(self, k, v):
        self.extra[k] = v

    def get_field(self, k):
        return self.extra[k]

    def fields(self):
        return list(self.extra)

    def __len__(self):
        return int(self.bbox.shape[0])


def test_mask_post_processor(ifx, ef):
    """Two images in one call: the field "mask" is the statement's sigmoid of each row's own channel, [n,1,M,M], in the rows' own order; boxes, size and the
    other fields are carried over; the result has the class of the lists given."""
    import torch

    Cn, M = 7, 14
    post = ifx.mask_post_processor(ef)
    assert post.masker is None
    heads = [mc.head(51, 9, Cn, M, in_size=(640, 480)), mc.head(52, 4, Cn, M, in_size=(333, 217))]
    x = torch.from_numpy(np.concatenate([h["logits"] for h in heads])).cuda()
    boxes = []
    for h in heads:
        bl = _Boxes(torch.from_numpy(h["boxes"]).cuda(), h["in_size"])
        bl.add_field("scores", torch.from_numpy(h["scores"]).cuda())
        bl.add_field("labels", torch.from_numpy(h["labels"]).cuda())
        bl.add_field("note", "kept as it is")
        boxes.append(bl)
    out = post(x, boxes)
    assert len(out) == 2
    for h, bl, r in zip(heads, boxes, out):
        assert type(r) is _Boxes and r.size == bl.size and r.mode == "xyxy" and torch.equal(r.bbox, bl.bbox)
        assert r.fields() == ["scores", "labels", "note", "mask"] and r.get_field("note") == "kept as it is"
        assert torch.equal(r.get_field("scores"), bl.get_field("scores")) and torch.equal(r.get_field("labels"), bl.get_field("labels"))
        n = len(bl)
        want = mh.sigmoid(h["logits"][np.arange(n), h["labels"]])
        got = r.get_field("mask")
        assert tuple(got.shape) == (n, 1, M, M)
        _equal_f32(got.cpu().numpy()[:, 0], want, "mask")
