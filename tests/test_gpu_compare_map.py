"""The mask rule of the compare map (option compare_map 2, ifx_mask_compare_map, ifx_segmentation_matches) on the GPU against its numpy statement
(tests/compare_map_numpy.py).  The map is a sheet of stable surfels, one per pixel of a 100 x 52 image (a multiple of 4, not of the count kernel's 32 x 8 tile: both
edges end in partial tiles), whose instance table was filled by ordinary calls and whose votes were then rewritten surfel by surfel through the id image; every
expected value comes from the id image and the votes as downloaded afterwards."""
import numpy as np
import pytest

import compare_map_numpy as cm

pytestmark = pytest.mark.gpu

W, H, NI = 100, 52, 96
K = dict(fx=80.0, fy=80.0, cx=50.0, cy=26.0)
EYE = np.eye(4, dtype=np.float32)
HOLE = (slice(20, 24), slice(60, 65))                      # no depth here in any frame: pixels without a surfel
MAP_KEYS = ("pc", "nr", "col", "tm", "ic", "votes")


def cls_of(slot):
    return 10 + slot // 2                                   # slots 2k and 2k + 1 share a class


@pytest.fixture(scope="module")
def ifx():
    import instancefusion_amd as m

    m.lib()
    return m


def frame():
    rgb = np.random.default_rng(7).integers(30, 255, (H, W, 3)).astype(np.uint8)
    depth = np.full((H, W), 1500, np.uint16)
    depth[HOLE] = 0
    return rgb, depth


def reg_rects():
    """eight disjoint 20 x 20 rectangles away from the borders: the masks that fill the instance table"""
    out = np.zeros((8, H, W), np.uint8)
    for k in range(8):
        x0, y0 = 3 + (k % 4) * 24, 3 + (k // 4) * 24
        out[k, y0:y0 + 20, x0:x0 + 20] = 255
    return out


class Sheet:
    """A handle on the sheet with `slots` instance slots registered (slot s: class cls_of(s)), votes still to be written by put()."""

    def __init__(self, ifx, slots, depth=None, **opts):
        self.rgb, self.depth = frame()
        if depth is not None:
            self.depth = depth
        self.g = g = ifx.ElasticFusion(w=W, h=H, max_surfels=100000, **K)
        for k, v in opts.items():
            g.set_option(k, v)
        self.inst = ifx.InstanceFusion(g)
        for _ in range(3):
            g.processFrame(self.rgb, self.depth, inPose=EYE)
        def stable(m):
            m["pc"][:, 3] = 20.0                            # every surfel stable: the id image shows it
            m["nr"][:, 3] = 0.3 * 1.5 / K["fx"]             # ... and a third of a pixel in radius: under every pixel the surfel that pixel created, and no other
            m["votes"][:] = 0.0                             # (a surfel of the first frame starts with -1 in every word: "not projected" to the box kernels)

        self._settle(stable)
        rects = reg_rects()
        for c in range(0, slots, 8):
            n = min(8, slots - c)
            self.inst.ProcessSegmentation(None, None, rects[:n], np.asarray([cls_of(c + k) for k in range(n)], np.int32), 10 + c)
        self.table = self.inst.getInstanceTable()
        assert np.array_equal(self.table, [cls_of(s) if s < slots else -1 for s in range(NI)])
        self.frames = 100

    def _settle(self, edit):
        g = self.g
        m = g.download()
        edit(m)
        g.upload(m)
        g.set_pose(EYE, g.tick)
        g.processFrame(self.rgb, self.depth, inPose=EYE)

    def put(self, counts, raw=(), first_frame=None):
        """counts [H, W, 96]: the counters of the surfel under every pixel (every other surfel: 0); raw: (y, x, word, float32) written as they are;
        first_frame [H, W] bool: where no counter is written, the words of a first-frame surfel (-1.0: every counter -1)"""
        from instancefusion_amd import synth

        ids0 = self.g.image("ids_after")

        def edit(m):
            n = m["votes"].shape[0]
            ok = (ids0 > 0) & (ids0 < n)
            c = np.zeros((n, NI), np.int64)
            c[ids0[ok]] = counts[ok]
            m["votes"][:] = synth.encode_votes(c)
            if first_frame is not None:
                m["votes"][ids0[ok & first_frame & ~counts.any(axis=-1)]] = -1.0
            for (y, x, w, f) in raw:
                assert ok[y, x]
                m["votes"][ids0[y, x], w] = np.float32(f)
            m["col"][:, 1] = 0.0

        self._settle(edit)
        return self.state()

    def state(self):
        """(id image, votes, surfel count) as downloaded: what the expected values are computed from"""
        ids, votes = self.g.image("ids_after"), self.g.download()["votes"]
        has = (ids > 0) & (ids < votes.shape[0])
        assert has.mean() > 0.9, has.mean()                # no case is vacuous
        assert (~has[HOLE]).sum() >= 8                     # pixels without a surfel (the depth filter closes the hole's corners)
        return ids, votes

    def expect(self, masks, mask_cls, unavailable=None, table=None, state=None):
        ids, votes = state or self.state()
        table = self.table if table is None else table
        pres = cm.presence(ids, votes)
        I, U, _, _ = cm.tables(masks, pres, mask_cls, table)
        un = cm.surfel_boxes_degenerate(masks, ids, votes)
        if unavailable is not None:
            un |= np.asarray(unavailable) > 0
        return I, U, cm.decide(I, U, mask_cls, table, un), pres

    def call(self, masks, mask_cls, device=False, superpixels=False):
        self.frames += 3
        if device:
            import torch

            self.inst.process_segmentation_device(torch.from_numpy(masks).cuda(), np.asarray(mask_cls, np.int32), self.frames, superpixels=superpixels)
        else:
            self.inst.ProcessSegmentation(self.rgb if superpixels else None, self.depth if superpixels else None, masks, np.asarray(mask_cls, np.int32), self.frames,
                                          superpixels=superpixels)

    def everything(self):
        m = self.g.download()
        return [m[k].view(np.uint32) for k in MAP_KEYS] + [self.inst.labels(), self.inst.getInstanceTable(), *self.inst.segmentation_matches()]

    def close(self):
        self.g.close()


def same(a, b, what=""):
    ea, eb = a.everything(), b.everything()
    for k, (x, y) in enumerate(zip(ea, eb)):
        assert np.array_equal(x, y), (what, (MAP_KEYS + ("labels", "table", "best", "target"))[k])


def rect(y0, x0, hh, ww):
    a = np.zeros((H, W), bool)
    a[y0:y0 + hh, x0:x0 + ww] = True
    return a


# ---------------------------------------------------------------------------------------------------------------- 1. the stage against numpy
@pytest.fixture(scope="module")
def stage_case(ifx):
    s = Sheet(ifx, 80)                                     # slots 80 .. 95 unused: class -1
    rng = np.random.default_rng(3)
    counts = np.zeros((H, W, NI), np.int64)
    places = [(0, 0, 9, 12), (0, 88, 8, 12), (44, 0, 8, 11), (43, 90, 9, 10), (0, 40, 6, 20), (46, 30, 6, 25), (15, 0, 20, 5), (10, 95, 25, 5),
              (4, 26, 12, 12), (3, 58, 9, 12), (36, 60, 14, 9), (0, 0, H, W)]
    insts = [2, 3, 5, 31, 32, 33, 63, 64, 79, 40, 90, 6]   # both sides of the words' borders; 90: an unused slot
    vals = [1, 32767, 5, 1, 2, 32767, 1, 7, 1, 3, 9, 1]
    for (y0, x0, hh, ww), i, v in zip(places, insts, vals):
        counts[y0:y0 + hh, x0:x0 + ww, i] = v
    counts[:, :, 6] *= rng.random((H, W)) < 0.6             # the full-image instance: scattered
    ENC = lambda a, b: np.float32(a * 65536 + b)
    raw = [(26, 70, 4, ENC(300, 7)),                        # word 4 (instances 8 and 9, one class) beyond 2^24: the low half rounds
           (26, 72, 4, ENC(3, -1)), (26, 74, 4, ENC(-1, 4)),   # a negative half borrows
           (27, 70, 4, np.nan), (27, 72, 4, np.inf), (27, 74, 4, -np.inf)]
    state = s.put(counts, raw, first_frame=rect(30, 0, 22, 50) & (counts[..., :6].sum(-1) == 0))   # first-frame surfels: -1 in every counter
    masks = np.zeros((17, H, W), np.uint8)
    blobs = [(0, 0, 9, 12), (0, 89, 7, 11), (45, 0, 7, 10), (43, 90, 9, 10),           # the four corners
             (0, 42, 5, 17), (47, 31, 5, 22), (16, 0, 18, 4), (11, 96, 22, 4),         # the four borders
             (0, 0, H, W),                                                             # the whole image
             (4, 28, 12, 8), (3, 60, 9, 8),                                            # across the tile seams at x = 31 / 32 and 63 / 64
             (5, 27, 6, 12), (37, 61, 13, 7), (22, 66, 8, 12),                         # across the tile-row seams at y = 7 / 8 and 47 / 48; around the raw words
             (19, 58, 6, 9), (31, 5, 10, 30), (30, 30, 1, 9)]                          # over the hole; over the -1 surfels; one row high (a degenerate box)
    for k, (y0, x0, hh, ww) in enumerate(blobs):
        masks[k, y0:y0 + hh, x0:x0 + ww] = 255
    masks[13] &= (rng.random((H, W)) < 0.7).astype(np.uint8) * 255
    mcls = np.asarray([cls_of(i) for i in (2, 3, 5, 31, 32, 33, 63, 64, 6, 79, 40, 79, 90, 8, 6, 6, 2)], np.int32)   # (90: the class of no used slot)
    yield s, state, masks, mcls
    s.close()


@pytest.mark.parametrize("nm", [0, 1, 8, 9, 17])
def test_stage_equals_numpy(stage_case, nm):
    s, state, masks, mcls = stage_case
    un = np.zeros(nm, np.uint8)
    un[3:4] = 1
    I, U, best = s.g.mask_compare_map(masks[:nm], mcls[:nm], un)
    eI, eU, ebest, pres = s.expect(masks[:nm], mcls[:nm], un, state=state)
    print("nm", nm, "best", best.tolist(), "cells", int((I > 0).sum()))
    assert np.array_equal(I, eI) and np.array_equal(U, eU)
    assert np.array_equal(best, ebest)
    if nm == 17:
        assert pres[[2, 3, 5, 31, 32, 33, 63, 64, 79, 40, 90, 6]].any(axis=(1, 2)).all()
        assert (eI > 0).sum() > 10 and eI[13, 8] > 0 and eI[13, 9] > 0 and (ebest > 0).sum() >= 3 and not eI[:, 80:].any()
        ids, votes = state
        cnt = cm.decode_words(votes)
        for v in (-1, 1, 32767):
            assert (cnt == v).any()
        assert np.array_equal(s.g.mask_compare_map(masks, mcls)[2], s.expect(masks, mcls, state=state)[2])     # unavailable = NULL
        assert np.array_equal(s.g.download()["votes"].view(np.uint32), votes.view(np.uint32)) and np.array_equal(s.inst.getInstanceTable(), s.table)   # no state changed


# ---------------------------------------------------------------------------------------------------------------- 2. decision edges through geometry
def test_decision_edges_through_geometry(ifx):
    s = Sheet(ifx, 16)
    cell = lambda k: (6 + (k // 4) * 24, 6 + (k % 4) * 24)  # eight places, rectangles of 8 x 8 away from the borders: dilation adds one pixel per side
    counts = np.zeros((H, W, NI), np.int64)
    masks = np.zeros((8, H, W), np.uint8)
    for k in range(7):
        y, x = cell(k)
        masks[k, y:y + 8, x:x + 8] = 255

    def inst(i, k, ww=8, hh=8):
        y, x = cell(k)
        counts[y:y + hh, x:x + ww, i] = 2

    inst(2, 0, ww=3)                                        # a: dilated mask 10 x 10, dilated presence 10 x 5 inside it: I = 50, U = 100
    inst(4, 1, ww=4)                                        # b: 10 x 6: 0.6
    inst(6, 2); inst(7, 2)                                  # c: identical presence: the lower index
    inst(0, 3); inst(1, 3, ww=5)                            # d: best = instance 0, a second one at 0.7
    inst(8, 4)                                              # e: the class differs
    inst(90, 5)                                             # f: a slot of class -1
    inst(10, 6)                                             # g: an unavailable mask
    mcls = np.asarray([cls_of(2), cls_of(4), cls_of(6), cls_of(0), 999, -1, cls_of(10), cls_of(12)], np.int32)   # h: an empty mask against instance 12, no presence
    un = np.asarray([0, 0, 0, 0, 0, 0, 1, 0], np.uint8)
    state = s.put(counts)
    eI, eU, ebest, pres = s.expect(masks, mcls, un, state=state)
    assert np.array_equal(pres, np.moveaxis(counts > 0, -1, 0))      # one surfel per pixel here: the presence images are the rectangles as written
    I, U, best = s.g.mask_compare_map(masks, mcls, un)
    print("I/U a", I[0, 2], U[0, 2], "b", I[1, 4], U[1, 4], "d", I[3, 0], U[3, 0], I[3, 1], U[3, 1], "best", best.tolist())
    assert np.array_equal(I, eI) and np.array_equal(U, eU) and np.array_equal(best, ebest)
    assert (I[0, 2], U[0, 2]) == (50, 100) and (I[1, 4], U[1, 4]) == (60, 100) and (I[3, 0], U[3, 0], I[3, 1], U[3, 1]) == (100, 100, 70, 100)
    assert best.tolist() == [-1, 4, 6, -1, -1, -1, -1, -1]
    assert I[2, 6] == I[2, 7] == 100 and not I[4].any() and not I[5].any() and I[6, 10] == 100 and U[7, 12] == 0
    s.close()


# ---------------------------------------------------------------------------------------------------------------- 3. the rules differ where they should
def x_scene():
    """instances 2 and 3 (one class): the two diagonals of an X in one square, three pixels thick; masks A = "\\" and B = "/" """
    yy, xx = np.mgrid[0:H, 0:W]
    sq = (yy >= 10) & (yy < 40) & (xx >= 10) & (xx < 40)
    a = sq & (np.abs((yy - 10) - (xx - 10)) <= 1)
    b = sq & (np.abs((yy - 10) + (xx - 10) - 29) <= 1)
    counts = np.zeros((H, W, NI), np.int64)
    counts[a, 2] = 3
    counts[b, 3] = 3
    masks = np.stack([a, b]).astype(np.uint8) * 255
    return counts, masks, np.asarray([cls_of(2), cls_of(2)], np.int32), a, b


def run_x(ifx, **opts):
    s = Sheet(ifx, 16, **opts)
    counts, masks, mcls, a, b = x_scene()
    ids, votes = s.put(counts)
    s.call(masks, mcls)
    return s, ids, votes, masks, mcls, a, b


def test_rules_differ_on_an_x(ifx):
    s1, ids, votes, masks, mcls, a, b = run_x(ifx)
    assert np.array_equal(cm.box_rule(masks, ids, votes, mcls, s1.table), [3, 3])
    best1, target1 = s1.inst.segmentation_matches()
    assert best1.tolist() == [3, 3] and target1.tolist() == [3, 3]          # the box rule: identical boxes, the last instance wins for both masks
    s2, ids2, votes2, _, _, _, _ = run_x(ifx, compare_map=2)
    assert np.array_equal(ids, ids2) and np.array_equal(votes.view(np.uint32), votes2.view(np.uint32))
    best2, target2 = s2.inst.segmentation_matches()
    assert best2.tolist() == [2, 3] and target2.tolist() == [2, 3]
    before, after = cm.decode_words(votes2), cm.decode_words(s2.g.download()["votes"])
    assert after.shape == before.shape
    d = (after - before)[ids2]                                                # per pixel: what the call added to the counters of the surfel under it
    only_a = a & ~b                                                           # (the overlap clean gives the crossing to B, the later mask)
    assert (d[only_a][:, 2] == 1).all() and (d[only_a][:, 3] == 0).all()      # A (weight 1) voted for instance 2 and not for 3
    assert (d[b][:, 3] == 2).all() and (d[b][:, 2] == 0).all()                # B (weight 2) for instance 3
    s1.close(); s2.close()


# ---------------------------------------------------------------------------------------------------------------- 4. nothing else moved
def agree_scene():
    counts = np.zeros((H, W, NI), np.int64)
    rects = reg_rects()
    masks = rects[[1, 2, 5, 6, 7]].copy()
    for k, i in zip((1, 2, 5, 6), (2, 5, 8, 11)):
        counts[rects[k] > 0, i] = 4
    return counts, masks, np.asarray([cls_of(2), cls_of(5), cls_of(8), cls_of(11), 500], np.int32)   # four masks on their instances, one of a new class


def banded_depth():
    """three planes side by side (the steps between the columns of reg_rects()): the superpixel merge, which joins what lies in one plane, has three regions to find"""
    _, depth = frame()
    depth[:, 25:73] = 1900
    depth[:, 73:] = 2300
    depth[HOLE] = 0
    return depth


@pytest.mark.parametrize("entry", ["host", "device", "superpixels"])
def test_same_decisions_same_everything(ifx, entry):
    counts, masks, mcls = agree_scene()
    twins = [Sheet(ifx, 16, depth=banded_depth() if entry == "superpixels" else None, compare_map=t) for t in (1, 2)]
    seen = masks
    if entry == "superpixels":
        # The superpixel filter keeps a mask only where it covers most of a merged region: the masks ARE the largest merged regions (the stages, on both twins alike),
        # and every instance is put where the filter leaves its mask.
        for s in twins:
            seg, _ = s.inst.gSLICrInterface(s.rgb)
            _, fin, _ = s.inst.mergeSuperPixel(s.depth, seg)
        labels, areas = np.unique(fin[fin >= 0], return_counts=True)
        pick = labels[np.argsort(-areas, kind="stable")][:4]
        print("superpixels: merged regions", len(labels), "areas of the largest", sorted(areas.tolist(), reverse=True)[:6])
        masks = np.stack([(fin == l).astype(np.uint8) * 255 for l in pick])
        mcls = np.asarray([cls_of(2), cls_of(5), cls_of(8), cls_of(11)][:len(pick)], np.int32)
        for s in twins:
            seen = s.inst.maskSuperPixelFilter_OverSeg(fin, masks)
        counts[...] = 0
        for k, i in enumerate((2, 5, 8, 11)[:len(pick)]):
            counts[seen[k] > 0, i] = 4
        print("superpixels: the filter keeps", [int((m > 0).sum()) for m in seen], "of", [int((m > 0).sum()) for m in masks], "pixels")
    for s in twins:
        ids, votes = s.put(counts)
    _, _, ebest, _ = twins[1].expect(seen, mcls)
    print(entry, "numpy best", ebest.tolist())
    assert np.array_equal(ebest, cm.box_rule(seen, ids, votes, mcls, twins[1].table)) and (ebest > 0).sum() >= 3
    same(twins[0], twins[1], "before")
    for s in twins:
        s.call(masks, mcls, device=entry == "device", superpixels=entry == "superpixels")
    same(twins[0], twins[1], entry)
    best, target = twins[1].inst.segmentation_matches()
    print(entry, "best", best.tolist(), "target", target.tolist())
    assert (best > 0).sum() >= 3 and (target >= 0).sum() >= (best > 0).sum()
    if entry == "host":
        assert np.array_equal(best, ebest)
    for s in twins:
        s.close()


# ---------------------------------------------------------------------------------------------------------------- 5. the two schedules agree
def test_schedules_agree_on_the_x(ifx):
    a, b = (run_x(ifx, compare_map=2, seg_device=d)[0] for d in (1, 0))
    same(a, b, "x")
    assert a.inst.segmentation_matches()[0].tolist() == [2, 3]
    a.close(); b.close()


def test_schedules_agree_through_an_eviction(ifx):
    """A full table, and a call whose first mask is of a new class: the twenty weakest instances go, and the compare map is made again -- under the mask rule, on the
    votes as the eviction left them.  Weakest by construction: nineteen slots without a vote and slot 95, which mask 1 matched before the eviction."""
    rects = reg_rects()
    counts = np.zeros((H, W, NI), np.int64)
    quiet = list(range(20, 39))
    strong = {2: 1, 5: 2, 8: 5, 11: 6}                      # instance: the rectangle it fills
    for i, k in strong.items():
        counts[rects[k] > 0, i] = 5
    small = rect(30, 3, 3, 3)
    counts[small, 95] = 1                                   # sum 9
    for i in range(NI):
        if i not in quiet and i not in strong and i != 95:
            counts[4:8, 52:56, i] = 1                       # sum 16 each
    masks = np.stack([rects[7] > 0, small] + [rects[k] > 0 for k in strong.values()]).astype(np.uint8) * 255
    mcls = np.asarray([700, cls_of(95)] + [cls_of(i) for i in strong], np.int32)
    sheets = []
    for dev in (1, 0):
        s = Sheet(ifx, 96, compare_map=2, seg_device=dev)
        ids, votes = s.put(counts)
        pre = s.expect(masks, mcls, state=(ids, votes))[2]
        assert pre.tolist() == [-1, 95, 2, 5, 8, 11]        # before the eviction mask 1 matches slot 95
        s.call(masks, mcls)
        sheets.append(s)
    a, b = sheets
    same(a, b, "eviction")
    table = a.inst.getInstanceTable()
    gone = np.nonzero(table != a.table)[0]
    assert sorted(gone.tolist()) == sorted(quiet + [95])
    cnt = cm.decode_words(votes).astype(np.int64)
    cnt[:, gone] = 0                                        # cleanInstanceTableMap on the pre-call votes
    from instancefusion_amd import synth

    left = synth.encode_votes(cnt)
    after_table = a.table.copy()
    after_table[gone] = -1
    ebest = a.expect(masks, mcls, table=after_table, state=(ids, left))[2]
    best, target = a.inst.segmentation_matches()
    print("eviction: best", best.tolist(), "target", target.tolist())
    assert ebest.tolist() == [-1, -1, 2, 5, 8, 11] and np.array_equal(best, ebest)
    assert target.tolist() == [20, 21, 2, 5, 8, 11] and table[20] == 700 and table[21] == cls_of(95)
    a.close(); b.close()


# ---------------------------------------------------------------------------------------------------------------- 6. a deferred call
def test_deferred_call_under_the_mask_rule(ifx):
    counts, masks, mcls, _, _ = x_scene()
    a, b, c = Sheet(ifx, 16, compare_map=2), Sheet(ifx, 16, compare_map=2), Sheet(ifx, 16, compare_map=2, seg_device=0)
    for s in (a, b, c):
        ids, votes = s.put(counts)
    ticket, ticket_c = a.inst.snapshot(), c.inst.snapshot()
    for s in (a, b, c):
        for _ in range(2):
            s.g.processFrame(s.rgb, s.depth, inPose=EYE)
    ids_now, votes_now = a.state()
    assert np.array_equal(ids_now, ids)                     # a camera that stands still: the snapshot's id image, re-addressed, is today's
    ebest = a.expect(masks, mcls, state=(ids_now, votes_now))[2]
    a.inst.process_segmentation_deferred(ticket, masks, mcls, 400)
    b.inst.ProcessSegmentation(None, None, masks, mcls, 400)
    c.inst.process_segmentation_deferred(ticket_c, masks, mcls, 400)
    same(a, b, "deferred against the ordinary call")
    same(a, c, "deferred, seg_device 1 against 0")
    assert ebest.tolist() == [2, 3] and np.array_equal(a.inst.segmentation_matches()[0], ebest)
    a.close(); b.close(); c.close()


# ---------------------------------------------------------------------------------------------------------------- 7. refusals
def test_refusals_leave_the_handle_as_it_was(ifx):
    counts, masks, mcls, _, _ = x_scene()
    a, b = Sheet(ifx, 16), Sheet(ifx, 16)
    for s in (a, b):
        s.put(counts)
    L, hdl = a.g.L, a.g.handle
    for v in (0, 3):
        with pytest.raises(ifx.IfxError, match="compare_map must be"):
            a.g.set_option("compare_map", v)
    a.g.set_option("compare_map", 2)
    with pytest.raises(ifx.IfxError, match="ifx_set_shard"):
        a.g._chk(L.ifx_set_shard(hdl, 0, 2), "ifx_set_shard")
    a.g.set_option("compare_map", 1)
    c = ifx.ElasticFusion(w=W, h=H, max_surfels=100000, **K)   # a sharded handle
    c._chk(c.L.ifx_set_shard(c.handle, 0, 2), "ifx_set_shard")
    with pytest.raises(ifx.IfxError, match="sharded"):
        c.set_option("compare_map", 2)
    with pytest.raises(ifx.IfxError, match="sharded"):
        c.mask_compare_map(masks, mcls)
    c.close()
    i32 = np.zeros(257 * NI, np.int32)
    from instancefusion_amd import _ptr

    big = np.zeros((1, H, W), np.uint8)
    for n, mk, cl in ((-1, big, mcls), (257, big, mcls), (1, None, mcls), (1, big, None)):
        r = L.ifx_mask_compare_map(hdl, None if mk is None else _ptr(mk), None if cl is None else _ptr(cl), n, None, _ptr(i32), _ptr(i32), _ptr(i32))
        assert r < 0, (n, r)
    assert L.ifx_mask_compare_map(hdl, None, None, 0, None, None, None, None) == 0
    assert a.g.mask_compare_map(masks, mcls)[2].tolist() == [2, 3]     # (no outputs wanted, no masks: fine; and the stage works whatever the option says)
    for s in (a, b):
        s.call(masks, mcls)
    same(a, b, "after the refusals")
    assert a.inst.segmentation_matches()[0].tolist() == [3, 3]
    a.close(); b.close()
