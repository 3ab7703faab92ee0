"""Merging duplicate instances on the GPU (ifx_merge_instances, ifx_instance_duplicates) against their numpy statement (tests/instance_merge_numpy.py).  The handle is
a sheet of stable surfels, one per pixel of a 100 x 52 image, whose instance table was filled by ordinary calls; the word patterns go into uploaded maps whose count
ends around a block's share of records (128) and are read back slot by slot through ifx_map_view, tombstones included.  Votes are compared as uint32 bit patterns,
with labels, colours and the table; every expected value comes from the map as read before the call.  (The label of a tombstone is not visible on an unsharded
handle -- ifx_labels returns the live surfels -- so of a tombstone the votes and the untouched colour are checked.)"""
import numpy as np
import pytest

import instance_merge_numpy as im

pytestmark = pytest.mark.gpu

W, H, NI = 100, 52, 96
K = dict(fx=80.0, fy=80.0, cx=50.0, cy=26.0)
EYE = np.eye(4, dtype=np.float32)
HOLE = (slice(20, 24), slice(60, 65))
E_INVALID, E_STATE = "(-1)", "(-4)"


@pytest.fixture(scope="module")
def ifx():
    import instancefusion_amd as m

    m.lib()
    return m


def cls_of(slot):
    return 10 + slot // 2                                   # slots 2k and 2k + 1 share a class


def reg_rects():
    out = np.zeros((8, H, W), np.uint8)
    for k in range(8):
        x0, y0 = 3 + (k % 4) * 24, 3 + (k // 4) * 24
        out[k, y0:y0 + 20, x0:x0 + 20] = 255
    return out


def rect(y0, x0, hh, ww):
    a = np.zeros((H, W), bool)
    a[y0:y0 + hh, x0:x0 + ww] = True
    return a


class Sheet:
    """a handle on the sheet whose instance slots 0 .. len(classes) - 1 are registered with those classes (eight disjoint masks per call)"""

    def __init__(self, ifx, classes):
        self.rgb = np.random.default_rng(7).integers(30, 255, (H, W, 3)).astype(np.uint8)
        self.depth = np.full((H, W), 1500, np.uint16)
        self.depth[HOLE] = 0
        self.g = g = ifx.ElasticFusion(w=W, h=H, max_surfels=100000, **K)
        self.inst = ifx.InstanceFusion(g)
        for _ in range(3):
            g.processFrame(self.rgb, self.depth, inPose=EYE)

        def stable(m):
            m["pc"][:, 3] = 20.0
            m["nr"][:, 3] = 0.3 * 1.5 / K["fx"]
            m["votes"][:] = 0.0

        self.settle(stable)
        rects = reg_rects()
        for c in range(0, len(classes), 8):
            cl = np.asarray(classes[c:c + 8], np.int32)
            self.inst.ProcessSegmentation(None, None, rects[:len(cl)], cl, 10 + c)
        assert np.array_equal(self.inst.getInstanceTable(), list(classes) + [-1] * (NI - len(classes)))
        t = self.inst.getLoopClosureInstanceTable()
        self.inst_colour = ((t[:, 0] << 16) + (t[:, 1] << 8) + t[:, 2]).astype(np.float32)
        self.frames = 200

    def settle(self, edit):
        g = self.g
        m = g.download()
        edit(m)
        g.upload(m)
        g.set_pose(EYE, g.tick)
        g.processFrame(self.rgb, self.depth, inPose=EYE)

    def put(self, counts):
        """counts [H, W, 96]: the counters of the surfel under every pixel; colours as the label scan would have assigned them.  Returns (id image, votes)."""
        ids0 = self.g.image("ids_after")

        def edit(m):
            n = m["votes"].shape[0]
            ok = (ids0 > 0) & (ids0 < n)
            c = np.zeros((n, NI), np.int64)
            c[ids0[ok]] = counts[ok]
            m["votes"][:] = im.encode_word(c[:, 0::2], c[:, 1::2])
            m["col"][:, 1] = im.label_scan(m["votes"], m["tm"], np.zeros(n, np.float32), self.inst_colour)[1]

        self.settle(edit)
        ids, votes = self.g.image("ids_after"), self.g.download()["votes"]
        assert ((ids > 0) & (ids < votes.shape[0])).mean() > 0.9
        return ids, votes

    def close(self):
        self.g.close()


def _dev(g, ptr, n):
    import torch

    from instancefusion_amd import sharded

    return torch.as_tensor(sharded._DevWords(ptr, n, "<f4"), device=f"cuda:{g.cfgd['device']}")


def raw(g):
    """votes [n, 48], col [n, 2], tm [n, 2] of every slot below the count, tombstones included"""
    g.sync()
    v = g.map_view()
    n = v.count
    get = lambda p, wd: _dev(g, p, n * wd).cpu().numpy().reshape(n, wd).copy()
    return dict(votes=get(v.d_votes, 48), col=get(v.d_color, 2), tm=get(v.d_times, 2))


def bury(g, slots):
    """tombstones in place: the last-seen time of these slots below the marker"""
    import torch

    g.sync()
    v = g.map_view()
    _dev(g, v.d_times, v.count * 2).view(v.count, 2)[torch.as_tensor(slots, device=f"cuda:{g.cfgd['device']}"), 1] = -2.0e9
    torch.cuda.synchronize()


RAW_FLOATS = np.asarray([np.nan, np.inf, -np.inf, 2.0 ** 31, -2.0 ** 31, 0.5, -0.5, 1e10], np.float32)


def craft(base, n, pairs, inst_colour, rng):
    """A map of n surfels (rows of `base`, repeated) whose vote words run through the patterns, row i and pair k in pattern (i + k) % 14, and whose colours are drawn
    from: none, the default, a source's, a target's, a bystander's."""
    idx = np.arange(n) % base["pc"].shape[0]
    m = {k: base[k][idx].copy() for k in base}
    v = np.zeros((n, 48), np.float32)
    enc = im.encode_word
    busy = {i for p in pairs for i in p}
    idle = [i for i in range(NI) if i not in busy]
    rows = np.arange(n)
    noise = rows[rows % 14 >= 11]                            # (three patterns in fourteen start from counters all over the record)
    c = np.zeros((n, NI), np.int64)
    c[noise[:, None], rng.integers(0, NI, (len(noise), 6))] = rng.integers(1, 300, (len(noise), 6))
    v[:] = enc(c[:, 0::2], c[:, 1::2])

    def put(r, inst, val):
        a, b = im.decode_word(v[r, inst // 2])
        v[r, inst // 2] = enc(np.where(inst & 1, a, val), np.where(inst & 1, val, b))

    for k, (f, t) in enumerate(pairs):
        pat = (rows + k) % 14
        sel = lambda p: rows[pat == p]
        # 0: all zero
        apart = f // 2 != t // 2                             # (in one word the three first-frame patterns are one)
        v[sel(2), t // 2] = -1.0                             # a first-frame word in the target
        v[sel(3), f // 2] = -1.0                             # ... in both
        v[sel(3), t // 2] = -1.0
        if apart:
            v[sel(1), f // 2] = -1.0                         # ... in the source
            put(sel(1), t, 9)
            put(sel(2), f, 5)
        put(sel(4), f, rng.integers(1, 60, len(sel(4)))); put(sel(4), t, rng.integers(0, 60, len(sel(4))))
        put(sel(5), t, 65000); put(sel(5), f, 1000)          # the clamp's neighbourhood, as the packing shows it
        put(sel(6), f, 40000); put(sel(6), t, 3)             # a half above 32 767 as source
        put(sel(7), f, 32767); put(sel(7), t, 32767)         # the sum leaves the short
        put(sel(8), f, rng.integers(250, 400, len(sel(8)))); put(sel(8), t, rng.integers(250, 400, len(sel(8))))   # words beyond 2^24
        v[sel(9), f // 2] = RAW_FLOATS[sel(9) % len(RAW_FLOATS)]     # floats no encoding produces, in the source ...
        v[sel(10), t // 2] = RAW_FLOATS[sel(10) % len(RAW_FLOATS)]   # ... and in the target
        if apart:
            put(sel(9), t, 4)
            put(sel(10), f, 6)
        put(sel(12), f, rng.integers(1, 30, len(sel(12))))
    m["votes"] = v
    palette = np.asarray([0.0, im.DEFAULT_COLOUR] + [inst_colour[f] for f, _ in pairs[:3]] + [inst_colour[i] for i in [pairs[0][1]] + idle[:1]], np.float32)
    m["col"][:, 1] = palette[rng.integers(0, len(palette), n)]
    return m


def merge_and_check(ifx, s, m, pairs, dead=()):
    """upload m, bury `dead`, merge, and compare everything with the statement applied to the map as read back before the call"""
    g, inst = s.g, s.inst
    g.upload(m)
    if len(dead):
        bury(g, np.asarray(dead))
    before, table = raw(g), inst.getInstanceTable()
    assert before["votes"].shape[0] == m["votes"].shape[0] and np.array_equal(im.bits(before["votes"]), im.bits(m["votes"]))
    assert im.refusal(pairs, table) is None
    e_votes, e_labels, e_col, e_table = im.merge(before["votes"], before["tm"], before["col"][:, 1], table, s.inst_colour, pairs)
    done = inst.merge_instances(pairs, resolve=False)
    assert sorted(map(tuple, done.tolist())) == sorted(map(tuple, np.asarray(pairs).tolist()))
    after, labels = raw(g), inst.labels()
    live = before["tm"][:, 1] > im.DEAD_TIME
    changed = (im.bits(e_votes) != im.bits(before["votes"])).any(axis=1)
    print(f"n {len(live)} pairs {len(pairs)} dead {int((~live).sum())} records changed {int(changed.sum())} recoloured {int((e_col != before['col'][:, 1]).sum())}")
    assert np.array_equal(im.bits(after["votes"]), im.bits(e_votes))
    assert np.array_equal(inst.getInstanceTable(), e_table)
    assert np.array_equal(labels, e_labels[live])
    assert np.array_equal(im.bits(after["col"][:, 1]), im.bits(e_col)) and np.array_equal(im.bits(after["col"][:, 0]), im.bits(before["col"][:, 0]))
    assert np.array_equal(im.bits(after["tm"]), im.bits(before["tm"]))
    if len(dead):
        assert np.array_equal(after["col"][~live], before["col"][~live]) and (changed & ~live).any()     # votes merged in a tombstone, its colour left alone
    return before, e_votes, e_col, changed


@pytest.fixture(scope="module")
def full(ifx):
    s = Sheet(ifx, [cls_of(i) for i in range(NI)])
    s.base = s.g.download()
    yield s
    s.close()


# every case names instances of its own: the cases stand in any order and alone
CASES = {
    "one short of a block, two halves of one word": (127, [(1, 0)], 0),
    "a block, two quarters of the record": (128, [(9, 2)], 0),
    "one past a block, three sources into one target": (129, [(20, 5), (41, 5), (95, 5)], 0),
    "a single surfel": (1, [(7, 6)], 0),
    "forty blocks and a part, tombstones": (5200, [(10, 11), (30, 12), (13, 31), (50, 51), (66, 12)], 400),
}


@pytest.mark.parametrize("case", list(CASES))
def test_word_patterns(ifx, full, case):
    n, pairs, n_dead = CASES[case]
    rng = np.random.default_rng(n)
    m = craft(full.base, n, pairs, full.inst_colour, rng)
    if n == 1:
        m["votes"][0, 3] = im.encode_word(4, 21)             # (6 and 7: the halves of word 3)
        m["col"][0, 1] = full.inst_colour[7]
    dead = rng.choice(n, n_dead, replace=False) if n_dead else ()
    before, e_votes, e_col, changed = merge_and_check(ifx, full, m, pairs, dead)
    if n == 1:
        assert im.decode(e_votes)[0, [6, 7]].tolist() == [25, 0] and e_col[0] == full.inst_colour[6]
    else:
        assert changed.any() and (len(pairs) > 1 or not changed.all())     # (one pair: its all-zero rows are records nobody writes)
        cnt = im.decode(before["votes"])
        for f, t in pairs:
            assert (cnt[:, f] > 0).any() and (cnt[:, f] < 0).any() and (cnt[:, f] == 0).any() and (cnt[:, t] == -1).any()
        was_from = np.isin(before["col"][:, 1], full.inst_colour[[f for f, _ in pairs]]) & (before["tm"][:, 1] > im.DEAD_TIME)
        assert was_from.sum() > 10 and not np.isin(e_col[was_from], full.inst_colour[[f for f, _ in pairs]]).any()


def test_ninety_five_pairs(ifx):
    s = Sheet(ifx, [cls_of(i) for i in range(NI)])
    pairs = [(i, 0) for i in range(1, NI)]
    rng = np.random.default_rng(95)
    m = craft(s.g.download(), 300, pairs, s.inst_colour, rng)
    merge_and_check(ifx, s, m, pairs)
    assert s.inst.getInstanceTable().tolist() == [cls_of(0)] + [-1] * 95
    s.close()


def dup_counts():
    """instances 2 and 3 (one class) pixel by pixel over one rectangle; 4 and 5 (another class) each in a place of its own"""
    yy, xx = np.mgrid[0:H, 0:W]
    counts = np.zeros((H, W, NI), np.int64)
    r = rect(8, 8, 22, 30)
    counts[r & ((yy + xx) % 2 == 0), 2] = 50
    counts[r & ((yy + xx) % 2 == 1), 3] = 50
    counts[rect(34, 6, 12, 20), 4] = 7
    counts[rect(34, 40, 12, 20), 5] = 7
    return counts


def test_after_the_call(ifx):
    """duplicates found and merged on the sheet; then a ticket from before the merge is accepted, and new instances take the freed slots from zero"""
    s = Sheet(ifx, [cls_of(i) for i in range(8)])
    ids, votes = s.put(dup_counts())
    found = s.inst.duplicate_instances()
    assert found.tolist() == [[3, 2]] == im.duplicates(im.project_boxes(ids, votes, W, H), s.inst.getInstanceTable()).tolist()
    ticket = s.inst.snapshot()
    before, table = raw(s.g), s.inst.getInstanceTable()
    pairs = [(3, 2), (5, 4)]
    e_votes, e_labels, e_col, e_table = im.merge(before["votes"], before["tm"], before["col"][:, 1], table, s.inst_colour, pairs)
    s.inst.merge_instances(pairs)
    after = raw(s.g)
    assert np.array_equal(im.bits(after["votes"]), im.bits(e_votes)) and np.array_equal(im.bits(after["col"][:, 1]), im.bits(e_col))
    assert np.array_equal(s.inst.labels(), e_labels) and np.array_equal(s.inst.getInstanceTable(), e_table)
    was3 = before["col"][:, 1] == s.inst_colour[3]
    assert was3.sum() > 200 and (after["col"][was3, 1] == s.inst_colour[2]).all()      # the merged object has one colour
    cnt = im.decode(after["votes"])
    assert (cnt[:, 2] == 50).sum() == (im.decode(before["votes"])[:, [2, 3]] == 50).sum() and not cnt[:, [3, 5]].any()
    # the ticket taken before the merge, one mask of a new class over the idle lower right: the lowest freed slot, counted from zero
    mask = (rect(34, 70, 12, 24)[None] * 255).astype(np.uint8)
    s.inst.process_segmentation_deferred(ticket, mask, np.asarray([700], np.int32), 300)
    t = s.inst.getInstanceTable()
    assert t[3] == 700 and t[5] == -1
    c3 = im.decode(s.g.download()["votes"])[:, 3]
    assert set(np.unique(c3).tolist()) == {0, 1} and (c3 == 1).sum() > 100
    mask2 = (rect(4, 50, 12, 40)[None] * 255).astype(np.uint8)
    s.inst.ProcessSegmentation(None, None, mask2, np.asarray([701], np.int32), 303)
    assert s.inst.getInstanceTable()[5] == 701
    c5 = im.decode(s.g.download()["votes"])[:, 5]
    assert set(np.unique(c5).tolist()) == {0, 1} and (c5 == 1).sum() > 100
    s.close()


def test_refusals_change_nothing(ifx):
    s = Sheet(ifx, [cls_of(i) for i in range(8)])
    s.put(dup_counts())
    before, table = raw(s.g), s.inst.getInstanceTable()
    cases = {"range": [[(1, 96)], [(-1, 0)], [(96, 1)]], "self": [[(2, 2)]], "unused": [[(8, 0)], [(0, 9)]], "twice": [[(1, 0), (1, 2)]], "chain": [[(3, 1), (5, 3)], [(1, 0), (0, 2)]]}
    words = {"range": "outside", "self": "itself", "unused": "unused", "twice": "two pairs", "chain": "chain"}
    for why, lists in cases.items():
        for pairs in lists:
            assert im.refusal(pairs, table) == why
            with pytest.raises(ifx.IfxError, match=words[why]) as e:
                s.inst.merge_instances(pairs, resolve=False)
            assert E_INVALID in str(e.value) and "ifx_merge_instances" in str(e.value)
    with pytest.raises(ifx.IfxError, match="0 .. 95") as e:
        s.inst.merge_instances([(i % 7 + 1, 0) for i in range(96)], resolve=False)
    assert E_INVALID in str(e.value)
    with pytest.raises(ValueError):
        s.inst.merge_instances([(1, 2), (2, 1)])
    assert s.inst.merge_instances([]).shape == (0, 2) and s.g.L.ifx_merge_instances(s.g.handle, None, 0) == 0
    after = raw(s.g)
    for k in before:
        assert np.array_equal(im.bits(after[k]), im.bits(before[k])), k
    assert np.array_equal(s.inst.getInstanceTable(), table)
    s.close()


def test_duplicates_on_the_sheet(ifx):
    A, B, Cc = 31, 32, 33
    s = Sheet(ifx, [A, A, A, B, A, Cc, Cc, Cc])
    yy, xx = np.mgrid[0:H, 0:W]
    counts = np.zeros((H, W, NI), np.int64)
    r1, r3 = rect(8, 8, 20, 33), rect(8, 58, 21, 36)
    for k, i in enumerate((1, 2, 3)):                       # two of class A and one of class B, pixel by pixel over one rectangle
        counts[r1 & ((yy + xx) % 3 == k), i] = 9
    counts[rect(35, 5, 12, 20), 4] = 9                      # a third of class A elsewhere
    for k, i in enumerate((5, 6, 7)):                       # three of class C over one rectangle (the hole in it)
        counts[r3 & ((yy + 2 * xx) % 3 == k), i] = 9
    ids, votes = s.put(counts)
    table = s.inst.getInstanceTable()
    boxes = im.project_boxes(ids, votes, W, H)
    expect = im.duplicates(boxes, table)
    got = s.inst.duplicate_instances()
    print("boxes", boxes[:8].tolist(), "pairs", got.tolist())
    assert np.array_equal(got, expect) and got.tolist() == [[2, 1], [6, 5], [7, 5]]
    assert np.array_equal(s.inst.duplicate_instances(0.999), im.duplicates(boxes, table, 0.999))
    after = s.g.download()["votes"]
    assert np.array_equal(im.bits(after), im.bits(votes)) and np.array_equal(s.inst.getInstanceTable(), table)      # no state changed
    out = np.zeros((95, 2), np.int32)
    from instancefusion_amd import _ptr

    assert s.g.L.ifx_instance_duplicates(s.g.handle, 0.5, _ptr(out), 1) == 3 and out[0].tolist() == [2, 1] and not out[1:].any()
    assert s.g.L.ifx_instance_duplicates(s.g.handle, float("nan"), _ptr(out), 95) == -1
    s.close()
    c = ifx.ElasticFusion(w=W, h=H, max_surfels=100000, **K)   # a sharded handle
    c._chk(c.L.ifx_set_shard(c.handle, 0, 2), "ifx_set_shard")
    with pytest.raises(ifx.IfxError, match="sharded") as e:
        ifx.InstanceFusion(c).duplicate_instances()
    assert E_STATE in str(e.value)
    c.close()


def test_sharded_map_equals_the_unsharded_one(ifx, small_stream):
    """two emulated ranks and one GPU after the same segmentation calls, the same crafted votes and the same merge: shards merged by creation number"""
    from conftest import SMALL
    from instancefusion_amd import sharded, synth
    from test_gpu_owner_seg_device import _both, _frame, _device_frames, _merged, _stable

    st, NF = small_stream, 8
    rng = np.random.default_rng(2)
    d_rgb, d_dep = _device_frames(st, NF)
    one = ifx.ElasticFusion(**SMALL, max_surfels=400000)
    efs = [ifx.ElasticFusion(**SMALL, max_surfels=400000, n_ranks=2, rank=r) for r in range(2)]
    for i in range(NF):
        if i == 4:
            _stable(one, efs)
        _frame(one, efs, d_rgb, d_dep, i)
        if i >= 4 and synth.canned_masks(st["obj"][i], st["scene"])[0].shape[0]:
            _both(ifx, one, efs, st, i, "image-u8", -1, rng)
    inst_one = ifx.InstanceFusion(one)
    table = inst_one.getInstanceTable()
    used = np.nonzero(table != -1)[0]
    assert len(used) >= 2, table[:12]                      # (a floor of the scenario: instances to merge)
    pairs = sorted({(int(used[1]), int(used[0])), (int(used[-1]), int(used[0]))})
    m = one.download()                                      # the same crafted votes on both sides: counters in sources and target, first-frame words, large halves
    n = m["votes"].shape[0]
    c = np.zeros((n, NI), np.int64)
    for i in used[:6]:
        c[:, i] = np.where(rng.random(n) < 0.3, rng.integers(1, 300, n), 0)
    c[rng.random(n) < 0.05, used[1]] = 40000
    m["votes"][:] = im.encode_word(c[:, 0::2], c[:, 1::2])
    m["votes"][rng.random(n) < 0.1] = -1.0
    t = inst_one.getLoopClosureInstanceTable()
    colour = ((t[:, 0] << 16) + (t[:, 1] << 8) + t[:, 2]).astype(np.float32)
    m["col"][:, 1] = im.label_scan(m["votes"], m["tm"], np.zeros(n, np.float32), colour)[1]
    pose = one.getCurrPose()
    one.upload(m); one.set_pose(pose, one.tick)
    for e in efs:
        e.upload(m); e.set_pose(pose, one.tick)
    before = one.download()
    e_votes, e_labels, e_col, e_table = im.merge(before["votes"], before["tm"], before["col"][:, 1], table, colour, pairs)
    inst_one.merge_instances(pairs)
    for e in efs:
        sharded.OwnerShardedElasticFusion(e, dist=None, transport="torch").merge_instances(pairs)
    after = one.download()
    assert np.array_equal(im.bits(after["votes"]), im.bits(e_votes)) and np.array_equal(im.bits(after["col"][:, 1]), im.bits(e_col))
    assert (im.bits(e_votes) != im.bits(before["votes"])).any(axis=1).sum() > 100
    assert all(np.array_equal(ifx.InstanceFusion(e).getInstanceTable(), e_table) for e in efs) and np.array_equal(inst_one.getInstanceTable(), e_table)
    assert np.array_equal(im.bits(_merged(efs, lambda e: e.download()["votes"])), im.bits(after["votes"]))
    assert np.array_equal(im.bits(_merged(efs, lambda e: e.download()["col"])), im.bits(after["col"]))
    assert np.array_equal(_merged(efs, lambda e: ifx.InstanceFusion(e).labels()), inst_one.labels())
    for e in efs + [one]:
        e.close()
