"""Deferred segmentation on a spatially sharded map (ifx_owner_segmentation_snapshot / ifx_owner_segmentation_begin_deferred[_device] and the one-call forms):
emulated ranks in one process.  Lag 0 is the ordinary sharded call bit for bit; lag 4 with the camera moving equals the unsharded deferred call (maps merged by
creation number); the result does not depend on the shards' slot layout; the per-rank image equals its numpy statement; edges; refusals; a world of one through
the library's communicator.  All comparisons are equalities."""
import numpy as np
import pytest

from conftest import SMALL
from seg_deferred_owner_numpy import lost_owner, translate_ids_owner

pytestmark = pytest.mark.gpu

MAP_KEYS = ("pc", "nr", "col", "tm", "ic", "votes")
E_INVALID, E_CAPACITY, E_STATE = -1, -3, -4


@pytest.fixture(scope="module")
def ifx():
    import instancefusion_amd as m

    m.lib()
    return m


def _device_frames(st, n=10):
    import torch

    d = torch.from_numpy(st["rgb"][:n].copy()).cuda(), torch.from_numpy(st["depth"][:n].view(np.int16).copy()).cuda()
    torch.cuda.synchronize()
    return d


def _prepare(one, groups, reorder=None):
    """tests/test_gpu_seg_deferred.py::_prepare on the unsharded handle and every set of ranks: every surfel stable, votes cleared (reorder: a permutation of the rows)"""
    from instancefusion_amd import sharded

    m = one.download()
    m["pc"][:, 3] = 20.0
    m["votes"][:] = 0.0
    if reorder is not None:
        m = {k: np.ascontiguousarray(v[reorder]) for k, v in m.items()}
    pose = one.getCurrPose()
    one.upload(m); one.set_pose(pose, one.tick); one.combined_predict(pose, one.tick, one.tick)
    for efs in groups:
        for e in efs:
            e.upload(m); e.set_pose(pose, one.tick)
        sharded.emulate_owner_predict(efs)


def _frame(one, groups, d, i):
    from instancefusion_amd import sharded

    one.enqueue_frame_device(d[0][i].data_ptr(), d[1][i].data_ptr(), i)
    for efs in groups:
        sharded.emulate_owner_ranks(efs, d[0][i].data_ptr(), d[1][i].data_ptr())


def _ranks(ifx, G, **opts):
    efs = [ifx.ElasticFusion(**SMALL, max_surfels=400000, n_ranks=G, rank=r) for r in range(G)]
    for e in efs:
        for k, v in opts.items():
            e.set_option(k, v)
    return efs


def _merged(efs, of):
    parts = [(e.seq(), of(e)) for e in efs]
    seq = np.concatenate([p[0] for p in parts])
    return np.concatenate([p[1] for p in parts])[np.argsort(seq, kind="stable")]


def _equals_unsharded(ifx, one, efs, what):
    """tables on every rank, and -- merged by creation number -- the map and the labels, against the unsharded handle"""
    io = ifx.InstanceFusion(one)
    for e in efs:
        ie = ifx.InstanceFusion(e)
        assert np.array_equal(ie.getInstanceTable(), io.getInstanceTable()), what
        assert np.array_equal(ie.getLoopClosureInstanceTable(), io.getLoopClosureInstanceTable()), what
    assert np.array_equal(_merged(efs, lambda e: ifx.InstanceFusion(e).labels()), io.labels()), what
    parts = [(e.seq(), e.download()) for e in efs]
    order = np.argsort(np.concatenate([p[0] for p in parts]), kind="stable")
    mo = one.download()
    for k in MAP_KEYS:
        assert np.array_equal(np.concatenate([p[1][k] for p in parts])[order], mo[k]), (what, k)


def _same_ranks(ifx, A, B, what, maps=True):
    for a, b in zip(A, B):
        ia, ib = ifx.InstanceFusion(a), ifx.InstanceFusion(b)
        assert np.array_equal(ia.getInstanceTable(), ib.getInstanceTable()), what
        assert np.array_equal(ia.getLoopClosureInstanceTable(), ib.getLoopClosureInstanceTable()), what
        assert np.array_equal(ia.labels(), ib.labels()), what
        if maps:
            ma, mb = a.download(), b.download()
            for k in MAP_KEYS:
                assert np.array_equal(ma[k], mb[k]), (what, k)


def _shuffled_f32(masks, cls, rng):
    """the canned masks as float32 probabilities in shuffled order (inside > 0.5, outside <= 0.5)"""
    perm = rng.permutation(masks.shape[0])
    inside = rng.uniform(0.6, 1.0, masks.shape).astype(np.float32)
    outside = rng.uniform(0.0, 0.5, masks.shape).astype(np.float32)
    return np.where(masks > 0, inside, outside).astype(np.float32)[perm], np.asarray(cls, np.int32)[perm]


def _stats(ifx, e, t):
    return ifx.InstanceFusion(e).snapshot_stats(t)


@pytest.mark.parametrize("lazy_ids", [0, 1])
@pytest.mark.parametrize("variant", ["host", "device_root0", "device_all"])
def test_lag_0_equals_the_ordinary_sharded_call(ifx, small_stream, variant, lazy_ids):
    """Two sets of two ranks at frames 4..7: snapshot + deferred call at once on one, the ordinary sharded call on the other (superpixels on), then new classes
    until the table evicts; then two more frames on both: the call leaves no residue."""
    import torch

    from instancefusion_amd import sharded, synth

    st = small_stream
    rng = np.random.default_rng(7)
    d = _device_frames(st)
    one = ifx.ElasticFusion(**SMALL, max_surfels=400000)            # (only the source of the prepared map)
    A, B = _ranks(ifx, 2, own_lazy_ids=lazy_ids, own_key_rs=lazy_ids), _ranks(ifx, 2, own_lazy_ids=lazy_ids, own_key_rs=lazy_ids)
    root = 0 if variant == "device_root0" else -1

    def both(i, masks, cls, frame, superpixels):
        tk = sharded.emulate_owner_snapshot(A, superpixels)
        assert len(set(tk)) == 1 and tk[0] >= 0
        if variant == "host":
            sharded.emulate_owner_segmentation_deferred(A, tk, masks, cls, frame, superpixels)
            sharded.emulate_owner_segmentation(B, st["rgb"][i], st["depth"][i], masks, cls, frame, superpixels)
        else:
            fm, fc = _shuffled_f32(masks, cls, rng)
            dm = torch.from_numpy(fm).cuda()
            sharded.emulate_owner_segmentation_deferred_device(A, tk, root, dm, fc, frame, superpixels, max_n=32)
            sharded.emulate_owner_segmentation_device(B, root, st["rgb"][i], st["depth"][i], dm, fc, frame, superpixels, max_n=32)
        for e, t in zip(A, tk):
            assert _stats(ifx, e, t)["in_use"] == 0              # a call that completes releases its ticket on every rank

    for i in range(8):
        if i == 4:
            _prepare(one, (A, B))
        _frame(one, (A, B), d, i)
        assert np.array_equal(A[0].getCurrPose(), B[0].getCurrPose()), i
        if i >= 4:
            masks, cls = synth.canned_masks(st["obj"][i], st["scene"])
            both(i, masks, cls, 100 + 3 * i, True)
            _same_ranks(ifx, A, B, i)
    assert sum(int((ifx.InstanceFusion(e).labels() >= 0).sum()) for e in A) > 100
    masks, cls = synth.canned_masks(st["obj"][7], st["scene"])
    nm = masks.shape[0]
    evicted = False
    for call in range(60):
        classes = (1000 + call * nm + np.arange(nm)).astype(np.int32)
        before = (ifx.InstanceFusion(B[0]).getInstanceTable() >= 0).sum()
        both(7, masks, classes, 300 + 3 * call, False)
        _same_ranks(ifx, A, B, call, maps=False)
        evicted = evicted or (ifx.InstanceFusion(B[0]).getInstanceTable() >= 0).sum() < before
        if evicted:
            break
    assert evicted
    _same_ranks(ifx, A, B, "evicted")
    for i in (8, 9):
        _frame(one, (A, B), d, i)
        for a, b in zip(A, B):
            assert np.array_equal(a.getCurrPose(), b.getCurrPose()), i
    _same_ranks(ifx, A, B, "two more frames")
    for e in A + B + [one]:
        e.close()


def _lag4(ifx, st, G, superpixels, rank_opts=None, compact_before_call=False, observe=False):
    """Frames 0..9 on an unsharded handle and G ranks with the preparation in front of frame 4, a snapshot after frame 5 on both, the deferred call (host form)
    after frame 9 on both; asserts the comparison with the unsharded handle and returns what the callers look at."""
    from instancefusion_amd import sharded, synth

    d = _device_frames(st)
    one = ifx.ElasticFusion(**SMALL, max_surfels=400000)
    io = ifx.InstanceFusion(one)
    efs = _ranks(ifx, G, **(rank_opts or {}))
    out = dict(one=one, efs=efs)
    for i in range(10):
        if i == 4:
            _prepare(one, (efs,))
        _frame(one, (efs,), d, i)
        if i == 5:
            t_one = io.snapshot(superpixels=superpixels)
            tk = sharded.emulate_owner_snapshot(efs, superpixels)
            assert len(set(tk)) == 1
            if observe:   # (after the snapshot: seq() compacts the shard; the ticket pinned the layout the frame left)
                out["pinned"] = efs[0].image("ids_after")
                assert all(np.array_equal(e.image("ids_after"), out["pinned"]) for e in efs)
                out["seq5"] = [e.seq().copy() for e in efs]
    assert np.array_equal(efs[0].getCurrPose(), one.getCurrPose())
    if compact_before_call:
        for e in efs:
            e.compact()
    out["tombstones"] = [e.slots - e.count for e in efs]
    masks, cls = synth.canned_masks(st["obj"][5], st["scene"])
    io.process_segmentation_deferred(t_one, masks, cls, 100, superpixels=superpixels)
    sharded.emulate_owner_segmentation_deferred(efs, tk, masks, cls, 100, superpixels)
    out["snap_ids"] = [e.image("snap_ids") for e in efs]
    s_one = io.snapshot_stats(t_one)
    s_efs = [_stats(ifx, e, t) for e, t in zip(efs, tk)]
    print(f"G {G}: unsharded pixels {s_one['pixels']} lost {s_one['lost']}; ranks lost {[s['lost'] for s in s_efs]}")
    assert all(s["pixels"] == s_one["pixels"] and s["in_use"] == 0 and s["tick"] == s_one["tick"] for s in s_efs), (s_one, s_efs)
    assert sum(s["lost"] for s in s_efs) == s_one["lost"], (s_one, s_efs)
    assert s_one["lost"] >= 0.05 * s_one["pixels"]               # the comparison is not vacuous: the map moved on under the ticket
    _equals_unsharded(ifx, one, efs, ("lag 4", G, superpixels))
    out["stats"] = s_efs
    out["labelled"] = int((io.labels() >= 0).sum())
    return out


def _close(r):
    for e in r["efs"] + [r["one"]]:
        e.close()


@pytest.mark.parametrize("superpixels", [True, False])
@pytest.mark.parametrize("G", [2, 3])
def test_lag_4_equals_the_unsharded_deferred_call(ifx, small_stream, G, superpixels):
    """Snapshot after frame 5 on the ranks and on an unsharded handle, frames 6..9 (the camera moves, surfels die and are created, slots are renumbered), the
    deferred call on both: tables, labels and maps merged by creation number are equal; `pixels` is the unsharded figure on every rank, the ranks' `lost` sum to it."""
    r = _lag4(ifx, small_stream, G, superpixels)
    assert r["labelled"] >= (100 if superpixels else 1000)
    _close(r)


def test_layout_independence(ifx, small_stream):
    """The lag-4 sequence on ranks that compact every frame and on lazy ones (tombstones at the snapshot and at the call, nothing compacting them in between: the
    gallop and the liveness rule on a non-compact shard): both equal the unsharded call, hence each other."""
    res = []
    for cef in (1, 0):
        r = _lag4(ifx, small_stream, 2, True, rank_opts=dict(compact_every_frame=cef))
        if cef:
            assert r["tombstones"] == [0, 0]
        else:
            assert min(r["tombstones"]) > 0                      # every rank translated into a layout with tombstones
        res.append((_merged(r["efs"], lambda e: ifx.InstanceFusion(e).labels()), _merged(r["efs"], lambda e: e.download()["votes"]),
                    _merged(r["efs"], lambda e: e.download()["col"]), ifx.InstanceFusion(r["efs"][0]).getInstanceTable().copy()))
        _close(r)
    assert (res[0][0] >= 0).sum() >= 100
    for x, y in zip(res[0], res[1]):
        assert np.array_equal(x, y)


def test_the_translated_image_equals_the_numpy_statement(ifx, small_stream):
    """One lag-4 case on compacted shards (slot = index in seq() order, every slot alive): each rank's image, read back, is tests/seg_deferred_owner_numpy.py's, and
    so is its `lost`."""
    r = _lag4(ifx, small_stream, 2, False, compact_before_call=True, observe=True)
    assert r["tombstones"] == [0, 0]
    seqs = [e.seq() for e in r["efs"]]
    surfel0 = min(int(s[0]) for s in seqs if s.size)
    kept = np.zeros(r["pinned"].shape, bool)
    for k, e in enumerate(r["efs"]):
        T = translate_ids_owner(r["pinned"], seqs[k], np.ones(seqs[k].size, bool), surfel0)
        assert np.array_equal(r["snap_ids"][k], T), k
        assert r["stats"][k]["lost"] == lost_owner(r["pinned"], r["seq5"][k], seqs[k], np.ones(seqs[k].size, bool), surfel0), k
        assert not (kept & (T > 0)).any()
        kept |= T > 0
    assert kept.sum() > 10000
    _close(r)


def test_edges(ifx, small_stream):
    """Two tickets outstanding, applied in reverse order; a mask set under which one rank owns no surfel; n == 0."""
    from instancefusion_amd import sharded, synth

    st = small_stream
    d = _device_frames(st)
    one = ifx.ElasticFusion(**SMALL, max_surfels=400000)
    io = ifx.InstanceFusion(one)
    efs = _ranks(ifx, 2)
    t_one, tk = {}, {}
    for i in range(10):
        if i == 4:
            _prepare(one, (efs,))
        _frame(one, (efs,), d, i)
        if i in (5, 7):
            t_one[i] = io.snapshot(superpixels=True)
            tk[i] = sharded.emulate_owner_snapshot(efs, True)
    assert all(_stats(ifx, e, tk[7][k])["in_use"] == 2 for k, e in enumerate(efs))
    # reverse order: the younger ticket first
    for i, frame in ((7, 100), (5, 103)):
        masks, cls = synth.canned_masks(st["obj"][i], st["scene"])
        io.process_segmentation_deferred(t_one[i], masks, cls, frame, superpixels=True)
        sharded.emulate_owner_segmentation_deferred(efs, tk[i], masks, cls, frame, True)
        _equals_unsharded(ifx, one, efs, ("reverse", i))
    assert all(_stats(ifx, e, tk[5][k])["in_use"] == 0 for k, e in enumerate(efs))
    assert (io.labels() >= 0).sum() > 100
    # one rank owns nothing under the mask: the largest connected piece of a canned mask all of whose surfels rank 0 owns (the owner is the parity of an 8 cm
    # voxel: such pieces are stripes); rank 1 still takes part in every exchange
    from scipy import ndimage

    t1 = io.snapshot()
    tq = sharded.emulate_owner_snapshot(efs)
    pinned = efs[0].image("ids_after").view(np.uint32)
    own0 = np.isin(pinned, efs[0].seq()) & (pinned != 0)
    canned, _ = synth.canned_masks(st["obj"][9], st["scene"])
    lab, _ = ndimage.label((canned > 0).any(0) & own0)
    sizes = np.bincount(lab.ravel())[1:]
    masks = (255 * (lab == 1 + int(np.argmax(sizes)))).astype(np.uint8)[None]
    assert sizes.max() >= 300, sizes.max()
    votes = [e.download()["votes"].copy() for e in efs]
    classes = np.array([5000], np.int32)
    io.process_segmentation_deferred(t1, masks, classes, 106)
    sharded.emulate_owner_segmentation_deferred(efs, tq, masks, classes, 106)
    _equals_unsharded(ifx, one, efs, "one rank owns nothing")
    assert np.array_equal(efs[1].download()["votes"], votes[1])      # nothing of rank 1 was voted for ...
    assert not np.array_equal(efs[0].download()["votes"], votes[0])  # ... while rank 0's surfels were
    # n == 0 releases the ticket on every rank, and changes nothing
    tq = sharded.emulate_owner_snapshot(efs)
    sharded.emulate_owner_segmentation_deferred(efs, tq, np.zeros((0, SMALL["h"], SMALL["w"]), np.uint8), np.zeros(0, np.int32), 109)
    assert all(_stats(ifx, e, tq[k])["in_use"] == 0 for k, e in enumerate(efs))
    _equals_unsharded(ifx, one, efs, "n == 0")
    for e in efs + [one]:
        e.close()


def test_slot_0_of_a_shard_receives_its_votes(ifx, small_stream):
    """A surfel at slot 0 of a shard that is not the global "surfel 0": the prepared map is uploaded with eight surfels from well inside the largest mask moved to
    rows 1..8, so that the rank that does not own row 0 has one of them at its slot 0.  After a deferred call at lag 2 that surfel carries the unsharded
    handle's votes, and they are votes."""
    from instancefusion_amd import sharded, synth

    st = small_stream
    d = _device_frames(st)
    one = ifx.ElasticFusion(**SMALL, max_surfels=400000)
    io = ifx.InstanceFusion(one)
    efs = _ranks(ifx, 2)
    for i in range(8):
        if i == 4:
            _prepare(one, (efs,))
        if i == 5:   # the id image of frame 4 shows the stable map: upload it again with eight surfels seen well inside the largest mask at rows 1..8
            n = one.seq().size                                   # (compacts, and the image is drawn again in those slots: ids = rows of download())
            ids4 = one.image("ids_after")
            inside = np.ones(ids4.shape, bool)
            for j in (4, 5):                                     # ... at frames 4 and 5: still under it when the snapshot is taken
                big = synth.canned_masks(st["obj"][j], st["scene"])[0][0] > 0
                for dy in (-6, 0, 6):
                    for dx in (-6, 0, 6):
                        inside &= np.roll(np.roll(big, dy, 0), dx, 1)
            cand = np.unique(ids4[inside & (ids4 > 8) & (ids4 < n)])
            assert cand.size >= 8, cand.size
            pick = cand[np.linspace(0, cand.size - 1, 8).astype(int)]
            rest = np.setdiff1d(np.arange(1, n), pick)
            _prepare(one, (efs,), reorder=np.concatenate([[0], pick, rest]))
        _frame(one, (efs,), d, i)
        if i == 5:
            t_one = io.snapshot()
            tk = sharded.emulate_owner_snapshot(efs)
    firsts = [int(e.seq()[0]) for e in efs]
    r = int(np.argmax(firsts))                                   # the rank that does not hold creation number 0
    assert min(firsts) == 0 and 1 <= firsts[r] <= 8, firsts
    masks, cls = synth.canned_masks(st["obj"][5], st["scene"])
    io.process_segmentation_deferred(t_one, masks, cls, 100)
    sharded.emulate_owner_segmentation_deferred(efs, tk, masks, cls, 100)
    _equals_unsharded(ifx, one, efs, "slot 0")
    assert int(efs[r].seq()[0]) == firsts[r]                     # still the shard's slot 0
    v_rank = efs[r].download()["votes"][0]
    v_one = one.download()["votes"][int(np.searchsorted(one.seq(), firsts[r]))]
    assert np.array_equal(v_rank, v_one)
    assert (v_rank.view(np.uint32) != 0).any()                   # it was voted for
    for e in efs + [one]:
        e.close()


def test_refusals(ifx, small_stream):
    """Every refusal of the new entries: nothing is enqueued, ifx_last_error starts with the entry's name, and a frame and an ordinary segmentation call on the
    same handles still equal the unsharded twin's.  The old-named entries keep refusing a sharded handle."""
    import torch

    from instancefusion_amd import sharded, synth

    st = small_stream
    L = ifx.lib()
    d = _device_frames(st)
    one = ifx.ElasticFusion(**SMALL, max_surfels=400000)
    io = ifx.InstanceFusion(one)
    efs = _ranks(ifx, 2)
    SNAP, BEGIN, BEGIN_DEV = "ifx_owner_segmentation_snapshot", "ifx_owner_segmentation_begin_deferred", "ifx_owner_segmentation_begin_deferred_device"
    masks, cls = synth.canned_masks(st["obj"][5], st["scene"])
    cp = np.ascontiguousarray(cls, np.int32)
    nm = masks.shape[0]
    dm = torch.from_numpy(masks).cuda()
    dc = torch.from_numpy(cp).cuda()
    torch.cuda.synchronize()

    def refused(code, name, call, handles=None):
        for e in handles or efs:
            assert call(e) == code, (name, code)
            assert L.ifx_last_error(e.handle).decode().startswith(name), L.ifx_last_error(e.handle)

    def snap(flags=0):
        return lambda e: L.ifx_owner_segmentation_snapshot(e.handle, flags)

    def begin(t, flags=0, n=nm, mp=masks.ctypes.data, cptr=cp.ctypes.data):
        return lambda e: L.ifx_owner_segmentation_begin_deferred(e.handle, t, mp, cptr, n, 100, flags)

    def begin_dev(t, root=-1, max_n=32, fmt=0, flags=0, n=nm):
        return lambda e: L.ifx_owner_segmentation_begin_deferred_device(e.handle, t, root, max_n, dm.data_ptr(), fmt, 0.5, dc.data_ptr(), n, 100, flags, None)

    # no frame processed yet; more than one camera context
    refused(E_STATE, SNAP, snap())
    refused(E_STATE, BEGIN, begin(0))
    refused(E_STATE, BEGIN_DEV, begin_dev(0))
    cams = _ranks(ifx, 2)
    for e in cams:
        e.camera_count(2)
    refused(E_STATE, SNAP, snap(), cams)
    refused(E_STATE, BEGIN, begin(0), cams)
    assert b"camera" in L.ifx_last_error(cams[0].handle)
    for e in cams:
        e.close()
    for i in range(6):
        if i == 4:
            _prepare(one, (efs,))
        _frame(one, (efs,), d, i)
    step = [6, 100]

    def still_usable(what):
        i = min(step[0], 9)
        _frame(one, (efs,), d, i)
        m_, c_ = synth.canned_masks(st["obj"][i], st["scene"])
        io.ProcessSegmentation(st["rgb"][i], st["depth"][i], m_, c_, step[1], superpixels=True)
        sharded.emulate_owner_segmentation(efs, st["rgb"][i], st["depth"][i], m_, c_, step[1], True)
        for e in efs:
            assert np.array_equal(ifx.InstanceFusion(e).getInstanceTable(), io.getInstanceTable()), what
        assert np.array_equal(_merged(efs, lambda e: ifx.InstanceFusion(e).labels()), io.labels()), what
        step[0] += 1; step[1] += 3

    # an unsharded handle; the old-named entries on a sharded one
    refused(E_STATE, SNAP, snap(), [one])
    refused(E_STATE, BEGIN, begin(0), [one])
    refused(E_STATE, BEGIN_DEV, begin_dev(0), [one])
    for e in efs:
        assert L.ifx_segmentation_snapshot(e.handle, 0) == E_STATE and b"sharded" in L.ifx_last_error(e.handle)
        assert L.ifx_process_segmentation_deferred(e.handle, 0, masks.ctypes.data, cp.ctypes.data, nm, 100, 0) == E_STATE
    still_usable("mode")
    # capacity
    tickets = [sharded.emulate_owner_snapshot(efs)[0] for _ in range(4)]
    assert len(set(tickets)) == 4 and min(tickets) >= 0
    refused(E_CAPACITY, SNAP, snap())
    still_usable("capacity")
    # unknown and released tickets, flags bit 0, the arguments
    for e in efs:
        ifx.InstanceFusion(e).release_snapshot(tickets[0])
    for t in (tickets[0], 12345, -1):
        refused(E_INVALID, BEGIN, begin(t))
        refused(E_INVALID, BEGIN_DEV, begin_dev(t))
    still_usable("ticket")
    refused(E_INVALID, BEGIN, begin(tickets[1], flags=1))
    refused(E_INVALID, BEGIN_DEV, begin_dev(tickets[1], flags=1))
    refused(E_INVALID, SNAP, snap(4))
    still_usable("flags")
    refused(E_INVALID, BEGIN, begin(tickets[1], n=-1))
    refused(E_INVALID, BEGIN, begin(tickets[1], n=257))
    refused(E_INVALID, BEGIN, begin(tickets[1], mp=None))
    refused(E_INVALID, BEGIN, begin(tickets[1], cptr=None))
    refused(E_INVALID, BEGIN_DEV, begin_dev(tickets[1], root=2))
    refused(E_INVALID, BEGIN_DEV, begin_dev(tickets[1], root=-2))
    refused(E_INVALID, BEGIN_DEV, begin_dev(tickets[1], max_n=0))
    refused(E_INVALID, BEGIN_DEV, begin_dev(tickets[1], max_n=nm - 1))
    refused(E_INVALID, BEGIN_DEV, begin_dev(tickets[1], fmt=7))
    still_usable("arguments")
    # superpixels on a ticket taken without its frame
    refused(E_STATE, BEGIN, begin(tickets[1], flags=2))
    refused(E_STATE, BEGIN_DEV, begin_dev(tickets[1], flags=2))
    still_usable("superpixels")
    # a call in flight
    rs = [sharded._seg_begin(e, st["rgb"][5], st["depth"][5], masks, cls, 100, False) for e in efs]
    assert rs == [1, 1]
    refused(E_STATE, SNAP, snap())
    refused(E_STATE, BEGIN, begin(tickets[1]))
    refused(E_STATE, BEGIN_DEV, begin_dev(tickets[1]))
    for e in efs:
        assert L.ifx_owner_segmentation_abort(e.handle) == 0
    assert all(_stats(ifx, e, tickets[1])["in_use"] == 3 for e in efs)   # a refused call keeps its ticket
    still_usable("in flight")
    # ... the ticket itself is still good (lag: the frames of still_usable), against the unsharded deferred call on a twin's ticket of its own
    # a ticket older than an upload
    m = one.download()
    pose, tick = one.getCurrPose(), one.tick
    one.upload(m); one.set_pose(pose, tick); one.combined_predict(pose, tick, tick)
    for e in efs:
        e.upload(m); e.set_pose(pose, tick)
    sharded.emulate_owner_predict(efs)
    refused(E_STATE, BEGIN, begin(tickets[1]))
    refused(E_STATE, BEGIN_DEV, begin_dev(tickets[2]))
    assert all(_stats(ifx, e, tickets[2])["in_use"] == 3 for e in efs)
    still_usable("upload")
    for t in tickets[1:]:
        for e in efs:
            ifx.InstanceFusion(e).release_snapshot(t)
    # a fresh ticket works after all of it
    t_one = io.snapshot()
    tk = sharded.emulate_owner_snapshot(efs)
    m_, c_ = synth.canned_masks(st["obj"][9], st["scene"])
    io.process_segmentation_deferred(t_one, m_, c_, 400)
    sharded.emulate_owner_segmentation_deferred(efs, tk, m_, c_, 400)
    _equals_unsharded(ifx, one, efs, "after the refusals")
    for e in efs + [one]:
        e.close()


def test_owner_deferred_rccl_world_of_one(ifx, small_stream):
    """n_ranks = -1 with the library's communicator: ifx_owner_process_segmentation_deferred and _deferred_device at lag 4 against the unsharded deferred call."""
    import torch

    from instancefusion_amd import sharded, synth

    st = small_stream
    rng = np.random.default_rng(11)
    d = _device_frames(st)
    one = ifx.ElasticFusion(**SMALL, max_surfels=400000)
    ef = ifx.ElasticFusion(**SMALL, max_surfels=400000, n_ranks=-1, rank=0)
    osh = sharded.OwnerShardedElasticFusion(ef, None)
    io = ifx.InstanceFusion(one)
    for i in range(10):
        if i == 4:
            m = one.download(); m["pc"][:, 3] = 20.0; m["votes"][:] = 0.0
            pose = one.getCurrPose()
            one.upload(m); one.set_pose(pose, one.tick); one.combined_predict(pose, one.tick, one.tick)
            ef.upload(m); ef.set_pose(pose, one.tick)
            osh.predict()
        one.enqueue_frame_device(d[0][i].data_ptr(), d[1][i].data_ptr(), i)
        osh.process_frame_device(d[0][i].data_ptr(), d[1][i].data_ptr())
        if i == 5:
            t_one = [io.snapshot(superpixels=True), io.snapshot()]
            t_ef = [osh.snapshot(superpixels=True), osh.snapshot()]
            assert t_ef[0] != t_ef[1]
    assert np.array_equal(ef.getCurrPose(), one.getCurrPose())
    masks, cls = synth.canned_masks(st["obj"][5], st["scene"])
    io.process_segmentation_deferred(t_one[0], masks, cls, 100, superpixels=True)
    osh.process_segmentation_deferred(t_ef[0], masks, cls, 100, superpixels=True)
    s_one, s_ef = io.snapshot_stats(t_one[0]), osh.snapshot_stats(t_ef[0])
    assert (s_ef["pixels"], s_ef["lost"], s_ef["in_use"]) == (s_one["pixels"], s_one["lost"], 1), (s_one, s_ef)
    _equals_unsharded(ifx, one, [ef], "host form")
    fm, fc = _shuffled_f32(masks, (3000 + np.arange(masks.shape[0])).astype(np.int32), rng)
    dm = torch.from_numpy(fm).cuda()
    io.process_segmentation_deferred_device(t_one[1], dm, fc, 103)
    osh.process_segmentation_deferred_device(t_ef[1], dm, fc, 103, root=0, max_n=32)
    assert osh.snapshot_stats(t_ef[1])["in_use"] == 0
    _equals_unsharded(ifx, one, [ef], "device form")
    assert (io.labels() >= 0).sum() > 100
    ef.close(); one.close()
