"""Deferred segmentation (ifx_segmentation_snapshot / ifx_process_segmentation_deferred[_device]): the masks a slow detector made of frame t, applied at frame
t + k through a snapshot of frame t.  Lag 0 is the ordinary call bit for bit; lag 4 with the camera moving equals the CPU oracle fed the test's own numpy
translation of the frame-t id image; the result does not depend on the slot layout; a snapshot changes nothing for the frames; the refusals leave the handle usable."""
import numpy as np
import pytest

from conftest import SMALL
from seg_deferred_numpy import translate_ids

pytestmark = pytest.mark.gpu

MAP_KEYS = ("pc", "nr", "col", "tm", "ic", "votes")
E_INVALID, E_CAPACITY, E_STATE = -1, -3, -4


@pytest.fixture(scope="module")
def ifx():
    import instancefusion_amd as m

    m.lib()
    return m


def _prepare(e, pose):
    """test_gpu_seg_device_masks._twins' preparation after frame 3 -- every surfel stable -- with the votes cleared too: first-frame surfels carry the reference's
    -1 counters and register almost nothing."""
    m = e.download()
    m["pc"][:, 3] = 20.0
    m["votes"][:] = 0.0
    return m


def _twins(ifx, st, n_frames, **opts):
    a = ifx.ElasticFusion(**SMALL, max_surfels=400000)
    b = ifx.ElasticFusion(**SMALL, max_surfels=400000)
    for e in (a, b):
        for k, v in opts.items():
            e.set_option(k, v)
    for i in range(n_frames):
        pa = a.processFrame(st["rgb"][i], st["depth"][i]); pb = b.processFrame(st["rgb"][i], st["depth"][i])
        assert np.array_equal(pa, pb)
        if i == 3:
            m = _prepare(a, pa)
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


def _shuffled_f32(masks, cls, rng):
    """the canned masks as float32 probabilities in shuffled order (inside > 0.5, outside <= 0.5)"""
    perm = rng.permutation(masks.shape[0])
    inside = rng.uniform(0.6, 1.0, masks.shape).astype(np.float32)
    outside = rng.uniform(0.0, 0.5, masks.shape).astype(np.float32)
    return np.where(masks > 0, inside, outside).astype(np.float32)[perm], np.asarray(cls, np.int32)[perm]


@pytest.mark.parametrize("variant", ["host", "device_f32"])
def test_lag_0_equals_the_ordinary_call(ifx, small_stream, variant):
    """Twins at frames 4..7: snapshot + deferred call at once on one, the ordinary call on the other (superpixels, one call with the kNN smoothing), then new
    classes until the table evicts; then two more frames on both: the call leaves no residue."""
    import torch

    from instancefusion_amd import synth

    st = small_stream
    rng = np.random.default_rng(5)
    a = ifx.ElasticFusion(**SMALL, max_surfels=400000)
    b = ifx.ElasticFusion(**SMALL, max_surfels=400000)
    ia, ib = ifx.InstanceFusion(a), ifx.InstanceFusion(b)

    def both(masks, cls, frame, **kw):
        t = ia.snapshot(superpixels=kw.get("superpixels", False))
        if variant == "host":
            ia.process_segmentation_deferred(t, masks, cls, frame, **kw)
            ib.ProcessSegmentation(None, None, masks, cls, frame, **kw)
        else:
            fm, fc = _shuffled_f32(masks, cls, rng)
            dm, dc = torch.from_numpy(fm).cuda(), torch.from_numpy(fc).cuda()
            ia.process_segmentation_deferred_device(t, dm, dc, frame, **kw)
            ib.process_segmentation_device(dm, dc, frame, **kw)
        assert ia.snapshot_stats(t)["in_use"] == 0          # a successful call releases its ticket

    for i in range(8):
        pa = a.processFrame(st["rgb"][i], st["depth"][i]); pb = b.processFrame(st["rgb"][i], st["depth"][i])
        assert np.array_equal(pa, pb)
        if i == 3:
            m = _prepare(a, pa)
            for e in (a, b):
                e.upload(m); e.set_pose(pa, a.tick)
        if i >= 4:
            masks, cls = synth.canned_masks(st["obj"][i], st["scene"])
            both(masks, cls, 100 + 3 * i, isflann=(i == 6), superpixels=True)
            _same(ia, ib, i)
    assert (ia.labels() >= 0).sum() > 100
    masks, cls = synth.canned_masks(st["obj"][7], st["scene"])
    nm = masks.shape[0]
    evicted = False
    for call in range(60):
        classes = (1000 + call * nm + np.arange(nm)).astype(np.int32)
        before = (ib.getInstanceTable() >= 0).sum()
        both(masks, classes, 300 + 3 * call)
        _same(ia, ib, call)
        evicted = evicted or (ib.getInstanceTable() >= 0).sum() < before
        if evicted:
            break
    assert evicted
    _same_maps(a, b)
    assert np.array_equal(ia.renderProjectMap(), ib.renderProjectMap())
    for i in (8, 9):
        pa = a.processFrame(st["rgb"][i], st["depth"][i]); pb = b.processFrame(st["rgb"][i], st["depth"][i])
        assert np.array_equal(pa, pb), i
    _same_maps(a, b)
    a.close(); b.close()


def _lag4_run(ifx, st, compact_every_frame, superpixels, tickets=1, observe=False):
    """Frames 0..9 with the preparation after frame 3 and `tickets` snapshots after frame 5.  observe: also what the test's own translation needs of frame 5 --
    the id image and the creation numbers, both in download order (taken AFTER the snapshots: seq() compacts the map and re-renders the image, the snapshot has
    pinned the image in the layout the frame left, tombstones and all).  Both seq() here and the download() in front of the oracle compact the map, so against
    the oracle k_seg_translate always finds a compact layout; its liveness rule (a tombstone reads "no surfel") is covered by test_layout_independence, where
    nothing compacts the lazy handle between the snapshot and the call."""
    a = ifx.ElasticFusion(**SMALL, max_surfels=400000)
    a.set_option("compact_every_frame", compact_every_frame)
    ia = ifx.InstanceFusion(a)
    out = dict(a=a, ia=ia)
    for i in range(10):
        p = a.processFrame(st["rgb"][i], st["depth"][i])
        if i == 3:
            a.upload(_prepare(a, p)); a.set_pose(p, a.tick)
        if i == 5:
            out["pose5"] = p.copy()
            out["tickets"] = [ia.snapshot(superpixels=superpixels) for _ in range(tickets)]
            if observe:
                out["slots5"] = a.slots
                raw = a.image("ids_after")
                out["seq5"] = a.seq().copy()
                out["ids5"] = a.image("ids_after")
                assert (raw > 0).sum() == (out["ids5"] > 0).sum()      # the same pixels name a surfel before and after the compaction
                out["live5"] = a.count
    return out


@pytest.mark.parametrize("compact_every_frame", [1, 0])
@pytest.mark.parametrize("flags", [0, 2])
def test_lag_4_equals_the_oracle(ifx, orc, small_stream, flags, compact_every_frame):
    """Snapshot after frame 5, frames 6..9 (the camera moves, surfels die and are created, slots are renumbered), then the deferred call twice (the second call
    matches what the first registered) against the CPU oracle primed with today's map, the pose and frame of frame 5 and the test's own numpy translation of the
    frame-5 id image.  Figures of this input on the CPU oracle: 75 147 id pixels at frame 5, 13 253 of them (17.6 %) name surfels gone by frame 9, 61 357 name
    surfels whose slot moved; the oracle labels 4 681 surfels in 7 instances without superpixels and 647 in 1 with them."""
    from instancefusion_amd import synth

    st = small_stream
    sp = bool(flags & 2)
    r = _lag4_run(ifx, st, compact_every_frame, sp, tickets=2, observe=True)
    a, ia = r["a"], r["ia"]
    if not compact_every_frame:
        assert r["slots5"] > r["live5"]                  # the id image of frame 5 was pinned through tombstones
    m9 = a.download()
    seq9 = a.seq()
    T = translate_ids(r["ids5"], r["seq5"], seq9)
    id_px = int((r["ids5"] > 0).sum())
    lost = int(((r["ids5"] > 0) & (T == 0)).sum())
    moved = int(((r["ids5"] > 0) & (T > 0) & (T != r["ids5"])).sum())
    print(f"id pixels {id_px}, lost {lost} ({100.0 * lost / id_px:.1f} %), slot moved {moved}")
    assert lost >= 0.05 * id_px
    if compact_every_frame:
        assert moved >= 0.5 * id_px
    o = orc.Oracle(**SMALL, max_surfels=400000)
    o.process_frame(st["rgb"][0], np.zeros_like(st["depth"][0]))
    o.upload(m9)
    o.set_pose(r["pose5"], a.tick)
    o.set_frame(st["rgb"][5], st["depth"][5])
    o.set_ids_after(T)
    masks, cls = synth.canned_masks(st["obj"][5], st["scene"])
    for call, t in enumerate(r["tickets"]):
        o.process_segmentation(st["rgb"][5], st["depth"][5], masks, cls, 100, flags)
        ia.process_segmentation_deferred(t, masks, cls, 100, superpixels=sp)
        stats = ia.snapshot_stats(t)
        assert stats["pixels"] == id_px and stats["lost"] == lost, (stats, id_px, lost)
        assert np.array_equal(ia.getInstanceTable(), o.instance_table()), call
        assert np.array_equal(ia.labels(), o.labels()), call
        mg, mo = a.download(), o.download()
        assert np.array_equal(mg["votes"], mo["votes"]), call
        assert np.array_equal(mg["col"], mo["col"]), call
    labelled = int((ia.labels() >= 0).sum())
    print(f"labelled {labelled} in {(ia.getInstanceTable() >= 0).sum()} instances")
    assert labelled >= (100 if sp else 1000)
    a.close(); o.close()


def test_layout_independence(ifx, small_stream):
    """The same lag-4 sequence on a handle that compacts every frame and on a lazy one (tombstones at the snapshot and at the call): labels, votes and colours in
    download order are equal."""
    from instancefusion_amd import synth

    st = small_stream
    masks, cls = synth.canned_masks(st["obj"][5], st["scene"])
    res = []
    for cef in (1, 0):
        r = _lag4_run(ifx, st, cef, True)
        a, ia = r["a"], r["ia"]
        if not cef:
            assert a.slots > a.count                      # the call translates into a layout with tombstones
        ia.process_segmentation_deferred(r["tickets"][0], masks, cls, 100, superpixels=True)
        m = a.download()
        res.append((ia.labels().copy(), m["votes"], m["col"], ia.getInstanceTable().copy()))
        a.close()
    assert (res[0][0] >= 0).sum() >= 100
    for x, y in zip(res[0], res[1]):
        assert np.array_equal(x, y)


def test_a_snapshot_changes_nothing(ifx, small_stream):
    """One twin takes a snapshot after every frame (with and without the frame) and releases the oldest; the others take none: every pose, id image and count over
    the 10 frames and the final map are equal.  Reading the id image completes it on a handle that drew the lattice only (ifx_ids_ensure), which is also what a
    snapshot does: the second twin is read after every frame, the third is never read before the end, so a difference in the lazy-id state cannot hide."""
    st = small_stream
    a = ifx.ElasticFusion(**SMALL, max_surfels=400000)
    b = ifx.ElasticFusion(**SMALL, max_surfels=400000)
    c = ifx.ElasticFusion(**SMALL, max_surfels=400000)
    ia = ifx.InstanceFusion(a)
    held = []
    for i in range(10):
        pa = a.processFrame(st["rgb"][i], st["depth"][i]); pb = b.processFrame(st["rgb"][i], st["depth"][i]); pc = c.processFrame(st["rgb"][i], st["depth"][i])
        assert np.array_equal(pa, pb) and np.array_equal(pa, pc), i
        if len(held) == 4:
            ia.release_snapshot(held.pop(0))
        held.append(ia.snapshot(superpixels=bool(i % 2)))
        s = ia.snapshot_stats(held[-1])
        assert s["tick"] == a.tick and s["lost"] == -1 and s["in_use"] == len(held)
        ids_a = a.image("ids_after")
        assert np.array_equal(ids_a, b.image("ids_after")), i
        assert s["pixels"] == int((ids_a > 0).sum()), i
        assert a.count == b.count == c.count and a.slots == b.slots == c.slots, i
    assert np.array_equal(a.image("ids_after"), c.image("ids_after"))
    _same_maps(a, b)
    _same_maps(a, c)
    a.close(); b.close(); c.close()


def test_refusals(ifx, small_stream):
    """Capacity, unknown / released tickets, a ticket across an upload, superpixels on a ticket taken without the frame; after each refusal an ordinary call on the
    same handle still equals its twin's.  (The sharded handle and the camera contexts: the two tests below.)"""
    from instancefusion_amd import synth

    st = small_stream
    L = ifx.lib()
    a, b, ia, ib = _twins(ifx, st, 6)
    masks, cls = synth.canned_masks(st["obj"][5], st["scene"])
    mp, cp = masks.ctypes.data, np.ascontiguousarray(cls, np.int32)
    frame = [100]

    def deferred(t, flags=0):
        return L.ifx_process_segmentation_deferred(a.handle, t, mp, cp.ctypes.data, masks.shape[0], frame[0], flags)

    def still_usable(what):
        ia.ProcessSegmentation(None, None, masks, cls, frame[0], superpixels=True)
        ib.ProcessSegmentation(None, None, masks, cls, frame[0], superpixels=True)
        _same(ia, ib, what)
        frame[0] += 3

    tickets = [ia.snapshot() for _ in range(4)]
    assert len(set(tickets)) == 4 and min(tickets) >= 0
    assert L.ifx_segmentation_snapshot(a.handle, 0) == E_CAPACITY
    still_usable("capacity")
    ia.release_snapshot(tickets[0])
    assert L.ifx_segmentation_snapshot_release(a.handle, tickets[0]) == E_INVALID
    assert deferred(tickets[0]) == E_INVALID
    assert deferred(12345) == E_INVALID and deferred(-1) == E_INVALID
    still_usable("invalid")
    assert deferred(tickets[1], 2) == E_STATE                 # superpixels on a ticket taken without the frame
    still_usable("superpixels")
    assert deferred(tickets[1], 0) == 0                       # ... the ticket itself is still good
    ib.ProcessSegmentation(None, None, masks, cls, frame[0])  # (lag 0: the ordinary call on the twin)
    _same(ia, ib, "deferred")
    assert ia.snapshot_stats(tickets[2])["in_use"] == 2
    m = a.download()
    pose, tick = a.getCurrPose(), a.tick
    for e in (a, b):
        e.upload(m); e.set_pose(pose, tick)
    assert deferred(tickets[2]) == E_STATE                    # creation numbers renumbered since the ticket was taken
    pa = a.processFrame(st["rgb"][6], st["depth"][6]); pb = b.processFrame(st["rgb"][6], st["depth"][6])   # (id images of the uploaded map on both)
    assert np.array_equal(pa, pb)
    masks, cls = synth.canned_masks(st["obj"][6], st["scene"])
    mp, cp = masks.ctypes.data, np.ascontiguousarray(cls, np.int32)
    assert deferred(tickets[3]) == E_STATE                    # ... and it stays refused; a refused call keeps its ticket
    assert ia.snapshot_stats(tickets[3])["in_use"] == 2
    ia.release_snapshot(tickets[2]); ia.release_snapshot(tickets[3])
    t = ia.snapshot()
    still_usable("upload")
    ia.release_snapshot(t)
    a.set_option("seg_snapshots", 1)
    t = ia.snapshot()
    assert L.ifx_segmentation_snapshot(a.handle, 0) == E_CAPACITY
    ia.release_snapshot(t)
    assert L.ifx_set_option(a.handle, b"seg_snapshots", 9) == E_INVALID
    still_usable("option")
    _same_maps(a, b)
    a.close(); b.close()


def test_refusal_on_a_sharded_handle(ifx, small_stream):
    """A sharded handle (n_ranks = -1: a world of one, the collectives inside the library) refuses every entry with IFX_E_STATE; the frame and the segmentation call
    that follow still equal the unsharded twin's (test_owner_sharded_rccl_world_of_one_in_library's sequence)."""
    import torch

    from instancefusion_amd import sharded, synth

    st = small_stream
    L = ifx.lib()
    d_rgb = torch.from_numpy(st["rgb"][:8].copy()).cuda()
    d_dep = torch.from_numpy(st["depth"][:8].view(np.int16).copy()).cuda()
    torch.cuda.synchronize()
    one = ifx.ElasticFusion(**SMALL, max_surfels=400000)
    ef = ifx.ElasticFusion(**SMALL, max_surfels=400000, n_ranks=-1, rank=0)
    osh = sharded.OwnerShardedElasticFusion(ef, None)
    inst_one, inst = ifx.InstanceFusion(one), ifx.InstanceFusion(ef)

    def refused():
        masks, cls = synth.canned_masks(st["obj"][5], st["scene"])
        cp = np.ascontiguousarray(cls, np.int32)
        assert L.ifx_segmentation_snapshot(ef.handle, 0) == E_STATE and b"sharded" in L.ifx_last_error(ef.handle)
        assert L.ifx_segmentation_snapshot(ef.handle, 2) == E_STATE
        assert L.ifx_process_segmentation_deferred(ef.handle, 0, masks.ctypes.data, cp.ctypes.data, masks.shape[0], 100, 0) == E_STATE
        assert b"sharded" in L.ifx_last_error(ef.handle)

    refused()                                                  # before any frame
    for i in range(8):
        if i == 4:
            m = one.download(); m["pc"][:, 3] = 20.0; m["votes"][:] = 0.0
            pose = one.getCurrPose()
            one.upload(m); one.set_pose(pose, one.tick); one.combined_predict(pose, one.tick, one.tick)
            ef.upload(m); ef.set_pose(pose, one.tick)
            osh.predict()
        one.enqueue_frame_device(d_rgb[i].data_ptr(), d_dep[i].data_ptr(), i)
        osh.process_frame_device(d_rgb[i].data_ptr(), d_dep[i].data_ptr())
        assert np.array_equal(ef.getCurrPose(), one.getCurrPose()), i
        if i >= 5:
            refused()                                          # between a frame and its segmentation call
            masks, cls = synth.canned_masks(st["obj"][i], st["scene"])
            inst_one.ProcessSegmentation(st["rgb"][i], st["depth"][i], masks, cls, i, superpixels=True)
            osh.process_segmentation(st["rgb"][i], st["depth"][i], masks, cls, i, superpixels=True)
            refused()
            assert np.array_equal(inst.getInstanceTable(), inst_one.getInstanceTable()), i
            assert np.array_equal(inst.labels()[np.argsort(ef.seq(), kind="stable")], inst_one.labels()), i
    assert (inst_one.labels() >= 0).sum() > 100
    ef.close(); one.close()


def test_refusal_with_two_camera_contexts(ifx, small_stream):
    """A handle with more than one camera context refuses a snapshot (IFX_E_STATE); an ordinary call on it still equals its twin's."""
    from instancefusion_amd import synth

    st = small_stream
    L = ifx.lib()
    a, b, ia, ib = _twins(ifx, st, 6)
    for e in (a, b):
        e.camera_count(2)
    assert L.ifx_segmentation_snapshot(a.handle, 0) == E_STATE and b"camera" in L.ifx_last_error(a.handle)
    masks, cls = synth.canned_masks(st["obj"][5], st["scene"])
    ia.ProcessSegmentation(st["rgb"][5], st["depth"][5], masks, cls, 100, superpixels=True)
    ib.ProcessSegmentation(st["rgb"][5], st["depth"][5], masks, cls, 100, superpixels=True)
    _same(ia, ib, "cameras")
    assert (ia.getInstanceTable() >= 0).sum() >= 1
    _same_maps(a, b)
    a.close(); b.close()
