"""The device forms of a segmentation call on the spatially sharded map (ifx_owner_segmentation_begin_device / _rois / _detections and their one-call twins): the
detector's tensors on one rank's GPU (root) or on every rank (root = -1), emulated ranks in one process -- against one GPU, against the host form on the same
ranks, the record word for word against its numpy restatement (tests/owner_seg_record_numpy.py), the edges of the call, the refusals, and a world of one through
the library's communicator.  All comparisons are equalities."""
import ctypes as C

import numpy as np
import pytest

import mask_bridge_numpy as mb
import owner_seg_record_numpy as rec
from conftest import SMALL
from test_gpu_mask_head import _head_case
from test_gpu_seg_rois import _misaligned, _roi_case

pytestmark = pytest.mark.gpu

ODD = dict(w=324, h=244, fx=264.0, fy=264.0, cx=162.0, cy=122.0)   # P = 79 056: P % 32 == 16
E_INVALID, E_CAPACITY, E_STATE = "(-1)", "(-3)", "(-4)"


@pytest.fixture(scope="module")
def ifx():
    import instancefusion_amd as m

    m.lib()
    return m


def _stable(one, efs):
    """every surfel stable (confidence 20): from here on the id image is populated and the masks find surfels to vote for"""
    from instancefusion_amd import sharded

    m = one.download()
    m["pc"][:, 3] = 20.0
    pose = one.getCurrPose()
    one.upload(m); one.set_pose(pose, one.tick); one.combined_predict(pose, one.tick, one.tick)
    for e in efs:
        e.upload(m)
        e.set_pose(pose, one.tick)
    sharded.emulate_owner_predict(efs)


def _frame(one, efs, d_rgb, d_dep, i):
    from instancefusion_amd import sharded

    if one is not None:
        one.enqueue_frame_device(d_rgb[i].data_ptr(), d_dep[i].data_ptr(), i)
    sharded.emulate_owner_ranks(efs, d_rgb[i].data_ptr(), d_dep[i].data_ptr())


def _device_frames(st, n):
    import torch

    return torch.from_numpy(st["rgb"][:n].copy()).cuda(), torch.from_numpy(st["depth"][:n].view(np.int16).copy()).cuda()


def _ranks(ifx, st, cfg, world, n_frames, stable_at, with_one=True):
    """an unsharded handle (or none) and `world` emulated ranks after n_frames frames, the map made stable in front of frame stable_at"""
    d_rgb, d_dep = _device_frames(st, n_frames)
    one = ifx.ElasticFusion(**cfg, max_surfels=400000)
    efs = [ifx.ElasticFusion(**cfg, max_surfels=400000, n_ranks=world, rank=r) for r in range(world)]
    for i in range(n_frames):
        if i == stable_at:
            _stable(one, efs)
        _frame(one, efs, d_rgb, d_dep, i)
    if not with_one:
        one.close()
        one = None
    return one, efs


def _merged(efs, of):
    parts = [(e.seq(), of(e)) for e in efs]
    seq = np.concatenate([p[0] for p in parts])
    return np.concatenate([p[1] for p in parts])[np.argsort(seq, kind="stable")]


def _check(ifx, one, efs, tag):
    """test_owner_sharded_instance_emulated's check: tables on all ranks and the unsharded one, votes and labels merged by creation number, bit for bit"""
    inst_one = ifx.InstanceFusion(one)
    assert all(np.array_equal(ifx.InstanceFusion(e).getInstanceTable(), inst_one.getInstanceTable()) for e in efs), tag
    assert np.array_equal(_merged(efs, lambda e: e.download()["votes"]), one.download()["votes"]), tag
    assert np.array_equal(_merged(efs, lambda e: ifx.InstanceFusion(e).labels()), inst_one.labels()), tag


def _f32_masks(masks, rng):
    """0/255 masks as a detector's probabilities: inside above 0.5, outside at or below it (0.5 itself is outside), a NaN outside"""
    f = np.where(masks != 0, rng.uniform(0.51, 1.0, masks.shape), rng.uniform(0.0, 0.5, masks.shape)).astype(np.float32)
    out = np.argwhere(masks == 0)
    if len(out) >= 2:
        f[tuple(out[0])] = np.nan
        f[tuple(out[1])] = 0.5
    return f


def _both(ifx, one, efs, st, i, form, root, rng, max_n=16):
    """one call of `form` on the unsharded handle and on the ranks, the tensors shuffled (not sorted by area)"""
    import torch

    from instancefusion_amd import sharded, synth

    inst_one = ifx.InstanceFusion(one)
    rgb, depth = st["rgb"][i], st["depth"][i]
    if form in ("image-u8", "image-f32"):
        masks, cls = synth.canned_masks(st["obj"][i], st["scene"])
        perm = rng.permutation(len(masks))
        masks, cls = masks[perm], np.asarray(cls, np.int32)[perm]
        t = torch.from_numpy(masks if form == "image-u8" else _f32_masks(masks, rng)).cuda()
        inst_one.process_segmentation_device(t, cls, i, superpixels=True)
        sharded.emulate_owner_segmentation_device(efs, root, rgb, depth, t, cls, i, superpixels=True, max_n=max_n)
    elif form == "rois":
        rois, boxes, cls, _ = _roi_case(st, i, rng)
        tr, tb = torch.from_numpy(rois).cuda(), torch.from_numpy(boxes).cuda()
        inst_one.process_segmentation_rois(tr, tb, cls, i, superpixels=True)
        sharded.emulate_owner_segmentation_rois(efs, root, rgb, depth, tr, tb, cls, i, superpixels=True, max_n=max_n)
    else:
        c, stage = _head_case(st, i, rng)
        t = [torch.from_numpy(c[k]).cuda() for k in ("logits", "boxes", "scores", "labels")]
        cmap = torch.from_numpy(c["class_map"]).cuda()
        k1 = inst_one.process_segmentation_detections(*t, c["in_size"], i, c["score_thresh"], class_map=cmap, superpixels=True)
        k2 = sharded.emulate_owner_segmentation_detections(efs, root, rgb, depth, *t, c["in_size"], i, c["score_thresh"], class_map=cmap, superpixels=True, max_n=max_n)
        assert k1 == k2 == len(stage[3])


FORMS = ("image-u8", "image-f32", "rois", "detections")
PARITY = [(w, r, f, 0) for w in (2, 3) for r in (-1, 0, w - 1) for f in FORMS] + [(2, 0, "rois", 1), (3, -1, "rois", 1), (3, 2, "rois", 1), (2, 1, "image-f32", 1)]


@pytest.mark.parametrize("world,root,form,lazy_ids", PARITY)
def test_parity_with_one_gpu(ifx, small_stream, world, root, form, lazy_ids):
    """test_owner_sharded_instance_emulated's scenario up to its segmentation calls with superpixels: the unsharded handle takes the device entry of the form, the
    ranks the new form with the same tensors."""
    from instancefusion_amd import synth

    st = small_stream
    NF = 10
    rng = np.random.default_rng(100 * world + 10 * (root + 1) + FORMS.index(form))
    d_rgb, d_dep = _device_frames(st, NF)
    one = ifx.ElasticFusion(**SMALL, max_surfels=400000)
    efs = [ifx.ElasticFusion(**SMALL, max_surfels=400000, n_ranks=world, rank=r) for r in range(world)]
    inst_one, insts = ifx.InstanceFusion(one), [ifx.InstanceFusion(e) for e in efs]
    for e in efs:
        e.set_option("own_lazy_ids", lazy_ids)
        e.set_option("own_key_rs", lazy_ids)
    calls = 0
    for i in range(NF):
        if i == 4:
            _stable(one, efs)
        _frame(one, efs, d_rgb, d_dep, i)
        want = inst_one.whetherDoSegmentation(i)
        assert [x.whetherDoSegmentation(i) for x in insts] == [want] * world, i
        if i >= 2 and (want or i % 3 == 0) and synth.canned_masks(st["obj"][i], st["scene"])[0].shape[0]:
            _both(ifx, one, efs, st, i, form, root, rng)
            calls += 1
            _check(ifx, one, efs, ("call", i))
    assert calls >= 2 and (inst_one.labels() >= 0).sum() > 30   # (sanity floors of the scenario, not parity figures)
    for e in efs + [one]:
        e.close()


def test_parity_with_the_host_form(ifx, small_stream):
    """One call each way on two fresh sets of ranks: the host form fed mask_bridge_numpy's output of the tensors, against the image form with root = 0."""
    import torch

    from instancefusion_amd import sharded, synth

    st, i = small_stream, 5
    rng = np.random.default_rng(5)
    masks, cls = synth.canned_masks(st["obj"][i], st["scene"])
    perm = rng.permutation(len(masks))
    f = _f32_masks(masks[perm], rng)
    cls = np.asarray(cls, np.int32)[perm]
    ori, _, _, cls_sorted = mb.bridge_masks(f, cls, 0.5)
    _, host = _ranks(ifx, st, SMALL, 2, i + 1, 4, with_one=False)
    _, dev = _ranks(ifx, st, SMALL, 2, i + 1, 4, with_one=False)
    sharded.emulate_owner_segmentation(host, st["rgb"][i], st["depth"][i], ori, cls_sorted, i, superpixels=True)
    sharded.emulate_owner_segmentation_device(dev, 0, st["rgb"][i], st["depth"][i], torch.from_numpy(f).cuda(), cls, i, superpixels=True, max_n=len(f))
    for a, b in zip(host, dev):
        ia, ib = ifx.InstanceFusion(a), ifx.InstanceFusion(b)
        assert np.array_equal(ia.getInstanceTable(), ib.getInstanceTable())
        assert np.array_equal(a.seq(), b.seq())
        assert np.array_equal(a.download()["votes"], b.download()["votes"])
        assert np.array_equal(ia.labels(), ib.labels())
    assert sum((ifx.InstanceFusion(e).labels() >= 0).sum() for e in dev) > 30
    for e in host + dev:
        e.close()


def _read_words(ef, ptr, nbytes):
    import torch

    from instancefusion_amd import sharded

    assert nbytes % 4 == 0
    ef.sync()
    return torch.as_tensor(sharded._DevWords(ptr, nbytes // 4, "<i4"), device=f"cuda:{ef.cfgd['device']}").cpu().numpy().copy()


def _begin_all(efs, form, root, max_n, rgb, depth, tensors, frame, superpixels=False):
    from instancefusion_amd import sharded

    order = [root] + [k for k in range(len(efs)) if k != root] if root >= 0 else list(range(len(efs)))
    rs, keep = [None] * len(efs), []
    for k in order:
        rs[k], kp, _ = sharded._device_form_begin(efs[k], form, root, max_n, rgb, depth, tensors, frame, superpixels)
        keep.append(kp)
    return rs, keep


def _finish(efs, rs):
    from instancefusion_amd import sharded

    n = 0
    while rs[0] == 1:
        assert all(r == 1 for r in rs)
        sharded._reduce_by_hand(efs, [sharded._exchange_spec(e, 200) for e in efs])
        rs = [e._chk(e.L.ifx_owner_segmentation_resume(e.handle), "ifx_owner_segmentation_resume") for e in efs]
        n += 1
    assert all(r == 0 for r in rs)
    return n


def _random_case(rng, kind, n, w, h):
    """(form, tensors as numpy, the restatement's record for max_n) of n random masks: image masks u8 / f32 with a NaN and a value at the threshold, or ROI masks"""
    cls = rng.integers(1, 80, n).astype(np.int32)
    if kind == "rois":
        rois = rng.random((n, 14, 14), dtype=np.float32)
        x0, y0 = rng.uniform(0, w * 0.6, n), rng.uniform(0, h * 0.6, n)
        boxes = np.stack([x0, y0, x0 + rng.uniform(4, w * 0.4, n), y0 + rng.uniform(4, h * 0.4, n)], axis=1).astype(np.float32)
        return "rois", dict(roi_masks=rois, boxes=boxes, class_ids=cls), lambda max_n: rec.record_rois(rois, boxes, cls, max_n, w * h)
    m = np.zeros((n, h, w), np.uint8)
    for k in range(n):
        y, x = int(rng.integers(0, h // 2)), int(rng.integers(0, w // 2))
        m[k, y:y + int(rng.integers(8, h // 2)), x:x + int(rng.integers(8, w // 2))] = rng.integers(1, 256)
    m[0, -1, -16:] = 7                      # the last, partial word of the mask
    if kind == "image-f32":
        m = _f32_masks(m, rng)
    return "device", dict(masks=m, class_ids=cls), lambda max_n: rec.record_image(m, cls, max_n, 0.5)


@pytest.mark.parametrize("cfg", [SMALL, ODD], ids=["320x240", "324x244"])
def test_record_word_for_word(ifx, small_stream, cfg):
    """root = 0, stopped at the first exchange point: one buffer, op 4 | 0 << 8, the restatement's byte count and words; then the call is finished.  On the 324 x 244
    handles P % 32 == 16: every mask ends in half a word."""
    import torch

    from instancefusion_amd import sharded, synth

    odd = cfg is ODD
    st = synth.make_stream(4, cfg["w"], cfg["h"], cfg["fx"], cfg["fy"], cfg["cx"], cfg["cy"], noise=True) if odd else small_stream
    assert (cfg["w"] * cfg["h"]) % 32 == (16 if odd else 0)
    _, efs = _ranks(ifx, st, cfg, 2, 4, 2, with_one=False)
    rng = np.random.default_rng(11)
    i = 3
    for kind in ("image-u8", "image-f32", "rois"):
        for n, max_n, mis in ((1, 1, False), (1, 8, True), (3, 3, True), (3, 8, False)):
            form, t, want = _random_case(rng, kind, n, cfg["w"], cfg["h"])
            dev = {k: torch.from_numpy(v).cuda() for k, v in t.items() if k != "class_ids"}
            if mis:   # one element past a 16-B boundary: the pack's pixel-per-lane path, a wave's ballot two words (324 x 244: P % 64 == 16, the last wave holds one)
                dev = {k: _misaligned(v) for k, v in dev.items()}
            tensors = dict(dev, class_ids=t["class_ids"], threshold=0.5, stream=None, roi_size=14)
            rs, keep = _begin_all(efs, form, 0, max_n, st["rgb"][i], st["depth"][i], tensors, 50 + n)
            assert rs == [1, 1]
            specs = [sharded._exchange_spec(e, 200) for e in efs]
            w = want(max_n)
            for sp in specs:
                assert len(sp) == 1 and sp[0][2] == (4 | 0 << 8) and sp[0][1] == w.nbytes and sp[0][1] % 4 == 0, (kind, n, max_n, sp)
            got = _read_words(efs[0], specs[0][0][0], specs[0][0][1])
            assert np.array_equal(got, w), (kind, n, max_n, np.flatnonzero(got != w)[:8])
            assert _finish(efs, rs) >= 3           # the record, the boxes, the model depth
            del keep
    for e in efs:
        e.close()


def test_odd_size_end_to_end(ifx):
    """324 x 244 (P % 32 == 16), a 4-frame stream: the image form end to end (f32 with root = 1, then u8 with root = 0) against an unsharded handle."""
    from instancefusion_amd import synth

    st = synth.make_stream(4, ODD["w"], ODD["h"], ODD["fx"], ODD["fy"], ODD["cx"], ODD["cy"], noise=True)
    one, efs = _ranks(ifx, st, ODD, 2, 4, 2)
    rng = np.random.default_rng(12)
    i = 3
    masks, _ = synth.canned_masks(st["obj"][i], st["scene"])
    assert masks.shape[0]
    for form, root in (("image-f32", 1), ("image-u8", 0)):
        _both(ifx, one, efs, st, i, form, root, rng)
        _check(ifx, one, efs, (form, root))
    for e in efs + [one]:
        e.close()


@pytest.fixture()
def pair(ifx, small_stream):
    one, efs = _ranks(ifx, small_stream, SMALL, 2, 6, 4)
    yield one, efs
    for e in efs + [one]:
        e.close()


def _state(ifx, efs):
    return [(e.download()["votes"].copy(), ifx.InstanceFusion(e).labels().copy(), ifx.InstanceFusion(e).getInstanceTable().copy()) for e in efs]


def _same_state(a, b):
    return all(all(np.array_equal(x, y) for x, y in zip(sa, sb)) for sa, sb in zip(a, b))


def test_edges_of_the_call(ifx, small_stream, pair):
    import torch

    from instancefusion_amd import sharded

    st, i = small_stream, 5
    one, efs = pair
    rgb, depth = st["rgb"][i], st["depth"][i]
    before = _state(ifx, efs)
    empty = dict(masks=torch.zeros((0, SMALL["h"], SMALL["w"]), dtype=torch.uint8, device="cuda"), class_ids=np.zeros(0, np.int32), threshold=0.5, stream=None)
    # n = 0 with a root: one exchange, 0 on every rank, the map untouched
    rs, _ = _begin_all(efs, "device", 0, 4, rgb, depth, empty, 60)
    assert rs == [1, 1]
    assert _finish(efs, rs) == 1
    assert _same_state(before, _state(ifx, efs))
    # n = 0 on every rank: 0 at once
    rs, _ = _begin_all(efs, "device", -1, 4, rgb, depth, empty, 61)
    assert rs == [0, 0]
    assert _same_state(before, _state(ifx, efs))
    # NULL tensors on the ranks that are not the root; a second call of the same sizes reuses the record
    rng = np.random.default_rng(3)
    ptrs = []
    for call in range(2):
        form, t, _ = _random_case(rng, "image-u8", 3, SMALL["w"], SMALL["h"])
        tensors = dict(masks=None, class_ids=None, threshold=0.5, stream=None)
        r1, _, _ = sharded._device_form_begin(efs[1], form, 1, 8, rgb, depth, dict(tensors, masks=torch.from_numpy(t["masks"]).cuda(), class_ids=t["class_ids"]), 62 + call, False)
        r0, _, _ = sharded._device_form_begin(efs[0], form, 1, 8, rgb, depth, tensors, 62 + call, False)
        assert (r0, r1) == (1, 1)
        specs = [sharded._exchange_spec(e, 200) for e in efs]
        assert all(len(sp) == 1 and sp[0][2] == (4 | 1 << 8) for sp in specs)
        ptrs.append([sp[0][0] for sp in specs])
        _finish(efs, [r0, r1])
    assert ptrs[0] == ptrs[1]


def test_refusals_leave_the_handles_usable(ifx, small_stream, pair):
    import torch

    from instancefusion_amd import sharded

    st, i = small_stream, 5
    one, efs = pair
    rgb, depth = st["rgb"][i], st["depth"][i]
    rng = np.random.default_rng(4)
    _, t, _ = _random_case(rng, "image-u8", 3, SMALL["w"], SMALL["h"])
    good = dict(masks=torch.from_numpy(t["masks"]).cuda(), class_ids=t["class_ids"], threshold=0.5, stream=None)
    _, tr, _ = _random_case(rng, "rois", 3, SMALL["w"], SMALL["h"])
    good_rois = dict(roi_masks=torch.from_numpy(tr["roi_masks"]).cuda(), boxes=torch.from_numpy(tr["boxes"]).cuda(), class_ids=tr["class_ids"], threshold=0.5, stream=None,
                     roi_size=14)
    before = _state(ifx, efs)

    def refused(code, what, fn, *a, **kw):
        with pytest.raises(ifx.IfxError) as ex:
            fn(*a, **kw)
        assert code in str(ex.value) and what in str(ex.value), str(ex.value)
        assert all(e.L.ifx_owner_segmentation_resume(e.handle) < 0 for e in efs), "nothing is in flight"
        assert _same_state(before, _state(ifx, efs))

    dev, rois = sharded.emulate_owner_segmentation_device, sharded.emulate_owner_segmentation_rois
    name = "ifx_owner_segmentation_begin_device: "
    # an unsharded handle
    refused(E_STATE, name + "the handle was not created for a sharded map", sharded._device_form_begin, one, "device", -1, 8, rgb, depth, good, 70, False)
    refused(E_INVALID, name + "root", dev, efs, 2, rgb, depth, good["masks"], good["class_ids"], 70, superpixels=False, max_n=8)
    for bad in (0, 257):
        refused(E_INVALID, name + "max_n", dev, efs, 0, rgb, depth, good["masks"], good["class_ids"], 70, superpixels=False, max_n=bad)
    refused(E_INVALID, name + "n is larger than max_n", dev, efs, 0, rgb, depth, good["masks"], good["class_ids"], 70, superpixels=False, max_n=2)
    refused(E_INVALID, name + "n is larger than max_n", dev, efs, -1, rgb, depth, good["masks"], good["class_ids"], 70, superpixels=False, max_n=2)
    # flags & 1 on a begin form
    L = efs[0].L
    r = L.ifx_owner_segmentation_begin_device(efs[0].handle, 0, 8, None, None, C.c_void_p(good["masks"].data_ptr()), ifx.MASK_U8, 0.5, None, 0, 70, 1, None)
    assert r == -1 and L.ifx_last_error(efs[0].handle).decode().startswith(name + "kNN")
    # an unknown mask format (the reading rank), a bad roi_size (every rank)
    cls = torch.from_numpy(good["class_ids"]).cuda()
    r = L.ifx_owner_segmentation_begin_device(efs[0].handle, 0, 8, None, None, C.c_void_p(good["masks"].data_ptr()), 7, 0.5, C.c_void_p(cls.data_ptr()), 3, 70, 0, None)
    assert r == -1 and L.ifx_last_error(efs[0].handle).decode() == name + "unknown mask format"
    for e in efs:
        for bad in (0, 65):
            r = L.ifx_owner_segmentation_begin_rois(e.handle, 0, 8, None, None, None, bad, None, 0.5, None, 0, 70, 0, None)
            assert r == -1 and L.ifx_last_error(e.handle).decode() == "ifx_owner_segmentation_begin_rois: roi_size must be 1 .. 64"
    assert all(e.L.ifx_owner_segmentation_resume(e.handle) < 0 for e in efs) and _same_state(before, _state(ifx, efs))
    # a call already in flight
    rs, keep = _begin_all(efs, "device", 0, 8, rgb, depth, good, 71)
    assert rs == [1, 1]
    for e in efs:
        with pytest.raises(ifx.IfxError) as ex:
            sharded._device_form_begin(e, "rois", 0, 8, rgb, depth, good_rois, 72, False)
        assert E_STATE in str(ex.value) and "ifx_owner_segmentation_begin_rois: a segmentation call is already in flight" in str(ex.value)
    _finish(efs, rs)
    del keep
    ifx.InstanceFusion(one).process_segmentation_device(good["masks"], good["class_ids"], 71)      # (the unsharded handle follows the ranks' one completed call)
    # ranks given different max_n: IFX_E_STATE at the first resume (on the rank whose arguments differ from the header), the call is over everywhere
    with pytest.raises(ifx.IfxError) as ex:
        dev(efs, 0, rgb, depth, good["masks"], good["class_ids"], 73, superpixels=False, max_n=[4, 8])
    assert E_STATE in str(ex.value) and "ifx_owner_segmentation_resume" in str(ex.value) and name + "the record's header" in str(ex.value)
    assert all(e.L.ifx_owner_segmentation_resume(e.handle) < 0 for e in efs)
    # more kept detections than the record holds: IFX_E_CAPACITY -- from the begin form where every rank runs the stage, at the first resume of EVERY rank with a root
    c, stage = _head_case(st, i, rng)
    assert len(stage[3]) > 2
    th = [torch.from_numpy(c[k]).cuda() for k in ("logits", "boxes", "scores", "labels")]
    cmap = torch.from_numpy(c["class_map"]).cuda()
    det = "ifx_owner_segmentation_begin_detections: more than max_n detections kept"
    with pytest.raises(ifx.IfxError) as ex:
        sharded.emulate_owner_segmentation_detections(efs, -1, rgb, depth, *th, c["in_size"], 74, c["score_thresh"], class_map=cmap, superpixels=False, max_n=2)
    assert E_CAPACITY in str(ex.value) and "ifx_owner_segmentation_begin_detections failed" in str(ex.value) and det in str(ex.value)
    rs, keep = _begin_all(efs, "detections", 1, 2, rgb, depth, dict(mask_logits=th[0], boxes=th[1], scores=th[2], labels=th[3], in_size=c["in_size"], score_thresh=c["score_thresh"],
                                                                      class_map=cmap, count=None, threshold=0.5, stream=None, roi_size=28), 75)
    assert rs == [1, 1]
    sharded._reduce_by_hand(efs, [sharded._exchange_spec(e, 200) for e in efs])
    for e in efs:
        assert e.L.ifx_owner_segmentation_resume(e.handle) == -3 and e.L.ifx_last_error(e.handle).decode().startswith(det)
    del keep
    assert all(e.L.ifx_owner_segmentation_resume(e.handle) == -4 for e in efs)
    # correct calls afterwards: both forms, equal to the unsharded handle fed the same
    _both(ifx, one, efs, st, i, "image-u8", 0, rng)
    _both(ifx, one, efs, st, i, "rois", 1, rng)
    _check(ifx, one, efs, "after the refusals")


def test_owner_seg_device_rccl_world_of_one_in_library(ifx, small_stream):
    """n_ranks = -1 with the collectives inside the library: the ROI form with root = 0 and root = -1 against the unsharded handle; the record's broadcast is one
    collective more per call."""
    import torch

    from instancefusion_amd import sharded

    st = small_stream
    NF = 7
    d_rgb, d_dep = _device_frames(st, NF)
    torch.cuda.synchronize()
    one = ifx.ElasticFusion(**SMALL, max_surfels=400000)
    ef = ifx.ElasticFusion(**SMALL, max_surfels=400000, n_ranks=-1, rank=0)
    osh = sharded.OwnerShardedElasticFusion(ef, None, transport="library")
    inst_one, inst = ifx.InstanceFusion(one), ifx.InstanceFusion(ef)
    rng = np.random.default_rng(6)
    colls = {}
    for i in range(NF):
        if i == 4:
            m = one.download(); m["pc"][:, 3] = 20.0
            pose = one.getCurrPose()
            one.upload(m); one.set_pose(pose, one.tick); one.combined_predict(pose, one.tick, one.tick)
            ef.upload(m); ef.set_pose(pose, one.tick)
            osh.predict()
        one.enqueue_frame_device(d_rgb[i].data_ptr(), d_dep[i].data_ptr(), i)
        osh.process_frame_device(d_rgb[i].data_ptr(), d_dep[i].data_ptr())
        if i >= 5:
            root = 0 if i == 5 else -1
            rois, boxes, cls, _ = _roi_case(st, i, rng)
            tr, tb = torch.from_numpy(rois).cuda(), torch.from_numpy(boxes).cuda()
            inst_one.process_segmentation_rois(tr, tb, cls, i, superpixels=True)
            osh.exchange_stats(reset=True)
            osh.process_segmentation_rois(st["rgb"][i], st["depth"][i], tr, tb, cls, i, superpixels=True, root=root, max_n=16)
            colls[root] = osh.exchange_stats()["collectives"]
            order = np.argsort(ef.seq(), kind="stable")
            assert np.array_equal(inst.getInstanceTable(), inst_one.getInstanceTable()), i
            assert np.array_equal(ef.download()["votes"][order], one.download()["votes"]), i
            assert np.array_equal(inst.labels()[order], inst_one.labels()), i
    assert colls[0] == colls[-1] + 1, colls           # (no table eviction in either call: the boxes and the model depth, and the record in front of them)
    assert (inst_one.labels() >= 0).sum() > 30
    ef.close(); one.close()
