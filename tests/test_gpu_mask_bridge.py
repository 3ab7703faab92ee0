"""The bridge kernels of the device entry as a stage (ifx_ingest_masks: k_mask_area, k_mask_order, k_mask_gather as ifx_process_segmentation_device launches them)
against the numpy statement (tests/mask_bridge_numpy.py): all four outputs -- the 0/255 masks in sorted order, the overlap-cleaned copy, the order, the class ids --
with np.array_equal, on dense random fields at every alignment, mask count, format and threshold; the shared counters across calls; the handle left as it was."""
import ctypes as C
import time

import numpy as np
import pytest

import mask_bridge_numpy as mb
import roi_paste_numpy as rp
from conftest import SMALL

pytestmark = pytest.mark.gpu

MAP_KEYS = ("pc", "nr", "col", "tm", "ic", "votes")
TINY = dict(w=160, h=120, fx=132.0, fy=132.0, cx=80.0, cy=60.0)     # 1200 16-B words of uint8 per mask: a second, partly filled area block; 4800 of float
NARROW = dict(w=100, h=76, fx=82.0, fy=82.0, cx=50.0, cy=38.0)      # 475 words of uint8: one block with idle lanes; 1900 of float
SIZES = {"tiny": TINY, "narrow": NARROW, "small": SMALL}
DENSITIES = (0.5, 0.01, 0.99, 0.0, 1.0)


@pytest.fixture(scope="module")
def ifx():
    import instancefusion_amd as m

    m.lib()
    return m


@pytest.fixture(scope="module")
def handles(ifx):
    """One handle per image size (no frame is processed on them)."""
    made = {}

    def get(**k):
        key = (k["w"], k["h"])
        if key not in made:
            made[key] = ifx.ElasticFusion(**k, max_surfels=100000)
        return ifx.InstanceFusion(made[key])

    yield get
    for e in made.values():
        e.close()


def _at_offset(t, k):
    """The same values in a contiguous tensor that starts k elements past a 16-byte boundary; what lies before and behind it is non-zero (inside, for every format)."""
    import torch

    buf = torch.ones(t.numel() + 64, dtype=t.dtype, device=t.device)
    isz = buf.element_size()
    lead = ((-buf.data_ptr()) % 16) // isz + 16 // isz + k
    v = buf[lead:lead + t.numel()].view(t.shape)
    v.copy_(t)
    if t.numel():
        assert v.data_ptr() % 16 == k * isz and v.is_contiguous()
    return v


def _fields(rng, n, H, W):
    """n Bernoulli fields [n,H,W] bool, the densities cycling through DENSITIES (every bit position of a 16-pixel group, deep overlaps, empty and full masks)"""
    d = np.asarray([DENSITIES[i % len(DENSITIES)] for i in range(n)])
    return rng.random((n, H, W)) < d[:, None, None]


def _edge_pairs(rng, H, W):
    """Two pairs of masks that differ only inside the first 15 and the last 15 pixels, the smaller of each pair first in the input.  (b, a): a has 15 pixels in the
    tail, b 14 in the head, so a count that loses tail pixels puts b first (a tie keeps the input order: b first too).  (d, c): the mirror image for the head."""
    P = H * W
    x, y = rng.random(P) < 0.5, rng.random(P) < 0.3
    a, b, c, d = x.copy(), x.copy(), y.copy(), y.copy()
    a[:15] = False; a[-15:] = True
    b[:15] = True; b[14] = False; b[-15:] = False
    c[:15] = True; c[-15:] = False
    d[:15] = False; d[-15:] = True; d[-15] = False
    assert a.sum() == b.sum() + 1 and c.sum() == d.sum() + 1 and a.sum() != c.sum()
    return np.stack([b, a, d, c]).reshape(4, H, W)


def _u8(bm, how, rng):
    if how == "rand":
        return np.where(bm, rng.integers(1, 256, bm.shape), 0).astype(np.uint8)
    return np.where(bm, int(how), 0).astype(np.uint8)


def _f32(bm, thr, rng):
    """float32 samples that are inside exactly where bm is: the threshold itself and its two neighbours, NaN, both infinities, the largest finite values, both zeros
    and denormals of both signs (on whichever side of the threshold they belong), ordinary values.  Nothing is above +inf or compares with NaN: bm is ignored there."""
    t = np.float32(thr)
    den, big = np.float32(1e-45), np.float32(3.0e38)
    assert 0 < den < np.finfo(np.float32).tiny
    with np.errstate(all="ignore"):
        up, dn = np.nextafter(t, np.float32(np.inf)), np.nextafter(t, np.float32(-np.inf))
    lo = [t, t, dn, np.nan, -np.inf, -big]
    pick = lambda pool: np.asarray(pool, np.float32)[rng.integers(0, len(pool), bm.shape)]
    if t < np.inf:
        out = np.where(bm, pick([up, up, np.inf, big]), pick(lo)).astype(np.float32)
        u = rng.uniform(1e-3, 2.0, bm.shape).astype(np.float32)
        r = rng.random(bm.shape) < 0.25
        out[r] = np.where(bm, t + u, t - u)[r]
        for s in (np.float32(0.0), np.float32(-0.0), den, -den):
            out[(rng.random(bm.shape) < 0.05) & (bm == bool(s > t))] = s
        assert np.array_equal(mb.inside(out, thr), bm)
    else:
        out = pick(lo + [np.inf, big, 0.0, -0.0, den, -den])
        assert not mb.inside(out, thr).any()
    if bm.size >= 4000 and bm.any() and not bm.all():
        same = lambda v: out == v if v == v else np.isnan(out)
        for want in (same(t), same(up), same(dn), np.isnan(out), out == np.inf, out == -np.inf, (out == 0) & np.signbit(out), (out == 0) & ~np.signbit(out),
                     out == den, out == -den):
            assert want.any()
    return out


def _check(inst, raw, cls, thr=0.5, k=0, tensor=None, what=None):
    """One stage call on `raw` (numpy, uploaded k elements past alignment) or on `tensor` (whose values are raw's) against the statement."""
    import torch

    t = tensor if tensor is not None else _at_offset(torch.from_numpy(np.ascontiguousarray(raw)).cuda(), k)
    got = inst.ingest_masks(t, cls, threshold=thr)
    want = mb.bridge_masks(raw, cls, thr)
    for g, w, name in zip(got, want, ("ori", "clean", "order", "class ids")):
        assert g.dtype == w.dtype and g.shape == w.shape, (what, name, g.shape, w.shape)
        assert np.array_equal(g, w), (what, name, np.argwhere(g != w)[:5])
    return got


def _as_format(bm, fmt, rng, thr):
    if fmt == "bool":
        return bm.copy()
    if fmt == "uint8":
        return _u8(bm, "rand", rng)
    return _f32(bm, thr, rng)


@pytest.mark.parametrize("size", ["tiny", "narrow"])
@pytest.mark.parametrize("fmt", ["uint8", "bool", "float32"])
def test_every_alignment(handles, fmt, size):
    """The masks start 0 .. 15 bytes (uint8, bool) or 0 .. 3 elements (float32) past a 16-byte boundary: the head and tail counts of k_mask_area at every split,
    the 16-B path of k_mask_gather at 0 and its element path elsewhere.  Two pairs of masks differ only inside the first and the last 15 pixels, so the order -- and
    with it the clean -- hangs on those counts."""
    inst = handles(**SIZES[size])
    W, H = inst.ef.w, inst.ef.h
    rng = np.random.default_rng(31)
    for k in range(16 if fmt != "float32" else 4):
        bm = np.concatenate([_edge_pairs(rng, H, W), _fields(rng, 5, H, W)])
        cls = rng.integers(0, 80, len(bm)).astype(np.int32)
        thr = 0.7 if k % 2 else 0.5
        _, clean, order, _ = _check(inst, _as_format(bm, fmt, rng, thr), cls, thr, k, what=(fmt, size, k))
        rank = {int(src): r for r, src in enumerate(order)}
        assert rank[1] < rank[0] and rank[3] < rank[2]          # the larger of each pair first, against the input order
        assert not clean[rank[1]].reshape(-1)[15:-15].any() and not clean[rank[3]].reshape(-1)[15:-15].any()      # the later twin of each pair holds them


@pytest.mark.parametrize("n", [0, 1, 2, 3, 4, 5, 7, 8, 9])
def test_mask_counts(handles, n):
    """Every remainder of k_mask_gather's four-at-a-time loop (aligned) and its one-at-a-time loop (misaligned), both formats, both small sizes."""
    rng = np.random.default_rng(40 + n)
    for size in ("tiny", "narrow"):
        inst = handles(**SIZES[size])
        W, H = inst.ef.w, inst.ef.h
        for fmt, k, thr in (("uint8", 0, 0.5), ("uint8", 3, 0.5), ("float32", 0, 0.25), ("float32", 1, 0.5), ("bool", 0, 0.5)):
            bm = _fields(rng, n, H, W)
            if n >= 3:
                bm[2] = np.roll(bm[0], 7, axis=1)             # a tie
            cls = rng.integers(0, 80, n).astype(np.int32)
            ori, clean, order, out_cls = _check(inst, _as_format(bm, fmt, rng, thr), cls, thr, k, what=(n, size, fmt, k))
            assert ori.shape == (n, H, W) and order.shape == (n,)
            if n >= 3:
                assert (clean != ori).any()


def test_256_masks_stable_order(handles):
    """n = 256 at 160x120: 32 sparse fields, each shifted eight times (equal areas), twelve masks emptied -- the order is the stable one and a permutation."""
    inst = handles(**TINY)
    W, H = inst.ef.w, inst.ef.h
    rng = np.random.default_rng(256)
    n = 256
    base = rng.random((32, H, W)) < rng.uniform(0.002, 0.2, 32)[:, None, None]
    bm = np.stack([np.roll(base[i % 32], 3 * (i // 32), axis=1) for i in range(n)])
    bm[rng.choice(n, 12, replace=False)] = False
    cls = rng.permutation(n).astype(np.int32)
    for fmt, k in (("uint8", 0), ("float32", 0), ("uint8", 9)):
        t0 = time.perf_counter()
        ori, clean, order, out_cls = _check(inst, _as_format(bm, fmt, rng, 0.5), cls, 0.5, k, what=(fmt, k))
        print(f"n = 256 {fmt} offset {k}: {time.perf_counter() - t0:.2f} s (stage call, statement and comparison)")
        area = (ori != 0).sum(axis=(1, 2))
        assert sorted(order.tolist()) == list(range(n)) and np.array_equal(out_cls, cls[order])
        assert (np.diff(area) <= 0).all() and len(set(area.tolist())) <= 33 and (area == 0).sum() == 12
        assert all(order[r] < order[r + 1] for r in range(n - 1) if area[r] == area[r + 1])
        assert (clean != ori).any()


def test_formats_and_values(handles):
    """bool; uint8 with inside values 1, 128, 255 and random ones; float32 at every threshold of the list with the values at which `>` can go wrong; [N,1,H,W];
    a non-contiguous input (the copy _device_masks makes); one case at 320x240."""
    import torch

    rng = np.random.default_rng(50)
    for size in ("tiny", "narrow"):
        inst = handles(**SIZES[size])
        W, H = inst.ef.w, inst.ef.h
        n = 7
        cls = rng.integers(0, 80, n).astype(np.int32)
        _check(inst, _fields(rng, n, H, W), cls, what="bool")
        for how in ("1", "128", "255", "rand"):
            _check(inst, _u8(_fields(rng, n, H, W), how, rng), cls, k=(0 if how != "128" else 5), what=("uint8", how))
        for thr in (0.5, 0.25, 0.7, 0.0, -1.0, 1.0, float("inf"), float("nan")):
            for k in (0, 2):
                raw = _f32(_fields(rng, n, H, W), thr, rng)
                ori, _, _, _ = _check(inst, raw, cls, thr, k, what=("float32", thr, k))
                assert ori.any() == (thr == thr and thr != float("inf"))          # nothing is above +inf, nothing compares with NaN
        raw = _f32(_fields(rng, n, H, W), 0.5, rng)
        _check(inst, raw, cls, 0.5, tensor=torch.from_numpy(raw).cuda().unsqueeze(1), what="[N,1,H,W]")
        _check(inst, raw, cls.tolist(), 0.5, tensor=torch.from_numpy(raw).cuda(), what="class ids as a list")
        two = torch.from_numpy(np.stack([_f32(_fields(rng, n, H, W), 0.5, rng), raw], axis=1)).cuda()      # [N,2,H,W]
        assert not two[:, 1].is_contiguous()
        _check(inst, raw, cls, 0.5, tensor=two[:, 1], what="channel slice")
        _check(inst, raw, cls, 0.5, tensor=two[:, 1:2], what="channel slice [N,1,H,W]")
        u = _u8(_fields(rng, n, H, W), "rand", rng)
        wide = torch.from_numpy(np.concatenate([u, u[:, :, ::-1]], axis=2)).cuda()                         # [N,H,2W]
        _check(inst, u, cls, tensor=wide[:, :, :W], what="column slice")
        _check(inst, u != 0, cls, tensor=(wide[:, :, :W] != 0), what="bool made on the device")
    inst = handles(**SMALL)
    bm = np.concatenate([_edge_pairs(rng, 240, 320), _fields(rng, 5, 240, 320)])
    cls = np.arange(9, dtype=np.int32)
    _check(inst, _u8(bm, "rand", rng), cls, k=5, what="320x240 uint8")
    _check(inst, _f32(bm, 0.7, rng), cls, 0.7, k=0, what="320x240 float32")
    _check(inst, _f32(bm, 0.7, rng), cls, 0.7, k=3, what="320x240 float32 misaligned")


def test_counters_are_reused_across_calls(handles):
    """The counters k_mask_order zeroes are shared with the ROI path: n = 256, then n = 3, then ROI masks, then n = 5 again on one handle, each against its statement."""
    import torch

    inst = handles(**TINY)
    W, H = inst.ef.w, inst.ef.h
    rng = np.random.default_rng(60)
    bm = rng.random((256, H, W)) < rng.uniform(0.0, 0.3, 256)[:, None, None]
    _check(inst, _u8(bm, "rand", rng), np.arange(256, dtype=np.int32), what="n = 256")
    _check(inst, _f32(_fields(rng, 3, H, W), 0.5, rng), [3, 4, 5], 0.5, k=1, what="n = 3")
    M, n = 14, 6
    rois = rng.random((n, M, M)).astype(np.float32)
    xy = np.stack([rng.uniform(0, W - 40, n), rng.uniform(0, H - 40, n)], axis=1)
    boxes = np.concatenate([xy, xy + rng.uniform(5, 60, (n, 2))], axis=1).astype(np.float32)
    rcls = (10 + np.arange(n)).astype(np.int32)
    got = inst.paste_roi_masks(torch.from_numpy(rois).cuda(), torch.from_numpy(boxes).cuda(), rcls, threshold=0.5)
    want = rp.paste_rois(rois, boxes, rcls, W, H, 0.5)
    for g, w, name in zip(got, want, ("ori", "clean", "order", "class ids")):
        assert np.array_equal(g, w), ("ROIs", name)
    assert got[0].any()
    _check(inst, _u8(_fields(rng, 5, H, W), "rand", rng), np.arange(5, dtype=np.int32), k=7, what="n = 5 after the ROIs")
    _check(inst, np.zeros((0, H, W), np.uint8), np.zeros(0, np.int32), what="n = 0")
    _check(inst, _fields(rng, 2, H, W), [1, 2], what="n = 2 after n = 0")


def test_refusals(ifx, handles):
    """The argument checks of ifx_process_segmentation_device: n outside 0 .. 256, an unknown format, null pointers -> IFX_E_INVALID; a sharded handle -> IFX_E_STATE;
    a valid call on the same handle afterwards equals the statement."""
    import torch

    L = ifx.lib()
    inst = handles(**TINY)
    W, H = inst.ef.w, inst.ef.h
    rng = np.random.default_rng(70)
    d_m = torch.zeros((257, H, W), dtype=torch.uint8, device="cuda")
    d_c = torch.zeros(257, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    pm, pc, h = C.c_void_p(d_m.data_ptr()), C.c_void_p(d_c.data_ptr()), inst.ef.handle
    assert L.ifx_ingest_masks(h, pm, ifx.MASK_U8, 0.5, pc, 257, None, None, None, None, None) == -1
    assert L.ifx_ingest_masks(h, pm, ifx.MASK_U8, 0.5, pc, -1, None, None, None, None, None) == -1
    assert L.ifx_ingest_masks(h, pm, 7, 0.5, pc, 3, None, None, None, None, None) == -1
    assert L.ifx_ingest_masks(h, None, ifx.MASK_U8, 0.5, pc, 3, None, None, None, None, None) == -1
    assert L.ifx_ingest_masks(h, pm, ifx.MASK_F32, 0.5, None, 3, None, None, None, None, None) == -1
    assert L.ifx_ingest_masks(h, pm, ifx.MASK_U8, 0.5, pc, 3, None, None, None, None, None) == 0         # every download is optional
    e = ifx.ElasticFusion(**TINY, max_surfels=100000, n_ranks=-1, rank=0)
    try:
        assert L.ifx_ingest_masks(e.handle, pm, ifx.MASK_U8, 0.5, pc, 3, None, None, None, None, None) == -4
        assert b"sharded" in L.ifx_last_error(e.handle)
    finally:
        e.close()
    with pytest.raises(TypeError):
        inst.ingest_masks(d_m[:3].to(torch.int32), [1, 2, 3])
    with pytest.raises(ValueError):
        inst.ingest_masks(d_m[:3, :-1], [1, 2, 3])
    with pytest.raises(ValueError):
        inst.ingest_masks(d_m[:3], [1, 2])
    _check(inst, _u8(_fields(rng, 4, H, W), "rand", rng), [1, 2, 3, 4], what="after the refusals")


def test_stage_calls_leave_the_handle_as_it_was(ifx, small_stream):
    """Twins (test_gpu_seg_device_masks._twins): one gets stage calls between its frames and right before each of its segmentation calls, the other none --
    poses, labels, tables and maps stay equal."""
    import torch

    from instancefusion_amd import synth

    st = small_stream
    rng = np.random.default_rng(80)
    a = ifx.ElasticFusion(**SMALL, max_surfels=400000)
    b = ifx.ElasticFusion(**SMALL, max_surfels=400000)
    ia, ib = ifx.InstanceFusion(a), ifx.InstanceFusion(b)
    W, H = SMALL["w"], SMALL["h"]

    def stage(n, fmt, k):
        bm = _fields(rng, n, H, W)
        _check(ia, _as_format(bm, fmt, rng, 0.5), rng.integers(0, 80, n).astype(np.int32), 0.5, k, what=("stage", n, fmt))

    for i in range(8):
        if i in (1, 2, 5, 7):
            stage(11 if i == 5 else 3, "uint8" if i % 2 else "float32", i % 4)
        pa = a.processFrame(st["rgb"][i], st["depth"][i]); pb = b.processFrame(st["rgb"][i], st["depth"][i])
        assert np.array_equal(pa, pb), i
        if i == 3:
            m = a.download(); m["pc"][:, 3] = 20.0
            for e in (a, b):
                e.upload(m); e.set_pose(pa, a.tick)
        if i >= 4:
            masks, cls = synth.canned_masks(st["obj"][i], st["scene"])
            stage(20 if i == 6 else 2, "uint8", 0)          # (more masks than the call that follows: the mask buffers grow under it)
            for inst in (ia, ib):
                inst.process_segmentation_device(torch.from_numpy(masks).cuda(), cls, 100 + 3 * i, isflann=(i == 6), superpixels=(i != 5))
            assert np.array_equal(ia.getInstanceTable(), ib.getInstanceTable()), i
            assert np.array_equal(ia.getLoopClosureInstanceTable(), ib.getLoopClosureInstanceTable()), i
            assert np.array_equal(ia.labels(), ib.labels()), i
    assert (ia.labels() >= 0).sum() > 100 and (ia.getInstanceTable() >= 0).sum() >= 2
    ma, mb_ = a.download(), b.download()
    for key in MAP_KEYS:
        assert np.array_equal(ma[key], mb_[key]), key
    assert np.array_equal(ia.renderProjectMap(), ib.renderProjectMap())
    assert np.array_equal(a.image("ids_after"), b.image("ids_after"))
    a.close(); b.close()
