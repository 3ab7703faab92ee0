"""The default detector's output on the GPU (ifx_unmold_detections / ifx_process_segmentation_unmolded / ifx_process_segmentation_deferred_unmolded): the stage
byte for byte against the numpy statement (tests/unmold_numpy.py, itself held against the reference's Python in tests/test_unmold_cpu.py) -- every case of the
rule's step 8, both layouts, every output size (the device's f64 taps), the row limits; the full and the deferred call bit for bit against the existing device
entries fed the statement's masks; the producer stream; the refusals."""
import ctypes as C

import numpy as np
import pytest

import unmold_numpy as un
from conftest import SMALL

pytestmark = pytest.mark.gpu

MAP_KEYS = ("pc", "nr", "col", "tm", "ic", "votes")
TINY = dict(w=160, h=120, fx=132.0, fy=132.0, cx=80.0, cy=60.0)
NARROW = dict(w=100, h=76, fx=82.0, fy=82.0, cx=50.0, cy=38.0)    # a width that is no multiple of the paste's 64-column tile
WINDOWS = {160: (16, 0, 112, 128), 100: (15, 0, 113, 129)}        # molded_input_size of the two at (128, 128) and (128, 129): scales 1.25 and 0.7752
SEG_WINDOW = (32, 0, 224, 256)                                    # 320 x 240 molded to (256, 256): scale 1.25 back


@pytest.fixture(scope="module")
def ifx():
    import instancefusion_amd as m

    m.lib()
    return m


@pytest.fixture(scope="module")
def handles(ifx):
    """One handle per image size of the stage tests (no frame is processed on them)."""
    made = {}

    def get(**k):
        key = (k["w"], k["h"])
        if key not in made:
            made[key] = ifx.ElasticFusion(**k, max_surfels=100000)
        return made[key]

    yield get
    for e in made.values():
        e.close()


def _smooth(rng, M):
    y, x = np.mgrid[0:M, 0:M].astype(np.float64) / max(M - 1, 1)
    cx, cy = rng.uniform(0.3, 0.7, 2)
    p = 1.0 / (1.0 + np.exp((np.hypot(x - cx, y - cy) - rng.uniform(0.25, 0.6)) * rng.uniform(6, 20)))
    return (p * rng.uniform(0.6, 1.0)).astype(np.float32)


def _masks_for(rng, det, M, Cn):
    """mrcnn_mask [R, M, M, C]: noise in every channel, a smooth field in the channel each row's class id names"""
    R = len(det)
    masks = rng.random((R, M, M, Cn)).astype(np.float32)
    for r in range(R):
        c = det[r, 4]
        if 1 <= c < Cn:
            masks[r, :, :, int(c)] = _smooth(rng, M)
    return masks


def _molded(box, window, W, H):
    """image-pixel box (y1, x1, y2, x2) -> molded coordinates a quarter pixel inside, so that the truncation gives the box back"""
    s = un.box_scale(window, W, H)
    return [(box[0] + 0.25) / s + window[0], (box[1] + 0.25) / s + window[1], (box[2] + 0.25) / s + window[0], (box[3] + 0.25) / s + window[1]]


def _run_stage(ef, det, masks, window, W, H, layout="nhwc", class_map=None, stream=None):
    import torch

    m = masks if layout == "nhwc" else np.ascontiguousarray(masks.transpose(0, 3, 1, 2))
    cm = None if class_map is None else torch.from_numpy(class_map).cuda()
    out = ef.unmold_detections(torch.from_numpy(det).cuda(), torch.from_numpy(m).cuda(), window, (W, H), layout=layout, class_map=cm, padded=True, stream=stream)
    torch.cuda.synchronize()
    return [t.cpu().numpy() for t in out]


def _check_stage(ef, det, masks, window, W, H, layout="nhwc", class_map=None):
    g_m, g_c, g_b, g_s, g_r, g_k = _run_stage(ef, det, masks, window, W, H, layout, class_map)
    m = masks if layout == "nhwc" else np.ascontiguousarray(masks.transpose(0, 3, 1, 2))
    w_m, w_c, w_b, w_s, w_r, w_k = un.unmold_detections(det, m, window, W, H, layout, class_map)
    assert int(g_k[0]) == w_k
    assert np.array_equal(g_r, w_r) and np.array_equal(g_b, w_b) and np.array_equal(g_c, w_c)
    assert np.array_equal(g_s.view(np.int32), w_s.view(np.int32))
    bad = [(k, w_b[k].tolist(), int((g_m[k] != w_m[k]).sum())) for k in range(len(det)) if not np.array_equal(g_m[k], w_m[k])]
    assert not bad, bad[:8]
    return w_m, w_k


def _step8_case(rng, W, H, M, Cn):
    """Every case of step 8 between ordinary rows, excluded rows and a zero class followed by rows that no longer count."""
    win = WINDOWS[W]
    rows = []

    def box(y1, x1, y2, x2, cid, score=None):
        rows.append(_molded((y1, x1, y2, x2), win, W, H) + [cid, rng.uniform(0.1, 1.0) if score is None else score])

    box(5, 7, 60, 90, 1)
    box(0, 0, H, W, 2)                                         # the whole image
    box(H - 1, W - 1, H, W, 3)                                 # the last pixel
    box(10, 20, 10, 50, 1)                                     # zero height: excluded
    box(40, 20, 10, 50, 1)                                     # negative height: excluded
    box(40, 50, 10, 20, 4)                                     # both negative: counts, empty
    box(-3, 10, 30, 40, 4)                                     # above the image: counts, empty
    box(10, 10, H + 1, 40, 4)                                  # below it
    box(10, 10, 40, W + 1, 4)                                  # beyond the right edge
    box(10, -2, 40, 30, 4)
    box(3, 3, 3 + M, 3 + M, 5)                                 # exactly M: both passes the identity
    box(3, 60, 3 + M, 61, 5)                                   # M tall, one wide
    for bad in (np.nan, np.inf, -np.inf, 3.0e7, -3.0e7, 1.6e7):
        rows.append(_molded((10, 10, 40, 40), win, W, H)[:3] + [bad, 2, 0.5])      # x2 not finite / beyond 2^24 (1.6e7: beyond it behind the scale 1.25 only)
    rows.append([np.nan] + _molded((10, 10, 40, 40), win, W, H)[1:] + [2, 0.5])
    for cid in (np.nan, float(Cn), float(Cn + 5), -3.0, 0.5, -0.5, np.inf, 2.75, Cn - 0.25):
        box(20, 30, 70, 95, cid)                               # a class id that names no channel (2.75 -> 2 and C - 0.25 -> C - 1 do)
    first_special = len(rows)
    for _ in range(9):
        box(15, 25, 75, 95, 6)                                 # their channel is spoilt below
    box(30, 30, 31, 31, 7)
    box(0, 0, 1, W, 7)
    box(0, W - 1, H, W, 7)
    rows.append([0.0, 0.0, 0.0, 0.0, -0.0, 0.0])               # the first zero class id
    box(5, 7, 60, 90, 1)                                       # no longer counted
    rows.append([0.0] * 6)
    det = np.array(rows, np.float32)
    masks = _masks_for(rng, det, M, Cn)
    ch = masks[first_special:first_special + 9, :, :, 6]
    ch[0, M // 2, M // 3] = np.nan
    ch[1, 0, 0] = np.inf
    ch[2, M - 1, M - 1] = -np.inf
    ch[3] = 0.25                                               # constant: cs == 0 -> 1, every byte 0
    ch[4, 0, 0], ch[4, 0, M - 1] = 3.0e38, -3.0e38             # cmax - cmin overflows
    ch[5] = np.float32(1e-40) * (ch[5] > 0.5)                  # cs = 1e-40: 255 / cs overflows
    ch[6] = ch[6] * np.float32(1e30)                           # a huge but finite range
    ch[7] = ch[7] * np.float32(1e-30) - np.float32(5.0)
    masks[first_special + 8, 1, 1, 5] = np.nan                 # a NaN in ANOTHER channel does not matter
    return det, masks, win


@pytest.mark.parametrize("size", [TINY, NARROW], ids=["160x120", "100x76"])
def test_stage_equals_the_statement_on_every_case_of_step_8(handles, size):
    rng = np.random.default_rng(31)
    W, H, M, Cn = size["w"], size["h"], 28, 8
    ef = handles(**size)
    det, masks, win = _step8_case(rng, W, H, M, Cn)
    cmap = np.array([0, 11, 22, 33, 44, 55, 66, 77], np.int32)
    for layout in ("nhwc", "nchw"):
        for cm in (None, cmap):
            w_m, kept = _check_stage(ef, det, masks, win, W, H, layout, cm)
    assert kept == len(det) - 5                                # two excluded, the zero class and the two rows behind it
    areas = w_m.reshape(len(det), -1).sum(1)
    assert areas[0] > 0 and areas[1] > 0 and areas[2] <= 1 and (areas[3:8] == 0).all() and areas[8] > 0      # (output rows: the two excluded ones are gone)


def _size_rows(W, H, pairs, win, cid=1):
    """one detection per (w, h), its box placed at a varying corner inside the image"""
    rows = []
    for i, (w, h) in enumerate(pairs):
        x1, y1 = (i * 37) % (W - w + 1), (i * 11) % (H - h + 1)
        rows.append(_molded((y1, x1, y1 + h, x1 + w), win, W, H) + [cid, 0.5])
    return np.array(rows, np.float32)


def test_every_output_size_at_28(handles):
    """M = 28: every width 1 .. 160 and every height 1 .. 120 in two calls of <= 256 rows -- the device's taps against the host's, every ksize, both identities"""
    rng = np.random.default_rng(32)
    ef, (W, H), win = handles(**TINY), (160, 120), WINDOWS[160]
    first = [(w, (w * 7) % H + 1) for w in range(1, W + 1)]
    second = [((h * 13) % W + 1, h) for h in range(1, H + 1)] + [(28, 28), (28, 120), (160, 28), (160, 120)]
    for pairs in (first, second):
        det = _size_rows(W, H, pairs, win)
        masks = _masks_for(rng, det, 28, 3)
        _, kept = _check_stage(ef, det, masks, win, W, H)
        assert kept == len(pairs)


@pytest.mark.parametrize("M", [1, 2, 27, 64])
def test_other_mask_sizes_hold_every_ksize(handles, M):
    rng = np.random.default_rng(33 + M)
    ef, (W, H), win = handles(**TINY), (160, 120), WINDOWS[160]
    ws, hs = {1, 2, 3, M - 1, M, M + 1, 2 * M + 3, 100, 159, 160}, {1, 2, 3, M - 1, M, M + 1, 2 * M + 3, 77, 119, 120}
    for k in range(1, M + 1):                                  # the first output size of every ksize = 2 ceil(M / out) + 1
        ws.add(-(-M // k)); hs.add(-(-M // k))
    ws, hs = sorted(v for v in ws if 1 <= v <= W), sorted(v for v in hs if 1 <= v <= H)
    pairs = [(w, hs[i % len(hs)]) for i, w in enumerate(ws)] + [(ws[(i * 3) % len(ws)], h) for i, h in enumerate(hs)]
    assert len({2 * -(-M // w) + 1 for w, _ in pairs if w <= M}) == len({-(-M // k) for k in range(1, M + 1)})
    det = _size_rows(W, H, pairs, win)
    _, kept = _check_stage(ef, det, _masks_for(rng, det, M, 3), win, W, H, "nchw" if M == 27 else "nhwc")
    assert kept == len(pairs)


def test_no_rows_every_row_excluded_and_1024_rows(handles):
    import torch

    rng = np.random.default_rng(34)
    ef, (W, H), win = handles(**NARROW), (100, 76), WINDOWS[100]
    masks, cls, boxes, scores, rows, kept = ef.unmold_detections(torch.zeros((0, 6), device="cuda"), torch.zeros((0, 28, 28, 81), device="cuda"), win, (W, H), padded=True)
    assert int(kept.item()) == 0 and masks.shape == (0, H, W)
    assert [t.shape[0] for t in ef.unmold_detections(torch.zeros((0, 6), device="cuda"), torch.zeros((0, 81, 28, 28), device="cuda"), win, (W, H), layout="nchw")] == [0] * 5
    det = np.array([_molded((10, 20, 10, 50), win, W, H) + [1, 0.5], _molded((40, 20, 10, 50), win, W, H) + [2, 0.5], _molded((9, 9, 9, 9), win, W, H) + [1, 0.5]], np.float32)
    w_m, k = _check_stage(ef, det, _masks_for(rng, det, 28, 3), win, W, H)
    assert k == 0 and not w_m.any()
    R, M, Cn = 1024, 7, 3
    rows = []
    for i in range(R):
        y1, x1 = int(rng.integers(0, H)), int(rng.integers(0, W))
        y2, x2 = (y1, x1) if i % 5 == 0 else (int(rng.integers(y1, H + 2)), int(rng.integers(x1, W + 2)))      # every fifth excluded, a few beyond the edges
        rows.append(_molded((y1, x1, y2, x2), win, W, H) + [1 + i % 2, rng.uniform()])
    det = np.array(rows, np.float32)
    w_m, k = _check_stage(ef, det, _masks_for(rng, det, M, Cn), win, W, H)
    assert 600 < k < 1024 and w_m[:k].any()


# ---- the full calls against the existing device entries on twins

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


CLASS_MAP = np.array([0, 3, 5, 7, 9, 11, 13, 15], np.int32)


def _area_average(n_out, n_in):
    """[n_out, n_in]: the share of each input sample in each of n_out equal cells (roi_paste_numpy.rois_from_masks' averaging)"""
    e = np.linspace(0.0, n_in, n_out + 1)
    j = np.arange(n_in)
    return np.clip(np.minimum(e[1:, None], j[None, :] + 1.0) - np.maximum(e[:-1, None], j[None, :]), 0.0, None) / (e[1:] - e[:-1])[:, None]


def _unmold_case(st, i, rng, layout="nhwc"):
    """The canned masks of frame i as the default detector would hand them over -- tight boxes in molded coordinates, 28 x 28 area averages in the channel of a
    class id, shuffled, an excluded row among them, zero rows behind -- and the statement's masks and class ids of them:
    (detections, mrcnn_mask in `layout`, masks uint8 [kept, H, W], class ids [kept])."""
    from instancefusion_amd import synth

    W, H, M, Cn = SMALL["w"], SMALL["h"], 28, 8
    canned, _ = synth.canned_masks(st["obj"][i], st["scene"])
    perm = rng.permutation(len(canned))
    rows, chans = [], []
    for j, p in enumerate(perm):
        ys, xs = np.nonzero(canned[p])
        box = (max(ys.min() - 2, 0), max(xs.min() - 2, 0), min(ys.max() + 3, H), min(xs.max() + 3, W))     # two pixels of margin, as a detector's box has
        rows.append(_molded(box, SEG_WINDOW, W, H) + [1 + j % (Cn - 1), rng.uniform(0.7, 1.0)])
        crop = (canned[p][box[0]:box[2], box[1]:box[3]] != 0).astype(np.float64)
        chans.append((_area_average(M, crop.shape[0]) @ crop @ _area_average(M, crop.shape[1]).T).astype(np.float32))
        if j == 1:
            rows.append(_molded((50, 60, 50, 90), SEG_WINDOW, W, H) + [2, 0.9])          # excluded
            chans.append(chans[-1])
    n = len(rows)
    rows += [[0.0] * 6] * 3
    det = np.array(rows, np.float32)
    masks = rng.random((len(det), M, M, Cn)).astype(np.float32)
    for r in range(n):
        masks[r, :, :, int(det[r, 4])] = chans[r]
    w_m, w_c, _, _, w_r, k = un.unmold_detections(det, masks, SEG_WINDOW, W, H, "nhwc", CLASS_MAP)
    assert k == len(canned)
    for kk, p in enumerate(perm):
        m = canned[p]
        if (m != 0).sum() > 50:
            assert ((w_m[kk] != 0) & (m != 0)).sum() / ((w_m[kk] != 0) | (m != 0)).sum() > 0.8    # (the unmolded form is a faithful one of the canned mask)
    if layout == "nchw":
        masks = np.ascontiguousarray(masks.transpose(0, 3, 1, 2))
    return det, masks, w_m[:k], w_c[:k]


def test_full_call_equals_the_device_entry_on_the_statements_masks(ifx, small_stream):
    """Twins at frames 4..7, superpixels on and off, one call with the kNN smoothing, both layouts: the default detector's output on one, the device entry fed
    the statement's u8 masks and class ids on the other."""
    import torch

    st = small_stream
    rng = np.random.default_rng(41)
    cmap = torch.from_numpy(CLASS_MAP).cuda()
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
            layout = "nchw" if i == 7 else "nhwc"
            det, masks, w_m, w_c = _unmold_case(st, i, rng, layout)
            kw = dict(isflann=(i == 6), superpixels=(i != 5))
            kept = ia.process_segmentation_unmolded(torch.from_numpy(det).cuda(), torch.from_numpy(masks).cuda(), SEG_WINDOW, 100 + 3 * i, class_map=cmap, layout=layout, **kw)
            assert kept == len(w_m)
            ib.process_segmentation_device(torch.from_numpy(w_m).cuda(), w_c, 100 + 3 * i, **kw)
            _same(ia, ib, i)
    assert (ia.labels() >= 0).sum() > 100
    assert (ia.getInstanceTable() >= 0).sum() >= 2
    _same_maps(a, b)
    assert np.array_equal(ia.renderProjectMap(), ib.renderProjectMap())
    a.close(); b.close()


def test_deferred_unmolded(ifx, small_stream):
    """Lag 0: snapshot + deferred call equals the ordinary call.  Lag 4 with the camera moving: equals the deferred device entry fed the statement's masks."""
    import torch

    st = small_stream
    rng = np.random.default_rng(42)
    cmap = torch.from_numpy(CLASS_MAP).cuda()
    a, b, ia, ib = _twins(ifx, st, 5, clear_votes=True)
    for k, sp in enumerate((True, False)):
        det, masks, w_m, _ = _unmold_case(st, 4, rng)
        td, tm = torch.from_numpy(det).cuda(), torch.from_numpy(masks).cuda()
        t = ia.snapshot(superpixels=sp)
        assert ia.process_segmentation_deferred_unmolded(t, td, tm, SEG_WINDOW, 100 + 3 * k, class_map=cmap, superpixels=sp) == len(w_m)
        assert ia.snapshot_stats(t)["in_use"] == 0          # a successful call releases its ticket
        ib.process_segmentation_unmolded(td, tm, SEG_WINDOW, 100 + 3 * k, class_map=cmap, superpixels=sp)
        _same(ia, ib, ("lag 0", sp))
    assert (ia.getInstanceTable() >= 0).sum() >= 1
    _same_maps(a, b)
    pose5 = None
    for i in range(5, 10):
        pa = a.processFrame(st["rgb"][i], st["depth"][i]); pb = b.processFrame(st["rgb"][i], st["depth"][i])
        assert np.array_equal(pa, pb)
        if i == 5:
            pose5 = pa.copy()
            ta, tb_ = ia.snapshot(superpixels=True), ib.snapshot(superpixels=True)
    assert not np.array_equal(pose5, pa)                       # the camera moved
    det, masks, w_m, w_c = _unmold_case(st, 5, rng)
    ia.process_segmentation_deferred_unmolded(ta, torch.from_numpy(det).cuda(), torch.from_numpy(masks).cuda(), SEG_WINDOW, 200, class_map=cmap, superpixels=True)
    ib.process_segmentation_deferred_device(tb_, torch.from_numpy(w_m).cuda(), w_c, 200, superpixels=True)
    _same(ia, ib, "lag 4")
    assert (ia.labels() >= 0).sum() > 100
    _same_maps(a, b)
    a.close(); b.close()


def test_tensors_written_on_a_producer_stream(ifx, small_stream):
    """Detections and masks written into zeroed tensors on a side stream behind several milliseconds of other work there; the call gets that stream and no host
    synchronisation: it must wait on the device (a call that does not reads zero class ids, keeps nothing and registers nothing)."""
    import torch

    st = small_stream
    a, b, ia, ib = _twins(ifx, st)
    det, masks, w_m, w_c = _unmold_case(st, 7, np.random.default_rng(43))
    src_d, src_m = torch.from_numpy(det).cuda(), torch.from_numpy(masks).cuda()
    dst_d, dst_m = torch.zeros_like(src_d), torch.zeros_like(src_m)
    cmap = torch.from_numpy(CLASS_MAP).cuda()
    x = torch.randn(4096, 4096, device="cuda") / 64.0
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        y = x
        for _ in range(8):
            y = y @ x
        one = (y[0, 0] == y[0, 0]).to(torch.float32)           # (depends on the chain's result; 1 unless the chain produced NaN)
        dst_d.copy_(src_d * one)
        dst_m.copy_(src_m * one)
    assert ia.process_segmentation_unmolded(dst_d, dst_m, SEG_WINDOW, 100, class_map=cmap, superpixels=True, stream=s) == len(w_m)
    ib.process_segmentation_device(torch.from_numpy(w_m).cuda(), w_c, 100, superpixels=True)
    torch.cuda.synchronize()
    assert torch.equal(dst_d, src_d) and torch.equal(dst_m, src_m)
    assert (ib.getInstanceTable() >= 0).sum() >= 1            # (zeros would register nothing)
    _same(ia, ib, "producer stream")
    _same_maps(a, b)
    a.close(); b.close()


def test_refusals_leave_the_handle_usable(ifx, small_stream):
    """Sharded handle -> IFX_E_STATE for the process entries (the stage runs there); R, M, C, layout, window, NULL pointers -> IFX_E_INVALID with the entry's name
    in front; TypeError / ValueError in Python for a wrong dtype, shape or layout.  After each refusal a valid call on the same handle still equals its twin."""
    import torch

    st = small_stream
    L = ifx.lib()
    det, masks, w_m, w_c = _unmold_case(st, 7, np.random.default_rng(44))
    R = len(det)
    d_d, d_m, d_p = torch.from_numpy(det).cuda(), torch.from_numpy(masks).cuda(), torch.from_numpy(w_m).cuda()
    big_d, big_m = torch.zeros((257, 6), device="cuda"), torch.zeros((257, 2, 2, 2), device="cuda")
    cmap = torch.from_numpy(CLASS_MAP).cuda()
    torch.cuda.synchronize()
    P = lambda t: C.c_void_p(t.data_ptr())
    win = (C.c_int32 * 4)(*SEG_WINDOW)
    kept = C.c_int32(-7)

    e = ifx.ElasticFusion(**SMALL, max_surfels=100000, n_ranks=-1, rank=0)
    try:
        r = L.ifx_process_segmentation_unmolded(e.handle, P(d_d), P(d_m), win, None, R, 28, 8, 0, 100, 0, None, C.byref(kept))
        assert r == -4 and L.ifx_last_error(e.handle).startswith(b"ifx_process_segmentation_unmolded") and b"sharded" in L.ifx_last_error(e.handle)
        assert L.ifx_process_segmentation_deferred_unmolded(e.handle, 0, P(d_d), P(d_m), win, None, R, 28, 8, 0, 100, 0, None, None) == -4
        with pytest.raises(ifx.IfxError, match=r"\(-4\)"):
            ifx.InstanceFusion(e).process_segmentation_unmolded(d_d, d_m, SEG_WINDOW, 100)
        g = e.unmold_detections(d_d, d_m, SEG_WINDOW, (SMALL["w"], SMALL["h"]), class_map=cmap)      # the stage: any handle
        assert np.array_equal(g[0].cpu().numpy(), w_m) and np.array_equal(g[1].cpu().numpy(), w_c)
    finally:
        e.close()

    a, b, ia, ib = _twins(ifx, st)
    frame = 100

    def valid_call(what):
        nonlocal frame
        assert ia.process_segmentation_unmolded(d_d, d_m, SEG_WINDOW, frame, class_map=cmap, superpixels=True) == len(w_m)
        ib.process_segmentation_device(d_p, w_c, frame, superpixels=True)
        _same(ia, ib, what)
        frame += 3

    bad_win = (C.c_int32 * 4)(32, 0, 32, 256)
    refusals = [
        ("R = 257", (P(big_d), P(big_m), win, 257, 2, 2, 0)),
        ("R < 0", (P(d_d), P(d_m), win, -1, 28, 8, 0)),
        ("M = 0", (P(d_d), P(d_m), win, R, 0, 8, 0)),
        ("M = 65", (P(d_d), P(d_m), win, R, 65, 8, 0)),
        ("C = 1", (P(d_d), P(d_m), win, R, 28, 1, 0)),
        ("C = 1025", (P(d_d), P(d_m), win, R, 28, 1025, 0)),
        ("layout 2", (P(d_d), P(d_m), win, R, 28, 8, 2)),
        ("null window", (P(d_d), P(d_m), None, R, 28, 8, 0)),
        ("empty window", (P(d_d), P(d_m), bad_win, R, 28, 8, 0)),
        ("null detections", (None, P(d_m), win, R, 28, 8, 0)),
        ("null masks", (P(d_d), None, win, R, 28, 8, 0)),
    ]
    o_m = torch.zeros((257, SMALL["h"], SMALL["w"]), dtype=torch.uint8, device="cuda")
    o_c, o_b, o_k = torch.zeros(257, dtype=torch.int32, device="cuda"), torch.zeros((257, 4), dtype=torch.int32, device="cuda"), torch.zeros(1, dtype=torch.int32, device="cuda")
    for what, (pd, pm, pw, rr, M, Cn, lay) in refusals:
        assert L.ifx_process_segmentation_unmolded(a.handle, pd, pm, pw, None, rr, M, Cn, lay, frame, 2, None, None) == -1, what
        assert L.ifx_last_error(a.handle).startswith(b"ifx_process_segmentation_unmolded"), what
        t = ia.snapshot()
        assert L.ifx_process_segmentation_deferred_unmolded(a.handle, t, pd, pm, pw, None, rr, M, Cn, lay, frame, 0, None, None) == -1, what
        assert ia.snapshot_stats(t)["in_use"] == 1             # a refused call keeps its ticket
        ia.release_snapshot(t)
        if what != "R = 257":                                  # (the stage takes up to 1024 rows)
            assert L.ifx_unmold_detections(a.handle, pd, pm, pw, None, rr, M, Cn, lay, SMALL["w"], SMALL["h"], P(o_m), P(o_c), P(o_b), None, None, P(o_k), None) == -1, what
            assert L.ifx_last_error(a.handle).startswith(b"ifx_unmold_detections"), what
        valid_call(what)
    for what, args in (("width 0", (0, SMALL["h"], P(o_m), P(o_c), P(o_b), None, None, P(o_k))), ("null kept", (SMALL["w"], SMALL["h"], P(o_m), P(o_c), P(o_b), None, None, None)),
                       ("null masks out", (SMALL["w"], SMALL["h"], None, P(o_c), P(o_b), None, None, P(o_k)))):
        assert L.ifx_unmold_detections(a.handle, P(d_d), P(d_m), win, None, R, 28, 8, 0, *args, None) == -1, what
    valid_call("stage refusals")
    with pytest.raises(TypeError):
        ia.process_segmentation_unmolded(d_d.double(), d_m, SEG_WINDOW, frame)
    with pytest.raises(ValueError):
        ia.process_segmentation_unmolded(d_d[:, :5].contiguous(), d_m, SEG_WINDOW, frame)
    with pytest.raises(ValueError):
        ia.process_segmentation_unmolded(d_d, d_m, SEG_WINDOW, frame, layout="hwc")
    with pytest.raises(ValueError):
        ia.process_segmentation_unmolded(d_d, d_m, (32, 0, 32, 256), frame)
    with pytest.raises(ValueError):
        ia.process_segmentation_unmolded(d_d, d_m.cpu(), SEG_WINDOW, frame)
    valid_call("python refusals")
    _same_maps(a, b)
    a.close(); b.close()
