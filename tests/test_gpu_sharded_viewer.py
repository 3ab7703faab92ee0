"""ifx_owner_render_view on the GPU (ifx_map.hip k_view_quad<true> / k_view_big<true> / k_view_own_resolve / k_view_own_final): ifx_render_view on a spatially sharded map.

Ranks are emulated in one process (sharded.emulate_owner_render_view: the exchanges by hand) unless stated.  Every comparison is an array equality -- ids as integers,
rgba as bit patterns -- between tests/viewer_numpy.py on the whole map, the unsharded GPU render and every rank's sharded output.  Hand-built maps are uploaded:
ifx_map_upload gives row i creation number i on every side, so the three id images are equal as they are."""
import ctypes as C

import numpy as np
import pytest

import viewer_numpy as V
from conftest import SMALL
from test_gpu_owner_seg_device import _both, _check, _device_frames, _frame, _merged, _ranks
from test_gpu_viewer import FACING, FRAME, THR, bits, cam, full_map, ifx_params, rgbw, surfels

pytestmark = pytest.mark.gpu

E_INVALID, E_STATE = -1, -4
VOX = 0.08      # ifx_owner_of: the owner is a hash of the 8 cm voxel of the position


@pytest.fixture(scope="module")
def ifx():
    import instancefusion_amd as m

    m.lib()
    return m


@pytest.fixture(scope="module")
def one(ifx):
    e = ifx.ElasticFusion(**FRAME, max_surfels=1 << 16, confidence=THR)
    yield e
    e.close()


def _make_ranks(ifx, G, cfg=FRAME, cap=1 << 16):
    return [ifx.ElasticFusion(**cfg, max_surfels=cap, confidence=THR, n_ranks=G, rank=r) for r in range(G)]


@pytest.fixture(scope="module")
def ranks(ifx):
    made = {G: _make_ranks(ifx, G) for G in (2, 3)}
    yield made
    for efs in made.values():
        for e in efs:
            e.close()


def owners(ifx, xyz, G):
    p = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)
    out = np.zeros(len(p), np.int32)
    assert ifx.lib().ifx_owner_of(p.ctypes.data_as(C.c_void_p), len(p), G, out.ctypes.data_as(C.c_void_p)) == 0
    return out


def spot(ifx, G, rank, z, x=0.0, y=0.0, avoid=()):
    """the centre of the voxel nearest to (x, y, z) in its z layer that rank `rank` of G owns (positions in `avoid` excluded): at most a few voxels away"""
    kz = np.floor(z / VOX)
    best = None
    for dy in range(-4, 5):
        for dx in range(-4, 5):
            p = ((np.floor(x / VOX) + dx + 0.5) * VOX, (np.floor(y / VOX) + dy + 0.5) * VOX, (kz + 0.5) * VOX)
            if owners(ifx, p, G)[0] == rank and p not in avoid and (best is None or abs(dx) + abs(dy) < best[0]):
                best = (abs(dx) + abs(dy), p)
    assert best is not None
    return best[1]


def render_all(ifx, one, efs, m, mvp, size, what, upload=True, device=False, want_rgba=True, want_ids=True, exchanges=None, **kw):
    """upload everywhere, draw with the numpy rule, on the unsharded handle and on the ranks, ask for equal arrays; -> (rgba, ids) of the rule, the ranks' big quads"""
    from instancefusion_amd import sharded

    kw = dict(dict(threshold=THR, color_type=2, unstable=0, draw_window=0, time=17, time_delta=200, clear_rgb=(1.0, 1.0, 1.0)), **kw)
    if upload:
        for e in [one] + list(efs):
            e.upload(full_map(m))
    w, h = size
    want_rgba_, want_ids_ = V.render_view(m, mvp, w, h, kw["threshold"], kw["color_type"], kw["unstable"], kw["draw_window"], kw["time"], kw["time_delta"], clear_rgb=kw["clear_rgb"])
    rgba, ids = one.render_view(mvp, size, **kw)
    assert np.array_equal(ids, want_ids_) and np.array_equal(bits(rgba), bits(want_rgba_)), what
    outs = sharded.emulate_owner_render_view(efs, mvp, size, device=device, want_rgba=want_rgba, want_ids=want_ids, exchanges=exchanges, **kw)
    for r, (s_rgba, s_ids) in enumerate(outs):
        if device:
            s_rgba, s_ids = (None if t is None else t.cpu().numpy() for t in (s_rgba, s_ids))
        assert (s_ids is None) == (not want_ids) and (s_rgba is None) == (not want_rgba)
        if want_ids:
            assert s_ids.shape == (h, w) and np.array_equal(s_ids, want_ids_), (what, r, int((s_ids != want_ids_).sum()))
        if want_rgba:
            assert s_rgba.shape == (h, w, 4) and np.array_equal(bits(s_rgba), bits(want_rgba_)), (what, r, int((bits(s_rgba) != bits(want_rgba_)).any(-1).sum()))
    big = [e.L.ifx_owner_render_view_big_quads(e.handle) for e in efs]
    return want_rgba_, want_ids_, big


def own_big(ifx, m, G, mvp, size, **kw):
    """big quads per rank by the rule: V.render_view's count on the rows each rank owns"""
    own = owners(ifx, m["pc"][:, :3], G)
    out = []
    for r in range(G):
        info = {}
        sub = {k: v[own == r] for k, v in m.items()}
        V.render_view(sub, mvp, size[0], size[1], kw.get("threshold", THR), 2, kw.get("unstable", 0), 0, 17, 200, info=info)
        out.append(info["big"])
    return out


# ------------------------------------------------------------------ hand-built maps
@pytest.mark.parametrize("G", [2, 3])
@pytest.mark.parametrize("case", ["ranks 0 1", "ranks 1 0", "same rank"])
def test_depth_tie_goes_to_the_lower_creation_number(ifx, one, ranks, G, case):
    """two facing surfels at one depth, a voxel or so apart and wide enough to overlap: where both draw the same 24-bit depth, the lower row wins, whoever owns it.
    A tie pixel is one that the rule gives to row 0 in BOTH row orders (a strictly nearer surfel would win in both)."""
    ra, rb = {"ranks 0 1": (0, 1), "ranks 1 0": (1, 0), "same rank": (G - 1, G - 1)}[case]
    pa = spot(ifx, G, ra, 1.0)
    pb = spot(ifx, G, rb, 1.0, avoid=(pa,))
    rows = [(*pa, 10, *FACING, 0.3, rgbw(255, 0, 0), rgbw(1, 1, 1), 1, 1), (*pb, 10, *FACING, 0.3, rgbw(0, 0, 255), rgbw(2, 2, 2), 1, 1)]
    m, swapped = surfels(rows), surfels(rows[::-1])
    assert list(owners(ifx, m["pc"][:, :3], G)) == [ra, rb]
    ids_ab = V.render_view(m, cam(), 64, 48, THR, 2)[1]
    ids_ba = V.render_view(swapped, cam(), 64, 48, THR, 2)[1]
    tie = (ids_ab == 0) & (ids_ba == 0)
    assert tie.sum() > 100
    for mm, what in ((m, case), (swapped, case + ", rows swapped")):
        rgba, ids, _ = render_all(ifx, one, ranks[G], mm, cam(), (64, 48), what)
        assert np.all(ids[tie] == 0)
        assert np.array_equal(bits(rgba[tie][0]), bits(V.render_view({k: v[:1] for k, v in mm.items()}, cam(), 64, 48, THR, 2)[0][tie][0]))      # row 0's colour


@pytest.mark.parametrize("small_z", [1.0, 3.0])
def test_large_quad_meets_small_quads_of_another_rank(ifx, one, ranks, small_z):
    G = 2
    pb = spot(ifx, G, 0, 2.0)
    ps = [spot(ifx, G, 1, small_z, x=0.05 * small_z, y=0.02 * small_z), spot(ifx, G, 1, small_z, x=-0.2 * small_z, y=-0.1 * small_z)]
    m = surfels([(*pb, 10, *FACING, 2.0, rgbw(10, 200, 10), rgbw(1, 1, 1), 1, 1)] + [(*p, 10, *FACING, 0.04 * small_z, rgbw(200, 10, 10), rgbw(2, 2, 2), 1, 1) for p in ps])
    assert list(owners(ifx, m["pc"][:, :3], G)) == [0, 1, 1]
    _, ids, big = render_all(ifx, one, ranks[G], m, cam(), (64, 48), f"small quads at {small_z}")
    assert big == own_big(ifx, m, G, cam(), (64, 48)) == [1, 0]
    assert ((ids == 1).sum() > 5 and (ids == 2).sum() > 5) == (small_z < 2.0) and (ids == 0).sum() > 2000


def test_unstable_surfel_pushed_back_on_another_rank(ifx, one, ranks):
    """test_gpu_viewer's case across the shard boundary: the unstable surfel one voxel in front (0.009 in window depth) is pushed back by its radius (0.09) and loses to
    the stable one behind it"""
    G = 2
    pst = spot(ifx, G, 0, 1.0)
    pun = spot(ifx, G, 1, 1.0 - VOX, x=pst[0], y=pst[1])
    m = surfels([(*pst, 10, *FACING, 0.2, rgbw(200, 0, 0), rgbw(1, 1, 1), 1, 1), (*pun, 1.0, *FACING, 0.09, rgbw(0, 200, 0), rgbw(2, 2, 2), 1, 1)])
    assert list(owners(ifx, m["pc"][:, :3], G)) == [0, 1] and 0 < m["pc"][0, 2] - m["pc"][1, 2] < 0.2
    alone = V.render_view({k: v[1:] for k, v in m.items()}, cam(), 64, 48, THR, 2, 1)[1] == 0
    _, ids, _ = render_all(ifx, one, ranks[G], m, cam(), (64, 48), "unstable in front", unstable=1)
    both = alone & (V.render_view({k: v[:1] for k, v in m.items()}, cam(), 64, 48, THR, 2, 1)[1] == 0)
    assert both.sum() > 50 and np.all(ids[both] == 0)      # behind after the push
    _, ids, _ = render_all(ifx, one, ranks[G], m, cam(), (64, 48), "both stable", upload=False, threshold=0.5)
    assert np.all(ids[both] == 1)


def random_map(seed, n=64):
    rs = np.random.default_rng(seed)
    nrm = rs.normal(size=(n, 3)); nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    return dict(pc=np.c_[rs.uniform(-1, 1, n), rs.uniform(-0.7, 0.7, n), rs.uniform(0.05, 4.0, n), rs.choice([1.0, 10.0], n)].astype(np.float32),
                nr=np.c_[nrm, rs.uniform(0.01, 0.4, n)].astype(np.float32),
                col=np.c_[rs.integers(0, 1 << 24, n), np.where(rs.random(n) < 0.8, rs.integers(0, 1 << 24, n), -1)].astype(np.float32),
                tm=np.c_[rs.integers(1, 17, n), rs.integers(1, 17, n)].astype(np.float32))


@pytest.mark.parametrize("G", [2, 3])
def test_random_surfels_every_colour_type(ifx, one, ranks, G):
    """64 random surfels on a 37 x 29 viewport (1073 pixels: no multiple of 256), colour types 0..4, stable only and with the unstable ones, the time window on and off"""
    m = random_map(5 + G)
    size = (37, 29)
    mvp = cam(w=37, h=29, f=35.0)
    own = owners(ifx, m["pc"][:, :3], G)
    seen_big = 0
    for ct in range(5):
        unstable = ct % 2
        _, ids, big = render_all(ifx, one, ranks[G], m, mvp, size, f"random type {ct}", upload=ct == 0, color_type=ct, unstable=unstable, draw_window=int(ct in (1, 2)), time_delta=5)
        winners = np.unique(ids[ids >= 0])
        assert set(own[winners]) == set(range(G)), (ct, "every rank owns a surfel that wins a pixel")
        assert big == own_big(ifx, m, G, mvp, size, unstable=unstable)
        seen_big += sum(big)
    assert seen_big > 0


def test_a_rank_that_owns_nothing_and_an_empty_map(ifx, one):
    G = 2
    efs = _make_ranks(ifx, G, cap=1 << 12)
    fresh = ifx.ElasticFusion(**FRAME, max_surfels=1 << 12, confidence=THR)
    try:
        clear = (0.25, 0.5, 0.75)
        rgba, ids, big = render_all(ifx, fresh, efs, surfels([]), cam(), (64, 48), "empty map", upload=False, clear_rgb=clear)
        assert np.all(ids == -1) and big == [0, 0]
        assert np.array_equal(rgba, np.broadcast_to(np.array([*clear, 0.0], np.float32), (48, 64, 4)))
        ps = [spot(ifx, G, 1, 1.0), spot(ifx, G, 1, 1.5, x=0.3)]
        m = surfels([(*p, 10, *FACING, 0.1, rgbw(200, 100, 0), rgbw(1, 1, 1), 1, 1) for p in ps])
        assert list(owners(ifx, m["pc"][:, :3], G)) == [1, 1]
        rgba, ids, _ = render_all(ifx, fresh, efs, m, cam(), (64, 48), "rank 0 owns nothing", clear_rgb=clear)
        assert efs[0].count == 0 and efs[1].count == 2 and (ids == 0).any() and (ids == 1).any() and (ids == -1).any()
        assert np.array_equal(rgba[ids == -1][0], np.array([*clear, 0.0], np.float32))
    finally:
        for e in efs + [fresh]:
            e.close()


def test_one_output_calls(ifx, one, ranks):
    m = random_map(3)
    ex = []
    render_all(ifx, one, ranks[2], m, cam(), (64, 48), "ids only", want_rgba=False, exchanges=ex)
    assert ex == [400]      # the keys; no colour block, no second exchange
    ex = []
    render_all(ifx, one, ranks[2], m, cam(), (64, 48), "rgba only", upload=False, want_ids=False, exchanges=ex, color_type=4)
    assert ex == [400, 401]
    ex = []
    render_all(ifx, one, ranks[2], m, cam(), (64, 48), "both", upload=False, exchanges=ex, color_type=1)
    assert ex == [400, 401]
    from instancefusion_amd import sharded
    assert sharded.emulate_owner_render_view(ranks[2], cam(), (64, 48), want_rgba=False, want_ids=False) == [(None, None)] * 2      # nothing asked for: no exchange


def test_back_to_back_calls_do_not_see_each_other(ifx, one, ranks):
    a, b = random_map(11), random_map(12, n=40)
    efs = ranks[3]
    _, ids_a, _ = render_all(ifx, one, efs, a, cam(), (64, 48), "map a")
    _, ids_b, _ = render_all(ifx, one, efs, b, cam(), (64, 48), "map b behind map a")
    assert not np.array_equal(ids_a, ids_b)
    close = cam(w=128, h=96, f=120.0)
    _, big_ids, _ = render_all(ifx, one, efs, b, close, (128, 96), "a larger viewport: the buffers regrow", upload=False, color_type=4)
    assert (big_ids >= 0).sum() > 2000
    _, ids_b2, _ = render_all(ifx, one, efs, b, cam(), (64, 48), "64 x 48 behind 128 x 96", upload=False)
    assert np.array_equal(ids_b2, ids_b)
    render_all(ifx, one, efs, b, cam(w=37, h=29, f=35.0), (37, 29), "37 x 29 behind it", upload=False, color_type=0)


def test_device_outputs_equal_host_outputs(ifx, one, ranks):
    m = random_map(21)
    render_all(ifx, one, ranks[2], m, cam(), (64, 48), "host outputs", color_type=4)
    render_all(ifx, one, ranks[2], m, cam(), (64, 48), "device outputs", upload=False, device=True, color_type=4)
    render_all(ifx, one, ranks[2], m, cam(), (64, 48), "device ids alone", upload=False, device=True, want_rgba=False)


# ------------------------------------------------------------------ refusals
def _bad_params(e):
    bad = [ifx_params(e, cam(), w, h) for w, h in ((0, 48), (64, 0), (4097, 48), (64, 4097), (-1, 48))]
    bad += [ifx_params(e, cam(), 64, 48, color_type=ct) for ct in (-1, 5)]
    for v in (float("nan"), float("inf")):
        mvp = cam().copy(); mvp[2, 1] = v
        bad.append(ifx_params(e, mvp, 64, 48))
    return bad


def test_refusals_write_nothing(ifx, one, small_stream):
    """IFX_E_INVALID where ifx_render_view returns it; IFX_E_STATE on an unsharded handle, without a communicator, _resume without _begin, between the phases of a
    frame, while a segmentation call or an id render waits for its exchange -- the outputs untouched every time"""
    import torch

    from instancefusion_amd import sharded, synth

    st = small_stream
    L = ifx.lib()
    rgba, ids = np.full((48, 64, 4), 7.0, np.float32), np.full((48, 64), 7, np.int32)
    outs = (rgba.ctypes.data_as(C.c_void_p), ids.ctypes.data_as(C.c_void_p), None, None)

    def untouched():
        return bool(np.all(rgba == 7.0) and np.all(ids == 7))

    def begin(e, p):
        return L.ifx_owner_render_view_begin(e.handle, C.byref(p), 1, 1)

    def one_call(e, p):
        return L.ifx_owner_render_view(e.handle, C.byref(p), *outs)

    def resume(e):
        return L.ifx_owner_render_view_resume(e.handle, *outs)

    def idle(e):      # no exchange of the viewer is listed
        return not sharded._exchange_spec(e, 400) and not sharded._exchange_spec(e, 401)

    good = ifx_params(one, cam(), 64, 48)
    d_rgb, d_dep = _device_frames(st, 3)
    ef = ifx.ElasticFusion(**SMALL, max_surfels=400000, n_ranks=-1, rank=0)
    try:
        # an unsharded handle
        assert begin(one, good) == E_STATE and one_call(one, good) == E_STATE and resume(one) == E_STATE and untouched()
        assert L.ifx_owner_render_view_big_quads(one.handle) == E_STATE
        # bad parameters, through both forms; the one-call form without a communicator
        for p in _bad_params(ef):
            assert begin(ef, p) == E_INVALID and one_call(ef, p) == E_INVALID and idle(ef) and untouched()
        assert one_call(ef, good) == E_STATE and b"communicator" in L.ifx_last_error(ef.handle) and idle(ef) and untouched()
        assert resume(ef) == E_STATE and untouched()      # no _begin
        # between the phases of a frame (a world of one: every exchange is the identity)
        ef.set_option("own_lazy_ids", 1)
        for i in range(2):
            for phase in (310, 300, 301) + tuple(range(8)):
                assert L.ifx_owner_frame_phase(ef.handle, phase, C.c_void_p(d_rgb[i].data_ptr()), C.c_void_p(d_dep[i].data_ptr())) == 0
                if 0 <= phase < 7:
                    assert begin(ef, good) == E_STATE and b"phases of a frame" in L.ifx_last_error(ef.handle) and idle(ef)
        for step in range(3):
            assert L.ifx_owner_predict_phase(ef.handle, step) == 0
            assert (begin(ef, good) == E_STATE) == (step < 2)
            if step == 2:      # behind the last phase the call is taken: a pending render refuses a second one, and a frame
                assert begin(ef, good) == E_STATE and b"already waiting" in L.ifx_last_error(ef.handle)
                assert L.ifx_owner_frame_phase(ef.handle, 0, C.c_void_p(d_rgb[2].data_ptr()), C.c_void_p(d_dep[2].data_ptr())) == E_STATE
                assert resume(ef) == 1 and untouched()      # (the colour block's exchange is pending: no output is written yet)
                assert sharded._exchange_spec(ef, 401) and not sharded._exchange_spec(ef, 400)
                assert resume(ef) == 0 and idle(ef) and not untouched()
                rgba[:] = 7.0; ids[:] = 7
        # an id render of the shard waits for its exchange (option own_lazy_ids: the frame left the sampled lattice)
        sharded.emulate_owner_ranks([ef], d_rgb[2].data_ptr(), d_dep[2].data_ptr())
        assert L.ifx_owner_ids_begin(ef.handle) == 1
        assert begin(ef, good) == E_STATE and idle(ef) and untouched()
        assert L.ifx_owner_ids_resume(ef.handle) == 0
        # a segmentation call waits for its exchange
        masks, cls = synth.canned_masks(st["obj"][2], st["scene"])
        assert sharded._seg_begin(ef, st["rgb"][2], st["depth"][2], masks, cls, 2, False) == 1
        assert begin(ef, good) == E_STATE and idle(ef) and untouched()
        r = 1
        while r == 1:
            r = L.ifx_owner_segmentation_resume(ef.handle)
        assert r == 0
        # an output _begin was not asked for
        assert L.ifx_owner_render_view_begin(ef.handle, C.byref(good), 0, 1) == 1
        assert resume(ef) == E_INVALID and untouched()
        assert L.ifx_owner_render_view_resume(ef.handle, None, outs[1], None, None) == 0 and idle(ef) and np.all(rgba == 7.0) and not np.all(ids == 7)
        torch.cuda.synchronize()
    finally:
        ef.close()


# ------------------------------------------------------------------ live maps
def _live_cameras(ifx, pose):
    moved = np.array(pose, np.float32).copy()
    a = np.float32(0.35)
    moved[:3, :3] = moved[:3, :3] @ np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]], np.float32)
    moved[:3, 3] += np.array([0.25, -0.1, -0.3], np.float32)
    return [("tracked pose", ifx.viewer_mvp(SMALL["fx"] / 2, SMALL["fy"] / 2, 80.0, 60.0, 160, 120, 0.1, 1000.0, pose), (160, 120)),
            ("displaced camera", ifx.viewer_mvp(90.0, 90.0, 100.5, 45.5, 201, 91, 0.1, 1000.0, moved), (201, 91))]


@pytest.mark.parametrize("world", [2, 3])
def test_live_map_equals_the_unsharded_render(ifx, small_stream, world):
    """a few frames on one handle and on emulated ranks: colours bit-equal; the unsharded slots (compacted) are creation numbers through the merged, sorted seq() of
    the ranks, and the ids are equal under that map"""
    from instancefusion_amd import sharded

    one, efs = _ranks(ifx, small_stream, SMALL, world, 6, 4)
    try:
        one.compact()
        seqs = [e.seq() for e in efs]
        seq_all = np.sort(np.concatenate(seqs)).astype(np.int64)
        assert one.count == len(seq_all) > 5000
        for name, mvp, size in _live_cameras(ifx, one.getCurrPose()):
            for kw in (dict(color_type=4, unstable=True, draw_window=True), dict(color_type=2), dict(color_type=3, time_delta=2, draw_window=True)):
                rgba, ids = one.render_view(mvp, size, **kw)
                want = np.where(ids >= 0, seq_all[np.maximum(ids, 0)], -1)
                assert (ids >= 0).sum() > 1000, name
                for r, (s_rgba, s_ids) in enumerate(sharded.emulate_owner_render_view(efs, mvp, size, **kw)):
                    assert np.array_equal(s_ids.astype(np.int64), want), (name, kw, r)
                    assert np.array_equal(bits(s_rgba), bits(rgba)), (name, kw, r)
                won = np.unique(want[want >= 0])
                assert all(np.isin(won, s.astype(np.int64)).any() for s in seqs), (name, "winners come from every rank")
    finally:
        for e in efs + [one]:
            e.close()


def test_read_only_between_frames_on_the_ranks(ifx, small_stream):
    """renders on the ranks between frame 6 and frame 7 (none on the unsharded handle): the shards are unchanged, and the next frame and the next segmentation call
    still equal the unsharded run -- the sharded analogue of test_gpu_viewer.py::test_read_only_between_frames"""
    from instancefusion_amd import sharded

    st = small_stream
    world = 2
    one, efs = _ranks(ifx, st, SMALL, world, 6, 4)
    try:
        d_rgb, d_dep = _device_frames(st, 8)
        before = [e.download() for e in efs]
        one.download()      # (a download compacts: the same on both sides)
        for name, mvp, size in _live_cameras(ifx, one.getCurrPose()):
            first = sharded.emulate_owner_render_view(efs, mvp, size, color_type=4, unstable=True, draw_window=True)
            again = sharded.emulate_owner_render_view(efs, mvp, size, color_type=4, unstable=True, draw_window=True)      # the call after it gives the same result
            assert (first[0][1] >= 0).sum() > 2000
            assert all(np.array_equal(a[1], b[1]) and np.array_equal(bits(a[0]), bits(b[0])) for a, b in zip(first, again))
        for e, b in zip(efs, before):
            a = e.download()
            assert all(np.array_equal(bits(a[k]), bits(b[k])) for k in b)
        one.download()
        for i in (6, 7):
            _frame(one, efs, d_rgb, d_dep, i)
            assert all(np.array_equal(e.getCurrPose(), one.getCurrPose()) for e in efs), i
        _both(ifx, one, efs, st, 7, "image-u8", -1, np.random.default_rng(1))
        _check(ifx, one, efs, "behind the renders")
        for k in ("pc", "nr", "col", "tm"):
            assert np.array_equal(bits(_merged(efs, lambda e: e.download()[k])), bits(one.download()[k])), k
    finally:
        for e in efs + [one]:
            e.close()


@pytest.mark.parametrize("transport", ["library", "torch"])
def test_world_of_one_equals_the_unsharded_render(ifx, one, transport):
    """n_ranks = -1: OwnerShardedElasticFusion.render_view, host and device outputs; with the library's communicator the call is two collectives and 24 B / pixel"""
    from instancefusion_amd import sharded

    m = random_map(31)
    ef = ifx.ElasticFusion(**FRAME, max_surfels=1 << 16, confidence=THR, n_ranks=-1, rank=0)
    try:
        osh = sharded.OwnerShardedElasticFusion(ef, None, transport=transport)
        one.upload(full_map(m)); ef.upload(full_map(m))
        w, h = 37, 29
        mvp = cam(w=w, h=h, f=35.0)
        kw = dict(color_type=4, threshold=THR, unstable=True, time=17, time_delta=5, draw_window=True, clear_rgb=(0.0, 0.5, 1.0))
        rgba, ids = one.render_view(mvp, (w, h), **kw)
        assert len(np.unique(ids)) > 8
        if transport == "library":
            osh.exchange_stats(reset=True)
        s_rgba, s_ids = osh.render_view(mvp, (w, h), **kw)
        if transport == "library":
            assert osh.exchange_stats(reset=True) == dict(collectives=2, bytes=24 * w * h)
        assert np.array_equal(s_ids, ids) and np.array_equal(bits(s_rgba), bits(rgba))
        d_rgba, d_ids = osh.render_view(mvp, (w, h), device=True, **kw)
        assert d_rgba.is_cuda and np.array_equal(d_ids.cpu().numpy(), ids) and np.array_equal(bits(d_rgba.cpu().numpy()), bits(rgba))
        assert ef.L.ifx_owner_render_view_big_quads(ef.handle) == one.L.ifx_render_view_big_quads(one.handle)
        if transport == "library":      # the ids alone: one collective, 8 B / pixel
            p = ifx_params(ef, mvp, w, h)
            only = np.zeros((h, w), np.int32)
            osh.exchange_stats(reset=True)
            assert ef.L.ifx_owner_render_view(ef.handle, C.byref(p), None, only.ctypes.data_as(C.c_void_p), None, None) == 0
            assert osh.exchange_stats(reset=True) == dict(collectives=1, bytes=8 * w * h)
            assert np.array_equal(only, one.render_view(mvp, (w, h), threshold=THR, color_type=0, time=17, time_delta=200)[1])
    finally:
        ef.close()
