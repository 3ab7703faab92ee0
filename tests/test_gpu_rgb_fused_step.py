"""The photometric step inside the residual launch (option rgb_fuse, a bit per pyramid level): in a list run the photometric blocks of a prologue-chain iteration
run their residual pass, meet -- bounded -- and step the records by chunks claimed from a counter, so the iteration is one launch instead of two.  The sums are
exact sums of grid-valued terms and integer atomics: which block steps which chunk, and whether a block gave up waiting, must not show.

Every case runs the same frames through two handles, rgb_fuse = 7 (or the mask under test) and rgb_fuse = 0 (the two-launch form), and demands the poses, the
surfel-id image and the surfel count equal in every bit and no reduction outside the exact range.  The two-launch run of a (size, case) is computed once and shared."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SIZES = {"160x120": dict(w=160, h=120, fx=132.0, fy=132.0, cx=80.0, cy=60.0), "320x240": dict(w=320, h=240, fx=264.0, fy=264.0, cx=160.0, cy=120.0)}


@pytest.fixture(scope="module")
def ifx():
    import instancefusion_amd as m

    m.lib()
    return m


@pytest.fixture(scope="module")
def streams():
    """12 synthetic frames per size, rendered once and left unchanged (the tests derive their frames from copies)."""
    from instancefusion_amd import synth

    return {name: synth.make_stream(12, K["w"], K["h"], K["fx"], K["fy"], K["cx"], K["cy"], noise=True) for name, K in SIZES.items()}


def _frames(st, K, case):
    rgb, dep = st["rgb"].copy(), st["depth"].copy()
    if case == "constant":      # no gradient anywhere: every list is empty, the meeting and the chunk loop run with n = 0
        rgb[:] = 128
    if case == "half_map":      # the map covers half the view, the candidates all of it: the model depth's NaN test decides in every iteration
        dep[:, :, K["w"] // 2:] = 0
    if case == "noise":         # nearly every interior pixel is a candidate (about 52 200 at level 0 of 320x240): many more chunks than photometric blocks; the real depth stream
        rgb[:] = np.random.RandomState(1234).randint(0, 256, (K["h"], K["w"], 3)).astype(np.uint8)[None]
    return rgb, dep


def _drive(ifx, K, rgb, dep, opts_list, lookahead=False, order=None):
    """The frames `order` (default: all, in turn) through one handle per entry of opts_list, all alive at once and fed frame by frame in turn."""
    import torch

    order = list(range(rgb.shape[0])) if order is None else list(order)
    hs = []
    for opts in opts_list:
        g = ifx.ElasticFusion(max_surfels=400000, confidence=3.0, **K)
        g.set_option("gn_persist", 0)
        for k, v in opts.items():
            g.set_option(k, v)
        hs.append(g)
    if lookahead:
        d_rgb = torch.from_numpy(rgb.copy()).cuda()
        d_dep = torch.from_numpy(dep.view(np.int16).copy()).cuda()
        torch.cuda.synchronize()
        for i, f in enumerate(order):
            for g in hs:
                if lookahead == "wrong" and i % 12 == 5:   # the next frame announced with frame 0's images: its tracker runs ahead on them and is dropped while the slot is prepared again
                    g.hint_next_frame_device(d_rgb[0].data_ptr(), d_dep[0].data_ptr())
                elif i + 1 < len(order):
                    g.hint_next_frame_device(d_rgb[order[i + 1]].data_ptr(), d_dep[order[i + 1]].data_ptr())
                g.enqueue_frame_device(d_rgb[f].data_ptr(), d_dep[f].data_ptr(), i)
        for g in hs:
            g.sync()
        poses = [g.trajectory() for g in hs]
    else:
        poses = [[] for _ in hs]
        for f in order:
            for k, g in enumerate(hs):
                poses[k].append(g.processFrame(rgb[f], dep[f]))
        poses = [np.stack(p) for p in poses]
    outs = []
    for g, p in zip(hs, poses):
        outs.append(dict(poses=p, ids=g.image("ids_after"), count=g.count, range_exceeded=g.tracker_range_exceeded(), giveups=g.tracker_meet_giveups(),
                         cand_n=[int(g.tracker_buffer("cand_n", lvl)[0]) for lvl in range(3)]))
    for g in hs:
        g.close()
    return outs


_LA = {"lookahead": True, "wrong_hint": "wrong"}
_two_launch = {}


def _reference(ifx, streams, size, case):
    """The two-launch form (rgb_fuse = 0) of a (size, case): computed once, shared, left unchanged."""
    key = (size, case)
    if key not in _two_launch:
        K = SIZES[size]
        rgb, dep = _frames(streams[size], K, case)
        _two_launch[key] = _drive(ifx, K, rgb, dep, [dict(rgb_fuse=0)], _LA.get(case, False))[0]
    return _two_launch[key]


def _bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


def _assert_same(a, b, n=12):
    assert a["poses"].shape == b["poses"].shape and a["poses"].shape[0] == n
    assert np.array_equal(_bits(a["poses"]), _bits(b["poses"]))          # the raw words: NaN patterns included
    assert np.array_equal(a["ids"], b["ids"]) and a["count"] == b["count"]
    assert a["range_exceeded"] == 0 and b["range_exceeded"] == 0
    assert a["cand_n"] == b["cand_n"]


def _fused(ifx, streams, size, case, **opts):
    K = SIZES[size]
    rgb, dep = _frames(streams[size], K, case)
    o = dict(rgb_fuse=7)
    o.update(opts)
    return _drive(ifx, K, rgb, dep, [o], _LA.get(case, False))[0]


@pytest.mark.parametrize("size", list(SIZES))
@pytest.mark.parametrize("case", ["plain", "lookahead", "wrong_hint", "constant", "half_map"])
def test_fused_form_equals_two_launch_form_bit_for_bit(ifx, streams, size, case):
    """wrong_hint: a dropped run still executes while its slot -- list, count and records -- is rewritten: it may read any count and any record, must stay in its
    buffers, and must leave the three sets zero for the run that follows.  constant: n = 0 on every level (160x120 has n = 0 at level 2 in every case)."""
    a, b = _fused(ifx, streams, size, case), _reference(ifx, streams, size, case)
    print(f"{size} {case}: candidates of the last frame per level {a['cand_n']}, {a['count']} surfels, meeting give-ups {a['giveups']}")
    _assert_same(a, b)
    assert b["giveups"] == 0                                   # (the two-launch form has no meeting)
    if case == "constant":
        assert a["cand_n"] == [0, 0, 0]
    else:
        assert a["cand_n"][0] > 0 and a["cand_n"][1] > 0
    if size == "160x120":
        assert a["cand_n"][2] == 0


def test_many_chunks_noise_frame(ifx, streams):
    """320x240, a colour image of noise over the real depth stream: about 52 200 candidates at level 0 -- a hundred chunks for 32 photometric blocks, so every block
    claims many times.  The tracker's poses are compared as raw words, finite or not."""
    a, b = _fused(ifx, streams, "320x240", "noise"), _reference(ifx, streams, "320x240", "noise")
    print(f"noise: candidates per level {a['cand_n']}, poses finite: fused {bool(np.isfinite(a['poses']).all())}, two-launch {bool(np.isfinite(b['poses']).all())}, give-ups {a['giveups']}")
    _assert_same(a, b)
    assert a["cand_n"][0] > 45000


@pytest.mark.parametrize("case", ["plain", "noise"])
def test_give_up_path_alone(ifx, streams, case):
    """rgb_fuse_poll = 0: nobody waits at the meeting -- every photometric block but the last arriver leaves at once and the last arriver steps every chunk alone.
    Same bits, and the blocks that left are counted."""
    a, b = _fused(ifx, streams, "320x240", case, rgb_fuse_poll=0), _reference(ifx, streams, "320x240", case)
    print(f"{case}, nobody polls: give-ups {a['giveups']}")
    _assert_same(a, b)
    assert a["giveups"] > 0


@pytest.mark.parametrize("g", [1, 2])
def test_one_and_two_photometric_blocks(ifx, streams, g):
    """res_blocks / rgb_blocks force G = 1 (the block is its own last arriver: no meeting partner, every chunk its own) and G = 2."""
    a, b = _fused(ifx, streams, "320x240", "plain", res_blocks=g, rgb_blocks=g), _reference(ifx, streams, "320x240", "plain")
    _assert_same(a, b)
    if g == 1:
        assert a["giveups"] == 0                               # a last arriver never waits


@pytest.mark.parametrize("mask", [5, 2])
def test_mixed_mask_shares_the_rotation(ifx, streams, mask):
    """rgb_fuse = 5 (levels 0 and 2 fused, level 1 two-launch) and its complement: fused and two-launch iterations alternate across the level changes of a run, so
    the rotation of the three sets is carried by both forms."""
    a, b = _fused(ifx, streams, "320x240", "plain", rgb_fuse=mask), _reference(ifx, streams, "320x240", "plain")
    _assert_same(a, b)


def test_two_handles_alive_and_a_long_run(ifx, streams):
    """Two handles alive at once, fed in turn, over 24 frames (the stream forth and back) with every next frame announced and two of them announced wrongly: the
    rotation crosses many runs, runs that follow a dropped run included, and neither handle's meeting words see the other's."""
    K = SIZES["320x240"]
    rgb, dep = _frames(streams["320x240"], K, "plain")
    order = list(range(12)) + list(range(11, -1, -1))
    a, b = _drive(ifx, K, rgb, dep, [dict(rgb_fuse=7), dict(rgb_fuse=0)], "wrong", order)
    print(f"24 frames, two handles: give-ups {a['giveups']}")
    _assert_same(a, b, 24)
    assert np.isfinite(a["poses"]).all()
