"""The own-records form of the fused photometric step (option rgb_own, a bit per pyramid level): in a fused iteration every photometric block steps the records
it wrote itself -- each thread's first from the registers of its residual pass, the later rounds read back -- instead of claiming chunks, and a block that stops
waiting at the meeting hands its share to the last arriver through the set's orphan and taken masks.  The sums are exact sums of grid-valued terms: which block
steps which record, and whether a share was adopted, must not show.

Every case runs the same frames (the streams of tests/test_gpu_rgb_fused_step.py) through rgb_own = 7 (or the mask under test), rgb_own = 0 (the chunk form) and
rgb_fuse = 0 (the two-launch form), and demands the poses -- as raw words --, the surfel-id image and the surfel count equal and no reduction outside the exact
range.  The two reference runs of a (size, case) are computed once and shared.  A case that polls must count no give-up and no adopted share; a case that does
not (rgb_fuse_poll = 0) must count as many adopted shares as give-ups."""
import numpy as np
import pytest

from test_gpu_rgb_fused_step import SIZES, _bits, _frames

pytestmark = pytest.mark.gpu


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
        g.sync()
        outs.append(dict(poses=p, ids=g.image("ids_after"), count=g.count, range_exceeded=g.tracker_range_exceeded(), giveups=g.tracker_meet_giveups(),
                         adopted=g.tracker_meet_adopted(), cand_n=[int(g.tracker_buffer("cand_n", lvl)[0]) for lvl in range(3)]))
    for g in hs:
        g.close()
    return outs


_LA = {"lookahead": True, "wrong_hint": "wrong"}
_refs = {}


def _references(ifx, streams, size, case):
    """The chunk form (rgb_own = 0) and the two-launch form (rgb_fuse = 0) of a (size, case): computed once, shared, left unchanged."""
    key = (size, case)
    if key not in _refs:
        K = SIZES[size]
        rgb, dep = _frames(streams[size], K, case)
        _refs[key] = tuple(_drive(ifx, K, rgb, dep, [dict(rgb_own=0)], _LA.get(case, False)) + _drive(ifx, K, rgb, dep, [dict(rgb_fuse=0)], _LA.get(case, False)))
    return _refs[key]


def _own(ifx, streams, size, case, **opts):
    K = SIZES[size]
    rgb, dep = _frames(streams[size], K, case)
    o = dict(rgb_own=7)
    o.update(opts)
    return _drive(ifx, K, rgb, dep, [o], _LA.get(case, False))[0]


def _assert_same(a, b, n=12):
    assert a["poses"].shape == b["poses"].shape and a["poses"].shape[0] == n
    assert np.array_equal(_bits(a["poses"]), _bits(b["poses"]))          # the raw words: NaN patterns included
    assert np.array_equal(a["ids"], b["ids"]) and a["count"] == b["count"]
    assert a["range_exceeded"] == 0 and b["range_exceeded"] == 0
    assert a["cand_n"] == b["cand_n"]


def _assert_equals_both(ifx, streams, a, size, case, polls=True):
    chunk, two = _references(ifx, streams, size, case)
    _assert_same(a, chunk)
    _assert_same(a, two)
    assert chunk["giveups"] == 0 and chunk["adopted"] == 0 and two["giveups"] == 0 and two["adopted"] == 0
    if polls:
        assert a["giveups"] == 0 and a["adopted"] == 0
    else:
        assert a["giveups"] > 0 and a["adopted"] == a["giveups"]


@pytest.mark.parametrize("size", list(SIZES))
@pytest.mark.parametrize("case", ["plain", "lookahead", "wrong_hint", "constant", "half_map"])
def test_own_form_equals_chunk_form_and_two_launch_form(ifx, streams, size, case):
    """wrong_hint: a dropped run still executes while its slot -- list, count and records -- is rewritten: it may read any count and any record, must stay in its
    buffers, and must leave the three sets, mask words included, zero for the run that follows.  constant: n = 0 on every level -- no block has a record, all arrive."""
    a = _own(ifx, streams, size, case)
    print(f"{size} {case}: candidates of the last frame per level {a['cand_n']}, {a['count']} surfels, give-ups {a['giveups']}, adopted {a['adopted']}")
    _assert_equals_both(ifx, streams, a, size, case)
    if case == "constant":
        assert a["cand_n"] == [0, 0, 0]
    else:
        assert a["cand_n"][0] > 0 and a["cand_n"][1] > 0


def test_many_rounds_noise_frame(ifx, streams):
    """320x240, a colour image of noise over the real depth stream: about 52 200 candidates at level 0 -- 6 to 7 rounds per thread of the 32 photometric blocks,
    all but the first read back, an odd and an even number of them."""
    a = _own(ifx, streams, "320x240", "noise")
    print(f"noise: candidates per level {a['cand_n']}")
    _assert_equals_both(ifx, streams, a, "320x240", "noise")
    assert a["cand_n"][0] > 45000


@pytest.mark.parametrize("g", [1, 2])
def test_one_and_two_photometric_blocks(ifx, streams, g):
    """res_blocks / rgb_blocks force G = 1 (the block is its own last arriver and runs 9 rounds at level 0) and G = 2."""
    a = _own(ifx, streams, "320x240", "plain", res_blocks=g, rgb_blocks=g)
    _assert_equals_both(ifx, streams, a, "320x240", "plain")


@pytest.mark.parametrize("extra", [0, 1, 2])
def test_round_boundary(ifx, streams, extra):
    """G = n // 256 (+ 0, 1, 2) photometric blocks for the n candidates of level 0 (about 2283 on this stream): some threads get a second round; the last block has a
    partial share; one block has no record at all and must still arrive."""
    n = _references(ifx, streams, "320x240", "plain")[0]["cand_n"][0]
    assert n >= 2 * 256
    a = _own(ifx, streams, "320x240", "plain", rgb_blocks=n // 256 + extra)
    print(f"level 0 has {n} candidates: {n // 256 + extra} photometric blocks")
    _assert_equals_both(ifx, streams, a, "320x240", "plain")


@pytest.mark.parametrize("case,g", [("plain", 0), ("noise", 0), ("plain", 2)])
def test_take_over(ifx, streams, case, g):
    """rgb_fuse_poll = 0: nobody waits -- every photometric block but the last arriver hands its share over (or, where the meeting completed behind its OR, takes
    it back), and the last arriver steps the shares it adopted from memory.  Same bits; every block that left had its share adopted."""
    opts = dict(rgb_fuse_poll=0)
    if g:
        opts.update(res_blocks=g, rgb_blocks=g)
    a = _own(ifx, streams, "320x240", case, **opts)
    print(f"{case}, G = {g or 'default'}, nobody polls: give-ups {a['giveups']}, adopted {a['adopted']}")
    _assert_equals_both(ifx, streams, a, "320x240", case, polls=False)


@pytest.mark.parametrize("own,fuse", [(5, 7), (2, 7), (7, 5)])
def test_mixed_masks_share_the_rotation(ifx, streams, own, fuse):
    """Own-records, chunk and two-launch iterations alternate across the level changes of a run: the rotation of the three sets, mask words included, is carried by
    all forms."""
    a = _own(ifx, streams, "320x240", "plain", rgb_own=own, rgb_fuse=fuse)
    _assert_equals_both(ifx, streams, a, "320x240", "plain")


@pytest.mark.parametrize("other", ["rgb_own=0", "rgb_fuse=0"])
def test_two_handles_alive_and_a_long_run(ifx, streams, other):
    """Two handles alive at once, fed in turn, over 24 frames (the stream forth and back) with every next frame announced and two of them announced wrongly, as
    in tests/test_gpu_rgb_fused_step.py: the rotation crosses many runs, runs that follow a dropped run included, and neither handle's meeting words -- mask
    words included -- see the other's.  Once beside the chunk form, once beside the two-launch form."""
    K = SIZES["320x240"]
    rgb, dep = _frames(streams["320x240"], K, "plain")
    order = list(range(12)) + list(range(11, -1, -1))
    name, value = other.split("=")
    a, b = _drive(ifx, K, rgb, dep, [dict(rgb_own=7), {name: int(value)}], "wrong", order)
    print(f"24 frames, two handles, rgb_own=7 beside {other}: give-ups {a['giveups']}, adopted {a['adopted']}, range guard {a['range_exceeded']} / {b['range_exceeded']}")
    _assert_same(a, b, 24)
    assert np.isfinite(a["poses"]).all()
    assert a["giveups"] == 0 and a["adopted"] == 0
