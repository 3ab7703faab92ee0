"""The photometric tracker term over the frame slot's candidate list (option rgb_cand, default): the frame side decides the pose-independent part of the residual's gate
once per frame (k_frame_maps appends the pixels that pass, with their gradients, to a per-level list), and the residual pass and the step of the frame-to-model
tracker's two-launch iterations run over that list instead of over every pixel.

  1. the list against a numpy statement of the gate (tests/rgb_candidates_numpy.py), as sets -- the list has no order;
  2. the list form against the dense form (rgb_cand = 0), bit for bit: the sums are exact sums of grid-valued terms and integer atomics, so order and partition
     of the pixels do not show;
  3. the same where the model's depth has holes (the NaN test of the model depth is not part of the list: it stays per iteration)."""
import numpy as np
import pytest

import rgb_candidates_numpy as rc

pytestmark = pytest.mark.gpu

SIZES = {"160x120": dict(w=160, h=120, fx=132.0, fy=132.0, cx=80.0, cy=60.0), "320x240": dict(w=320, h=240, fx=264.0, fy=264.0, cx=160.0, cy=120.0)}
BAND_ROWS, BAND_COLS = (50, 56), (70, 77)   # the zero-intensity bands of the "band" frames: rows [50, 56) and columns [70, 77) of level 0


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


def _frame(st, kind, K):
    """The colour image of the frame whose list is read back (its depth is frame 1's)."""
    h, w = K["h"], K["w"]
    rgb = st["rgb"][1].copy()
    if kind in ("noise", "noise_band"):      # nearly every interior pixel is a candidate: the list's capacity is exercised
        rgb = np.random.RandomState(1234).randint(0, 256, (h, w, 3)).astype(np.uint8)
    if kind == "constant":                   # no gradient anywhere: nothing passes
        rgb[:] = 128
    if kind in ("band", "noise_band"):       # zero intensity in a row band and a column band: the 4x4 non-zero rule at their edges
        rgb[BAND_ROWS[0]:BAND_ROWS[1]] = 0
        rgb[:, BAND_COLS[0]:BAND_COLS[1]] = 0
    return rgb


@pytest.mark.parametrize("size", list(SIZES))
@pytest.mark.parametrize("kind", ["synth", "noise", "constant", "band", "noise_band"])
def test_candidate_list_equals_the_numpy_gate(ifx, streams, size, kind):
    """The list of every level against the numpy statement of the gate, evaluated on the level's own intensity and gradient images: equal as sets, gradients included.
    160x120: level 2 (40x30) has no pixel inside the 16-pixel border -- its count is 0 and the tracker still runs.  constant: 0 on every level.  band / noise_band: a
    pixel is excluded exactly when its 4x4 block (2 to the left / above, 1 to the right / below) touches the band."""
    K, st = SIZES[size], streams[size]
    g = ifx.ElasticFusion(max_surfels=400000, **K)
    g.set_option("rgb_cand", 1); g.set_option("gn_persist", 0)
    g.processFrame(st["rgb"][0], st["depth"][0])
    pose = g.processFrame(_frame(st, kind, K), st["depth"][1])
    if kind in ("synth", "constant", "band"):   # (the noise frames are there for the list; what the tracker makes of a frame of noise is not this test's subject)
        assert np.isfinite(pose).all()
    counts = []
    for lvl in range(3):
        img, dx, dy = g.tracker_buffer("next_img", lvl), g.tracker_buffer("didx", lvl), g.tracker_buffer("didy", lvl)
        want = rc.gate_entries(img, dx, dy, lvl)
        n = int(g.tracker_buffer("cand_n", lvl)[0])
        got = g.tracker_buffer("cand", lvl)
        counts.append(n)
        print(f"{size} {kind} level {lvl}: {n} candidates of {img.size} pixels ({100.0 * n / img.size:.1f} %)")
        assert n == got.shape[0] == want.shape[0], (lvl, n, want.shape[0])
        assert np.array_equal(rc.sorted_entries(got), want), lvl
        assert np.unique(got["pixel"]).shape[0] == n, lvl   # no pixel twice
    if size == "160x120":
        assert counts[2] == 0
    if kind == "constant":
        assert counts == [0, 0, 0]
    if kind == "noise":
        inner = (K["h"] - 32) * (K["w"] - 32)
        assert counts[0] > 0.8 * inner, (counts[0], inner)
    if kind in ("band", "noise_band"):   # level 0, in terms of the band itself: columns c0 - 1 .. c1 + 1 and rows r0 - 1 .. r1 + 1 are out, c0 - 2 / c1 + 2 / r0 - 2 / r1 + 2 are not
        got = g.tracker_buffer("cand", 0)
        i, j = got["pixel"] // K["w"], got["pixel"] % K["w"]
        (r0, r1), (c0, c1) = BAND_ROWS, BAND_COLS
        assert not ((j >= c0 - 1) & (j <= c1 + 1)).any() and not ((i >= r0 - 1) & (i <= r1 + 1)).any()
        if kind == "noise_band":   # (on the noise frame the neighbours of the excluded stripes are candidates for certain)
            for edge in (j == c0 - 2, j == c1 + 2, i == r0 - 2, i == r1 + 2):
                assert edge.any()
    g.close()


def _run(ifx, K, rgb, dep, cand, lookahead):
    import torch

    n = rgb.shape[0]
    g = ifx.ElasticFusion(max_surfels=400000, confidence=3.0, **K)
    g.set_option("rgb_cand", cand); g.set_option("gn_persist", 0)
    if lookahead:
        d_rgb = torch.from_numpy(rgb.copy()).cuda()
        d_dep = torch.from_numpy(dep.view(np.int16).copy()).cuda()
        torch.cuda.synchronize()
        for i in range(n):
            if lookahead == "wrong" and i == 5:   # frame 6 announced with frame 0's images: its tracker runs ahead on them and is dropped, its slot is prepared again
                g.hint_next_frame_device(d_rgb[0].data_ptr(), d_dep[0].data_ptr())
            elif i + 1 < n:
                g.hint_next_frame_device(d_rgb[i + 1].data_ptr(), d_dep[i + 1].data_ptr())
            g.enqueue_frame_device(d_rgb[i].data_ptr(), d_dep[i].data_ptr(), i)
        g.sync()
        poses = g.trajectory()
    else:
        poses = np.stack([g.processFrame(rgb[i], dep[i]) for i in range(n)])
    out = dict(poses=poses, ids=g.image("ids_after"), count=g.count, range_exceeded=g.tracker_range_exceeded(),
               cand_n=[int(g.tracker_buffer("cand_n", lvl)[0]) for lvl in range(3)])
    g.close()
    return out


@pytest.mark.parametrize("size", list(SIZES))
@pytest.mark.parametrize("case", ["plain", "lookahead", "wrong_hint", "constant", "half_map"])
def test_list_form_equals_dense_form_bit_for_bit(ifx, streams, size, case):
    """The same 12 frames through two handles, rgb_cand = 1 and 0: every pose of the trajectory, the surfel-id image and the surfel count after the last frame are
    equal in every bit, and no reduction left the exact range.  lookahead: every next frame announced (its frame side, the list included, runs on the side stream; the
    tracker is enqueued ahead).  wrong_hint: one frame is announced with another frame's images -- the tracker enqueued ahead for it is dropped, and while it still runs
    the slot, list and count included, is prepared again for the frame that came: the dropped run must stay inside its buffers whatever count it reads.  constant: a colour image without gradients -- the lists are empty and the photometric sums all zero.  half_map: the right half of
    every depth image is missing, so the map and with it the model's depth cover half the view while the candidates cover all of it: the NaN test of the model
    depth, which is not part of the list, decides there in every iteration."""
    K, st = SIZES[size], streams[size]
    rgb, dep = st["rgb"].copy(), st["depth"].copy()
    if case == "constant":
        rgb[:] = 128
    if case == "half_map":
        dep[:, :, K["w"] // 2:] = 0
    la = {"lookahead": True, "wrong_hint": "wrong"}.get(case, False)
    a = _run(ifx, K, rgb, dep, 1, la)
    b = _run(ifx, K, rgb, dep, 0, la)
    print(f"{size} {case}: candidates of the last frame per level {a['cand_n']}, {a['count']} surfels")
    assert a["poses"].shape == b["poses"].shape and a["poses"].shape[0] == 12
    bits = lambda x: np.ascontiguousarray(x, np.float32).view(np.uint32)
    assert np.array_equal(bits(a["poses"]), bits(b["poses"]))
    assert np.array_equal(a["ids"], b["ids"]) and a["count"] == b["count"]
    assert a["range_exceeded"] == 0 and b["range_exceeded"] == 0
    assert a["cand_n"] == b["cand_n"]                     # (the list is built whatever the option says)
    if case == "constant":
        assert a["cand_n"] == [0, 0, 0]
    else:
        assert a["cand_n"][0] > 0 and a["cand_n"][1] > 0   # the list form had something to run over
