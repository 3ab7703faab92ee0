"""The numpy statement of the proposal stage and of the box decoding (tests/rpn_proposals_numpy.py) against maskrcnn-benchmark's own Python
(tests/golden/rpn_proposals_ref.npz, written by tools/make_golden_rpn_proposals.py), its exponential against exp, and the directed cases: what each is for.
No GPU needed."""
import os

import numpy as np
import pytest

import rpn_proposals_cases as rc
import rpn_proposals_numpy as rp
from conftest import ROOT

F = np.float32
GOLDEN = os.path.join(ROOT, "tests", "golden", "rpn_proposals_ref.npz")


@pytest.fixture(scope="module")
def golden():
    return dict(np.load(GOLDEN))


@pytest.fixture(scope="module")
def directed():
    return rc.directed()


def test_the_statement_has_the_references_proposals(golden):
    """Equal count, equal order, and every coordinate within 2 ulp of the largest magnitude among pcx, pcy, pw and ph of its box.  The bound is derived: EXP and
    torch.exp are each within 1 ulp of the true value, and the products and sums add one rounding each.  The largest difference seen is the golden file's."""
    worst, proposals = 0.0, 0
    shapes = set()
    for k in range(int(golden["counts"][0])):
        obj, reg, anc = golden[f"rpn{k}_objectness"], golden[f"rpn{k}_regression"], golden[f"rpn{k}_anchors"]
        iw, ih, pre, post, thr, min_size, ties, at_thr, at_size = golden[f"rpn{k}_par"]
        assert ties == 0 and at_thr == 0 and at_size == 0                              # what the tool stores of the draws it rejects
        assert anc.shape[0] <= 3000
        boxes, logits, index = rp.rpn_proposals(obj, reg, anc, (int(iw), int(ih)), int(pre), int(post), thr, min_size)
        ref = golden[f"rpn{k}_boxes"]
        assert boxes.shape == ref.shape and np.array_equal(index, golden[f"rpn{k}_index"]), k
        with np.errstate(over="ignore"):
            assert np.array_equal((F(1) / (F(1) + np.exp(-logits.astype(np.float64)))).astype(F).argsort(), golden[f"rpn{k}_score"].argsort())
        if index.size:
            _, codes = rp.flatten(obj, reg)
            unit = rp.coordinate_ulp(codes[index], anc[index])
            err = float((np.abs(boxes.astype(np.float64) - ref) / unit).max())
            assert err <= 2.0, (k, err)
            worst = max(worst, err)
        proposals += index.size
        shapes.add(obj.shape[0])
    print(f"{proposals} proposals; largest difference {worst:.3f} of the unit (the tool saw {golden['worst_ulp'][0]:.3f}; bound 2)")
    assert shapes == {1, 3, 15} and proposals > 500
    assert worst == golden["worst_ulp"][0]


def test_the_statement_has_the_references_decoded_boxes(golden):
    worst, ks = 0.0, set()
    for k in range(int(golden["counts"][1])):
        codes, boxes, weights, ref = golden[f"dec{k}_codes"], golden[f"dec{k}_boxes"], golden[f"dec{k}_weights"], golden[f"dec{k}_out"]
        mine = rp.box_decode(codes, boxes, weights)
        unit = np.repeat(rp.coordinate_ulp(codes, boxes, weights), 4, axis=1)
        assert mine.shape == ref.shape
        err = float((np.abs(mine.astype(np.float64) - ref) / unit).max())
        assert err <= 2.0, (k, err)
        worst = max(worst, err)
        ks.add(codes.shape[1] // 4)
        assert (codes[:, 2::4] / weights[2] > rp.XFORM_CLIP).any() or codes.shape[0] * codes.shape[1] < 40     # the clip is at work
    print(f"largest difference {worst:.3f} of the unit (the tool saw {golden['worst_ulp'][1]:.3f}; bound 2)")
    assert ks == {1, 2, 81} and worst == golden["worst_ulp"][1]


def test_exp_is_within_one_ulp_of_exp(golden):
    x = rp.exp_sweep()
    assert x.size == int(golden["exp_differs"][1]) and x[0] == -104 and x[-2] == 90 and x[-1] == rp.XFORM_CLIP
    with np.errstate(over="ignore", under="ignore"):
        mine, lib = rp.EXP(x), np.exp(x.astype(np.float64)).astype(F)
    steps = np.abs(mine.view(np.int32).astype(np.int64) - lib.view(np.int32).astype(np.int64))
    print(f"EXP differs from float32(exp(float64(x))) on {int((steps != 0).sum())} of {x.size} arguments (the tool saw {int(golden['exp_differs'][0])})")
    assert steps.max() <= 1
    assert int((steps != 0).sum()) == int(golden["exp_differs"][0])
    assert np.isnan(rp.EXP(F(np.nan))) and rp.EXP(F(-200)) == 0 and rp.EXP(F(0)) == 1 and rp.EXP(F(-0.0)) == 1


def _run(case):
    obj, reg, anc, img, pre, post, thr, min_size = case
    return rp.rpn_proposals(obj, reg, anc, img, pre, post, thr, min_size)


def test_all_logits_equal_selects_the_lowest_indices(directed):
    obj, reg, anc, img, pre, post, thr, min_size = directed["all_equal"]
    _, logits, index = rp.candidates(obj, reg, anc, img, pre, min_size)
    assert index.tolist() == list(range(pre)) and (logits == F(0.25)).all()
    _, _, kept = _run(directed["all_equal"])
    assert 0 < kept.size < pre and (np.diff(kept) > 0).all()


def test_ties_that_straddle_the_rank(directed):
    obj, reg, anc, img, pre, post, thr, min_size = directed["ties_straddle"]
    logits, _ = rp.flatten(obj, reg)
    boxes, lg, index = _run(directed["ties_straddle"])
    assert index.size == pre                                                          # nothing filtered, nothing suppressed: the selection itself
    last = lg[-1]
    tied = np.nonzero(logits == last)[0]
    inside = index[lg == last]
    assert 0 < inside.size < tied.size and np.array_equal(inside, tied[:inside.size])     # of the tied anchors, the lowest indices, ascending
    assert (logits[np.setdiff1d(np.arange(logits.size), index)] <= last).all() and (np.diff(lg) <= 0).all()


def test_nan_and_infinite_logits(directed):
    obj, reg, anc, img, pre, post, thr, min_size = directed["nan_inf_logits"]
    logits, _ = rp.flatten(obj, reg)
    _, lg, index = _run(directed["nan_inf_logits"])
    assert index.size == pre and index[0] == 3                                        # +inf first
    nan = np.nonzero(np.isnan(logits))[0]
    numbers = logits.size - nan.size
    assert np.isnan(lg[numbers:]).all() and not np.isnan(lg[:numbers]).any()          # every NaN behind every number ...
    assert np.array_equal(index[numbers:], nan[:pre - numbers])                       # ... by ascending index
    assert index[numbers - 1] == 4                                                    # -inf: the last number
    zeros = index[lg == 0]
    assert np.array_equal(zeros, np.sort(zeros)) and {5, 6} <= set(zeros.tolist())    # -0 == +0: by index


def test_nan_codes_are_removed(directed):
    obj, reg, anc, img, pre, post, thr, min_size = directed["nan_codes"]
    _, codes = rp.flatten(obj, reg)
    bad = np.nonzero(np.isnan(codes).any(axis=1))[0]
    _, _, index = rp.candidates(obj, reg, anc, img, pre, min_size)
    assert bad.size > 10 and index.size == obj.size - bad.size and not np.intersect1d(index, bad).size
    boxes, _, kept = _run(directed["nan_codes"])
    assert kept.size and not np.isnan(boxes).any()


def test_width_zero_is_kept_at_min_size_0_and_removed_at_1(directed):
    boxes, _, index = _run(directed["width0_kept"])
    n = directed["width0_kept"][0].size
    assert index.size == n and (boxes[:, 2] - boxes[:, 0] + F(1) == 0).any()
    wide = boxes[:, 2] - boxes[:, 0] + F(1) >= 1                                      # (clipped at the image's left edge: x0 = x1 = 0, width 1)
    boxes1, _, index1 = _run(directed["width0_removed"])
    assert 0 < index1.size < n and np.array_equal(index1, index[wide])


def test_everything_removed_and_pre_above_n(directed):
    boxes, logits, index = _run(directed["all_removed"])
    assert boxes.shape == (0, 4) and logits.size == 0 and index.size == 0
    pb, pl, pi, c = rp.padded((boxes, logits, index), 20)
    assert c == 0 and not pb.any() and not pl.any() and (pi == -1).all()
    obj, reg, anc, img, pre, post, thr, min_size = directed["pre_above_n"]
    assert pre > obj.size
    a = _run(directed["pre_above_n"])
    b = rp.rpn_proposals(obj, reg, anc, img, obj.size, post, thr, min_size)
    assert a[2].size == post and all(np.array_equal(x, y) for x, y in zip(a, b))


def test_the_indexing_is_permute_and_flatten(directed):
    """A = 3, H = 2, W = 5, all values distinct: the stage on [A][H][W] equals decode + suppression on a plainly permuted copy"""
    obj, reg, anc, img, pre, post, thr, min_size = directed["ahw_distinct"]
    A, H, W = obj.shape
    logits = np.zeros(A * H * W, F)
    codes = np.zeros((A * H * W, 4), F)
    for a in range(A):
        for y in range(H):
            for x in range(W):
                i = (y * W + x) * A + a
                logits[i] = obj[a, y, x]
                for c in range(4):
                    codes[i, c] = reg[4 * a + c, y, x]
    order = np.argsort(-logits)[:pre]
    boxes = rp.box_decode(codes[order], anc[order], clip_to=img)
    keep = rp.suppress(boxes, thr, post)
    got = _run(directed["ahw_distinct"])
    assert 0 < keep.size < pre
    assert np.array_equal(got[0], boxes[keep]) and np.array_equal(got[1], logits[order][keep]) and np.array_equal(got[2], order[keep])
