"""The numpy statement of the proposal stage over an FPN (tests/rpn_fpn_numpy.py) against maskrcnn-benchmark's own RPNPostProcessor.forward
(tests/golden/rpn_fpn_ref.npz, written by tools/make_golden_rpn_fpn.py), its per-level part against the single-level statement, and the rank-merge formulation of
the selection -- what the kernel does -- against a sort of the concatenated keys on directed inputs.  No GPU needed.
The rank-merge tests hold one numpy function (rf.select_ranked, written after k_rpn_fpn_merge) to another (rf.select_sorted, the rule): they show that the
formulation is right, not that the kernel follows it -- nothing but reading ties select_ranked to the kernel, whose key packing and searches are held by
tests/test_gpu_rpn_fpn.py alone (ties, NaN logits and empty levels on the device).  In the golden file's case with an empty level the reference itself ran on
the other levels only (it cannot reshape a level of no cells): that such a level contributes nothing is this project's rule, not a figure of the reference."""
import numpy as np

import rpn_fpn_cases as fc
import rpn_fpn_numpy as rf
import rpn_proposals_numpy as rp

F = np.float32


def test_the_statement_has_the_references_proposals():
    """Equal count, equal level and anchor of every row, equal order, every coordinate within 2 ulp of the largest magnitude among pcx, pcy, pw and ph of its box
    (the single-level fixture's bound and unit).  The largest difference seen is the golden file's.  (The case with an empty level: the reference was given
    the levels that have cells; see the module's docstring.)"""
    g = fc.golden()
    cases, quota, empty = (int(v) for v in g["counts"])
    worst, proposals, Ls, As, modes = 0.0, 0, set(), set(), set()
    for k in range(cases):
        levels, image, pre, post, thr, min_size, Fn = fc.golden_case(k)
        ties, at_thr, at_size = g[f"fpn{k}_par"][8:11]
        assert ties == 0 and at_thr == 0 and at_size == 0                              # what the tool stores of the draws it rejects
        assert sum(lv[2].shape[0] for lv in levels) <= 3000
        boxes, logits, level, index, level_counts = fc.statement(f"golden{k}", levels, image, pre, post, thr, min_size, Fn)
        ref = g[f"fpn{k}_boxes"]
        T = int(level_counts.sum())
        assert boxes.shape == ref.shape and boxes.shape[0] == min(Fn, T), k
        assert np.array_equal(level, g[f"fpn{k}_level"]) and np.array_equal(index, g[f"fpn{k}_index"]), k
        assert np.array_equal(level_counts, g[f"fpn{k}_level_counts"])
        with np.errstate(over="ignore"):
            mine = (F(1) / (F(1) + np.exp(-logits.astype(np.float64)))).astype(F)
        assert np.array_equal(mine.argsort(), g[f"fpn{k}_score"].argsort()) and (np.diff(g[f"fpn{k}_score"]) < 0).all()
        for l, (obj, reg, anc) in enumerate(levels):
            w = level == l
            if w.any():
                _, codes = rp.flatten(obj, reg)
                unit = rp.coordinate_ulp(codes[index[w]], anc[index[w]])
                err = float((np.abs(boxes[w].astype(np.float64) - ref[w]) / unit).max())
                assert err <= 2.0, (k, l, err)
                worst = max(worst, err)
        proposals += index.size
        Ls.add(len(levels))
        As.add(levels[0][0].shape[0])
        modes.add(-1 if Fn < T else (0 if Fn == T else 1))
        if k == quota:
            assert level_counts.max() == post and 0 < level_counts.min() < 5
        if k == empty:
            assert levels[1][0].size == 0 and level_counts[1] == 0 and len(levels) == 3 and level_counts[0] > 0 and level_counts[2] > 0
    print(f"{proposals} proposals; largest difference {worst:.3f} of the unit (the tool saw {g['worst_ulp'][0]:.3f}; bound 2)")
    assert Ls == {2, 3, 5, 8} and As == {1, 3} and modes == {-1, 0, 1} and proposals > 500
    assert worst == g["worst_ulp"][0]


def test_the_per_level_part_is_the_single_level_statement():
    """bit for bit: every row of the result is the row of rp.rpn_proposals of its level, and the level's rows appear in that call's order"""
    for k in (0, 6, 10, 13, 23):
        levels, image, pre, post, thr, min_size, _ = fc.golden_case(k)
        boxes, logits, level, index, level_counts = rf.rpn_proposals_fpn(levels, image, pre, post, thr, min_size, 8192)
        for l, (obj, reg, anc) in enumerate(levels):
            w = level == l
            if obj.size == 0:
                assert not w.any() and level_counts[l] == 0
                continue
            b, lg, idx = rp.rpn_proposals(obj, reg, anc, image, pre, post, thr, min_size)
            assert level_counts[l] == idx.size
            assert np.array_equal(index[w], idx) and np.array_equal(boxes[w].view(np.uint32), b.view(np.uint32)) and np.array_equal(logits[w].view(np.uint32), lg.view(np.uint32))


def _both(lists, Fn):
    a, b = rf.select_sorted(lists, Fn), rf.select_ranked(lists, Fn)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]), (lists, Fn)
    return a


def test_rank_merge_equal_logits_go_by_level_then_row():
    lists = [np.asarray([2, 1, 1, 0], F), np.asarray([1, 1], F), np.asarray([3, 1, -5], F)]
    level, row = _both(lists, 9)
    assert level.tolist() == [2, 0, 0, 0, 1, 1, 2, 0, 2] and row.tolist() == [0, 0, 1, 2, 0, 1, 1, 3, 2]
    level, row = _both(lists, 4)                                                        # the cut falls inside the tie: the lowest level, the lowest rows
    assert level.tolist() == [2, 0, 0, 0] and row.tolist() == [0, 0, 1, 2]
    level, row = _both([np.full(5, 0.25, F)] * 3, 7)
    assert level.tolist() == [0] * 5 + [1] * 2 and row.tolist() == [0, 1, 2, 3, 4, 0, 1]


def test_rank_merge_zeros_and_nans():
    lists = [np.asarray([1, -0.0, 0.0, -1], F), np.asarray([0.0, -0.0, -0.5], F)]      # -0 == +0: by position
    level, row = _both(lists, 7)
    assert level.tolist() == [0, 0, 0, 1, 1, 1, 0] and row.tolist() == [0, 1, 2, 0, 1, 2, 3]
    nan = np.nan
    lists = [np.asarray([5, -np.inf], F), np.asarray([np.inf, 1, nan, nan], F), np.asarray([-7, nan], F)]     # a NaN behind every number, -inf included
    level, row = _both(lists, 8)
    assert level.tolist() == [1, 0, 1, 2, 0, 1, 1, 2] and row.tolist() == [0, 0, 1, 0, 1, 2, 3, 1]
    assert _both(lists, 5)[0].tolist() == [1, 0, 1, 2, 0]                                # the cut in front of the NaNs
    assert _both([np.full(3, nan, F), np.full(2, nan, F)], 4)[0].tolist() == [0, 0, 0, 1]


def test_rank_merge_empty_levels_and_the_cut():
    e = np.zeros(0, F)
    lists = [np.asarray([4, 2], F), e, np.asarray([3, 1], F)]
    assert _both(lists, 10)[0].tolist() == [0, 2, 0, 2]                                  # F > T
    assert _both(lists, 4)[1].tolist() == [0, 0, 1, 1]                                   # F == T
    level, row = _both(lists, 1)                                                         # F == 1
    assert level.tolist() == [0] and row.tolist() == [0]
    level, row = _both([e, e, e], 5)                                                     # all levels empty
    assert level.size == 0 and row.size == 0
    assert _both([e, np.asarray([1], F)], 3)[0].tolist() == [1]
    rng = np.random.default_rng(7)
    for trial in range(20):                                                              # random lists of few distinct values, each in the order
        lists = []
        for l in range(int(rng.integers(1, 9))):
            v = rng.integers(-3, 4, int(rng.integers(0, 40))).astype(F)
            v[rng.random(v.size) < 0.1] = np.nan
            lists.append(v[rf.nms_order(v)])
        T = sum(v.size for v in lists)
        for Fn in (1, max(T // 2, 1), max(T, 1), T + 3):
            _both(lists, Fn)


def test_the_padded_form():
    levels, image, pre, post, thr, min_size, Fn = fc.golden_case(2)
    res = fc.statement("golden2", levels, image, pre, post, thr, min_size, Fn)
    pb, pl, pv, pi, c, lc = rf.padded(res, Fn + 5)
    assert c == res[0].shape[0] and pb.shape == (Fn + 5, 4) and not pb[c:].any() and not pl[c:].any() and (pv[c:] == -1).all() and (pi[c:] == -1).all()
    assert np.array_equal(pb[:c], res[0]) and np.array_equal(pv[:c], res[2]) and np.array_equal(lc, res[4])
