"""The float64 kNN reference (tests/knn_numpy.py) on the clouds of tests/knn_clouds.py, no GPU: the comparison rule accepts a float32 brute force on every cloud and
rejects lists that are wrong by one neighbour or by the order of one tie; the vote's limbs on hand-made lists; the scenario floors of the GPU vote test."""
import numpy as np
import pytest

import knn_clouds as kc
import knn_numpy as kn


def f32_lists(pos):
    """the brute force restated in float32 with the kernel's expression, (ex*ex + ey*ey) + ez*ez, sorted by (distance, index)"""
    p = np.ascontiguousarray(pos, np.float32)
    e = [p[:, None, k] - p[None, :, k] for k in range(3)]
    d = (e[0] * e[0] + e[1] * e[1]) + e[2] * e[2]
    assert d.dtype == np.float32
    out = np.full((p.shape[0], kn.K), -1, np.int64)
    k = min(p.shape[0], kn.K)
    out[:, :k] = np.argsort(d, axis=1, kind="stable")[:, :k]
    return out


@pytest.mark.parametrize("name", sorted(kc.EXACT))
def test_rule_accepts_float32_on_exact_clouds(name):
    pos = kc.EXACT[name]()
    assert pos.dtype == np.float32 and kc.is_exact_grid(pos)
    lists = f32_lists(pos)
    assert np.array_equal(lists, kn.knn_lists(pos))           # float32 is exact here: the lists themselves
    assert kn.knn_check(pos, lists) == (pos.shape[0], 0)
    k = min(pos.shape[0], kn.K)
    assert (lists[:, 0] >= 0).all() and (lists[:, k:] == -1).all() and (lists[:, :k] >= 0).all()


def test_rule_accepts_float32_on_inexact_clouds():
    pos = kc.lattice16_cm()
    exact, band = kn.knn_check(pos, f32_lists(pos))
    print(f"lattice16_cm: {exact} exact, {band} in the band")
    assert exact + band == 4096 and band >= 1                 # the band is exercised: float32 does order some near ties otherwise
    pos = kc.uniform3000()
    exact, band = kn.knn_check(pos, f32_lists(pos))
    print(f"uniform3000: {exact} exact, {band} in the band")
    assert exact >= 0.99 * 3000


def test_rule_rejects_the_eleventh_neighbour():
    pos = kc.uniform3000()
    d = kn.sqdist(pos)
    ds = np.sort(d, axis=1)
    q = int(np.argmax(ds[:, 10] / ds[:, 9] < 1.001))          # the query whose 11th neighbour is nearly as close as its 10th, yet far outside the band
    assert 1 + 100 * kn.EPS < ds[q, 10] / ds[q, 9] < 1.001
    lists = kn.knn_lists(pos, d)
    kn.knn_check(pos, lists)
    lists[q, 9] = np.argsort(d[q], kind="stable")[10]
    with pytest.raises(AssertionError):
        kn.knn_check(pos, lists)


def test_rule_rejects_a_tie_in_the_wrong_index_order():
    pos = kc.lattice16()
    d = kn.sqdist(pos)
    good = kn.knn_lists(pos, d)
    q = 77
    assert d[q, good[q, 1]] == d[q, good[q, 2]]
    lists = good.copy()
    lists[q, [1, 2]] = lists[q, [2, 1]]                       # inside the list
    with pytest.raises(AssertionError):
        kn.knn_check(pos, lists)
    ds = np.sort(d, axis=1)
    inner = int(np.argmax(ds[:, 9] == ds[:, 10]))             # a query whose tenth and eleventh neighbours tie
    order = np.argsort(d[inner], kind="stable")
    assert d[inner, order[9]] == d[inner, order[10]]
    lists = good.copy()
    lists[inner, 9] = order[10]                               # across its end: the higher index of a tie in, the lower out
    with pytest.raises(AssertionError):
        kn.knn_check(pos, lists)
    with pytest.raises(AssertionError):                       # and the plain faults: a point twice, an entry behind a short list
        bad = good.copy(); bad[5, 3] = bad[5, 2]
        kn.knn_check(pos, bad)
    p9 = kc.small(9, "space")
    bad = kn.knn_lists(p9); bad[0, 9] = 0
    with pytest.raises(AssertionError):
        kn.knn_check(p9, bad)


def test_vote_limbs():
    lists = np.array([[0, 1, 2, 3, 4, 5, 6, 7, 8, 9],         # 3 x id 95, 3 x id 2, 2 x id 94, 2 unlabelled: the tie goes to the lower id
                      [1, 2, 3, 9, 9, 9, 9, 9, 9, 9],         # unlabelled neighbours do not count: one vote for 95 beats seven times -1
                      [8, 9, -1, -1, -1, -1, -1, -1, -1, -1],  # no labelled neighbour
                      [3, 4, 5, 6, 7, -1, -1, -1, -1, -1],    # a short list: 2 x 2, 2 x 94, 1 x 95
                      [6, 7, 0, 8, 9, -1, -1, -1, -1, -1]])   # the highest id wins when it has the most
    labels = np.array([95, 95, 95, 2, 2, 2, 94, 94, -1, -1])
    assert kn.knn_vote(lists, labels).tolist() == [2, 95, -1, 2, 94]
    c = kn.vote_counts(lists, labels)
    assert c.shape == (5, 96) and c[0, 95] == 3 and c[0, 2] == 3 and c[0, 94] == 2 and c[0].sum() == 8 and c[2].sum() == 0


@pytest.mark.parametrize("name", ["lattice16", "cluster_strays"])
def test_vote_scenario_floors(name):
    """what the GPU vote test needs from its labels, from the reference alone"""
    pos = kc.EXACT[name]()
    lab = kc.planted_labels(pos)
    counts = kn.vote_counts(kn.knn_lists(pos), lab)
    top = np.sort(counts, axis=1)
    ties = int(((top[:, -1] == top[:, -2]) & (top[:, -1] > 0)).sum())
    win = kn.knn_vote(kn.knn_lists(pos), lab)
    print(f"{name}: {ties} count ties, {(win < 0).sum()} queries without a labelled neighbour, {(win >= 94).sum()} winners >= 94")
    assert ties >= 100 and (win < 0).sum() >= 1 and (win >= 94).sum() >= 1
    assert set(np.unique(lab)) == {-1, *kc.VOTE_IDS}
