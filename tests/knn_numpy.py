"""A plain float64 reference of the kNN colour smoothing (instancefusion_amd/csrc/ifx_knn.hip): brute-force neighbour lists, the rule a float32 search is compared
with, and the vote.  numpy only, n <= 4096.

The comparison rule's band, EPS = 2^-20: with u = 2^-24, the float32 value of (ex*ex + ey*ey) + ez*ez from rounded differences carries a relative error below 5u, so
a float32 search can order two candidates differently from the true distances only where their ratio is within 1 + 10u = 1 + 6e-7; EPS is that with a 1.6 x margin."""
import numpy as np

K = 10
EPS = 2.0 ** -20
IDS = 96   # instance ids 0 .. 95


def sqdist(pos):
    """[n, n] squared distances in float64 from the float32 coordinates"""
    p = np.ascontiguousarray(pos, np.float32).astype(np.float64)
    d = np.zeros((p.shape[0], p.shape[0]), np.float64)
    for k in range(3):
        e = p[:, None, k] - p[None, :, k]
        d += e * e
    return d


def knn_lists(pos, d=None):
    """for every point the indices of its min(n, 10) nearest points, itself included, sorted by (distance, index); -1 behind them"""
    d = sqdist(pos) if d is None else d
    n = d.shape[0]
    assert n <= 4096
    out = np.full((n, K), -1, np.int64)
    k = min(n, K)
    kth = np.partition(d, k - 1, axis=1)[:, k - 1]
    for q in range(n):
        c = np.flatnonzero(d[q] <= kth[q])                     # every candidate up to the k-th distance, ties included, in index order
        out[q, :k] = c[np.argsort(d[q, c], kind="stable")][:k]   # (stable: equal distances stay in index order)
    return out


def knn_check(pos, lists):
    """The neighbour lists of a float32 search against the true distances.  For every query: min(n, 10) distinct valid entries and -1 behind them; every listed point
    within D10 * (1 + EPS) of the query, D10 = the true distance of rank min(n, 10); every unlisted point no closer than the farthest listed one * (1 - EPS); the listed
    distances non-decreasing within (1 - EPS); and candidates whose distances are EQUAL (float32 computes equal distances from equal or mirrored differences) in index
    order, in the list and across its end.  Raises AssertionError; returns (queries whose list equals knn_lists' exactly, queries that differ inside the band)."""
    d = sqdist(pos)
    n = d.shape[0]
    k = min(n, K)
    lists = np.asarray(lists).astype(np.int64)
    assert lists.shape == (n, K), lists.shape
    head, tail = lists[:, :k], lists[:, k:]
    assert (tail == -1).all(), "entries behind the min(n, 10) neighbours"
    assert ((head >= 0) & (head < n)).all(), "an entry that is no point of the cloud"
    assert (np.diff(np.sort(head, axis=1), axis=1) > 0).all(), "a point listed twice"
    rows = np.arange(n)[:, None]
    dl = d[rows, head]                                        # listed distances
    d10 = np.partition(d, k - 1, axis=1)[:, k - 1]
    assert (dl <= d10[:, None] * (1 + EPS)).all(), "a listed point beyond the tenth distance"
    listed = np.zeros((n, n), bool)
    listed[rows, head] = True
    far, last = dl.max(axis=1), head[:, -1]
    dun = np.where(listed, np.inf, d)                         # unlisted distances
    assert (dun >= far[:, None] * (1 - EPS)).all(), "an unlisted point closer than a listed one"
    assert (dl[:, 1:] >= dl[:, :-1] * (1 - EPS)).all(), "listed distances out of order"
    assert (head[:, 1:] > head[:, :-1])[dl[:, 1:] == dl[:, :-1]].all(), "equidistant neighbours not in index order"
    cut = (dun == dl[:, -1:]) & (np.arange(n)[None, :] < last[:, None])
    assert not cut.any(), "an unlisted point as far as the last listed one with a lower index"
    exact = int((lists == knn_lists(pos, d)).all(axis=1).sum())
    return exact, n - exact


def vote_counts(lists, labels):
    """[n, 96]: how many of a point's listed neighbours carry each instance id (labels < 0: unlabelled, ignored)"""
    lists, labels = np.asarray(lists).astype(np.int64), np.asarray(labels).astype(np.int64)
    lab = np.where(lists >= 0, labels[np.maximum(lists, 0)], -1)
    counts = np.zeros((lists.shape[0], IDS), np.int64)
    q, j = np.nonzero(lab >= 0)
    np.add.at(counts, (q, lab[q, j]), 1)
    return counts


def knn_vote(lists, labels):
    """the winning instance per point: the highest count among the labelled neighbours, the lowest id on a tie, -1 where no neighbour is labelled"""
    counts = vote_counts(lists, labels)
    return np.where(counts.max(axis=1) > 0, counts.argmax(axis=1), -1)   # (argmax: the first maximum = the lowest id)
