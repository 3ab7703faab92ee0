"""The point clouds of the kNN tests (test_knn_numpy_cpu.py, test_gpu_knn_clouds.py): small, seeded, and shaped to break a grid search -- grids that collapse to a plane,
a line or one cell, fewer points than neighbours, lattices where the tenth neighbour is decided by index, negative coordinates, a cluster with far strays.
Every cloud is shuffled with a fixed seed, so index order is unrelated to position.

EXACT clouds have coordinates that are multiples of 1/16 in [-8, 8): differences, squares and sums are exact in float32, so a float32 search must return the
float64 lists themselves.  INEXACT clouds are compared under knn_numpy.knn_check."""
import numpy as np


def _shuffled(p, seed):
    p = np.ascontiguousarray(p, np.float32).reshape(-1, 3)
    return np.ascontiguousarray(p[np.random.RandomState(seed).permutation(p.shape[0])])


def _lattice(side, lo):
    """side^3 points, integer coordinates lo .. lo + side - 1 (float64; the caller scales)"""
    a = np.arange(lo, lo + side, dtype=np.float64)
    return np.stack(np.meshgrid(a, a, a, indexing="ij"), -1).reshape(-1, 3)


def lattice16():
    """16^3, spacing 1/16, the box astride zero: every inner query has 6 + 12 equidistant neighbours, the tenth is decided by index"""
    return _shuffled(_lattice(16, -8) / 16.0, 1)


def lattice16_negative():
    """the same lattice with every sign bit set: coordinates -15/16 .. -0.0, the corner point at (-0.0, -0.0, -0.0)"""
    p = (_lattice(16, -15) / 16.0).astype(np.float32)
    p[p == 0] = np.float32(-0.0)
    assert np.signbit(p).all()
    return _shuffled(p, 2)


def plane64():
    """64 x 64 points, spacing 1/16, one cell in z"""
    a = np.arange(-32, 32, dtype=np.float64) / 16.0
    x, y = np.meshgrid(a, a, indexing="ij")
    return _shuffled(np.stack([x, y, np.full_like(x, 0.25)], -1), 3)


def line2000():
    """2000 points on 256 positions of a line: one cell in y and z, about eight coincident points a position"""
    x = np.random.RandomState(4).randint(-128, 128, 2000) / 16.0
    return _shuffled(np.stack([x, np.full_like(x, -1.5), np.full_like(x, 2.0)], -1), 5)


def coincident300():
    return np.tile(np.array([0.5, -1.25, 3.0], np.float32), (300, 1))


def small(n, shape):
    """n points at distinct multiples of 1/16 in [-8, 8): on a line (x), a plane (x, z) or spread in 3-D"""
    rng = np.random.RandomState(100 + 7 * n + {"line": 0, "plane": 1, "space": 2}[shape])
    p = np.zeros((n, 3), np.float64)
    p[:, 1] = 12                                          # (y = 0.75 where y is not free)
    axes = {"line": (0,), "plane": (0, 2), "space": (0, 1, 2)}[shape]
    for k in axes:
        p[:, k] = rng.permutation(256)[:n] - 128          # (distinct along every free axis: no coincident points)
    return _shuffled(p / 16.0, 6)


def cluster_strays():
    """a 12^3 lattice of spacing 1/16 and five points 7 units away: the strays' lists reach back into the cluster, over a grid that is empty in between"""
    strays = np.array([[7.0, 0.0, 0.0], [7.0625, 0.125, -0.0625], [7.125, -0.25, 0.1875], [7.25, 0.0625, 0.25], [7.375, -0.125, -0.1875]])
    return _shuffled(np.concatenate([_lattice(12, -6) / 16.0, strays]), 7)


def lattice16_cm():
    """16^3 at spacing 0.01f, the coordinates rounded products: near ties everywhere, float32 may order them otherwise than the true distances"""
    p = _lattice(16, -8).astype(np.float32) * np.float32(0.01)
    return _shuffled(p, 8)


def uniform3000():
    """3000 uniform points in a 6 x 3 x 6 box astride zero: no near ties"""
    rng = np.random.RandomState(9)
    return _shuffled((rng.rand(3000, 3) - 0.5) * np.array([6.0, 3.0, 6.0]), 10)


SMALL_NS = (1, 9, 10, 11)
SMALL_SHAPES = ("line", "plane", "space")

EXACT = {"lattice16": lattice16, "lattice16_negative": lattice16_negative, "plane64": plane64, "line2000": line2000, "coincident300": coincident300,
         "cluster_strays": cluster_strays}
EXACT.update({f"n{n}_{s}": (lambda n=n, s=s: small(n, s)) for n in SMALL_NS for s in SMALL_SHAPES})
INEXACT = {"lattice16_cm": lattice16_cm, "uniform3000": uniform3000}


VOTE_IDS = (0, 1, 2, 3, 94, 95)


def planted_labels(p, seed=11):
    """instance ids for the vote tests: drawn from VOTE_IDS, 30 % unlabelled (-1), and the octant x, y, z < 0 wholly unlabelled, so that some queries have no
    labelled neighbour at all"""
    rng = np.random.RandomState(seed)
    lab = np.array(VOTE_IDS, np.int32)[rng.randint(0, len(VOTE_IDS), p.shape[0])]
    lab[rng.rand(p.shape[0]) < 0.3] = -1
    lab[(p < 0).all(axis=1)] = -1
    return lab


def is_exact_grid(p):
    """multiples of 1/16 in [-8, 8)"""
    q = p.astype(np.float64) * 16.0
    return bool((q == np.round(q)).all() and (p >= -8).all() and (p < 8).all())
