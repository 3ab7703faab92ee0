"""Inputs the box-detection tests share (test_box_detections_cpu.py holds the numpy statement to what each case is for, test_gpu_box_detections.py the kernels to the
statement): random box heads with clustered proposals, heads with a chosen number of candidates, and the head that fills the cap."""
import numpy as np

F = np.float32
WEIGHTS = (10.0, 10.0, 5.0, 5.0)
IMAGE = (333, 217)


def proposals(rng, R, image=IMAGE):
    """[R,4] in clusters, some over the border: boxes of a class suppress each other and some decoded boxes are clipped"""
    clusters = max(1, R // 5)
    ctr = rng.uniform(-0.05, 1.05, (clusters, 2)) * np.asarray(image)
    size = rng.uniform(16, 120, (clusters, 2))
    which = rng.integers(0, clusters, R)
    c = ctr[which] + rng.normal(0, 4, (R, 2))
    s = size[which] * rng.uniform(0.85, 1.15, (R, 2))
    return np.concatenate([c - s / 2, c + s / 2], axis=1).astype(F).reshape(R, 4)


def regression(rng, R, creg, weights=WEIGHTS):
    reg = rng.standard_normal((R, creg, 4)) * 0.25
    reg[..., 2:][rng.random((R, creg, 2)) < 0.05] = 7.0                             # beyond the clip
    return (reg * np.asarray(weights)).reshape(R, 4 * creg).astype(F)


def head(seed, R, C, scale=2.0, creg=None, weights=WEIGHTS):
    """one random box head: (class_logits [R,C], box_regression [R,4 creg], proposals [R,4], image (width, height))"""
    rng = np.random.default_rng(seed)
    logits = (rng.standard_normal((R, C)) * scale).astype(F)
    return logits, regression(rng, R, C if creg is None else creg, weights), proposals(rng, R), IMAGE


def with_k(seed, R, C, K):
    """a head with K candidates at score_thresh 0.05 (at most 12 per row): the background and the chosen (row, class) pairs share a row's probability, the rest is
    e^-12 of it.  The chosen pairs are spread over the rows in turn."""
    rng = np.random.default_rng(seed)
    logits = (rng.standard_normal((R, C)) * 0.05).astype(F)
    if R:
        logits[:, 0] += F(12)
        assert K <= R * min(C - 1, 12)
        per_row = np.full(R, K // R) + (np.arange(R) < K % R)
        for r in np.nonzero(per_row)[0]:
            logits[r, 1 + rng.choice(C - 1, per_row[r], replace=False)] += F(12)
    return logits, regression(rng, R, C), proposals(rng, R), IMAGE


def at_the_cap(R):
    """C = 3, two near-equal foreground probabilities above the threshold in every row: K = 2 R"""
    rng = np.random.default_rng(R)
    logits = np.zeros((R, 3), F)
    logits[:, 1] = F(1)
    logits[:, 2] = F(1) + rng.uniform(0, 1e-3, R).astype(F)
    return logits, regression(rng, R, 3), proposals(rng, R), IMAGE
