"""The edges of ifx_mask_head_select's rule as inputs, shared by tests/test_mask_head_cpu.py (the numpy statement) and tests/test_gpu_mask_head.py (the kernels)."""
import numpy as np

F = np.float32
IN_SIZE = (801, 607)
OUT_SIZE = (320, 240)
INF = float("inf")


def head(seed, R, C, M, in_size=IN_SIZE):
    """A random mask head: logits [R,C,M,M], boxes [R,4] inside in_size, scores [R] with many exact ties, labels [R] int64 in 0 .. C - 1"""
    rng = np.random.default_rng(seed)
    logits = (rng.standard_normal((R, C, M, M)) * 4.0).astype(F)
    x0 = rng.uniform(0, in_size[0] * 0.8, R); y0 = rng.uniform(0, in_size[1] * 0.8, R)
    boxes = np.stack([x0, y0, x0 + rng.uniform(1, in_size[0] * 0.2, R), y0 + rng.uniform(1, in_size[1] * 0.2, R)], axis=1).astype(F)
    scores = (rng.integers(0, 24, R) / 23.0).astype(F) if R else np.zeros(0, F)      # 24 values: ties from R = 25 on; 16 / 23 < 0.7 < 17 / 23
    labels = rng.integers(0, C, R).astype(np.int64)
    return dict(logits=logits, boxes=boxes, scores=scores, labels=labels, in_size=in_size, out_size=OUT_SIZE, score_thresh=0.7, sort_by_score=True, count=None,
                class_map=None)


def _with(c, **kw):
    d = dict(c)
    d.update(kw)
    return d


def edge_cases(R=64, C=5, M=7, seed=1):
    """[(name, case)]: every edge the rule names, on one head of R rows (R >= 12)"""
    assert R >= 12
    base = head(seed, R, C, M)
    out = [("plain", base), ("no sort", _with(base, sort_by_score=False))]
    for name, cnt in (("count 0", 0), ("count R", R), ("count above R", R + 7), ("count negative", -3), ("count in the middle", R // 2 + 1)):
        out.append((name, _with(base, count=cnt)))
        out.append((name + ", no sort", _with(base, count=cnt, sort_by_score=False)))
    s = base["scores"].copy()
    s[1] = np.nan; s[2] = INF; s[3] = -INF; s[4] = F(0.7); s[5] = np.nextafter(F(0.7), F(1)); s[6] = F(-0.0); s[7] = F(0.0); s[8] = np.nan
    out.append(("NaN, +-inf, score == thresh, +-0", _with(base, scores=s)))
    out.append(("the same, thresh -inf", _with(base, scores=s, score_thresh=-INF)))
    out.append(("the same, thresh -inf, no sort", _with(base, scores=s, score_thresh=-INF, sort_by_score=False)))
    out.append(("the same, thresh 0", _with(base, scores=s, score_thresh=0.0)))
    out.append(("the same, thresh -0", _with(base, scores=s, score_thresh=-0.0)))
    out.append(("thresh +inf: none kept", _with(base, scores=s, score_thresh=INF)))
    lab = base["labels"].copy()
    lab[0] = -1; lab[1] = C; lab[2] = C - 1; lab[3] = 0; lab[4] = 1 << 40; lab[5] = -(1 << 40)
    hi = np.full(R, F(0.9))
    out.append(("labels -1, C, C - 1, 0, +-2^40", _with(base, labels=lab, scores=hi)))
    out.append(("the same, thresh -inf, no sort", _with(base, labels=lab, score_thresh=-INF, sort_by_score=False)))
    out.append(("every row kept", _with(base, scores=hi)))
    out.append(("none kept", _with(base, scores=np.full(R, F(0.1)))))
    x = base["logits"].copy()
    keep = np.nonzero(base["scores"] > F(0.7))[0]
    r0 = int(keep[0]) if len(keep) else 0
    ch = int(base["labels"][r0])
    vals = np.asarray([200, -200, INF, -INF, np.nan, 104, -104, 88.5, -88.5, 89, -89, 90, -90, 103.9, 17, -17, 0.0, -0.0], F)
    x[r0, ch].reshape(-1)[:min(len(vals), M * M)] = vals[:M * M]
    out.append(("logits +-200, +-inf, NaN, EXP's clamps", _with(base, logits=x)))
    cmap = (1000 + 7 * np.arange(C)).astype(np.int32)
    out.append(("class map", _with(base, class_map=cmap)))
    out.append(("class map, no sort, count", _with(base, class_map=cmap, sort_by_score=False, count=R - 3)))
    out.append(("equal ratios", _with(base, in_size=(800, 600))))
    out.append(("out == in", _with(base, out_size=base["in_size"])))
    return out


def many_equal_scores(C=2, M=2):
    """R = 1024 with three score values, all above the threshold but one"""
    c = head(5, 1024, C, M)
    c["scores"] = np.asarray([0.9, 0.8, 0.5], F)[np.random.default_rng(6).integers(0, 3, 1024)]
    return c
