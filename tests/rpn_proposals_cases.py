"""Inputs the proposal-stage tests share (test_rpn_proposals_cpu.py holds the numpy statement to what each case is for, test_gpu_rpn_proposals.py the kernels to the
statement): anchors on a grid, random levels, and the directed cases."""
import numpy as np

F = np.float32


def grid_anchors(A, H, W, stride=16):
    """[H W A, 4], row (y W + x) A + a: A boxes of growing size and alternating aspect ratio around the centre of every cell"""
    a = np.arange(A)
    size = 16.0 + 88.0 * (a + 1) / A
    ratio = np.asarray([0.5, 1.0, 2.0])[a % 3]
    w, h = size / np.sqrt(ratio), size * np.sqrt(ratio)
    base = np.stack([-(w - 1) / 2, -(h - 1) / 2, (w - 1) / 2, (h - 1) / 2], axis=1)
    ys, xs = np.mgrid[0:H, 0:W]
    ctr = np.stack([xs, ys, xs, ys], axis=-1).reshape(H * W, 1, 4) * stride + (stride - 1) / 2
    return (ctr + base[None]).reshape(-1, 4).astype(F)


def level(seed, A, H, W, stride=16, spread=0.5):
    """one random level: (objectness [A,H,W], regression [4A,H,W], anchors, image (width, height) -- not a multiple of the stride)"""
    rng = np.random.default_rng(seed)
    obj = (rng.standard_normal((A, H, W)) * 2).astype(F)
    reg = (rng.standard_normal((4 * A, H, W)) * spread).astype(F)
    r4 = reg.reshape(A, 4, H, W)
    big = rng.random((A, 2, H, W)) < 0.03
    r4[:, 2:][big] = rng.uniform(4.2, 9.0, int(big.sum())).astype(F)              # beyond the clip
    return obj, reg, grid_anchors(A, H, W, stride), (W * stride - 5, H * stride - 3)


def directed():
    """name -> (objectness, regression, anchors, image, pre_nms_top_n, post_nms_top_n, nms_thresh, min_size)"""
    cases = {}
    obj, reg, anc, img = level(1, 3, 6, 7)
    n = obj.size
    cases["all_equal"] = (np.full_like(obj, 0.25), reg, anc, img, 40, 40, 0.7, 0)
    q = np.round(obj).astype(F)                                                     # a handful of values: ties straddle every rank
    cases["ties_straddle"] = (q, reg, anc, img, 37, 37, 2.0, 0)                     # (threshold 2: nothing is suppressed, the selection itself comes out)
    o = np.ascontiguousarray(obj.transpose(1, 2, 0)).reshape(-1)                   # by flat anchor index
    o[::7] = np.nan
    o[3], o[4], o[5], o[6] = np.inf, -np.inf, -0.0, 0.0
    cases["nan_inf_logits"] = (np.ascontiguousarray(o.reshape(6, 7, 3).transpose(2, 0, 1)), reg, anc, img, n - 10, n, 2.0, 0)
    r = reg.copy()
    r.reshape(3, 4, 6, 7)[:, :, 1::2, ::3] = np.nan                                  # NaN codes: their boxes are NaN and fail the size test
    r.reshape(3, 4, 6, 7)[1, 2, 0, 0] = np.nan                                       # one code of a box
    cases["nan_codes"] = (obj, r, anc, img, n, n, 0.7, 0)
    r = reg.copy()
    r.reshape(3, 4, 6, 7)[:, 2] = -200.0                                             # EXP gives 0: width 0
    cases["width0_kept"] = (obj, r, anc, img, n, n, 2.0, 0)
    cases["width0_removed"] = (obj, r, anc, img, n, n, 2.0, 1)
    cases["all_removed"] = (obj, reg, anc, img, 50, 20, 0.7, 1e6)
    cases["pre_above_n"] = (obj, reg, anc, img, 8192, 30, 0.7, 0)
    rng = np.random.default_rng(2)
    A, H, W = 3, 2, 5
    cases["ahw_distinct"] = (rng.permutation(A * H * W).astype(F).reshape(A, H, W), (rng.permutation(4 * A * H * W).astype(F).reshape(4 * A, H, W) - 60) / 100,
                             grid_anchors(A, H, W), (W * 16 - 5, H * 16 - 3), 20, 20, 0.7, 0)
    return cases
