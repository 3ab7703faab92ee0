"""Inputs the tests of the proposal stage over an FPN share (test_rpn_fpn_cpu.py, test_gpu_rpn_fpn.py): the golden cases as level lists, pyramids out of
rpn_proposals_cases.level, and the statement's results, computed once per process and never changed."""
import functools
import os

import numpy as np

import rpn_fpn_numpy as rf
import rpn_proposals_cases as rc
from conftest import ROOT

F = np.float32
GOLDEN = os.path.join(ROOT, "tests", "golden", "rpn_fpn_ref.npz")


@functools.lru_cache(maxsize=None)
def golden():
    return dict(np.load(GOLDEN))


def golden_case(k):
    """-> (levels, image, pre, post, thr, min_size, F) of golden case k"""
    g = golden()
    iw, ih, pre, post, thr, min_size, Fn, L = g[f"fpn{k}_par"][:8]
    levels = [(g[f"fpn{k}_l{l}_objectness"], g[f"fpn{k}_l{l}_regression"], g[f"fpn{k}_l{l}_anchors"]) for l in range(int(L))]
    return levels, (int(iw), int(ih)), int(pre), int(post), float(thr), float(min_size), int(Fn)


def pyramid(seed, shapes, stride=16):
    """levels out of rpn_proposals_cases.level, one seed and a doubling stride per level: (levels [(objectness, regression, anchors)], image of level 0).
    A shape with H == 0 or W == 0 gives a level without anchors."""
    levels, image = [], None
    for l, (A, H, W) in enumerate(shapes):
        obj, reg, anc, img = rc.level(seed + l, A, H, W, stride << l)
        levels.append((obj, reg, anc))
        image = image or (img if H * W else None)
    return levels, image or (64, 48)


_memo = {}


def statement(name, levels, image, pre, post, thr, min_size, Fn):
    """rf.rpn_proposals_fpn, computed once per name"""
    if name not in _memo:
        _memo[name] = rf.rpn_proposals_fpn(levels, image, pre, post, thr, min_size, Fn)
        for a in _memo[name]:
            a.setflags(write=False)
    return _memo[name]
