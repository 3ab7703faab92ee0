"""The RPN's proposal stage over all levels of an FPN, in numpy, as include/ifx_c_api.h states it (ifx_rpn_proposals_fpn; k_rpn_fpn_* in csrc/ifx_detector.hip).

maskrcnn-benchmark's RPNPostProcessor.forward for one image, not training (modeling/rpn/inference.py:123-179): forward_for_single_feature_map per level -- that is
rpn_proposals_numpy.rpn_proposals, used here and not repeated -- then select_over_all_levels: the levels concatenated in ascending order, the best
fpn_post_nms_top_n by logit.  The order among equal logits, which torch's topk leaves open, is fixed: by ascending position in the concatenation (level, then row).
Held against the reference's own Python by tests/test_rpn_fpn_cpu.py through tests/golden/rpn_fpn_ref.npz."""
import numpy as np

import rpn_proposals_numpy as rp
from detector_ops_numpy import nms_order

F = np.float32


def per_level(levels, image_size, pre_nms_top_n, post_nms_top_n, nms_thresh, min_size=0, weights=(1, 1, 1, 1)):
    """levels: a list of (objectness [A,H,W], regression [4A,H,W], anchors [H W A,4]) -> per level (boxes [c_l,4], logits [c_l], index [c_l] int64); a level
    without anchors contributes nothing"""
    out = []
    for obj, reg, anc in levels:
        if np.asarray(obj).size == 0:
            out.append((np.zeros((0, 4), F), np.zeros(0, F), np.zeros(0, np.int64)))
        else:
            out.append(rp.rpn_proposals(obj, reg, anc, image_size, pre_nms_top_n, post_nms_top_n, nms_thresh, min_size, weights))
    return out


def key32(logits):
    """the high word of the library's order key (nms_key): ascending key = descending logit, -0 == +0, a NaN behind every number"""
    s = np.asarray(logits, F)
    u = np.where(s == 0, F(0), s).view(np.uint32).astype(np.uint64)
    u = np.where(u & 0x80000000, ~u & 0xFFFFFFFF, u | 0x80000000)
    return np.where(np.isnan(s), np.uint64(0xFFFFFFFF), ~u & 0xFFFFFFFF).astype(np.uint64)


def select_sorted(logit_lists, fpn_post_nms_top_n):
    """the selection as the rule states it: the first min(F, T) positions of the concatenation in nms_order's order -> (level [k], row [k])"""
    counts = [int(np.asarray(l).size) for l in logit_lists]
    T = sum(counts)
    cat = np.concatenate([np.asarray(l, F) for l in logit_lists]) if T else np.zeros(0, F)
    top = nms_order(cat)[:min(int(fpn_post_nms_top_n), T)].astype(np.int64)
    off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    level = np.searchsorted(off, top, side="right") - 1
    return level.astype(np.int32), top - off[level]


def select_ranked(logit_lists, fpn_post_nms_top_n):
    """the selection as the kernel forms it: every list is in the order already, so row r of level l has rank r + sum over the other levels of the number of their
    rows with a smaller 64-bit key (key32 of the logit, position); rank < F writes output row rank -> (level [k], row [k])"""
    counts = [int(np.asarray(l).size) for l in logit_lists]
    T = sum(counts)
    off = np.concatenate([[0], np.cumsum(counts)]).astype(np.uint64)
    keys = [(key32(l) << np.uint64(32)) | (off[i] + np.arange(counts[i], dtype=np.uint64)) for i, l in enumerate(logit_lists)]
    k = min(int(fpn_post_nms_top_n), T)
    level, row, seen = np.full(k, -1, np.int32), np.full(k, -1, np.int64), np.zeros(T, bool)
    for i, mine in enumerate(keys):
        assert (mine[1:] > mine[:-1]).all(), "a level's list is not in the order"
        rank = np.arange(counts[i], dtype=np.int64)
        for j, other in enumerate(keys):
            if j != i:
                rank += np.searchsorted(other, mine, side="left")
        assert not seen[rank].any()
        seen[rank] = True
        w = rank < k
        level[rank[w]], row[rank[w]] = i, np.arange(counts[i], dtype=np.int64)[w]
    assert seen.all()                                       # the ranks are a permutation of 0 .. T - 1
    return level, row


def rpn_proposals_fpn(levels, image_size, pre_nms_top_n, post_nms_top_n, nms_thresh, min_size=0, fpn_post_nms_top_n=None, weights=(1, 1, 1, 1)):
    """-> (boxes [c,4] f32, logits [c] f32, level [c] int32, index [c] int64, level_counts [L] int32): the proposals of one image over all levels, best first"""
    Fn = int(post_nms_top_n if fpn_post_nms_top_n is None else fpn_post_nms_top_n)
    parts = per_level(levels, image_size, pre_nms_top_n, post_nms_top_n, nms_thresh, min_size, weights)
    level, row = select_sorted([p[1] for p in parts], Fn)
    k = level.size
    boxes, logits, index = np.zeros((k, 4), F), np.zeros(k, F), np.zeros(k, np.int64)
    for i in range(k):
        boxes[i], logits[i], index[i] = parts[level[i]][0][row[i]], parts[level[i]][1][row[i]], parts[level[i]][2][row[i]]
    return boxes, logits, level, index, np.asarray([p[1].size for p in parts], np.int32)


def padded(result, fpn_post_nms_top_n):
    """the device's uncut form: zeros and -1 behind the count -> (boxes [F,4], logits [F], level [F], index [F], count, level_counts)"""
    boxes, logits, level, index, level_counts = result
    c, n = boxes.shape[0], int(fpn_post_nms_top_n)
    pb, pl, pv, pi = np.zeros((n, 4), F), np.zeros(n, F), np.full(n, -1, np.int32), np.full(n, -1, np.int64)
    pb[:c], pl[:c], pv[:c], pi[:c] = boxes, logits, level, index
    return pb, pl, pv, pi, c, level_counts
