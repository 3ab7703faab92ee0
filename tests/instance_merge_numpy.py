"""Merging duplicate instances (ifx_merge_instances, ifx_instance_duplicates) restated in numpy: the vote packing, the merge pair by pair, the clear, the label scan
and the recolouring that follow, the refusals, the projected boxes of the instances, the box rule between two of them, and the resolution of chains.  Nothing here
calls the library or the oracle; tests/test_instance_merge_cpu.py holds the packing against the oracle's."""
import numpy as np

NI, NW = 96, 48                                           # instances; vote words per surfel: word w holds instance 2w (high half) and 2w + 1 (low half)
DEFAULT_COLOUR = np.float32(7434609)
DEAD_TIME = np.float32(-1.0e9)                            # tm[:, 1] of a tombstone


# ---------------------------------------------------------------------------------------------------------------- the packing
def f2i_rz(f):
    """float32 -> int32 toward zero, saturating, NaN -> 0"""
    f = np.asarray(f, np.float32)
    with np.errstate(invalid="ignore"):
        inside = np.abs(f) < np.float32(2.0 ** 31)        # (false for NaN)
        v = np.where(inside, f, np.float32(0)).astype(np.int32)
        v = np.where(f >= np.float32(2.0 ** 31), np.int32(2 ** 31 - 1), v)
        v = np.where(f <= np.float32(-2.0 ** 31), np.int32(-2 ** 31), v)
    return v.astype(np.int32)


def decode_word(f):
    """one packed word -> (high half, low half), each as a signed short"""
    v = f2i_rz(f)
    return (v >> 16).astype(np.int16).astype(np.int32), v.astype(np.int16).astype(np.int32)


def encode_word(a, b):
    """(short)a in the high half plus (short)b, in wrapping 32-bit arithmetic, converted to float32 (round to nearest even)"""
    sa = np.asarray(a, np.int64).astype(np.int16).astype(np.int64)
    sb = np.asarray(b, np.int64).astype(np.int16).astype(np.int64)
    info = ((sa << 16) + sb + 2 ** 31) % 2 ** 32 - 2 ** 31
    return info.astype(np.int32).astype(np.float32)


def decode(votes):
    """[n, 48] float32 words -> [n, 96] int32 counters"""
    votes = np.ascontiguousarray(votes, np.float32)
    out = np.zeros(votes.shape[:-1] + (2 * votes.shape[-1],), np.int32)
    out[..., 0::2], out[..., 1::2] = decode_word(votes)
    return out


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ---------------------------------------------------------------------------------------------------------------- the pairs
def resolve(pairs):
    """chains resolved to their roots, ascending in from: 5 -> 3, 3 -> 1 becomes 3 -> 1, 5 -> 1.  ValueError: a from with two targets, a cycle."""
    to = {}
    for f, t in np.asarray(pairs, np.int64).reshape(-1, 2).tolist():
        if f in to and to[f] != t:
            raise ValueError(f"instance {f} is merged into two targets")
        to[f] = t
    out = []
    for f in sorted(to):
        seen, t = {f}, to[f]
        while t in to and t != f:
            if t in seen:
                raise ValueError(f"a cycle behind instance {f}")
            seen.add(t)
            t = to[t]
        if t == f and to[f] != f:
            raise ValueError(f"a cycle through instance {f}")
        out.append((f, t))
    return np.asarray(out, np.int32).reshape(-1, 2)


def refusal(pairs, table):
    """why ifx_merge_instances refuses these pairs on this instance table (class per slot, -1 unused), or None"""
    pairs = np.asarray(pairs, np.int64).reshape(-1, 2)
    if len(pairs) > NI - 1:
        return "count"
    froms = []
    for f, t in pairs.tolist():
        if not (0 <= f < NI and 0 <= t < NI):
            return "range"
        if f == t:
            return "self"
        if table[f] == -1 or table[t] == -1:
            return "unused"
        if f in froms:
            return "twice"
        froms.append(f)
    if set(froms) & set(pairs[:, 1].tolist()):
        return "chain"
    return None


# ---------------------------------------------------------------------------------------------------------------- the merge
def merge_votes(votes, pairs):
    """The votes after the merge, [n, 48] float32, bit for bit.  Pair by pair in ascending from, each on the words as the pairs before left them: f = the from-counter
    as decoded; where f > 0 the target's word is decoded, f added to the target's half, clamped at 65535, encoded; elsewhere the word stays as it is.  Then every word
    that holds a from-half is decoded, those halves set to zero, and encoded -- whatever it held."""
    w = bits(votes).copy()
    pairs = sorted(np.asarray(pairs, np.int64).reshape(-1, 2).tolist())
    for f, t in pairs:
        fa, fb = decode_word(w[:, f // 2].view(np.float32))
        give = fb if f & 1 else fa
        ta, tb = decode_word(w[:, t // 2].view(np.float32))
        if t & 1:
            tb = np.minimum(tb + give, 65535)
        else:
            ta = np.minimum(ta + give, 65535)
        w[:, t // 2] = np.where(give > 0, bits(encode_word(ta, tb)), w[:, t // 2])
    for word in sorted({f // 2 for f, _ in pairs}):
        a, b = decode_word(w[:, word].view(np.float32))
        if any(f == 2 * word for f, _ in pairs):
            a = np.zeros_like(a)
        if any(f == 2 * word + 1 for f, _ in pairs):
            b = np.zeros_like(b)
        w[:, word] = bits(encode_word(a, b))
    return w.view(np.float32)


def label_scan(votes, tm, colour, inst_colour):
    """countAndColourSurfelMap over the whole map: (labels, colours).  The first largest counter above zero, -1 without one and for a tombstone; a live surfel without a
    colour (0 or the default) takes its label's."""
    cnt = decode(votes)
    best = np.where(cnt.max(axis=1) > 0, cnt.argmax(axis=1), -1).astype(np.int32)
    live = np.asarray(tm)[:, 1] > DEAD_TIME
    labels = np.where(live, best, -1).astype(np.int32)
    c = np.asarray(colour, np.float32).copy()
    take = live & ((c == 0) | (c == DEFAULT_COLOUR))
    c[take] = np.where(best[take] >= 0, inst_colour[np.maximum(best[take], 0)], DEFAULT_COLOUR)
    return labels, c


def merge(votes, tm, colour, table, inst_colour, pairs):
    """ifx_merge_instances on a map as downloaded: (votes, labels, colours, table) afterwards.  colour: col[:, 1]; inst_colour: [96] float32 table colours."""
    inst_colour = np.asarray(inst_colour, np.float32)
    pairs = np.asarray(pairs, np.int64).reshape(-1, 2)
    out = merge_votes(votes, pairs)
    labels, c = label_scan(out, tm, colour, inst_colour)
    live = np.asarray(tm)[:, 1] > DEAD_TIME
    was = live & np.isin(c, inst_colour[pairs[:, 0]])
    c[was] = np.where(labels[was] >= 0, inst_colour[np.maximum(labels[was], 0)], DEFAULT_COLOUR)
    table = np.asarray(table, np.int32).copy()
    table[pairs[:, 0]] = -1
    return out, labels, c, table


# ---------------------------------------------------------------------------------------------------------------- the duplicates
def project_boxes(ids, votes, w, h):
    """[96, 4] {minX, maxX, minY, maxY} over the pixels whose surfel votes most for the instance (the first largest counter above zero); a surfel whose first counter
    is -1 is "not projected"; an instance nobody shows keeps {w + 1, -1, h + 1, -1}"""
    boxes = np.tile(np.asarray([w + 1, -1, h + 1, -1], np.int32), (NI, 1))
    has = (ids > 0) & (ids < votes.shape[0])
    cnt = decode(votes[np.where(has, ids, 0)])
    best = np.where(has & (cnt[..., 0] != -1) & (cnt.max(axis=-1) > 0), cnt.argmax(axis=-1), -1)
    for i in np.unique(best[best >= 0]):
        ys, xs = np.nonzero(best == i)
        boxes[i] = xs.min(), xs.max(), ys.min(), ys.max()
    return boxes


def box_iou(bi, bm):
    """computeCompareMap's I / U of two boxes in float32, or None where that rule does not get as far (an empty box, no overlap)"""
    minX_i, maxX_i, minY_i, maxY_i = (int(v) for v in bi)
    minX_m, maxX_m, minY_m, maxY_m = (int(v) for v in bm)
    if maxX_i <= minX_i or maxY_i <= minY_i or maxX_m <= minX_m or maxY_m <= minY_m:
        return None
    IW = np.float32(min(maxX_i, maxX_m) - max(minX_i, minX_m))
    IH = np.float32(min(maxY_i, maxY_m) - max(minY_i, minY_m))
    if IW <= 0 or IH <= 0:
        return None
    I = np.float32(IW * IH)
    U = np.float32(np.float32((maxX_i - minX_i) * (maxY_i - minY_i) + (maxX_m - minX_m) * (maxY_m - minY_m)) - I)
    return np.float32(I / U)


def duplicates(boxes, table, thresh=0.5):
    """(from = h, to = root) ascending in from: every registered h takes the registered l < h of its class with the largest I / U above thresh (ties: the lower l)"""
    thresh = np.float32(thresh)
    parent = {}
    for hi in range(NI):
        if table[hi] == -1:
            continue
        best = None
        for lo in range(hi):
            if table[lo] == -1 or table[lo] != table[hi]:
                continue
            iou = box_iou(boxes[lo], boxes[hi])
            if iou is not None and iou > thresh and (best is None or iou > best):
                best, parent[hi] = iou, lo
    return resolve([(hi, lo) for hi, lo in parent.items()])
