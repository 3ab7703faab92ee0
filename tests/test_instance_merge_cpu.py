"""The numpy statement of the instance merge (tests/instance_merge_numpy.py) on its own: its packing against the oracle's, chain resolution (the statement's, the
package's), the refusals, and the box rule on hand-made boxes.  No GPU."""
import ctypes as C

import numpy as np
import pytest

import instance_merge_numpy as im
import oracle_lib as orc

OTHER = (-2, -1, 0, 1, 255, 256, 257, 32767, 32768, 65535)


def _oracle_words(a, b):
    L = orc.lib()
    return np.asarray([L.orc_vote_encode(int(x), int(y)) for x, y in zip(a, b)], np.float32)


def _oracle_decode(words):
    L = orc.lib()
    x, y = C.c_int(0), C.c_int(0)
    out = np.zeros((len(words), 2), np.int32)
    for k, f in enumerate(words):
        L.orc_vote_decode(C.c_float(f), C.byref(x), C.byref(y))
        out[k] = x.value, y.value
    return out


@pytest.mark.parametrize("other", OTHER)
def test_packing_equals_the_oracle(other):
    """every half in -2 .. 65535, in either position, beside `other` in the second one"""
    full = np.arange(-2, 65536, dtype=np.int64)
    fixed = np.full_like(full, other)
    for a, b in ((full, fixed), (fixed, full)):
        words = _oracle_words(a, b)
        assert np.array_equal(im.bits(im.encode_word(a, b)), im.bits(words))
        da, db = im.decode_word(words)
        assert np.array_equal(np.stack([da, db], axis=1), _oracle_decode(words))


def test_packing_of_the_words_that_are_no_encoding():
    words = np.asarray([0.0, -1.0, np.nan, np.inf, -np.inf, 2.0 ** 31, -2.0 ** 31, 0.5, -0.5, 1e10, -65536.0], np.float32)
    da, db = im.decode_word(words)
    assert np.array_equal(np.stack([da, db], axis=1), _oracle_decode(words))
    assert (da[0], db[0]) == (0, 0) and (da[1], db[1]) == (-1, -1)
    cnt = im.decode(np.full((2, 48), -1.0, np.float32))
    assert cnt.shape == (2, 96) and (cnt == -1).all()


def test_resolution():
    import instancefusion_amd as ifx

    for fn in (im.resolve, ifx.resolve_merge_pairs):
        assert fn([(5, 3), (3, 1)]).tolist() == [[3, 1], [5, 1]]
        assert fn([(9, 7), (7, 5), (5, 2), (4, 2)]).tolist() == [[4, 2], [5, 2], [7, 2], [9, 2]]
        assert fn([(2, 0)]).tolist() == [[2, 0]] and fn([]).shape == (0, 2)
        assert fn([(2, 0), (2, 0)]).tolist() == [[2, 0]]
        for bad in ([(1, 2), (2, 1)], [(1, 2), (2, 3), (3, 1)], [(4, 1), (1, 2), (2, 1)], [(1, 2), (1, 3)]):
            with pytest.raises(ValueError):
                fn(bad)


def test_refusals_of_the_statement():
    table = np.full(96, -1, np.int32)
    table[:8] = 7
    assert im.refusal([(1, 0), (3, 0), (5, 4)], table) is None
    assert im.refusal([(1, 96)], table) == "range" and im.refusal([(-1, 0)], table) == "range"
    assert im.refusal([(2, 2)], table) == "self"
    assert im.refusal([(8, 0)], table) == "unused" and im.refusal([(0, 8)], table) == "unused"
    assert im.refusal([(1, 0), (1, 2)], table) == "twice"
    assert im.refusal([(3, 1), (5, 3)], table) == "chain"


def test_merge_on_hand_made_words():
    enc = lambda a, b: im.encode_word(a, b)
    v = np.zeros((6, 48), np.float32)
    v[0, 0] = enc(7, 5)                                    # source (instance 1) and target (instance 0) in one word
    v[1, 0] = enc(7, -1)                                   # a negative source: the target stays
    v[2, 0] = -1.0                                         # a first-frame surfel
    v[3, 0] = enc(300, 9)                                  # beyond 2^24: the low half was rounded on the way in
    v[4, 0] = enc(0, 40000)                                # a half above 32 767 reads as negative
    v[5, 0] = enc(32700, 256)                              # (the float's step is 128 up here: 256 survives)
    out = im.merge_votes(v, [(1, 0)])
    cnt = im.decode(out)[:, :2]
    assert cnt[0].tolist() == [12, 0]
    assert cnt[1].tolist() == [6, 0]                                                # (7, -1) reads as (6, -1): the target kept with its borrow, the source cleared
    assert im.bits(out)[2, 0] == im.bits(np.float32(-65536.0))                      # -1.0 -> (-1, -1) -> (-1, 0): what an eviction makes of it
    assert cnt[3, 1] == 0 and cnt[3, 0] == 300 + im.decode_word(v[3, 0])[1]
    assert cnt[4].tolist() == [-1, 0] and cnt[5].tolist() == [32956 - 65536, 0]     # (0, 40 000) reads as (-1, -25 536): nothing to give; 32 700 + 256 wraps the short
    assert np.array_equal(im.bits(out[:, 1:]), im.bits(v[:, 1:]))


def test_box_rule_on_hand_made_boxes():
    table = np.full(96, -1, np.int32)
    boxes = np.tile(np.asarray([101, -1, 53, -1], np.int32), (96, 1))
    table[[0, 1, 2, 3, 4, 5, 6, 7, 8]] = [1, 1, 2, 1, 3, 3, 3, 4, 4]
    boxes[0] = 10, 30, 10, 30
    boxes[1] = 10, 30, 10, 30                              # equal class, equal box: 1 -> 0 (instance 0 may be a target)
    boxes[2] = 10, 30, 10, 30                              # another class
    boxes[3] = 10, 30, 10, 19                              # 9 of 20 rows: I / U = 0.45
    boxes[4] = 40, 60, 10, 30
    boxes[5] = 42, 62, 10, 30                              # 5 against 4: 18 / 22
    boxes[6] = 41, 61, 10, 30                              # 6 against 4 and 5: 19 / 21 both -- the tie goes to 4
    boxes[8] = 70, 90, 10, 30                              # 7 is registered and has no box: never a match
    got = im.duplicates(boxes, table)
    assert got.tolist() == [[1, 0], [5, 4], [6, 4]]
    assert im.box_iou(boxes[4], boxes[6]) == im.box_iou(boxes[5], boxes[6]) == np.float32(np.float32(19 * 20) / np.float32(800 - 380))
    assert im.box_iou(boxes[7], boxes[8]) is None
    boxes[6] = 43, 63, 10, 30                              # now 6 is nearer to 5 (19 / 21) than to 4 (17 / 23): 6 -> 5 -> 4 resolves to 6 -> 4
    assert im.duplicates(boxes, table).tolist() == [[1, 0], [5, 4], [6, 4]]
    assert im.duplicates(boxes, table, 0.85).tolist() == [[1, 0], [6, 5]]
    boxes[3] = 10, 30, 10, 21                              # 11 of 20 rows: 0.55
    assert im.duplicates(boxes, table).tolist()[:2] == [[1, 0], [3, 0]]
    boxes[1] = 10, 10, 10, 30                              # one column wide: empty by the rule
    assert [1, 0] not in im.duplicates(boxes, table).tolist()
