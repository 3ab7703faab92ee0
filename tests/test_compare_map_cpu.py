"""The mask rule of the compare map on the CPU: the two numpy statements of the rule agree (tests/compare_map_numpy.py), the union identity, the decision's
edge cases on hand-written tables, and the two new entries in header, library and binding."""
import os
import re
import subprocess

import numpy as np
import pytest

import compare_map_numpy as cm

NI = cm.NI
H, W = 16, 24


def _blob(rng, y0, x0, hh, ww):
    a = np.zeros((H, W), bool)
    a[y0:y0 + hh, x0:x0 + ww] = True
    a &= rng.random((H, W)) < 0.8
    a[y0, x0] = True
    return a


def _case(seed):
    """Masks and presence whose blobs touch every border and corner; mixed classes, unused slots."""
    rng = np.random.default_rng(seed)
    corners = [(0, 0), (0, W - 5), (H - 4, 0), (H - 4, W - 5)]
    edges = [(0, 9), (H - 3, 8), (6, 0), (5, W - 4)]
    spots = corners + edges + [(5, 9), (7, 12)]
    masks = np.stack([_blob(rng, y, x, int(rng.integers(3, 5)), int(rng.integers(3, 6))) for (y, x) in spots]).astype(np.uint8) * 255
    masks[0, 0, 0] = masks[1, 0, W - 1] = masks[2, H - 1, 0] = masks[3, H - 1, W - 1] = 255
    masks[-1] = 255 * (rng.random((H, W)) < 0.5)           # a scattered one
    pres = np.zeros((NI, H, W), bool)
    used = [0, 1, 2, 5, 31, 32, 63, 64, 95]
    for k, i in enumerate(used):
        y, x = spots[(k * 3 + seed) % len(spots)]
        pres[i] = _blob(rng, y, x, int(rng.integers(3, 6)), int(rng.integers(3, 7)))
    pres[used[0], 0, 0] = pres[used[1], 0, W - 1] = pres[used[2], H - 1, 0] = pres[used[3], H - 1, W - 1] = True
    pres[7, H - 1, W - 1] = True                          # presence under an unused slot: its class is -1, so it counts nowhere
    inst_cls = np.full(NI, -1, np.int32)
    inst_cls[used] = rng.integers(1, 4, len(used))
    mask_cls = rng.integers(1, 4, len(masks)).astype(np.int32)
    return masks, pres, mask_cls, inst_cls


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_tables_equal_literal_loops(seed):
    masks, pres, mask_cls, inst_cls = _case(seed)
    for blobs in (masks, pres):                             # every border and corner is touched by a mask and by a presence image of a used or unused slot
        any_ = (blobs > 0).any(axis=0)
        assert any_[0].any() and any_[-1].any() and any_[:, 0].any() and any_[:, -1].any()
    anym = (masks > 0).any(axis=0)
    assert anym[0, 0] and anym[0, -1] and anym[-1, 0] and anym[-1, -1]
    I, U, AM, AI = cm.tables(masks, pres, mask_cls, inst_cls)
    Il, Ul = cm.tables_literal(masks, pres, mask_cls, inst_cls)
    assert np.array_equal(I, Il) and np.array_equal(U, Ul)
    assert I.any() and (U > I).any()
    same = (inst_cls[None, :] != -1) & (mask_cls[:, None] == inst_cls[None, :])
    assert np.array_equal(U, np.where(same, AM[:, None] + AI[None, :] - I, 0))       # U == A_M + A_I - I everywhere the classes agree, 0 elsewhere
    assert not I[~same].any() and not U[~same].any()
    assert (~same).any() and same.any()


def _tables(rows):
    """hand-written tables for one mask: {instance: (I, U)}"""
    I, U = np.zeros((1, NI), np.int32), np.zeros((1, NI), np.int32)
    for i, (a, b) in rows.items():
        I[0, i], U[0, i] = a, b
    return I, U


def _decide(rows, classes, mask_class=3, unavailable=None):
    inst_cls = np.full(NI, -1, np.int32)
    for i, c in classes.items():
        inst_cls[i] = c
    I, U = _tables(rows)
    return int(cm.decide(I, U, np.asarray([mask_class], np.int32), inst_cls, unavailable)[0])


def test_decision_edges():
    assert _decide({4: (50, 100)}, {4: 3}) == -1                                      # exactly 0.5 is no match
    assert _decide({4: (60, 100)}, {4: 3}) == 4
    assert _decide({4: (60, 100), 9: (60, 100)}, {4: 3, 9: 3}) == 4                   # equal maxima: the lowest index
    assert _decide({4: (60, 100), 9: (61, 100)}, {4: 3, 9: 3}) == 9
    assert _decide({4: (3, 5), 9: (6, 10)}, {4: 3, 9: 3}) == 4                        # equal as f32 quotients, not only as the same integers
    assert _decide({0: (90, 100), 9: (60, 100)}, {0: 3, 9: 3}) == -1                  # best = instance 0: no match at all, not the runner-up
    assert _decide({0: (60, 100), 9: (90, 100)}, {0: 3, 9: 3}) == 9
    assert _decide({4: (90, 100)}, {4: 2}) == -1                                      # class mismatch
    assert _decide({4: (90, 100)}, {}) == -1                                          # a slot of class -1 ...
    assert _decide({4: (90, 100)}, {}, mask_class=-1) == -1                           # ... even for a mask of class -1
    assert _decide({4: (90, 100)}, {4: 3}, unavailable=np.asarray([1], np.uint8)) == -1
    assert _decide({4: (0, 0)}, {4: 3}) == -1                                         # 0 / 0 matches nothing
    assert _decide({4: (16777217, 33554432)}, {4: 3}) == -1                           # one f32 division of f32 operands: 2^24 + 1 rounds to 2^24, the quotient is 0.5


def test_new_entries_declared_exported_bound():
    import instancefusion_amd as ifx

    src = re.sub(r"/\*.*?\*/", "", open(ifx.HEADER_PATH).read(), flags=re.S)
    declared = set(re.findall(r"\b(ifx_[a-z0-9_]+)\s*\(", src))
    new = {"ifx_mask_compare_map", "ifx_segmentation_matches"}
    assert new <= declared
    assert new <= set(ifx.exported_symbols())
    out = subprocess.check_output(["nm", "-D", "--defined-only", ifx.LIB_PATH]).decode()
    assert new <= set(re.findall(r"\bT (ifx_[a-z0-9_]+)", out))
    assert re.search(r'"compare_map" 1\|2', open(ifx.HEADER_PATH).read())              # the option is in the header's option list
