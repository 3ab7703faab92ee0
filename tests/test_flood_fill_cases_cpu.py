"""CPU side of the adversarial flood-fill cases (tests/flood_fill_cases.py): the oracle's maskGeometricFilter against a second, independent restatement -- labels as
the fixpoint of "label = min over the pixels that reach me along source-threshold edges", then the 25 % and 65 % rules in float32 -- on every case up to 68 x 44, and
the conditions the cases are built for, asserted on the oracle's results alone, so that a later change of the builders cannot quietly empty the GPU tests."""
import numpy as np
import pytest

import flood_fill_cases as fc


def _oracle(orc, w, h):
    return orc.Oracle(w=w, h=h, max_surfels=1000, fx=0.8 * w, fy=0.8 * w, cx=w / 2.0, cy=h / 2.0)


@pytest.fixture(scope="module")
def results(orc):
    """name -> (case, masks after the oracle's filter, unavailable after it), computed once: every small case and the two serpentines at 320 x 240."""
    cases = fc.small_cases()
    cases.update(fc.big_cases())
    made, out = {}, {}
    for name, case in cases.items():
        w, h = case[:2]
        if (w, h) not in made:
            made[(w, h)] = _oracle(orc, w, h)
        out[name] = (case,) + made[(w, h)].mask_geometric_filter(*case[2:])
    for o in made.values():
        o.close()
    return out


def restated(depth, masks, ori, unavailable):
    """filterAreaCompute + maskGeometricFilter without a queue: every visited pixel starts with its own row-major index as label and takes the smallest label of a
    4-neighbour q with |depth[q] - depth[p]| < threshold(depth[q]) -- the edge q -> p, the threshold of the SOURCE -- until nothing changes.  A region is the set of
    pixels with one label (the earliest pixel that reaches them); regions in ascending label order are the reference's seeds in scan order."""
    h, w = depth.shape
    d = depth.astype(np.int32)
    thr = fc.threshold(depth)
    big = w * h
    masks, un = masks.copy(), unavailable.copy()
    interior = np.zeros((h, w), bool)
    interior[1:-1, 1:-1] = True
    for m in range(masks.shape[0]):
        if un[m]:
            continue
        v = fc.fill_pixels(depth, masks[m])
        lab = np.where(v, np.arange(big).reshape(h, w), big)
        while True:
            new = lab.copy()
            for me, q in ((np.s_[:, 1:], np.s_[:, :-1]), (np.s_[:, :-1], np.s_[:, 1:]), (np.s_[1:, :], np.s_[:-1, :]), (np.s_[:-1, :], np.s_[1:, :])):
                edge = v[me] & v[q] & (np.abs(d[q] - d[me]).astype(np.float32) < thr[q])
                new[me] = np.where(edge, np.minimum(new[me], lab[q]), new[me])
            if np.array_equal(new, lab):
                break
            lab = new
        ori_points = np.float32((interior & (ori[m] != 0)).sum())
        roots, counts = np.unique(lab[v], return_counts=True)
        with np.errstate(divide="ignore", invalid="ignore"):
            kept = [r for r, c in zip(roots, counts) if np.float32(c) / ori_points > np.float32(0.25)][:20]
            keep = v & np.isin(lab, kept)
            masks[m] = np.where(keep, 255, 0)
            if np.float32(keep.sum()) / ori_points < np.float32(0.65):
                un[m] = 1
    return masks, un


def test_oracle_equals_the_restatement(results):
    """Measured: the two readings agree on every byte of every case up to 68 x 44."""
    checked = 0
    for name, (case, mo, uo) in results.items():
        if case[:2] == fc.BIG:
            continue
        mr, ur = restated(*case[2:])
        assert np.array_equal(uo, ur), (name, np.nonzero(uo != ur)[0][:8].tolist())
        assert np.array_equal(mo, mr), (name, [i for i in range(len(mo)) if not np.array_equal(mo[i], mr[i])][:8])
        checked += 1
    assert checked == len(fc.small_cases())


def _kept(mo):
    return [int((m != 0).sum()) for m in mo]


def test_one_way_edges_where_the_cases_claim_them(results):
    """Every far or one-way case holds, inside a mask, at least one pair of fill pixels joined in one direction only (measured: 119 in the 36 x 36 serpentine, 281 at
    68 x 44, 7592 at 320 x 240; exactly 1 in each one-way tile-border case; 16 per step image; 81 over the 256 masks)."""
    for name, (case, mo, uo) in results.items():
        _, _, depth, masks, _, _ = case
        n = sum(fc.one_way_edges(depth, masks[i]) for i in range(masks.shape[0]))
        if name.startswith("serpentine") or name.startswith("steps") or name.startswith("many_masks") or name.startswith("sequence") or "_to_" in name:
            assert n >= 1, name
        if name.startswith("tile_border") and "_to_" in name:
            assert n == 1, (name, n)
        if name.startswith("tile_border") and "_to_" not in name:
            assert n == 0, (name, n)
    for (w, h) in fc.SIZES:     # the random family: at least one such edge in every image
        for seed in fc.RANDOM_SEEDS:
            case = results[f"random_{w}x{h}_{seed}"][0]
            assert sum(fc.one_way_edges(case[2], case[3][i]) for i in range(8)) >= 1, (w, h, seed)


@pytest.mark.parametrize("w,h", fc.SIZES, ids=lambda v: str(v))
def test_random_family_ends_on_both_sides(results, w, h):
    """Of the 48 masks of a size, at least 20 % end usable with pixels kept and at least 20 % end unusable (measured: 14 and 34 at 36 x 36, 21 and 27 at 68 x 44)."""
    usable = unusable = 0
    for seed in fc.RANDOM_SEEDS:
        _, mo, uo = results[f"random_{w}x{h}_{seed}"]
        usable += sum(1 for i in range(8) if mo[i].any() and not uo[i])
        unusable += int(uo.sum())
    print(w, h, "usable with pixels", usable, "unusable", unusable)
    assert usable >= 10 and unusable >= 10, (usable, unusable)


@pytest.mark.parametrize("w,h", fc.SIZES, ids=lambda v: str(v))
def test_exact_ratios_land_on_their_side(results, w, h):
    _, mo, uo = results[f"ratios_{w}x{h}"]
    for i, name in enumerate(fc.RATIOS):
        assert (_kept(mo)[i], int(uo[i])) == fc.RATIO_EXPECT[name], (name, _kept(mo)[i], int(uo[i]))


@pytest.mark.parametrize("name", ["steps_rows", "steps_columns"])
def test_exact_steps_land_on_their_side(results, name):
    _, expect = fc.steps(name == "steps_columns")
    case, mo, uo = results[name]
    assert case[3].shape[0] == 4 * len(fc.STEPS)
    assert _kept(mo) == expect.tolist(), [(i // 4, i % 4, k, e) for i, (k, e) in enumerate(zip(_kept(mo), expect.tolist())) if k != e]
    assert np.array_equal(uo, expect == 0)
    # the table's own claims, from the threshold function: strict "less than", the threshold of the source
    for a, b, ab, ba in fc.STEPS:
        if b:
            assert (np.float32(abs(a - b)) < fc.threshold(a)) == bool(ab) and (np.float32(abs(a - b)) < fc.threshold(b)) == bool(ba), (a, b)
    assert fc.threshold(5000) == np.float32(124.0) and fc.threshold(3999) == 50 and fc.threshold(9000) == 420 and fc.threshold(65535) == 420


def test_tile_border_cases_split_or_not(results):
    for name, one, case in fc.tile_border():
        _, mo, uo = results[f"tile_border_{name}"]
        total = int((case[3][0] != 0).sum())
        if name == "diagonal":
            assert _kept(mo) == [0] and uo[0] == 1
        else:
            assert total in (189, 190) and _kept(mo) == [total if one else total - 45] and uo[0] == 0, (name, _kept(mo))


def test_serpentines(results):
    """Forward: one region that holds the whole mask, at every size.  Reverse: whole-row regions only (measured: 280 of 594 pixels kept at 36 x 36, 660 of 1406 at
    68 x 44 -- 8 and 10 rows with their connector pixel minus the two-way group at the row's far end...), nothing at 320 x 240 where `ori` is the mask."""
    for (w, h) in fc.SIZES + (fc.BIG,):
        case, mo, uo = results[f"serpentine_{w}x{h}"]
        assert np.array_equal(mo, case[3]) and uo[0] == 0 and int((mo != 0).sum()) == len(fc.serpentine_path(w, h)[0])
        case, mo, uo = results[f"serpentine_reverse_{w}x{h}"]
        kept = int((mo != 0).sum())
        print(w, h, "reverse serpentine keeps", kept, "of", int((case[3] != 0).sum()))
        if (w, h) == fc.BIG:
            assert kept == 0 and uo[0] == 1
        else:
            rows = np.unique(np.nonzero(mo[0])[0])
            assert 0 < kept < int((case[3] != 0).sum()) and uo[0] == 0 and 8 <= len(rows[rows % 2 == 1]) <= 20
    assert len(fc.serpentine_path(*fc.BIG)[0]) == 37960


def test_other_cases_are_what_they_say(results):
    for (w, h) in fc.SIZES:
        s = f"{w}x{h}"
        case, mo, uo = results[f"borders_{s}"]
        assert _kept(mo) == [0, (w - 2) * (h - 2), 2 * 2 * (w - 2) + 2 * 2 * (h - 6), w - 2] and not uo.any()   # (mask 0: 0 / 0 is NaN, not below 0.65)
        assert not mo[:, 0, :].any() and not mo[:, -1, :].any() and not mo[:, :, 0].any() and not mo[:, :, -1].any()
        case, mo, uo = results[f"checkerboard_{s}"]
        assert not mo.any() and uo.all()
        case, mo, uo = results[f"zero_depth_{s}"]
        assert not mo.any() and uo.all()
        case, mo, uo = results[f"all_unavailable_{s}"]
        assert np.array_equal(mo, case[3]) and uo.all() and case[3].any()
    case, mo, uo = results["many_masks_256"]
    assert case[3].shape[0] == 256 and len({m.tobytes() for m in case[3]}) == 256
    assert np.array_equal(case[5], np.arange(256) % 8 == 7) and np.array_equal(mo[case[5] != 0], case[3][case[5] != 0])
    usable = sum(1 for i in range(256) if mo[i].any() and not uo[i])
    print("256 masks: usable with pixels", usable, "unusable", int(uo.sum()))
    assert usable >= 64 and int(uo.sum()) >= 64
    assert [results[f"sequence_{k}"][0][3].shape[0] for k in range(4)] == [3, 256, 1, 40]
