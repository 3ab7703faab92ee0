"""The oracle's f-4 readers (orc_map_bounding_boxes, orc_instance_point_cloud) and orc_precision_recall on the hand-built maps of tests/store_readers_cases.py, against
what the construction of each map says: surfels per instance, the precision / recall tables, point-cloud membership, order, truncation and colours from the uploaded
arrays alone; the ground votes of centre normals, the winner of a tie, the seam's `- 1` and the heading rules from the grid restated in store_readers_cases.py.
tests/test_gpu_store_readers_cases.py then holds the HIP library to the oracle on the same uploads."""
import numpy as np
import pytest

import store_readers_cases as sc

UPLOADS = sc.all_uploads()


@pytest.fixture(scope="module")
def sheet(orc):
    o = sc.oracle_sheet(orc)
    yield o
    o.close()


@pytest.fixture(scope="module")
def results(sheet):
    return {up["name"]: sc.run_oracle(sheet, up) for up in UPLOADS}


def test_table_colours_are_the_oracles(sheet):
    """the colours the cases are painted with are the oracle's table: one surfel per colour is counted once per instance, a neighbouring float is not"""
    m = sc.blank(2 * sc.NI, 9)
    m["col"][:sc.NI, 1] = sc.COLOURS
    m["col"][sc.NI:, 1] = sc.COLOURS + np.float32(1.0)
    sheet.upload(m)
    assert len(set(sc.COLOURS.tolist())) == sc.NI and not np.isin(sc.COLOURS + np.float32(1.0), sc.COLOURS).any()
    assert np.array_equal(sheet.precision_recall()[0], np.ones(sc.NI, np.int32))
    assert np.array_equal(sheet.instance_point_cloud(-1)[0], np.ones(sc.NI, np.int32))


def test_centre_normals_vote_for_their_cell_only():
    """the construction's premise, checked where the cases use it: a normal at the centre of a cell of the two equatorial rows votes for that cell alone, with a margin
    (0.03) that no f32 rounding of the cell table (1e-7) reaches"""
    for row in (8, 9):
        for col in range(sc.COLS):
            p = sc.cell(row, col)
            for length in (1.0, 3.0):
                cells, margin = sc.votes_of(sc.normal_of_cell(p, length))
                assert cells.tolist() == [p] and margin > 0.03, (row, col, cells, margin)
    for up in UPLOADS:      # ... and every map's f32 normals keep that margin wherever the construction states the votes
        if up["ground_votes"] is not None:
            for nrm in np.unique(up["m"]["nr"][:, :3], axis=0):
                assert sc.votes_of(nrm)[1] > 0.03, up["name"]


@pytest.mark.parametrize("up", UPLOADS, ids=[u["name"] for u in UPLOADS])
def test_oracle_against_the_construction(results, up):
    sc.compare_with_construction(results[up["name"]], up)


def test_every_slot_one_surfel_boxes_hold_their_surfel(results):
    """case 2: a box is the surfel's own frame coordinate widened to the 1 / ratio lattice on the side the reference's comparison with the WORLD coordinate asks for:
    within two lattice steps of it (the truncation loses up to one, the comparison moves one more), on negative coordinates too"""
    up = next(u for u in UPLOADS if u["name"] == "every_slot_one_surfel")
    out = results[up["name"]]
    owner = sc.instance_of(up["m"]["col"][:, 1])
    for (bt, ratio), (boxes, gn, gc, im, gv) in out["boxes"].items():
        for row, q in enumerate(owner):
            M = np.linalg.inv((gc if bt else im[q]).astype(np.float64))
            g = (M @ np.append(up["m"]["pc"][row, :3].astype(np.float64), 1.0))[:3]
            lo, hi = boxes[q, 0::2].astype(np.float64), boxes[q, 1::2].astype(np.float64)
            step = 1.0 / ratio
            assert (lo <= hi).all() and (hi - lo <= 2.0 * step + 1e-5).all(), (bt, ratio, row)
            assert (np.abs(lo - g) <= 2.0 * step + 1e-5).all() and (np.abs(hi - g) <= 2.0 * step + 1e-5).all(), (bt, ratio, row, lo, hi, g)


def test_seam_and_pole_winners(results):
    """case 3: the winner in the first column reads longitude index -1 (-5 degrees), in the last column 34; at the pole rows the ground normal is the cell centre at
    85 degrees of latitude.  A zero-length normal votes for nothing and leaves NaN in its record only."""
    for up in (u for u in UPLOADS if u["name"].startswith(("seam", "pole"))):
        out = results[up["name"]]
        boxes, gn, gc, im, gv = out["boxes"][True, 1e6]
        assert gv.max() >= 140
        counts, rec = out["clouds"][12, 5, True]
        assert counts[12] == 1 and rec.shape == (1, 10) and rec[0, 0] == 70 and np.isnan(rec[0, 4:7]).all() and np.isfinite(rec[0, 1:4]).all()
        for q in (5, 7, 8, 9):
            assert np.isfinite(out["clouds"][q, 50, True][1]).all()
        assert np.isfinite(im).all() and np.isfinite(gc).all()
    first = results["seam_first_column"]["boxes"][True, 1e6][1]
    assert first[2] < 0 and abs(np.degrees(np.arctan2(first[2], first[0])) + 5.0) < 1e-3              # longitude -5 degrees
    last = results["seam_last_column"]["boxes"][True, 1e6][1]
    assert abs(np.degrees(np.arctan2(last[2], last[0])) % 360.0 - 345.0) < 1e-3                          # column 35 reads 34.5 * 10 degrees
    assert abs(np.degrees(np.arcsin(results["pole_north"]["boxes"][True, 1e6][1][1])) - 85.0) < 1e-3
    assert abs(np.degrees(np.arcsin(results["pole_south"]["boxes"][True, 1e6][1][1])) + 85.0) < 1e-3


def test_ties_go_to_the_lower_index(results):
    """case 4: ground votes 12 : 12, the lower cell wins (asserted with the construction above); instance 3's heading bins 6 : 6, the frame is that of the lower bin;
    instance 4 votes along the ground normal only: heading index 0, the frame of an instance without surfels"""
    gn = sc.centre_of_winner(sc.TIE_LOW)
    bp, mp = sc.heading_bin(gn, sc.HEAD_P)
    bq, mq = sc.heading_bin(gn, sc.HEAD_Q)
    assert bp is not None and bq is not None and bp != bq and min(mp, mq) > 0.1, (bp, mp, bq, mq)
    assert sc.heading_bin(gn, sc.TIE_LOW)[0] is None                        # instance 4's cell lies beyond the 0.525 cosine
    frames = {k: results[k]["boxes"][True, 1e6][3] for k in ("ties", "ties_only_p", "ties_only_q")}
    assert not np.allclose(frames["ties_only_p"][3], frames["ties_only_q"][3], atol=1e-3)
    low = "ties_only_p" if bp < bq else "ties_only_q"
    assert np.array_equal(frames["ties"][3], frames[low][3])
    for k in frames:
        assert np.array_equal(frames[k][4], frames[k][50])                  # instance 50 owns nothing
        gv = results[k]["boxes"][True, 1e6][4]
        assert gv[sc.TIE_HIGH] == gv[sc.TIE_LOW] == 12 == gv.max() and sc.TIE_LOW < sc.TIE_HIGH
