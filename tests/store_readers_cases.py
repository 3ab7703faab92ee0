"""Hand-built labelled maps for the f-4 readers (computeMapBoundingBox, getInstancePointCloud) and computePrecisionAndRecall, numpy only.

A case is a list of uploads; an upload is a dict with the six map arrays (`m`), the reader calls to make on it and what the construction says about the outcome.
Everything that follows from the uploaded arrays alone -- surfels per instance, the three precision / recall tables, which rows a point cloud holds and in which
order, the record colours decoded from col.x -- is computed here; votes, normals, frames and boxes are the oracle's (tests/test_store_readers_cases_cpu.py checks the
oracle against what the construction says about them, tests/test_gpu_store_readers_cases.py the HIP library against the oracle).

Every value that meets a float -> int conversion (col.x, ic.w, a coordinate times `ratio`) is finite and below 2^31 in magnitude: the conversion is defined in C."""
import numpy as np

f32 = np.float32
NI = 96
SEG = 18
CELLS = SEG * SEG * 2
COLS = 2 * SEG
PI = f32(3.1415926)
SCAN_TILE = 256 * 8                     # MAP_THREADS * SCAN_ITEMS of ifx_map.hip: the tile of the exclusive scan behind the point cloud's ranks
DEFAULT_CONF = 20.0
DEFAULT_COLOUR = 7434609.0              # countAndColourSurfelMap's colour of a surfel without a label
W, H = 100, 52                          # the sheet the instance table is registered on (tests/test_gpu_compare_map.py)
K = dict(fx=80.0, fy=80.0, cx=50.0, cy=26.0)
GT_IDS = (-2.0, -1.0, -0.5, 0.0, 0.9, 254.0, 255.0, 255.9, 256.0, 1000.0)


def table_colours():
    """the instance table's colours: a fixed LCG on both sides (ifx_alloc_instance, orc_instance_init), packed r << 16 | g << 8 | b as a float"""
    s, out = 0x1F5, []
    for _ in range(NI):
        c = []
        for _ in range(3):
            s = (s * 1664525 + 1013904223) & 0xFFFFFFFF
            c.append((s >> 8) % 255)
        out.append(float((c[0] << 16) + (c[1] << 8) + c[2]))
    return np.asarray(out, f32)


COLOURS = table_colours()


def reg_rects():
    """eight disjoint 20 x 20 rectangles: the masks that register eight instances per segmentation call"""
    out = np.zeros((8, H, W), np.uint8)
    for k in range(8):
        x0, y0 = 3 + (k % 4) * 24, 3 + (k // 4) * 24
        out[k, y0:y0 + 20, x0:x0 + 20] = 255
    return out


def cls_of(slot):
    return 10 + slot                        # one class per slot: no mask ever matches a registered instance


def sheet_frame():
    rgb = np.random.default_rng(7).integers(30, 255, (H, W, 3)).astype(np.uint8)
    return rgb, np.full((H, W), 1500, np.uint16)


# ------------------------------------------------------------------ the vote grid (testAllSurfelNormalVoteKernel)
def cell_table():
    """centres [648, 3] and radii [648] of the 18 x 36 latitude / longitude cells, f64 (the libraries build theirs in f32 with libm: the cases keep their normals
    far enough from every cell's rim that the difference cannot matter, and votes_of says how far)"""
    pi = float(PI)
    c, r = np.zeros((CELLS, 3)), np.zeros(CELLS)
    p = 0
    for i in range(-SEG // 2, SEG // 2):
        tv, tm = i * pi / SEG, (i + 0.5) * pi / SEG
        for j in range(COLS):
            av, am = j * pi / SEG, (j + 0.5) * pi / SEG
            v = np.array([np.cos(tv) * np.cos(av), np.sin(tv), np.cos(tv) * np.sin(av)])
            m = np.array([np.cos(tm) * np.cos(am), np.sin(tm), np.cos(tm) * np.sin(am)])
            c[p], r[p] = m, np.linalg.norm(v - m)
            p += 1
    return c, r


CENTRES, RADII = cell_table()


def cell(row, col):
    return row * COLS + col


def normal_of_cell(p, length=1.0):
    """the surfel normal that votes at the centre of cell p: the kernel flips y and z ("surfels normal in (Map) is inconsistent with (World)")"""
    c = CENTRES[p]
    return np.array([c[0], -c[1], -c[2]]) * length


def votes_of(normal):
    """(cells the normal votes for, the smallest |distance - radius| over all cells): with a margin far above f32 rounding (1e-4) the vote set is certain"""
    n = np.asarray(normal, np.float64)
    v = np.array([n[0], -n[1], -n[2]]) / np.linalg.norm(n)
    d = np.linalg.norm(CENTRES - v, axis=1)
    return np.nonzero(d < RADII)[0], float(np.abs(d - RADII).min())


def centre_of_winner(p):
    """the ground normal the host code derives from the winning cell p, with its `- 1` on the longitude index (IF/Core/InstanceFusion.cpp:1289-1328)"""
    pi = float(PI)
    i, j = p // COLS - SEG // 2, p % COLS - 1
    th, al = (i + 0.5) * pi / SEG, (j + 0.5) * pi / SEG
    v = np.array([np.cos(th) * np.cos(al), np.sin(th), np.cos(th) * np.sin(al)])
    return v / np.linalg.norm(v)


def heading_bin(ground_normal, p):
    """the heading bin (0..35) cell p votes for around `ground_normal`, or None inside the 0.525 cosine band (setGroundandInstanceCoordinateKernel); with the
    margin between the best and the second-best distance, f64"""
    by = np.asarray(ground_normal, np.float64) / np.linalg.norm(ground_normal)
    tz = centre_of_winner(p)                                  # (the same `- 1` on the longitude index)
    cs = float(by @ tz)
    if abs(cs) > 0.525:
        return None, abs(abs(cs) - 0.525)
    ox = np.cross(by, [0.0, 0.0, -1.0]); ox /= np.linalg.norm(ox)
    step = float(PI) / SEG
    d = []
    for j in range(COLS):
        a = j * step
        rv = np.cos(a) * ox + (1 - np.cos(a)) * (ox @ by) * by + np.sin(a) * np.cross(ox, by)
        d.append(np.linalg.norm(rv / np.linalg.norm(rv) - tz))
    o = np.argsort(d, kind="stable")
    return int(o[0]), float(d[o[1]] - d[o[0]])


# ------------------------------------------------------------------ what the uploaded arrays alone say
def instance_of(col_y):
    """first table colour equal to the surfel's instance colour, -1 for none"""
    eq = np.asarray(col_y, f32)[:, None] == COLOURS[None, :]
    return np.where(eq.any(1), eq.argmax(1), -1)


def trunc_i(x):
    """C's (int)x for finite |x| < 2^31: toward zero"""
    x = np.asarray(x, np.float64)
    assert np.isfinite(x).all() and (np.abs(x) < 2.0 ** 31).all()
    return np.trunc(x).astype(np.int64)


def expected_counts(m):
    inst = instance_of(m["col"][:, 1])
    return np.bincount(inst[inst >= 0], minlength=NI).astype(np.int32)


def expected_pr(m):
    inst, gt = instance_of(m["col"][:, 1]), trunc_i(m["ic"][:, 3])
    ok = (gt >= 0) & (gt < 256)
    a = np.bincount(inst[inst >= 0], minlength=NI).astype(np.int32)
    b = np.bincount(gt[ok], minlength=256).astype(np.int32)
    c = np.zeros((256, NI), np.int32)
    both = ok & (inst >= 0)
    np.add.at(c, (gt[both], inst[both]), 1)
    return a, b, c


def expected_cloud(m, inst, max_records):
    """(rows of the map in the point cloud of `inst`, in map order and cut at max_records; their colours [k, 3] decoded from col.x)"""
    rows = np.nonzero(instance_of(m["col"][:, 1]) == inst)[0][:max_records]
    c = trunc_i(m["col"][rows, 0])
    rgb = np.stack([((c >> s) & 0xFF).astype(f32) / f32(255.0) for s in (16, 8, 0)], 1) if rows.size else np.zeros((0, 3), f32)
    return rows, rgb


# ------------------------------------------------------------------ the maps
def blank(n, seed=0):
    """n stable surfels without an instance colour, positions on both sides of 0 on every axis, normals at the centre of an equatorial cell"""
    rng = np.random.default_rng(seed)
    m = dict(pc=np.zeros((n, 4), f32), nr=np.zeros((n, 4), f32), col=np.zeros((n, 2), f32), tm=np.zeros((n, 2), f32), ic=np.zeros((n, 4), f32), votes=np.zeros((n, 48), f32))
    m["pc"][:, :3] = rng.uniform(-3.0, 3.0, (n, 3))
    m["pc"][:, 3] = DEFAULT_CONF
    m["nr"][:, :3] = normal_of_cell(cell(9, 20))
    m["nr"][:, 3] = 0.01
    m["col"][:, 0] = rng.integers(0, 1 << 24, n) + rng.choice([0.0, 0.25, 0.75], n)      # packed rgb, some with a fraction the conversion drops
    m["tm"][:] = (1.0, 5.0)
    m["ic"][:, 3] = -2.0
    return m


def _set_normals(m, rows, cells, lengths=None):
    for k, (r, p) in enumerate(zip(rows, cells)):
        m["nr"][r, :3] = normal_of_cell(p, 1.0 if lengths is None else lengths[k])


def case_no_table_colour():
    """1. No surfel carries a table colour: 0, the default colour, -1, a fraction, white, and every table colour +- 1 (a float compare, not a nearest match).  Boxes stay
    "not found", all counts are 0, any point cloud is empty; the ground votes are still counted: each normal is the centre of one of twelve equatorial cells."""
    n = 3 * NI + 12
    m = blank(n, 1)
    m["col"][:NI, 1] = COLOURS + f32(1.0)
    m["col"][NI:2 * NI, 1] = COLOURS - f32(1.0)
    m["col"][2 * NI:, 1] = np.resize(np.asarray([0.0, DEFAULT_COLOUR, -1.0, 0.5, 16777215.0], f32), n - 2 * NI)
    assert (instance_of(m["col"][:, 1]) == -1).all()
    cells = [cell(8 + (k % 2), 3 * (k % 12)) for k in range(n)]
    _set_normals(m, range(n), cells)
    gv = np.bincount(cells, minlength=CELLS).astype(np.int32)
    m["ic"][:, 3] = np.resize(np.asarray([3.0, 7.0, -2.0], f32), n)
    return [dict(name="no_table_colour", m=m, ratios=(1e6,), ground_votes=gv, clouds=[(0, 5), (95, 5), (17, 1)], none_found=True)]


def case_every_slot_one_surfel():
    """2. All 96 slots own exactly one surfel (a permutation: map rows 0 and n - 1 included), coordinates on both sides of 0 on every axis -- the toward-zero
    conversion and the reference's comparison of box-frame with WORLD coordinates meet negative values --, some exactly 0 or on the 1 / ratio lattice; ratio 1e6 and 100."""
    m = blank(NI, 2)
    perm = np.random.default_rng(22).permutation(NI)
    m["col"][:, 1] = COLOURS[perm]
    m["pc"][:6, :3] = [[0.0, 0.0, 0.0], [-0.5, 0.25, -1.0], [1.23, -2.34, 0.01], [-0.01, -0.01, -0.01], [2.999, -2.999, 0.005], [-1e-7, 1e-7, -1e-7]]
    cells = [cell(8 + (k % 2), (5 * k) % COLS) for k in range(NI)]
    _set_normals(m, range(NI), cells)
    gv = np.bincount(cells, minlength=CELLS).astype(np.int32)
    m["ic"][:, 3] = (np.arange(NI) % 7).astype(f32)
    assert (expected_counts(m) == 1).all()
    return [dict(name="every_slot_one_surfel", m=m, ratios=(1e6, 100.0), ground_votes=gv, clouds=[(int(perm[0]), 4), (int(perm[-1]), 4), (0, 1)], none_found=False)]


def case_poles_and_seam():
    """3. Normals at the +-y poles and on the longitude seam.  Four uploads: the winning ground cell in the FIRST column of an equatorial row (the host code's `- 1`
    gives longitude index -1), in the LAST column, and at either pole row; in each, instances own normals in columns 0 and 35, at the exact poles (0, -+1, 0), on the
    seam itself (longitude 0: between columns 35 and 0), one zero-length normal (NaN after the normalisation: votes for nothing, NaN in its record) and normals of
    length 3.  A pole normal lies within the radius of every cell of its cap and a seam normal on the rim of two columns: their vote sets are the ORACLE's, not said
    in advance; only the winner cell is asserted from the construction (it holds a majority of centre normals whose vote set is certain)."""
    out = []
    for name, win in (("seam_first_column", cell(9, 0)), ("seam_last_column", cell(9, 35)), ("pole_north", cell(17, 4)), ("pole_south", cell(0, 30))):
        n = 200
        m = blank(n, 3)
        _set_normals(m, range(n), [win] * n)                                  # the majority: the winner
        m["col"][:, 1] = COLOURS[np.arange(n) % 5]                            # instances 0..4 share them
        rows = list(range(10, 60))
        for k, r in enumerate(rows):
            kind = k % 6
            if kind == 0: v = normal_of_cell(cell(8, 0), 3.0)
            elif kind == 1: v = normal_of_cell(cell(9, 35), 3.0)
            elif kind == 2: v = np.array([0.0, -1.0, 0.0])                   # votes at (0, +1, 0): the north pole
            elif kind == 3: v = np.array([0.0, 3.0, 0.0])                    # the south pole, length 3
            elif kind == 4: v = np.array([1.0, 0.0, 0.0])                    # the seam on the equator: a vertex of four cells
            else: v = np.array([np.cos(0.09), -np.sin(0.09), 0.0])           # the seam inside row 9
            m["nr"][r, :3] = v
            m["col"][r, 1] = COLOURS[5 + kind]
        m["nr"][70, :3] = 0.0                                                # the zero-length normal
        m["col"][70, 1] = COLOURS[12]
        up = dict(name=name, m=m, ratios=(1e6,), ground_votes=None, clouds=[(5, 50), (7, 50), (8, 50), (9, 50), (12, 5)], none_found=False)
        if name.startswith("seam"):
            up["winner"] = win
        else:
            up["winner_row"] = win // COLS      # (the centre of a pole-row cell lies inside its neighbours too: which cell of the row wins is the oracle's word)
        out.append(up)
    return out


TIE_LOW, TIE_HIGH = cell(9, 5), cell(9, 20)
HEAD_P, HEAD_Q = cell(9, 14), cell(7, 14)          # two cells a quarter turn from the ground normal of the tie case, on different great circles through it: two heading bins


def case_ties():
    """4. Two cells with equal ground votes: the lower index wins although the higher one comes first in the map.  The same for the 36 heading bins of instance 3
    (upload `ties`: as many votes for HEAD_P as for HEAD_Q; uploads `ties_only_p` / `ties_only_q` hold one of the two, and the tie's frame must be that of the
    lower bin), and instance 4, whose every vote lies along the ground normal -- beyond the 0.525 cosine, so none is counted and its heading index is 0: the frame of an
    instance without surfels."""
    out = []
    for name, kp, kq in (("ties", 6, 6), ("ties_only_p", 6, 0), ("ties_only_q", 0, 6)):
        n = 60
        m = blank(n, 4)
        m["col"][:, 1] = 0.0
        cells = [TIE_HIGH] * 12 + [TIE_LOW] * 7                                # the tie of the ground votes, 12 : 7 + 5, the higher cell first
        own = [-1] * 19
        cells += [HEAD_Q] * kq + [HEAD_P] * kp; own += [3] * (kp + kq)         # instance 3
        cells += [TIE_LOW] * 5; own += [4] * 5                                 # instance 4: along the ground normal (five of the lower cell's twelve)
        rows = range(len(cells))
        _set_normals(m, rows, cells)
        for r, q in zip(rows, own):
            if q >= 0:
                m["col"][r, 1] = COLOURS[q]
        rest = [cell(8, 28 + r % 4) for r in range(len(cells), n)]             # the rest: no instance, four more cells with fewer votes each
        _set_normals(m, range(len(cells), n), rest)
        cells += rest
        gv = np.bincount(cells, minlength=CELLS).astype(np.int32)
        out.append(dict(name=name, m=m, ratios=(1e6,), ground_votes=gv, winner=TIE_LOW, clouds=[(3, 20), (4, 20)], none_found=False))
    return out


def case_scan_edges():
    """5. Point-cloud truncation and the scan's tile border: instance 9 holds SCAN_TILE - 1, SCAN_TILE and SCAN_TILE + 1 surfels on every second row of the map, so its
    surfels lie in tiles 0, 1 and (from SCAN_TILE + 1 on) 2 and its ranks cross both borders; the rows between belong to instance 10 or to none.  max_records 1,
    count - 1 and count: the first max_records records in map order."""
    out = []
    for cnt in (SCAN_TILE - 1, SCAN_TILE, SCAN_TILE + 1):
        n = 2 * cnt + 37
        m = blank(n, 5)
        m["col"][:, 1] = np.where(np.arange(n) % 4 == 1, COLOURS[10], f32(0.0))
        m["col"][0:2 * cnt:2, 1] = COLOURS[9]
        assert expected_counts(m)[9] == cnt
        _set_normals(m, range(0, n, 97), [cell(8, 14)] * len(range(0, n, 97)))
        out.append(dict(name=f"scan_edges_{cnt}", m=m, ratios=(1e6,), ground_votes=None, clouds=[(9, 1), (9, cnt - 1), (9, cnt), (10, 3)], none_found=False))
    return out


def case_gt_ids():
    """6. Ground-truth ids -2, -1, -0.5, 0, 0.9, 254, 255, 255.9, 256, 1000 under three instances and under none: truncation toward zero (-0.5 and 0.9 are id 0, 255.9
    is 255), ids outside 0..255 are not counted."""
    n = 4 * len(GT_IDS) * 3
    m = blank(n, 6)
    m["ic"][:, 3] = np.resize(np.asarray(GT_IDS, f32), n)
    owner = (np.arange(n) // len(GT_IDS)) % 4
    m["col"][:, 1] = np.where(owner == 3, f32(0.0), COLOURS[[0, 41, 95, 0]][owner])
    return [dict(name="gt_ids", m=m, ratios=(1e6,), ground_votes=None, clouds=[(41, 7)], none_found=False)]


def all_uploads():
    out = []
    for f in (case_no_table_colour, case_every_slot_one_surfel, case_poles_and_seam, case_ties, case_scan_edges, case_gt_ids):
        out += f()
    return out


# ------------------------------------------------------------------ running an upload through a handle (the oracle's or the HIP library's) and comparing the two
EYE = np.eye(4, dtype=f32)
TABLE = np.asarray([cls_of(s) for s in range(NI)], np.int32)


def _stable(m):
    m["pc"][:, 3] = 20.0
    m["nr"][:, 3] = 0.3 * 1.5 / K["fx"]
    m["votes"][:] = 0.0


def oracle_sheet(orc):
    """an oracle whose 96 instance slots are registered by rectangle masks on the sheet, eight per segmentation call"""
    rgb, depth = sheet_frame()
    o = orc.Oracle(w=W, h=H, max_surfels=100000, **K)
    for _ in range(3):
        o.process_frame(rgb, depth, in_pose=EYE)
    m = o.download(); _stable(m); o.upload(m); o.set_pose(EYE, o.tick)
    o.process_frame(rgb, depth, in_pose=EYE)
    rects = reg_rects()
    for c in range(0, NI, 8):
        o.process_segmentation(rgb, depth, rects, TABLE[c:c + 8], 10 + c)
    assert np.array_equal(o.instance_table(), TABLE)
    return o


def hip_sheet(ifx):
    """the same on the HIP library: (ElasticFusion, InstanceFusion)"""
    rgb, depth = sheet_frame()
    g = ifx.ElasticFusion(w=W, h=H, max_surfels=100000, **K)
    inst = ifx.InstanceFusion(g)
    for _ in range(3):
        g.processFrame(rgb, depth, inPose=EYE)
    m = g.download(); _stable(m); g.upload(m); g.set_pose(EYE, g.tick)
    g.processFrame(rgb, depth, inPose=EYE)
    rects = reg_rects()
    for c in range(0, NI, 8):
        inst.ProcessSegmentation(None, None, rects, TABLE[c:c + 8], 10 + c)
    assert np.array_equal(inst.getInstanceTable(), TABLE)
    t = inst.getLoopClosureInstanceTable()
    assert np.array_equal(((t[:, 0] << 16) + (t[:, 1] << 8) + t[:, 2]).astype(f32), COLOURS)      # the table colours, read back
    return g, inst


def run_oracle(o, up):
    o.upload(up["m"])
    out = dict(boxes={}, clouds={}, pr=o.precision_recall())
    for bt in (True, False):
        for ratio in up["ratios"]:
            out["boxes"][bt, ratio] = o.map_bounding_boxes(bt, ratio)
        out["counts"] = o.instance_point_cloud(-1, bt)[0]
        for q, mr in up["clouds"]:
            out["clouds"][q, mr, bt] = o.instance_point_cloud(q, bt, mr)
    return out


def run_hip(g, inst, up):
    g.upload(up["m"])
    out = dict(boxes={}, clouds={}, pr=inst.precision_recall())
    for bt in (True, False):
        for ratio in up["ratios"]:
            out["boxes"][bt, ratio] = inst.computeMapBoundingBox(bt, ratio)
        out["counts"] = inst.getInstancePointCloud(-1, bt)[0]
        for q, mr in up["clouds"]:
            out["clouds"][q, mr, bt] = inst.getInstancePointCloud(q, bt, mr)
    return out


def close(a, b, atol):
    """np.allclose at the suite's absolute tolerance and no relative one; a NaN only where the other side has one (the record of a zero-length normal)"""
    return np.allclose(a, b, rtol=0.0, atol=atol, equal_nan=True)


def compare_boxes(got, want, what):
    """computeMapBoundingBox, got against want = (boxes, ground normal, ground frame, instance frames, 648 votes): integers exact, floats at the tolerances of
    tests/test_gpu_parity.py::test_bounding_boxes_and_instance_point_clouds (1e-6, 1e-6, 1e-5; boxes 2e-5)"""
    bg, ng, cg, mg, vg = got
    bo, no, co, mo, vo = want
    assert np.array_equal(vg, vo), (what, "ground votes")
    assert close(ng, no, 1e-6) and close(cg, co, 1e-6) and close(mg, mo, 1e-5), (what, "frames", np.abs(ng - no).max(), np.abs(cg - co).max(), np.nanmax(np.abs(mg - mo)))
    assert np.array_equal(bg[:, 0] < 900, bo[:, 0] < 900), (what, "found")
    assert close(bg, bo, 2e-5), (what, "boxes", np.abs(bg - bo).max())


def compare_cloud(got, want, what):
    """getInstancePointCloud: counts, slots and colours exact, positions and normals at 2e-5"""
    (cg, rg), (co, ro) = got, want
    assert np.array_equal(cg, co), (what, "counts")
    assert rg.shape == ro.shape, (what, rg.shape, ro.shape)
    assert np.array_equal(rg[:, 0], ro[:, 0]) and np.array_equal(rg[:, 7:], ro[:, 7:]), (what, "slots / colours")
    assert close(rg[:, 1:7], ro[:, 1:7], 2e-5), (what, "records")


def compare_with_construction(out, up):
    """what the uploaded arrays alone say, against the outputs of either side"""
    m, what = up["m"], up["name"]
    counts = expected_counts(m)
    assert np.array_equal(out["counts"], counts), (what, "counts")
    for a, b, name in zip(out["pr"], expected_pr(m), ("inst_num", "gt_num", "inst_gt_map")):
        assert np.array_equal(a, b), (what, name)
    for (q, mr, bt), (c, rec) in out["clouds"].items():
        rows, rgb = expected_cloud(m, q, mr)
        assert np.array_equal(c, counts), (what, q, mr, "counts")
        assert rec.shape == (min(int(counts[q]), mr), 10), (what, q, mr, rec.shape)
        assert np.array_equal(rec[:, 0], rows.astype(f32)) and np.array_equal(rec[:, 7:], rgb), (what, q, mr, "membership / order / colours")
    for (bt, ratio), (boxes, gn, gc, im, gv) in out["boxes"].items():
        found = boxes[:, 0] < 900
        assert np.array_equal(found, counts > 0), (what, "found")
        if up["none_found"]:
            assert not found.any() and counts.sum() == 0
            assert np.array_equal(boxes, np.tile(np.asarray([999999999, -999999999], f32), (NI, 3)) / f32(ratio)), what
        if up["ground_votes"] is not None:
            assert np.array_equal(gv, up["ground_votes"]), (what, "ground votes by construction")
        if "winner" in up:
            assert int(np.argmax(gv)) == up["winner"], (what, int(np.argmax(gv)))
            assert close(gn, centre_of_winner(up["winner"]), 1e-6), (what, "ground normal of the winner")
        if "winner_row" in up:
            assert int(np.argmax(gv)) // COLS == up["winner_row"], (what, int(np.argmax(gv)))
            assert close(gn, centre_of_winner(int(np.argmax(gv))), 1e-6), (what, "ground normal of the winner")
