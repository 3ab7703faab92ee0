"""The geometric mask filter on the GPU (ifx_instance.hip: k_ff_prep, _init, _tile_uf, _merge, _flatten, _relax, _count, _select, _apply, _verdict) on the adversarial
cases of tests/flood_fill_cases.py against the CPU oracle: every output mask byte and every `unavailable` byte, as a stage (ifx_mask_geometric_filter, where the
host looks every seven relaxations) and inside a segmentation call (a fixed schedule of relaxations with a device-side gate, and the host-driven resume when the
schedule was too short).  tests/test_flood_fill_cases_cpu.py holds the oracle to a second restatement on the same cases and asserts what the cases are built for.

Launch counts are read with option kernel_timing (ifx_kernel_ms counts the launches of a name).  The option only adds events around the launches of a
segmentation call; it does not change which path the call takes, so counts and comparison come from the same run.

Only ifx_mask_geometric_filter is called on the small handles; no frame is processed on them."""
import ctypes as C

import numpy as np
import pytest

import flood_fill_cases as fc

pytestmark = pytest.mark.gpu

SMALL_CASES = fc.small_cases()
K320 = dict(fx=264.0, fy=264.0, cx=160.0, cy=120.0)


@pytest.fixture(scope="module")
def ifx():
    import instancefusion_amd as m

    m.lib()
    return m


def _camera(w, h):
    return K320 if (w, h) == fc.BIG else dict(fx=0.8 * w, fy=0.8 * w, cx=w / 2.0, cy=h / 2.0)


@pytest.fixture(scope="module")
def handles(ifx, orc):
    """One HIP handle and one oracle per image size, shared by the stage tests of this module (the fill's scratch is reused from call to call, as in a run)."""
    made = {}

    def get(w, h):
        if (w, h) not in made:
            g = ifx.ElasticFusion(w=w, h=h, max_surfels=1000, **_camera(w, h))
            made[(w, h)] = (g, ifx.InstanceFusion(g), orc.Oracle(w=w, h=h, max_surfels=1000, **_camera(w, h)))
        return made[(w, h)]

    yield get
    for g, _, o in made.values():
        g.close(); o.close()


def check_stage(inst, o, case, what):
    w, h, depth, masks, ori, un = case
    mg, ug = inst.maskGeometricFilter(depth, masks, ori, un)
    mo, uo = o.mask_geometric_filter(depth, masks, ori, un)
    assert np.array_equal(ug, uo), (what, "unavailable", np.nonzero(ug != uo)[0][:8].tolist())
    bad = [i for i in range(masks.shape[0]) if not np.array_equal(mg[i], mo[i])]
    assert not bad, (what, "masks", bad[:8], int((mg[bad[0]] != mo[bad[0]]).sum()))
    return mo, uo


# ---------------------------------------------------------------- a. the stage
@pytest.mark.parametrize("name", [n for n in SMALL_CASES if not n.startswith("sequence_")])
def test_stage_equals_oracle(handles, name):
    case = SMALL_CASES[name]
    _, inst, o = handles(*case[:2])
    check_stage(inst, o, case, name)
    check_stage(inst, o, case, name + " again")      # the same handle again: labels, counters and tile flags are rebuilt, not accumulated


def test_stage_sequence_on_one_handle(ifx, orc):
    """n = 3, then 256, then 1, then 40 on a fresh handle: the scratch (labels, counters, per-mask table, skip bytes, tile flags: carved for 256 masks) is
    allocated for 3 masks, grows once, and is then reused with fewer masks than it holds."""
    w, h = 68, 44
    g = ifx.ElasticFusion(w=w, h=h, max_surfels=1000, **_camera(w, h))
    o = orc.Oracle(w=w, h=h, max_surfels=1000, **_camera(w, h))
    inst = ifx.InstanceFusion(g)
    cases = [SMALL_CASES[f"sequence_{k}"] for k in range(4)]
    assert [c[3].shape[0] for c in cases] == [3, 256, 1, 40]
    for k, case in enumerate(cases + cases[::-1]):
        check_stage(inst, o, case, ("sequence", k))
    g.close(); o.close()


def test_stage_limits(handles):
    """n = 257 is refused with IFX_E_INVALID and nothing is touched; n = 0 returns IFX_OK."""
    g, inst, o = handles(68, 44)
    w, h, depth, masks, ori, un = fc.many_masks(257)
    before = masks.copy()
    un = un.copy()
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    assert inst.L.ifx_mask_geometric_filter(g.handle, p(depth), p(masks), p(ori), 257, p(un)) == -1      # IFX_E_INVALID
    assert np.array_equal(masks, before)
    assert inst.L.ifx_mask_geometric_filter(g.handle, p(depth), p(masks), p(ori), 0, p(un)) == 0
    assert inst.L.ifx_mask_geometric_filter(g.handle, p(depth), None, None, 0, None) == 0
    assert np.array_equal(masks, before)
    check_stage(inst, o, SMALL_CASES["many_masks_256"], "256 after the refusal")


@pytest.mark.parametrize("reverse", [False, True])
def test_stage_serpentine_320x240(handles, reverse):
    """The one-pixel corridor through all 80 tiles of a 320 x 240 image, 37 960 pixels in 7 593 two-way components: one label has to travel the whole path.
    The stage's host loop looks after every 7 relaxation launches and gives up after 64 looks (448 launches).  Observed on an MI355X: 21 launches
    forward (three looks), 7 for the mirror image (whole rows at the most: one look).  Forward the count must exceed 7 -- more than one look -- and no upper
    bound is asserted.  Without the pointer jump of k_ff_relax the loop runs into that cap and the result is wrong."""
    g, inst, o = handles(*fc.BIG)
    case = fc.big_cases()["serpentine_reverse_320x240" if reverse else "serpentine_320x240"]
    g.set_option("kernel_timing", 1)
    g.kernel_ms("__reset__")
    try:
        mo, uo = check_stage(inst, o, case, ("serpentine", reverse))
        launches = g.kernel_ms("ff_relax")[1]
    finally:
        g.set_option("kernel_timing", 0)
    print("320x240 serpentine, reverse", reverse, ": ff_relax launches", launches, "(cap 448)")
    if not reverse:
        assert np.array_equal(mo, case[3]) and uo[0] == 0
        assert launches > 7, launches


# ---------------------------------------------------------------- b. inside a segmentation call
LAST_ROW = 229      # the corridor of the call ends there; rows 232 .. 237 hold the second, ordinary mask (masks that overlap are cut by maskCleanOverlap)
BLOCK = (slice(232, 238), slice(100, 120))
CLASSES = np.array([7, 9], np.int32)


def surfel_map(depth):
    """One stable surfel per pixel with a depth, on the ray through the pixel centre at distance (depth + 0.5) / 1186 (the model depth is the distance to the
    camera in those units, truncated), its normal towards the camera, its radius a quarter of a pixel's footprint there: the disc covers no other pixel centre.
    Surfel 0 is never drawn (0 means "empty" in the id image): a spare one behind the camera."""
    ys, xs = np.nonzero(depth)
    ray = np.stack([(xs + 0.5 - K320["cx"]) / K320["fx"], (ys + 0.5 - K320["cy"]) / K320["fy"], np.ones(len(xs))], 1)
    ray /= np.linalg.norm(ray, axis=1, keepdims=True)
    pos = ray * ((depth[ys, xs].astype(np.float64) + 0.5) / 1186.0)[:, None]
    n = len(xs) + 1
    pc = np.zeros((n, 4), np.float32); nr = np.zeros((n, 4), np.float32)
    pc[0] = (0, 0, -5, 20); nr[0] = (0, 0, 1, 0.001)
    pc[1:, :3] = pos; pc[1:, 3] = 20.0
    nr[1:, :3] = -ray; nr[1:, 3] = 0.25 * pos[:, 2] / K320["fx"]
    return dict(pc=pc, nr=nr, col=np.zeros((n, 2), np.float32), tm=np.ones((n, 2), np.float32), ic=np.zeros((n, 4), np.float32), votes=np.zeros((n, 48), np.float32))


@pytest.fixture(scope="module")
def corridor_map():
    w, h = fc.BIG
    _, _, depth, masks, _, _ = fc.serpentine(w, h, last_row=LAST_ROW)
    block = np.zeros((h, w), bool)
    block[BLOCK] = True
    assert not (block & (masks[0] != 0)).any()
    depth[block] = 2372
    return surfel_map(depth), depth, np.stack([masks[0], (block * 255).astype(np.uint8)])


def twins_on_map(ifx, orc, m, depth):
    """A HIP handle and an oracle holding map m, after one frame without depth at the held pose: ids_after is the render of the map (asserted equal, and to be
    exactly the pixels that have a depth, each with a surfel of its own)."""
    w, h = fc.BIG
    g = ifx.ElasticFusion(w=w, h=h, max_surfels=50000, **K320)
    o = orc.Oracle(w=w, h=h, max_surfels=50000, **K320)
    pose = np.eye(4, dtype=np.float32)
    g.upload(m); o.upload(m)
    g.set_pose(pose, 2); o.set_pose(pose, 2)
    g.processFrame(np.zeros((h, w, 3), np.uint8), np.zeros((h, w), np.uint16), inPose=pose)
    o.process_frame(np.zeros((h, w, 3), np.uint8), np.zeros((h, w), np.uint16), in_pose=pose)
    assert g.count == o.count == m["pc"].shape[0]
    ids = o.image("ids_after")
    assert np.array_equal(g.image("ids_after"), ids)
    assert np.array_equal(ids > 0, depth > 0) and len(np.unique(ids[ids > 0])) == m["pc"].shape[0] - 1
    return g, o, ifx.InstanceFusion(g)


def timed_call(g, inst, masks, classes, frame):
    """One ProcessSegmentation under kernel_timing: (ff_relax launches, ff_count launches)."""
    h, w = masks.shape[1:]
    g.set_option("kernel_timing", 1)
    g.kernel_ms("__reset__")
    try:
        inst.ProcessSegmentation(np.zeros((h, w, 3), np.uint8), np.zeros((h, w), np.uint16), masks, classes, frame)
        return g.kernel_ms("ff_relax")[1], g.kernel_ms("ff_count")[1]
    finally:
        g.set_option("kernel_timing", 0)


@pytest.mark.parametrize("ff_rounds", [0, 1, 64])
def test_serpentine_inside_a_call(ifx, orc, corridor_map, ff_rounds):
    """ProcessSegmentation with the corridor (rows 1 .. 229 of the 320 x 240 serpentine: the full one leaves no room for a second mask) and a small block as masks, on
    a map whose render gives exactly the serpentine's depth as model depth.  The call's fixed schedule -- 4 relaxations by default, ff_rounds otherwise -- is too
    short for this mask unless it is 64: the device-side gate then holds the tail back, the host finishes the fill (mask_geometric_filter_device with resume) and
    issues the tail again.  Launch counts of one call:
        ff_rounds   ff_relax        ff_count
        default     more than 4     2           the resume ran, the tail was issued twice
        1           more than 1     2           the same
        64          exactly 64      1           no resume
    Observed on an MI355X: 18 and 2 by default (4 scheduled + two looks of 7), 22 and 2 with a schedule of 1, 64 and 1 with 64."""
    w, h = fc.BIG
    m, depth, masks = corridor_map
    g, o, inst = twins_on_map(ifx, orc, m, depth)
    zero_rgb, zero_depth = np.zeros((h, w, 3), np.uint8), np.zeros((h, w), np.uint16)
    if ff_rounds:
        g.set_option("ff_rounds", ff_rounds)
    relax, count = timed_call(g, inst, masks, CLASSES, 10)
    o.process_segmentation(zero_rgb, zero_depth, masks, CLASSES, 10)
    print("ff_rounds", ff_rounds, ": ff_relax launches", relax, "ff_count launches", count)
    table = o.instance_table()
    assert np.array_equal(inst.getInstanceTable(), table)
    assert np.array_equal(inst.labels(), o.labels())
    assert np.array_equal(g.download()["votes"], o.download()["votes"])
    # the oracle registered both masks (otherwise the comparison is vacuous), and every surfel of the corridor is labelled with the corridor's instance
    slots = [int(np.nonzero(table == c)[0][0]) for c in CLASSES]
    assert (table == CLASSES[0]).sum() == 1 and (table == CLASSES[1]).sum() == 1
    lab = o.labels()
    n_path = int((masks[0] != 0).sum())
    assert (lab == slots[0]).sum() == n_path and (lab == slots[1]).sum() == 120 and lab[0] == -1
    best, target = inst.segmentation_matches()       # nothing was registered before the call: no match, each mask votes for the slot it took
    assert best.tolist() == [-1, -1] and target.tolist() == slots
    if ff_rounds == 64:
        assert (relax, count) == (64, 1)
    else:
        assert relax > (ff_rounds or 4) and count == 2, (relax, count)
    # a second call: the block finds its instance by its box; the corridor took slot 0, which the compare map never matches, and registers once more
    assert slots == [0, 1]
    inst.ProcessSegmentation(zero_rgb, zero_depth, masks, CLASSES, 13)
    o.process_segmentation(zero_rgb, zero_depth, masks, CLASSES, 13)
    assert np.array_equal(inst.getInstanceTable(), o.instance_table()) and o.instance_table()[:3].tolist() == [7, 9, 7]
    assert np.array_equal(inst.labels(), o.labels())
    assert np.array_equal(g.download()["votes"], o.download()["votes"])
    best, target = inst.segmentation_matches()
    assert best.tolist() == [-1, 1] and target.tolist() == [2, 1]
    g.close(); o.close()


@pytest.mark.parametrize("ff_rounds", [0, 1])
def test_two_way_call_needs_no_resume(ifx, orc, ff_rounds):
    """A plane at 2 m under two masks that span several tiles in both directions: every edge is two-way (one threshold below 4000 units), so the union-find start
    -- inside the tiles, then across EVERY tile border, vertical and horizontal -- is already the fixpoint, the first relaxation changes nothing and the gate
    stays clear even with a schedule of one: exactly the scheduled launches, the tail once.  (A union-find that missed a border would leave work to the
    relaxation: right results, but the resume would run.)"""
    w, h = fc.BIG
    depth = np.zeros((h, w), np.uint16)
    depth[10:111, 10:151] = 2372
    masks = np.zeros((2, h, w), np.uint8)
    masks[0, 10:81, 10:101] = 255
    masks[1, 85:111, 20:151] = 255
    g, o, inst = twins_on_map(ifx, orc, surfel_map(depth), depth)
    if ff_rounds:
        g.set_option("ff_rounds", ff_rounds)
    relax, count = timed_call(g, inst, masks, CLASSES, 10)
    o.process_segmentation(np.zeros((h, w, 3), np.uint8), np.zeros((h, w), np.uint16), masks, CLASSES, 10)
    print("two-way call, ff_rounds", ff_rounds, ": ff_relax launches", relax, "ff_count launches", count)
    assert np.array_equal(inst.getInstanceTable(), o.instance_table()) and o.instance_table()[:2].tolist() == CLASSES.tolist()
    assert np.array_equal(inst.labels(), o.labels()) and (o.labels() == 0).sum() == 71 * 91 and (o.labels() == 1).sum() == 26 * 131
    assert np.array_equal(g.download()["votes"], o.download()["votes"])
    assert (relax, count) == (ff_rounds or 4, 1)
    g.close(); o.close()
