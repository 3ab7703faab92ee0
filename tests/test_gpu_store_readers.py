"""Whole-store readers on the DEFAULT frame path, with overdue slots and tombstones in place, against the oracle.

The frame path keeps the store lazy: deleted surfels stay as tombstones until a compaction, and while a cached view list is valid a slot outside it meets the clean
pass's age rule only when a scan comes by (ifx_map.hip "View list").  Everything that looks at the whole store must therefore force that scan (ifx_vlist_reap) and
skip tombstones.  One scenario, built once on the oracle: a few frames of the small stream with a low confidence threshold and the instance ground truth on; into the
downloaded map go 350 junk surfels -- unstable, 30 m behind the camera, no votes, no instance colour, one ground-truth id, one common normal in a cell of the vote
grid nothing natural votes for -- as the map's first 100 slots, a block of 150 in the middle and its last 100 slots, their last-seen time set so that their age passes
20 in frame F0 + LATE.  The same arrays go into the oracle and into a HIP handle on its default options; frame F0 runs on both with the pose pinned, one segmentation
call gives both the same instance table, labels and colours (the table lives in the handle, not in the uploaded arrays), and LATE + 1 more pinned frames follow: the
oracle removed the junk in frame F0 + LATE, the HIP store still holds it, unlisted and overdue.  Each reader then runs on a fresh HIP handle as the FIRST whole-store
call after frame F0 + LATE + 1 and must return what the oracle's reader returns on the oracle's map.  (One exception, explained in build_scenario: the oracle keeps its
labels by position as of the last colour pass, so after three more frames they are the call's labels carried with their surfels, and the kNN vote uses those.)

Integers are exact; ground normal, frames, boxes and records keep the tolerances of tests/test_gpu_parity.py::test_bounding_boxes_and_instance_point_clouds.  Slot
numbers (point-cloud records, the free-viewpoint id image) are mapped to ranks among the live slots read through ifx_map_view."""
import numpy as np
import pytest

import instance_merge_numpy as im
import knn_numpy as kn
import store_readers_cases as sc
import viewer_numpy as V
from conftest import SMALL, assert_pose_equal

pytestmark = pytest.mark.gpu

CONF = 1.0                               # a low confidence threshold: most of the six-frame map is stable and the segmentation call finds its masks
NW = 6                                   # warm-up frames on the oracle
LATE = 2                                 # the junk's age passes 20 in frame F0 + LATE, between two scans
N_FIRST, N_MID, N_LAST = 100, 150, 100
N_JUNK = N_FIRST + N_MID + N_LAST
JUNK_GT = 200                            # a ground-truth id no natural surfel carries (asserted)
JUNK_CELL = sc.cell(9, 8)                # the junk's normal votes at the centre of this cell: it faces away from the camera, no natural surfel does (asserted)
MAP_KEYS = ("pc", "nr", "col", "tm", "ic", "votes")
VIEW = (96, 72)                          # the free-viewpoint render: a camera 1 m in front of the junk


@pytest.fixture(scope="module")
def ifx():
    import instancefusion_amd as m

    m.lib()
    return m


def junk_rows(pose, last_time, n):
    """n unstable surfels 30 m BEHIND the camera of `pose` (the recipe of tests/test_gpu_sweep.py::_junk_behind_the_camera) on a 2 cm grid across the optical axis"""
    T = np.asarray(pose, np.float64).reshape(4, 4)
    k = np.arange(n)
    p = T[:3, 3] - 30.0 * T[:3, 2] + np.outer((k % 20 - 9.5) * 0.02, T[:3, 0]) + np.outer((k // 20 - 8.5) * 0.02, T[:3, 1])
    m = dict(pc=np.zeros((n, 4), np.float32), nr=np.zeros((n, 4), np.float32), col=np.zeros((n, 2), np.float32), tm=np.full((n, 2), last_time, np.float32),
             ic=np.zeros((n, 4), np.float32), votes=np.zeros((n, 48), np.float32))
    m["pc"][:, :3], m["pc"][:, 3] = p, 0.25
    m["nr"][:, :3], m["nr"][:, 3] = sc.normal_of_cell(JUNK_CELL), 0.01
    m["ic"][:, 3] = JUNK_GT
    return m


def view_camera(pose):
    """the viewer 31 m behind the frame's camera, looking the same way: the junk grid 1 m ahead, the room 30 m behind it"""
    from instancefusion_amd import viewer_mvp

    T = np.asarray(pose, np.float64).reshape(4, 4).copy()
    T[:3, 3] -= 31.0 * T[:3, 2]
    return viewer_mvp(100.0, 100.0, VIEW[0] / 2.0, VIEW[1] / 2.0, VIEW[0], VIEW[1], 0.1, 100.0, T)


def labels_of(m):
    """countAndColourSurfelMap's label per surfel from its votes: the first largest counter above zero, -1 without one (tests/instance_merge_numpy.py)"""
    return im.label_scan(m["votes"], m["tm"], m["col"][:, 1], sc.COLOURS)[0].astype(np.int32)


def build_scenario(orc, st, verbose=False):
    """the oracle's side, once: the uploaded arrays, the frames to run and what every reader returns on the oracle's map after frame F0 + LATE + 1"""
    from instancefusion_amd import synth

    orc.set_threads(orc.usable_cores())
    o = orc.Oracle(**SMALL, max_surfels=400000, confidence=CONF)
    po = None
    for k in range(NW):
        o.set_instance_gt((st["obj"][k] % 250).astype(np.uint8) if k >= 1 else None)
        po = o.process_frame(st["rgb"][k], st["depth"][k])
    gt = (st["obj"][NW - 1] % 250).astype(np.uint8)
    rgb, depth = st["rgb"][NW - 1], st["depth"][NW - 1]
    m = o.download()
    F0 = o.tick                                               # the time of the first frame after the upload
    n = m["pc"].shape[0]
    assert not (m["ic"][:, 3] == JUNK_GT).any()
    last = F0 + LATE - 21                                     # age 21 (> 20: removed) at the end of frame F0 + LATE
    assert last != -1 and last < 0                            # (-1 alone means "delete me"; a time that is not > 0 never earns the time-window exemption)
    junk = junk_rows(po, last, N_JUNK)
    mid = n // 2
    cut = lambda a, lo, hi: a[lo:hi]
    m2 = {k: np.concatenate([cut(junk[k], 0, N_FIRST), m[k][:mid], cut(junk[k], N_FIRST, N_FIRST + N_MID), m[k][mid:], cut(junk[k], N_FIRST + N_MID, N_JUNK)]).astype(np.float32)
          for k in MAP_KEYS}
    o.upload(m2); o.set_pose(po, F0); o.set_instance_gt(gt)
    masks, cls = synth.canned_masks(st["obj"][NW - 1], st["scene"])
    poses, alive = [], []
    for k in range(LATE + 2):
        poses.append(o.process_frame(rgb, depth, in_pose=po))
        if k == 0:
            o.process_segmentation(rgb, depth, masks, cls, NW - 1)
            assert np.array_equal(o.labels(), labels_of(o.download()))        # the oracle's labels, fresh from its colour pass: the label rule on its votes
        alive.append(int((o.download()["ic"][:, 3] == JUNK_GT).sum()))
    # the scenario bites on the oracle's side: the junk lives through frame F0 + LATE - 1 and is gone, all of it, in frame F0 + LATE
    assert alive == [N_JUNK] * LATE + [0, 0], alive
    mo = o.download()
    # The oracle keeps its labels as the reference keeps bestIDInEachSurfel: by POSITION, as of the last colour pass.  The frames since then removed surfels in front of the
    # labelled ones, so o.labels() now names other surfels; the labels the call gave (asserted above) are carried with their surfels instead: no frame touches a vote.
    e = dict(count=o.count, map=mo, labels=labels_of(mo), table=o.instance_table(), pr=o.precision_recall(), sample=o.sample_graph_model(), project=o.render_project_map())
    e["boxes"] = {bt: o.map_bounding_boxes(bt) for bt in (True, False)}
    e["counts"] = o.instance_point_cloud(-1)[0]
    e["largest"] = int(np.argmax(e["counts"]))
    e["cloud"] = o.instance_point_cloud(e["largest"], True)
    mvp = view_camera(po)
    e["mvp"] = mvp
    e["view_oracle"] = V.render_view(mo, mvp, VIEW[0], VIEW[1], CONF, 4, 1, 0, o.tick, 200)
    e["view_with_junk"] = V.render_view(m2, mvp, VIEW[0], VIEW[1], CONF, 4, 1, 0, o.tick, 200)[1]
    # no case is vacuous
    assert (e["labels"] >= 0).sum() > 100 and (e["counts"] > 0).sum() >= 2 and e["counts"][e["largest"]] > 100
    assert e["sample"].shape[0] >= 3                                                              # several nodes: every rank behind the planted first slots counts
    junk_votes = e["boxes"][True][4][JUNK_CELL]
    assert junk_votes < N_JUNK // 10, junk_votes                                                  # few natural surfels vote for the junk's cell
    assert (e["view_with_junk"] >= 0).sum() > 100 and (e["view_oracle"][1] >= 0).sum() < (e["view_with_junk"] >= 0).sum()     # the camera does look at the junk
    assert e["pr"][1][JUNK_GT] == 0 and e["pr"][1].sum() > 1000 and e["pr"][2].sum() > 0
    # kNN colour smoothing: the oracle's neighbour lists on its map, voted with the carried labels (the oracle's own vote reads the positional array: see above)
    win = kn.knn_vote(o.knn_vote(with_neighbours=True), e["labels"])                              # (last: the call repaints the oracle's map)
    e["knn_col"] = mo["col"].copy()
    e["knn_col"][win >= 0, 1] = sc.COLOURS[win[win >= 0]]
    assert (e["knn_col"][:, 1] != mo["col"][:, 1]).sum() > 100
    if verbose:
        print("F0", F0, "count", e["count"], "labelled", int((e["labels"] >= 0).sum()), "instances", int((e["counts"] > 0).sum()), "largest", e["largest"],
              int(e["counts"][e["largest"]]), "nodes", e["sample"].shape[0], "natural votes in the junk's cell", int(junk_votes),
              "view pixels with / without junk", int((e["view_with_junk"] >= 0).sum()), int((e["view_oracle"][1] >= 0).sum()), "knn repainted",
              int((e["knn_col"][:, 1] != mo["col"][:, 1]).sum()))
    o.close()
    return dict(upload=m2, po=po, F0=F0, gt=gt, rgb=rgb, depth=depth, masks=masks, cls=cls, poses=poses, expect=e)


@pytest.fixture(scope="module")
def scenario(orc, small_stream):
    return build_scenario(orc, small_stream)


def _dev(g, ptr, n):
    import torch

    from instancefusion_amd import sharded

    return torch.as_tensor(sharded._DevWords(ptr, n, "<f4"), device=f"cuda:{g.cfgd['device']}")


def store(g):
    """the six arrays of every slot below the count through ifx_map_view, and the live flags a caller is told to derive (times.y above the tombstone marker)"""
    v = g.map_view()
    n = v.count
    width = dict(pc=4, nr=4, col=2, tm=2, ic=4, votes=48)
    ptrs = dict(pc=v.d_pos_conf, nr=v.d_norm_rad, col=v.d_color, tm=v.d_times, ic=v.d_img_corr, votes=v.d_votes)
    m = {k: _dev(g, ptrs[k], n * width[k]).cpu().numpy().reshape(n, width[k]).copy() for k in MAP_KEYS}
    return m, m["tm"][:, 1] > -1.0e9


def ranks_of(live):
    """slot -> rank among the live slots (exclusive cumulative sum of the live flags); -1 for a tombstone"""
    r = np.cumsum(live) - live
    return np.where(live, r, -1)


# ---- the readers: each takes (handle, instance layer, scenario) and asserts its outputs against the oracle's
def read_labels(g, inst, sn):
    assert np.array_equal(inst.labels(), sn["expect"]["labels"])


def read_knn(g, inst, sn):
    inst.flannKnnVoteSurfelMap()
    m, live = store(g)
    assert np.array_equal(m["col"][live], sn["expect"]["knn_col"])


def _boxes(bt):
    def read(g, inst, sn):
        bg, ng, cg, mg, vg = inst.computeMapBoundingBox(bt)
        bo, no, co, mo, vo = sn["expect"]["boxes"][bt]
        assert np.array_equal(vg, vo) and vo.sum() > 1000, int(np.abs(vg - vo).sum())
        sc.compare_boxes((bg, ng, cg, mg, vg), (bo, no, co, mo, vo), ("bbox_type", bt))
        found = bo[:, 0] < 900
        assert found.sum() >= 2 and (bg[found, 1] > bg[found, 0]).all()
    return read


def read_cloud_counts(g, inst, sn):
    cg, _ = inst.getInstancePointCloud(-1)
    assert np.array_equal(cg, sn["expect"]["counts"])


def read_cloud_largest(g, inst, sn):
    q = sn["expect"]["largest"]
    cg, rg = inst.getInstancePointCloud(q, True)
    co, ro = sn["expect"]["cloud"]
    assert np.array_equal(cg, co) and rg.shape == ro.shape == (co[q], 10)
    m, live = store(g)
    slots = rg[:, 0].astype(np.int64)
    assert live[slots].all() and slots.min() >= N_FIRST                                            # records name SLOTS: live ones, behind the planted first slots
    assert np.array_equal(ranks_of(live)[slots], ro[:, 0].astype(np.int64))                        # ... whose ranks are the oracle's indices, in map order
    assert np.array_equal(rg[:, 7:], ro[:, 7:])
    assert sc.close(rg[:, 1:7], ro[:, 1:7], 2e-5)


def read_precision_recall(g, inst, sn):
    for a, b, name in zip(inst.precision_recall(), sn["expect"]["pr"], ("inst_num", "gt_num", "inst_gt_map")):
        assert np.array_equal(a, b), (name, int(np.abs(a - b).sum()))


def read_sample_graph(g, inst, sn):
    assert np.array_equal(g.sample_graph_model(), sn["expect"]["sample"])


def read_render_project_map(g, inst, sn):
    assert np.array_equal(inst.renderProjectMap(), sn["expect"]["project"])


def read_render_view(g, inst, sn):
    rgba, ids = g.render_view(sn["expect"]["mvp"], VIEW, color_type=4, unstable=True)
    want_rgba, want_ids = sn["expect"]["view_oracle"]
    m, live = store(g)
    hit = ids >= 0
    assert np.array_equal(hit, want_ids >= 0), int((hit != (want_ids >= 0)).sum())                 # nothing of the junk is drawn
    assert live[ids[hit]].all() and np.array_equal(ranks_of(live)[ids[hit]], want_ids[hit])        # slots -> ranks: the oracle's indices
    assert np.array_equal(rgba.view(np.uint32), want_rgba.view(np.uint32))


def read_map_view(g, inst, sn):
    m, live = store(g)
    for k in MAP_KEYS:
        assert m[k][live].shape == sn["expect"]["map"][k].shape, (k, m[k][live].shape, sn["expect"]["map"][k].shape)
        assert np.array_equal(m[k][live], sn["expect"]["map"][k]), k


READERS = {
    "labels": (read_labels, True),
    "knn_vote_colour": (read_knn, True),
    "bounding_boxes_ground_frame": (_boxes(True), True),
    "bounding_boxes_instance_frames": (_boxes(False), True),
    "point_cloud_counts": (read_cloud_counts, True),
    "point_cloud_largest_instance": (read_cloud_largest, True),
    "precision_recall": (read_precision_recall, True),
    "sample_graph_model": (read_sample_graph, True),
    # renderProjectMap reads the store through the frame's id image alone, which never shows an unlisted slot: the one reader here that needs no scan
    "render_project_map": (read_render_project_map, False),
    "render_view": (read_render_view, True),
    "map_view": (read_map_view, True),
}


@pytest.mark.parametrize("reader", list(READERS))
def test_reader_is_the_first_whole_store_call(ifx, scenario, small_stream, reader):
    sn, e = scenario, scenario["expect"]
    read, forces_scan = READERS[reader]
    g = ifx.ElasticFusion(**SMALL, max_surfels=400000, confidence=CONF)                            # default options: no compact_every_frame, no reference_passes
    inst = ifx.InstanceFusion(g)
    g.processFrame(small_stream["rgb"][0], small_stream["depth"][0])
    g.upload(sn["upload"]); g.set_pose(sn["po"], sn["F0"]); g.set_instance_gt(sn["gt"])
    scans0 = None
    for k in range(LATE + 2):
        assert_pose_equal(g.processFrame(sn["rgb"], sn["depth"], inPose=sn["po"]), sn["poses"][k], f"frame F0 + {k}")
        if k == 0:
            inst.ProcessSegmentation(sn["rgb"], sn["depth"], sn["masks"], sn["cls"], NW - 1)
            assert np.array_equal(inst.getInstanceTable(), e["table"])
            scans0 = g.view_list_stats()["scans"]
    # the scenario bites: no scan since frame F0 (the junk, outside the list, has not met the age rule), while the oracle dropped every junk surfel (build_scenario)
    assert g.view_list_stats()["scans"] == scans0, "the view list was rebuilt after frame F0: the scenario does not hold the junk back"
    read(g, inst, sn)
    if forces_scan:
        assert g.view_list_stats()["scans"] > scans0, "the reader did not force the scan"
    slots, count = g.slots, g.count
    assert count == e["count"] and slots >= count + N_JUNK, (slots, count, e["count"])            # holes: the junk's tombstones at least
    g.close()
