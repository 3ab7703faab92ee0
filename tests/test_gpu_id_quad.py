"""Option "id_rule" = 1 on the GPU: the reference's screen-space quad rule for the surfel-id renders (ifx_map.hip k_raster_quad).

The stage call (ifx_render_ids, both modes) is held to the f32 numpy restatement of tests/quad_ids_numpy.py -- equal images -- and, through it, to the
reference's executed shaders (tests/golden/gl_ids_scenes.npz, floors of tests/test_id_quad_numpy.py).  The frame path's ids_after is held to the
restatement drawn on the downloaded map at the frame's pose after every segmentation call, and the results (labels, votes, poses, id images) to each
other across the launch forms that draw it: lazy lattice or dense, fused clean + raster walk or not, tiled rasteriser or not, lazy compaction or
compaction every frame."""
import numpy as np
import pytest

from conftest import SMALL
import quad_ids_numpy as Q
from test_id_quad_numpy import FLOORS, load_scenes

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ifx():
    import instancefusion_amd as m

    m.lib()
    return m


def _upload(ifx, e, pc, nr, votes=None):
    n = pc.shape[0]
    m = dict(pc=pc, nr=nr, col=np.zeros((n, 2), np.float32), tm=np.ones((n, 2), np.float32), ic=np.zeros((n, 4), np.float32),
             votes=np.zeros((n, 48), np.float32) if votes is None else votes)
    e.upload(m)


def test_render_ids_quad_rule_equals_restatement(ifx):
    for name, d in load_scenes().items():
        w, h = (int(x) for x in d["size"])
        fx, fy, cx, cy = (float(x) for x in d["K"])
        e = ifx.ElasticFusion(w=w, h=h, fx=fx, fy=fy, cx=cx, cy=cy, confidence=float(d["confidence"]), max_depth_processed=float(d["max_depth"]),
                              max_surfels=1 << 18, id_rule=ifx.ID_RULE_REFERENCE)
        try:
            votes = d.get("votes")
            _upload(ifx, e, d["pc"], d["nr"], votes)
            modes = (0, 1) if votes is not None else (0,)
            for mode in modes:
                got = e.render_ids(d["pose"], mode)
                want = Q.render_ids(d["pc"], d["nr"], d["pose"], d["K"], w, h, float(d["max_depth"]), float(d["confidence"]), votes if mode == 1 else None)
                assert np.array_equal(got, want), (name, mode, int((got != want).sum()))
                if mode == (1 if votes is not None else 0):     # the scene's GL image was drawn with this program
                    gl = d["gl_ids"]
                    eq = float((got == gl).mean() * 100)
                    cov = int(((got > 0) != (gl > 0)).sum())
                    assert eq >= FLOORS[name][0] and cov <= FLOORS[name][1], (name, eq, cov)
        finally:
            e.close()


def test_id_rule_refused_on_sharded_handle(ifx):
    e = ifx.ElasticFusion(**SMALL, max_surfels=100000, n_ranks=-1, rank=0)
    try:
        with pytest.raises(ifx.IfxError, match=r"\(-4\)"):
            e.set_option("id_rule", 1)
    finally:
        e.close()


FORMS = {   # name -> options (every form: id_rule 1)
    "base": dict(lazy_ids=1, clean_raster=1, raster_tiles=0, compact_every_frame=0),
    "dense": dict(lazy_ids=0, clean_raster=1, raster_tiles=0, compact_every_frame=0),
    "no_clean_raster": dict(lazy_ids=1, clean_raster=0, raster_tiles=0, compact_every_frame=0),
    "tiles": dict(lazy_ids=1, clean_raster=1, raster_tiles=1, compact_every_frame=0),
    "compact": dict(lazy_ids=1, clean_raster=1, raster_tiles=0, compact_every_frame=1),
}


def test_frame_path_quad_ids(ifx):
    from instancefusion_amd import synth

    NF = 30
    st = synth.make_stream(NF, SMALL["w"], SMALL["h"], SMALL["fx"], SMALL["fy"], SMALL["cx"], SMALL["cy"], noise=True)
    K = np.array([SMALL["fx"], SMALL["fy"], SMALL["cx"], SMALL["cy"]], np.float32)
    efs, insts = {}, {}
    try:
        for k, opts in FORMS.items():
            e = ifx.ElasticFusion(**SMALL, max_surfels=400000, id_rule=ifx.ID_RULE_REFERENCE)
            for o, v in opts.items():
                e.set_option(o, v)
            efs[k], insts[k] = e, ifx.InstanceFusion(e)
        calls = 0
        for i in range(NF):
            poses = {k: e.processFrame(st["rgb"][i], st["depth"][i]) for k, e in efs.items()}
            for k in efs:
                assert np.array_equal(poses[k], poses["base"]), (i, k)
            if i == 3:      # every surfel stable from here on: the id images are not empty from the first call
                m = efs["base"].download(); m["pc"][:, 3] = 20.0
                for e in efs.values():
                    e.upload(m); e.set_pose(poses["base"], efs["base"].tick)
            if i >= 4 and i % 3 == 1:
                masks, cls = synth.canned_masks(st["obj"][i], st["scene"])
                for k in efs:
                    insts[k].ProcessSegmentation(st["rgb"][i], st["depth"][i], masks, cls, i)
                calls += 1
                ids = {k: e.image("ids_after") for k, e in efs.items()}
                for k in ("dense", "no_clean_raster", "tiles"):      # same slots as the base form
                    assert np.array_equal(ids[k], ids["base"]), (i, k)
                # compaction every frame: the slots are the downloaded map's rows -- the restatement at the frame's pose
                m = efs["compact"].download(("pc", "nr"))
                want = Q.render_ids(m["pc"], m["nr"], efs["compact"].getCurrPose(), K, SMALL["w"], SMALL["h"], 20.0, 10.0)
                assert np.array_equal(ids["compact"], want), (i, int((ids["compact"] != want).sum()))
                assert (want > 0).sum() > 1000
                for k in efs:
                    assert np.array_equal(insts[k].labels(), insts["base"].labels()), (i, k)
                    assert np.array_equal(insts[k].getInstanceTable(), insts["base"].getInstanceTable()), (i, k)
        assert calls >= 8
        ma = efs["base"].download(("pc", "votes"))
        for k, e in efs.items():
            mb = e.download(("pc", "votes"))
            assert np.array_equal(mb["pc"], ma["pc"]) and np.array_equal(mb["votes"], ma["votes"]), k
        assert (insts["base"].labels() >= 0).sum() > 100
    finally:
        for e in efs.values():
            e.close()
