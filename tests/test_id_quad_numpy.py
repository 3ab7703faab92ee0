"""The numpy restatement of the reference's id rule (tests/quad_ids_numpy.py, option "id_rule" = 1) against the reference's executed shaders.

tests/golden/gl_ids_scenes.npz (tools/make_golden_gl_ids.py) holds seven id images of surfel_ids.vert / .geom / .frag and instance_surfel_ids.vert run under
llvmpipe on the scene each stores; gl_map_passes.npz holds gl_ids of the map-stage frame.  The floors are the measured agreement less a small margin;
every GENERAL scene is also held to be strictly better than the ray-disc rule (option "id_rule" = 0) was on the same scene in
profiles/r06_gl_agreement_*.txt.  What is left are near-ties at 24-bit depth and pixels where llvmpipe's plane evaluation of texcoord lands on the
other side of dot = 1."""
import os

import numpy as np
import pytest

import quad_ids_numpy as Q

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "gl_ids_scenes.npz")

# scene -> (pixels equal % floor, coverage differences at most); measured: profiles/r07_id_quad_rule.txt
FLOORS = {"frame": (99.80, 0), "frame_vga": (99.98, 3), "s11_nominal": (99.85, 2), "s23_fast": (99.93, 2), "s37_shake": (99.80, 1),
          "s53_spin": (99.90, 1), "frame_instcmp": (99.90, 5)}
# differing pixels of the ray-disc rule on the same scene (profiles/r06_gl_agreement.txt, r06_gl_agreement_other_scenes.txt, r06_gl_agreement_other_sizes.txt;
# frame_vga: that figure is of the whole 640x480 map, of which the scene keeps the middle fifth)
RAY_DISC_DIFFER = {"frame": 189, "frame_vga": 232, "s11_nominal": 150, "s23_fast": 141, "s37_shake": 206, "s53_spin": 126}


def load_scenes():
    g = np.load(GOLD)
    out = {}
    for name in (str(s) for s in g["scenes"]):
        d = {k[len(name) + 2:]: g[k] for k in g.files if k.startswith(name + "__")}
        if "pc" not in d:       # (INSTANCECOMPARE: the map of "frame")
            d["pc"], d["nr"] = g["frame__pc"], g["frame__nr"]
        out[name] = d
    return out


def agreement(mine, gl):
    same = mine == gl
    return float(same.mean() * 100), int((~same).sum()), int(((mine > 0) != (gl > 0)).sum())


@pytest.fixture(scope="module")
def scenes():
    return load_scenes()


def test_quad_rule_against_gl_scenes(scenes, capsys):
    rows = []
    for name, d in scenes.items():
        w, h = (int(x) for x in d["size"])
        mine = Q.render_ids(d["pc"], d["nr"], d["pose"], d["K"], w, h, float(d["max_depth"]), float(d["confidence"]), d.get("votes"))
        eq, differ, cov = agreement(mine, d["gl_ids"])
        rows.append(f"  {name:14s} {w}x{h}  pixels equal {eq:.3f} %  differ {differ:4d}  coverage differs {cov}  (ray-disc: {RAY_DISC_DIFFER.get(name, '-')} differ)")
        assert (d["gl_ids"] > 0).sum() > 1000, name
        assert eq >= 99.8 and eq >= FLOORS[name][0], (name, eq)
        assert cov <= FLOORS[name][1], (name, cov)
        if name in RAY_DISC_DIFFER:
            assert differ < RAY_DISC_DIFFER[name], (name, differ)
    with capsys.disabled():
        print("\nid_rule = 1 (numpy restatement) against the reference's shaders:\n" + "\n".join(rows))


def test_quad_rule_against_map_stage_frame():
    """gl_ids of gl_map_passes.npz, on the post-clean map rebuilt from the file (the GL clean's survivors + its new surfels: not exactly the oracle's map it
    was drawn from, which gl_ids_scenes.npz "frame" now stores)"""
    g = np.load(os.path.join(ROOT, "tests", "golden", "gl_map_passes.npz"))
    k = g["gl_clean_kept"]
    pc = np.concatenate([g["gl_fused_pc"][k], g["gl_clean_new_pc"]])
    nr = np.concatenate([g["gl_fused_nr"][k], g["gl_clean_new_nr"]])
    w, h = int(g["width"]), int(g["height"])
    mine = Q.render_ids(pc, nr, g["pose"], g["K"], w, h, 20.0, float(g["confidence"]))
    eq, differ, cov = agreement(mine, g["gl_ids"])
    assert eq >= 99.8 and cov == 0 and differ < 189, (eq, differ, cov)


def test_lattice_is_the_dense_image_sampled(scenes):
    """step > 1 (the frame's sparse id render) draws exactly the lattice pixels of the dense image"""
    d = scenes["frame"]
    w, h = (int(x) for x in d["size"])
    args = (d["pc"], d["nr"], d["pose"], d["K"], w, h, float(d["max_depth"]), float(d["confidence"]))
    dense, lat = Q.render_ids(*args), Q.render_ids(*args, step=10)
    mask = np.zeros((h, w), bool)
    mask[::10, ::10] = True
    assert np.array_equal(lat[mask], dense[mask]) and not lat[~mask].any()
