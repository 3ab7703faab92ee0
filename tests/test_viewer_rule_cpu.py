"""The viewer's rule (tests/viewer_numpy.py) against the reference's own shaders, executed: tests/golden/gl_viewer_scenes.npz holds what
draw_global_surface.* and draw_global_ID.* drew on Mesa's software rasteriser (tools/make_golden_gl_viewer.py), profiles/r28_viewer_rule_vs_gl.txt
what the generator measured when it wrote the fixture."""
import json
import os

import numpy as np
import pytest

import viewer_numpy as V

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "gl_viewer_scenes.npz")
REPORT = os.path.join(ROOT, "profiles", "r28_viewer_rule_vs_gl.txt")
COVERAGE_CAP = 0.005      # a condition, not a measurement: no scene may differ from GL in coverage on more than 0.5 % of its pixels
COLOUR_FACTOR = 4.0       # colour on pixels with equal id: within four times the largest difference the generator measured (other llvmpipe builds)


def generator_report():
    rep = {}
    with open(REPORT) as f:
        for line in f:
            if line.startswith("#") or not line.strip():
                continue
            name, js = line.split(" ", 1)
            rep[name] = json.loads(js)
    return rep


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(GOLD))


@pytest.fixture(scope="module")
def rendered(gold):
    """every scene through the numpy rule, once: name -> (rgba, ids, info)"""
    w, h = (int(v) for v in gold["size"])
    m = {k: gold[k] for k in ("pc", "nr", "col", "tm")}
    out = {}
    for name in gold["scenes"]:
        ct, unstable, window, t, tdelta = (int(v) for v in gold[f"{name}__flags"])
        info = {}
        rgba, ids = V.render_view(m, gold[f"{name}__mvp"], w, h, float(gold[f"{name}__threshold"]), ct, unstable, window, t, tdelta, clear_rgb=(0, 0, 0), info=info)
        out[str(name)] = (rgba, ids, info)
    return out


SCENES = ["a_type0", "a_type1", "a_type2", "a_type3", "a_type4", "b_unstable_window", "c_close"]


def test_fixture_holds_the_scenes(gold):
    assert [str(s) for s in gold["scenes"]] == SCENES
    assert os.path.getsize(GOLD) < (1 << 20)
    inst = gold["col"][:, 1]
    assert (inst == -1.0).any() and (inst != -1.0).any()      # the instance-colour cull has something to cull


@pytest.mark.parametrize("name", SCENES)
def test_ids_against_gl(gold, rendered, name):
    """pixels whose id differs from GL's: at most what the generator printed (fixed arrays, elementwise f32 and integer arithmetic: no margin)"""
    rep = generator_report()[name]
    _, ids, _ = rendered[name]
    differ = int((ids != gold[f"{name}__gl_ids"]).sum())
    print(f"{name}: {differ} of {ids.size} pixels differ from GL (generator: {rep['differ']})")
    assert differ <= rep["differ"]


@pytest.mark.parametrize("name", SCENES)
def test_coverage_against_gl(gold, rendered, name):
    _, ids, info = rendered[name]
    cov = int(((ids >= 0) != (gold[f"{name}__gl_ids"] >= 0)).sum())
    print(f"{name}: coverage differs on {cov} of {ids.size} pixels; the w > 0 rule skipped {info['w_skipped']} surfels, {info['big']} quads over 256 pixels")
    assert cov <= COVERAGE_CAP * ids.size


def test_close_camera_crosses_w0_and_has_big_quads(rendered):
    """camera (c) is the scene that exercises the deviation (quads GL would clip) and the quads of hundreds of pixels; it stays inside the cap above"""
    _, _, info = rendered["c_close"]
    assert info["w_skipped"] > 0 and info["big"] > 0
    assert generator_report()["c_close"]["w_skipped"] == info["w_skipped"]


@pytest.mark.parametrize("name", SCENES)
def test_colour_against_gl(gold, rendered, name):
    rep = generator_report()
    bound = COLOUR_FACTOR * max(r["max_colour_diff"] for r in rep.values())
    rgba, ids, _ = rendered[name]
    both = (ids == gold[f"{name}__gl_ids"]) & (ids >= 0)
    assert both.sum() > 1000
    diff = float(np.abs(rgba[..., :3][both] - gold[f"{name}__gl_rgb"][both]).max())
    print(f"{name}: largest colour difference {diff:.3e} on {int(both.sum())} pixels (bound {bound:.3e})")
    assert diff <= bound
    assert np.all(rgba[..., 3][ids >= 0] == 1.0) and np.all(rgba[..., 3][ids < 0] == 0.0)


def test_unstable_scene_draws_unstable_surfels(gold, rendered):
    _, ids, _ = rendered["b_unstable_window"]
    conf = gold["pc"][ids[ids >= 0], 3]
    assert (conf <= float(gold["b_unstable_window__threshold"])).any()


def test_viewer_mvp_has_the_orientation_of_pred_image():
    """With the frame's intrinsics at the tracked pose, a surface point lands within half a pixel of where the reference's prediction (combo_splat: gl_pred_vertex,
    the camera-frame point under each pixel of pred_image) has it."""
    d = np.load(os.path.join(ROOT, "tests", "golden", "gl_map_passes.npz"))
    fx, fy, cx, cy = (float(v) for v in d["K"])
    w, h = int(d["width"]), int(d["height"])
    pv = d["gl_pred_vertex"]
    ok = pv[..., 2] > 0
    assert ok.sum() > 5000
    j, i = np.nonzero(ok)
    T = d["pose"].astype(np.float64)
    world = pv[ok][:, :3].astype(np.float64) @ T[:3, :3].T + T[:3, 3]
    M = V.viewer_mvp(fx, fy, cx, cy, w, h, 0.1, 1000.0, d["pose"]).astype(np.float64)
    assert M.dtype == np.float64 and V.viewer_mvp(fx, fy, cx, cy, w, h, 0.1, 1000.0, d["pose"]).dtype == np.float32
    c = np.c_[world, np.ones(len(world))] @ M.T
    xw, yw = (c[:, 0] / c[:, 3] * 0.5 + 0.5) * w, (c[:, 1] / c[:, 3] * 0.5 + 0.5) * h
    assert np.abs(xw - (i + 0.5)).max() < 0.5
    assert np.abs((h - yw) - (j + 0.5)).max() < 0.5      # output row r is GL window row h - 1 - r
    zw = c[:, 2] / c[:, 3] * 0.5 + 0.5
    assert np.all((zw > 0) & (zw < 1))


def test_host_viewer_mvp_equals_python(tmp_path):
    """viewerMvp of ifx_host.hpp and viewer_mvp of the package: the same 16 floats, bit for bit (a header-only function: no library needed)"""
    import subprocess

    exe = str(tmp_path / "viewer_mvp_check")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-pthread", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "instancefusion_amd", "host"),
                    os.path.join(ROOT, "tests", "cpp", "viewer_mvp_check.cpp"), "-L", os.path.join(ROOT, "instancefusion_amd"), "-lifx", "-lz",
                    f"-Wl,-rpath,{os.path.join(ROOT, 'instancefusion_amd')}", "-o", exe], check=True)
    rs = np.random.default_rng(3)
    for _ in range(4):
        q, _r = np.linalg.qr(rs.normal(size=(3, 3)))
        pose = np.eye(4, dtype=np.float32)
        pose[:3, :3] = q.astype(np.float32)
        pose[:3, 3] = rs.normal(size=3).astype(np.float32)
        cam = [float(np.float32(v)) for v in (rs.uniform(80, 600), rs.uniform(80, 600), rs.uniform(50, 400), rs.uniform(50, 300), 640, 480, 0.1, 1000.0)]
        r = subprocess.run([exe] + [repr(v) for v in cam] + [repr(float(v)) for v in pose.reshape(16)], capture_output=True, text=True, check=True)
        got = np.array([int(x, 16) for x in r.stdout.split()], np.uint32).view(np.float32).reshape(4, 4)
        want = V.viewer_mvp(*cam, pose)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32))


def test_color_type_of_the_gui_flags():
    import instancefusion_amd as ifx
    assert ifx.view_color_type() == 0
    assert ifx.view_color_type(draw_times=True) == 3
    assert ifx.view_color_type(draw_colors=True, draw_times=True) == 2
    assert ifx.view_color_type(draw_normals=True, draw_colors=True, draw_times=True) == 1
    assert ifx.view_color_type(draw_instances=True, draw_normals=True, draw_colors=True, draw_times=True) == 4
