#!/usr/bin/env python3
"""Golden images of the reference viewer's OWN surfel pass (tests/golden/gl_viewer_scenes.npz): draw_global_surface.vert / .geom / .frag and
draw_global_ID.vert / .geom / .frag, UNMODIFIED, on Mesa's software rasteriser (oracle/gl, as tools/make_golden_gl_ids.py, whose map this reuses:
the post-clean map of its scene "frame").  Run in the development container only:

    python tools/make_golden_gl_viewer.py     # writes the fixture and profiles/r28_viewer_rule_vs_gl.txt: how tests/viewer_numpy.py compares

GL state per scene (GlobalModel::renderPointCloud / renderGlobalID, EF/GlobalModel.cpp:328-457; Gui::preCall): depth test on, GL_LESS, cleared;
an RGBA32F target for the surface program and an R32I target for the id program (it writes gl_VertexID); three attributes at Vertex::SIZE;
glDrawArrays(GL_POINTS).  The id program clears to 0 and cannot tell surfel 0 from the background: the stored id image takes its coverage from the
surface pass's alpha (the two programs draw the same geometry) and holds -1 where nothing was drawn, rows flipped to top-first.

Scenes: one map, a 160x120 viewport, near 0.1, far 1000, the GUI's focal length scaled to the viewport (420 * 160 / 640); three cameras --
(a) the tracked pose, every colorType 0..4; (b) pulled back 1 m and turned 30 degrees about y, unstable = 1 and drawWindow = 1; (c) moved forward
to 15 cm from the nearest surface on the optical axis, colorType 4.  The map is culled to the surfels whose bounding sphere reaches one of the
three frusta and keeps only what the pass reads: pc, col (colour word, instance-colour word), tm, nr.  The instance-colour word is a packed RGB
value on 60 % of the surfels and -1 (never drawn) on the rest, of which the stored map keeps one in eight (the size limit of a committed file)."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
OUT = os.path.join(ROOT, "tests", "golden", "gl_viewer_scenes.npz")
REPORT = os.path.join(ROOT, "profiles", "r28_viewer_rule_vs_gl.txt")
NF = 16
VW, VH = 160, 120
NEAR, FAR = 0.1, 1000.0
FOCAL = 420.0 * VW / 640.0


def post_clean_map():
    """the map of make_golden_gl_ids.py's scene "frame": 16 frames, then index map, fusion, index map, clean of the 17th"""
    import make_golden_gl as MG
    import oracle_lib as ol
    from instancefusion_amd import synth

    W, H, K, CONF = MG.W, MG.H, MG.K, MG.CONF
    ol.build()
    st = synth.make_stream(NF + 1, W, H, noise=True, **K)
    o = ol.Oracle(w=W, h=H, max_surfels=max(200000, W * H * 8), confidence=CONF, **K)
    o2 = ol.Oracle(w=W, h=H, max_surfels=max(200000, W * H * 8), confidence=CONF, **K)
    for i in range(NF):
        o.process_frame(st["rgb"][i], st["depth"][i]); o2.process_frame(st["rgb"][i], st["depth"][i])
    rgb, depth = st["rgb"][NF], st["depth"][NF]
    pose = o2.process_frame(rgb, depth).astype(np.float32)
    o2.close()
    t = int(o.tick)
    o.set_frame(rgb, depth)
    o.predict_indices(pose, t)
    o.fuse(pose, t, 1.0)
    o.predict_indices(pose, t)
    o.clean(pose, t)
    m = o.download()
    return m, pose, t, float(CONF)


def reaches(m, mvp):
    """bounding sphere (1.5 r: the quad's corners lie at r * 1.41421356) against the four side planes and w > 0 of the frustum, in f64"""
    M = mvp.astype(np.float64)
    p = m["pc"][:, :3].astype(np.float64)
    r = 1.5 * np.abs(m["nr"][:, 3].astype(np.float64))
    keep = np.ones(p.shape[0], bool)
    for pl in (M[3] + M[0], M[3] - M[0], M[3] + M[1], M[3] - M[1], M[3]):
        keep &= (p @ pl[:3] + pl[3]) >= -r * np.linalg.norm(pl[:3])
    return keep


def main():
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import make_golden_gl as MG
    import viewer_numpy as V
    G = MG.G

    m, pose, t, conf = post_clean_map()
    n_all = m["pc"].shape[0]
    rs = np.random.default_rng(7)
    word = (rs.integers(0, 256, n_all) << 16 | rs.integers(0, 256, n_all) << 8 | rs.integers(0, 256, n_all)).astype(np.float32)
    real = rs.random(n_all) < 0.6
    m["col"][:, 1] = np.where(real, word, np.float32(-1.0))
    drawable = real | (rs.random(n_all) < 0.125)      # a surfel whose word is -1 reaches no viewport: one in eight is kept, so that the cull has something to cull

    P64 = pose.astype(np.float64)
    back = np.eye(4); back[2, 3] = -1.0                       # (b) the camera pulled back 1 m along its axis, then turned 30 degrees about y
    a = np.deg2rad(30.0)
    turn = np.array([[np.cos(a), 0, np.sin(a), 0], [0, 1, 0, 0], [-np.sin(a), 0, np.cos(a), 0], [0, 0, 0, 1]])
    pose_b = P64 @ back @ turn
    Ti = np.linalg.inv(P64)                                  # (c) forward to 15 cm from the nearest stable surface within 8 px of the optical axis
    q = m["pc"][:, :3].astype(np.float64) @ Ti[:3, :3].T + Ti[:3, 3]
    with np.errstate(all="ignore"):
        near_axis = (q[:, 2] > 0) & (np.hypot(FOCAL * q[:, 0] / q[:, 2], FOCAL * q[:, 1] / q[:, 2]) < 8) & (m["pc"][:, 3] > conf)
    fwd = np.eye(4); fwd[2, 3] = float(q[near_axis, 2].min()) - 0.15
    pose_c = P64 @ fwd
    cam = lambda T: V.viewer_mvp(FOCAL, FOCAL, VW / 2.0, VH / 2.0, VW, VH, NEAR, FAR, T)
    mvps = dict(a=cam(P64), b=cam(pose_b), c=cam(pose_c))

    keep = (reaches(m, mvps["a"]) | reaches(m, mvps["b"]) | reaches(m, mvps["c"])) & drawable
    mm = {k: np.ascontiguousarray(m[k][keep]) for k in m}
    n = mm["pc"].shape[0]
    print(f"map: {n_all} surfels, {n} stored, tick {t}, confidence threshold {conf}")

    # name, camera, colorType, unstable, drawWindow, timeDelta
    scenes = [(f"a_type{ct}", "a", ct, 0, 0, 200) for ct in range(5)] + [("b_unstable_window", "b", 2, 1, 1, 4), ("c_close", "c", 4, 0, 0, 200)]

    gl = G.GL(VW, VH)
    print("GL:", *gl.version())
    gl.glEnable(G.GL_DEPTH_TEST)      # Gui::preCall, IF/gui/Gui.cpp:211-215
    gl.glDepthFunc(G.GL_LESS)
    surf = gl.program(MG.SHADERS, "draw_global_surface.vert", "draw_global_surface.frag", "draw_global_surface.geom")      # EF/GlobalModel.cpp:34-38
    idp = gl.program(MG.SHADERS, "draw_global_ID.vert", "draw_global_ID.frag", "draw_global_ID.geom")
    ctex = gl.tex2d(VW, VH, G.GL_RGBA32F, G.GL_RGBA, G.GL_FLOAT)
    itex = gl.tex2d(VW, VH, G.GL_R32I, G.GL_RED_INTEGER, G.GL_INT)
    cfbo, ifbo = gl.framebuffer(VW, VH, [ctex]), gl.framebuffer(VW, VH, [itex])
    vbo = gl.buffer(MG.pack_vbo(dict(mm, ic=np.zeros((n, 4), np.float32), votes=np.zeros((n, 48), np.float32))))

    gold = dict(scenes=np.array([s[0] for s in scenes]), pc=mm["pc"], nr=mm["nr"], col=mm["col"], tm=mm["tm"], size=np.array([VW, VH], np.int32))
    lines = [f"# tests/viewer_numpy.py against the reference's draw_global_surface.* / draw_global_ID.* on {' '.join(gl.version())}",
             f"# map of {n} surfels, viewport {VW}x{VH}; per scene: pixels, pixels with equal id, pixels whose id differs, pixels whose coverage differs,",
             "# the largest absolute colour difference on the pixels with equal id, surfels the w > 0 rule skipped, drawn quads with a box of more than 256 pixels"]
    for name, c, ct, unstable, window, tdelta in scenes:
        un = dict(MVP=mvps[c], threshold=float(conf), colorType=int(ct), unstable=int(unstable), drawWindow=int(window), time=int(t), timeDelta=int(tdelta), signMult=1.0)
        out = []
        for prog, fbo, kinds in ((surf, cfbo, "f"), (idp, ifbo, "i")):
            gl.begin_pass(fbo, VW, VH, kinds)
            gl.uniforms(prog, **un)
            gl.attribs(vbo, 3, MG.VSIZE)
            gl.glDrawArrays(G.GL_POINTS, 0, n)
            gl.attribs_off(3)
            gl.end_pass()
        rgba = gl.read_tex(ctex, VW, VH, G.GL_RGBA, G.GL_FLOAT, np.float32, 4)[::-1]
        ids = gl.read_tex(itex, VW, VH, G.GL_RED_INTEGER, G.GL_INT, np.int32, 1)[::-1]
        ids = np.where(rgba[..., 3] > 0, ids, -1).astype(np.int32)
        gold[f"{name}__mvp"] = mvps[c]
        gold[f"{name}__flags"] = np.array([ct, unstable, window, t, tdelta], np.int32)
        gold[f"{name}__threshold"] = np.float32(conf)
        gold[f"{name}__gl_ids"] = ids
        gold[f"{name}__gl_rgb"] = np.ascontiguousarray(rgba[..., :3])
        info = {}
        mine_rgba, mine_ids = V.render_view(mm, mvps[c], VW, VH, conf, ct, unstable, window, t, tdelta, clear_rgb=(0, 0, 0), info=info)
        same = mine_ids == ids
        both = same & (ids >= 0)
        rep = dict(pixels=VW * VH, equal=int(same.sum()), differ=int((~same).sum()), coverage_differs=int(((mine_ids >= 0) != (ids >= 0)).sum()),
                   max_colour_diff=float(np.abs(mine_rgba[..., :3][both] - rgba[..., :3][both]).max()) if both.any() else 0.0, gl_drawn=int((ids >= 0).sum()),
                   w_skipped=info["w_skipped"], big_quads=info["big"])
        lines.append(f"{name} {json.dumps(rep)}")
        print(lines[-1])
    np.savez_compressed(OUT, **gold)
    size = os.path.getsize(OUT)
    print(f"wrote {OUT} ({size / 1024:.0f} KiB)")
    assert size < (1 << 20), "a committed file stays under 1 MiB"
    with open(REPORT, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
