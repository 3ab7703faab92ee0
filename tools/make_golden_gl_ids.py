#!/usr/bin/env python3
"""Golden id images of the reference's OWN surfel-id shaders for more than one frame (tests/golden/gl_ids_scenes.npz): surfel_ids.vert / .geom / .frag
(GENERAL) and instance_surfel_ids.vert + surfel_ids.geom / .frag (INSTANCECOMPARE), UNMODIFIED, on Mesa's software rasteriser (oracle/gl, as
tools/make_golden_gl.py, whose scene set-up and vertex packing this reuses).  Run in the development container only:

    python tools/make_golden_gl_ids.py        # writes tests/golden/gl_ids_scenes.npz and prints how the numpy restatement of the quad rule compares

Scenes: the frame of gl_map_passes.npz (its post-clean map, the one gl_ids was drawn from) at 160x120 and at 640x480, four other seeds / camera motions
of profiles/r06_gl_agreement_other_scenes.txt at 160x120, and an INSTANCECOMPARE render of the first map with votes that are not uniform.  Each scene
keeps only what the id render reads: the STABLE surfels (confidence above the threshold; nothing else is ever drawn) whose centre is in front of the camera
and projects within 32 px of the image, in map order, their pc / nr (votes where the scene needs them; the INSTANCECOMPARE scene reads the map of "frame"),
pose, K, size, confidence and the GL image, drawn from exactly that stored map -- the ids are slots of the stored map.
The 640x480 map keeps the stable surfels whose centre projects into the middle fifth of the image on both axes (a 380 k-surfel map does not fit the
size limit of a committed file, 1 MiB)."""
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "gl_ids_scenes.npz")
NF = 16

# name, size, seed, motion, INSTANCECOMPARE
SCENES = [("frame", "160x120", 0, "", 0), ("frame_vga", "640x480", 0, "", 0), ("s11_nominal", "160x120", 11, "nominal", 0),
          ("s23_fast", "160x120", 23, "fast", 0), ("s37_shake", "160x120", 37, "shake", 0),
          ("s53_spin", "160x120", 53, "spin", 0), ("frame_instcmp", "160x120", 0, "", 1)]


def one(name, seed, motion, instcmp, out):
    """child process (IFX_GL_SIZE set before make_golden_gl is imported): the oracle's post-clean map of that scene, then the GL id render"""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import make_golden_gl as MG
    import oracle_lib as ol
    from instancefusion_amd import synth

    G = MG.G
    W, H, K, CONF = MG.W, MG.H, MG.K, MG.CONF
    ol.build()
    if seed or motion:
        scene = synth.Scene(seed or 1)
        st = synth.make_stream_from_poses(synth.trajectory_profile(motion or "nominal", NF + 1, seed or 1), scene, W, H, noise_seed=(seed or 1) + 1, **K)
    else:
        st = synth.make_stream(NF + 1, W, H, noise=True, **K)
    o = ol.Oracle(w=W, h=H, max_surfels=max(200000, W * H * 8), confidence=CONF, **K)
    o2 = ol.Oracle(w=W, h=H, max_surfels=max(200000, W * H * 8), confidence=CONF, **K)
    for i in range(NF):
        o.process_frame(st["rgb"][i], st["depth"][i]); o2.process_frame(st["rgb"][i], st["depth"][i])
    rgb, depth = st["rgb"][NF], st["depth"][NF]
    pose = o2.process_frame(rgb, depth).astype(np.float32)
    o2.close()
    t = int(o.tick)
    # the map stage of make_golden_gl.main on the oracle: index map, fusion, index map, clean -> the post-clean map the ids are drawn from
    o.set_frame(rgb, depth)
    o.predict_indices(pose, t)
    o.fuse(pose, t, 1.0)
    o.predict_indices(pose, t)
    o.clean(pose, t)
    m = o.download()
    # stable surfels whose centre projects into the image or within 32 px of it (the GL image is drawn from exactly what is kept)
    Ti = np.linalg.inv(pose.astype(np.float64))
    q = m["pc"][:, :3].astype(np.float64) @ Ti[:3, :3].T + Ti[:3, 3]
    with np.errstate(all="ignore"):
        u, v = K["fx"] * q[:, 0] / q[:, 2] + K["cx"], K["fy"] * q[:, 1] / q[:, 2] + K["cy"]
    keep = (m["pc"][:, 3] > np.float32(CONF)) & (q[:, 2] > 0)
    if W >= 640:    # centre of the surfel inside the middle fifth of the image (both axes)
        keep &= (u >= W * 0.4) & (u < W * 0.6) & (v >= H * 0.4) & (v < H * 0.6)
    else:
        keep &= (u >= -32) & (u < W + 32) & (v >= -32) & (v < H + 32)
    mm = {k: np.ascontiguousarray(m[k][keep]) for k in m}
    n = mm["pc"].shape[0]
    if instcmp:     # votes that are not uniform: one word of one vec4 set on a third of the surfels, every vote vec4 equal (culled) elsewhere
        rs = np.random.default_rng(7)
        votes = np.zeros((n, 48), np.float32)
        pick = np.nonzero(rs.random(n) < 1 / 3)[0]
        votes[pick, rs.integers(0, 48, pick.size)] = rs.integers(1, 40, pick.size).astype(np.float32)
        mm["votes"] = votes
    gl = G.GL(W, H)
    gl.glEnable(G.GL_DEPTH_TEST)      # Gui::preCall, IF/gui/Gui.cpp:211-215
    gl.glDepthFunc(G.GL_LESS)
    vert = "instance_surfel_ids.vert" if instcmp else "surfel_ids.vert"
    prog = gl.program(MG.SHADERS, vert, "surfel_ids.frag", "surfel_ids.geom")     # EF/IndexMap.cpp:40-49 (IF: the INSTANCECOMPARE program)
    tex = gl.tex2d(W, H, G.GL_R32I, G.GL_RED_INTEGER, G.GL_INT)
    fbo = gl.framebuffer(W, H, [tex])
    vbo = gl.buffer(MG.pack_vbo(mm))
    gl.begin_pass(fbo, W, H, "i")      # IndexMap::renderSurfelIds, EF/IndexMap.cpp:315-465
    gl.uniforms(prog, t_inv=np.linalg.inv(pose.astype(np.float32)), cam=[K["cx"], K["cy"], K["fx"], K["fy"]], maxDepth=MG.MAX_DEPTH, cols=float(W), rows=float(H),
                time=int(t), timeDelta=int(MG.TIME_DELTA), conf=float(CONF))
    nattr = 16 if instcmp else 3
    gl.attribs(vbo, nattr, MG.VSIZE)
    gl.glDrawArrays(G.GL_POINTS, 0, n)
    gl.attribs_off(nattr)
    gl.end_pass()
    ids = gl.read_tex(tex, W, H, G.GL_RED_INTEGER, G.GL_INT, np.int32, 1)
    rec = dict(pc=mm["pc"], nr=mm["nr"], pose=pose, K=np.array([K["fx"], K["fy"], K["cx"], K["cy"]], np.float32), size=np.array([W, H], np.int32),
               confidence=np.float32(CONF), max_depth=np.float32(MG.MAX_DEPTH), gl_ids=ids)
    if instcmp:
        rec["votes"] = mm["votes"]
    np.savez(out, **rec)
    print(f"{name}: {W}x{H}, {m['pc'].shape[0]} surfels, {n} stored, {(ids > 0).sum()} pixels drawn")


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "--one":
        name, seed, motion, instcmp, out = sys.argv[2], int(sys.argv[3]), sys.argv[4], int(sys.argv[5]), sys.argv[6]
        one(name, seed, motion, instcmp, out)
        return
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import oracle_lib as ol
    import quad_ids_numpy as Q

    ol.build()      # once, before the scenes run side by side

    tmp = os.path.join(ROOT, "build", "gl_ids_scenes")
    os.makedirs(tmp, exist_ok=True)
    procs = []
    for name, size, seed, motion, instcmp in SCENES:
        env = dict(os.environ, IFX_GL_SIZE=size)
        procs.append(subprocess.Popen([sys.executable, os.path.abspath(__file__), "--one", name, str(seed), motion, str(instcmp), os.path.join(tmp, name + ".npz")], env=env))
    for p in procs:
        if p.wait() != 0:
            raise SystemExit("a scene failed")
    gold = {"scenes": np.array([s[0] for s in SCENES])}
    report = {}
    for name, *_ in SCENES:
        d = dict(np.load(os.path.join(tmp, name + ".npz")))
        for k, v in d.items():
            if name == "frame_instcmp" and k in ("pc", "nr"):      # the map of "frame": stored once
                assert np.array_equal(v, gold["frame__" + k])
                continue
            gold[f"{name}__{k}"] = v
        w, h = (int(x) for x in d["size"])
        mine = Q.render_ids(d["pc"], d["nr"], d["pose"], d["K"], w, h, float(d["max_depth"]), float(d["confidence"]), d.get("votes"))
        same = mine == d["gl_ids"]
        report[name] = dict(equal_pct=round(float(same.mean() * 100), 3), differ=int((~same).sum()), coverage_differs=int(((mine > 0) != (d["gl_ids"] > 0)).sum()),
                            gl_drawn=int((d["gl_ids"] > 0).sum()))
        print(f"{name:14s} quad rule vs GL: {json.dumps(report[name])}")
    np.savez_compressed(OUT, **gold)
    print(f"wrote {OUT} ({os.path.getsize(OUT) / 1024:.0f} KiB)")


if __name__ == "__main__":
    main()
