"""What option "rgb_fuse" costs or saves on a frame whose candidate list is long: the 320x240 test stream with a colour image of uniform noise (about 52 200
candidates at level 0: a hundred chunks, or six to seven rounds per thread, for the fused form's 32 photometric blocks) and, for comparison, with its own colour
images.  Per form (rgb_fuse = 7 with rgb_own = 7, rgb_fuse = 7 with rgb_own = 0 -- the chunk claims --, rgb_fuse = 0; alternating, two runs each): HIP-event time
(option kernel_timing) of the tracker's iteration launches per frame, per level, the meeting give-ups and the adopted shares.

    python tools/rgb_fuse_cost.py [frames] [rgb_blocks: photometric blocks of the fused launches, 0 = the default]"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: F401,E402  (first: libifx.so binds to the HIP runtime torch ships)

import instancefusion_amd as ifx  # noqa: E402
from instancefusion_amd import synth  # noqa: E402

frames = int(sys.argv[1]) if len(sys.argv) > 1 else 36
blocks = int(sys.argv[2]) if len(sys.argv) > 2 else 0
W, H = 320, 240
K = dict(fx=264.0, fy=264.0, cx=160.0, cy=120.0)
st = synth.make_stream(12, W, H, noise=True, **K)
NOISE = np.random.RandomState(1234).randint(0, 256, (H, W, 3)).astype(np.uint8)
NAMES = [f"{fam}@L{l}" for fam in ("icp_residual", "rgb_step_solve") for l in range(3)]


def run(fuse, own, noise):
    ef = ifx.ElasticFusion(w=W, h=H, max_surfels=400000, confidence=3.0, **K)
    ef.set_option("gn_persist", 0); ef.set_option("rgb_fuse", fuse); ef.set_option("rgb_own", own)
    if blocks and fuse:
        ef.set_option("rgb_blocks", blocks)
    order = list(range(12)) + list(range(10, 0, -1))
    img = lambda i: NOISE if noise else st["rgb"][i]
    for i in order[:6]:
        ef.processFrame(img(i), st["depth"][i])
    ef.sync()
    ef.set_option("kernel_timing", 1); ef.kernel_ms("__reset__")
    for k in range(frames):
        i = order[(6 + k) % len(order)]
        ef.processFrame(img(i), st["depth"][i])
    ef.sync()
    t = {nm: ef.kernel_ms(nm) for nm in NAMES}
    cand = [int(ef.tracker_buffer("cand_n", lvl)[0]) for lvl in range(3)]
    gu, ad = ef.tracker_meet_giveups(), ef.tracker_meet_adopted()
    ef.close()
    per_frame = sum(avg * cnt for avg, cnt in t.values()) / frames * 1e3
    return per_frame, t, cand, gu, ad


for noise in (True, False):
    for fuse, own in ((7, 7), (7, 0), (0, 0)) * 2:
        per_frame, t, cand, gu, ad = run(fuse, own, noise)
        cols = "  ".join(f"{nm.replace('icp_residual', 'A').replace('rgb_step_solve', 'B')} {avg * 1e3:6.2f} x{cnt / frames:4.1f}" for nm, (avg, cnt) in t.items() if cnt)
        print(f"{'noise' if noise else 'plain'} rgb_fuse={fuse} rgb_own={own}: iteration launches {per_frame:7.1f} us per frame; candidates {cand}; give-ups {gu}, adopted {ad}\n    {cols}")
