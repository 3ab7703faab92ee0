"""What the device forms of the sharded segmentation call cost next to the host form (profiles/owner_seg_device.md): 640 x 480, a world of one
(n_ranks = -1, the collectives on the library's RCCL communicator), 8 masks, root = 0, max_n = 8.  The three forms take turns on one handle; per form the median
of 20 calls after 3 warm-up calls, device time from the handle's stage events (ifx_stage_ms "instance": the span of the call on its stream) and host wall time
around the call (it ends with the host waiting for its stream).  Needs a GPU; prints one JSON line and, with --out, writes it to a file.

    python tools/owner_seg_device_numbers.py [--out FILE]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    import torch

    import instancefusion_amd as ifx
    import mask_bridge_numpy as mb
    import owner_seg_record_numpy as rec
    import roi_paste_numpy as rp
    from instancefusion_amd import sharded, synth

    if not torch.cuda.is_available():
        raise SystemExit("no GPU: nothing is measured")
    W, H, NF, N = 640, 480, 6, 8
    st = synth.make_stream(NF, W, H, noise=True)
    d_rgb = torch.from_numpy(st["rgb"].copy()).cuda()
    d_dep = torch.from_numpy(st["depth"].view(np.int16).copy()).cuda()
    ef = ifx.ElasticFusion(w=W, h=H, max_surfels=1 << 20, n_ranks=-1, rank=0)
    osh = sharded.OwnerShardedElasticFusion(ef, None, transport="library")
    for i in range(NF):
        if i == 4:   # every surfel stable: the id image is populated and the masks find surfels to vote for
            m = ef.download(); m["pc"][:, 3] = 20.0
            pose = ef.getCurrPose()
            ef.upload(m); ef.set_pose(pose, ef.tick)
            osh.predict()
        osh.process_frame_device(d_rgb[i].data_ptr(), d_dep[i].data_ptr())
    i = NF - 1
    masks, cls = synth.canned_masks(st["obj"][i], st["scene"], max_masks=N)
    rng = np.random.default_rng(1)
    while masks.shape[0] < N:   # (fewer objects in view than masks wanted: rectangles make up the number)
        r = np.zeros((1, H, W), np.uint8)
        y, x = int(rng.integers(0, H - 80)), int(rng.integers(0, W - 80))
        r[0, y:y + 60, x:x + 70] = 255
        masks, cls = np.concatenate([masks, r]), np.concatenate([np.asarray(cls, np.int32), [int(rng.integers(1, 80))]])
    cls = np.asarray(cls, np.int32)
    perm = rng.permutation(N)
    prob = np.where(masks[perm] != 0, np.float32(0.9), np.float32(0.1)).astype(np.float32)   # a detector's probabilities, in any order
    ori, _, _, cls_sorted = mb.bridge_masks(prob, cls[perm], 0.5)                             # ... and what the host's bridge makes of them
    rois, boxes = rp.rois_from_masks(masks[perm])
    t_prob, t_rois, t_boxes = torch.from_numpy(prob).cuda(), torch.from_numpy(rois).cuda(), torch.from_numpy(boxes).cuda()
    rgb, depth = st["rgb"][i], st["depth"][i]
    torch.cuda.synchronize()

    def forms(sp):
        return {
            "host": lambda f: osh.process_segmentation(rgb, depth, ori, cls_sorted, f, superpixels=sp),
            "image_f32": lambda f: osh.process_segmentation_device(rgb, depth, t_prob, cls[perm], f, superpixels=sp, root=0, max_n=N),
            "rois": lambda f: osh.process_segmentation_rois(rgb, depth, t_rois, t_boxes, cls[perm], f, superpixels=sp, root=0, max_n=N),
        }

    out = dict(width=W, height=H, masks=N, world=1, calls=a.calls, warmup=a.warmup,
               record_bytes=dict(image=4 * rec.record_words(1, N, 0, W * H), rois=4 * rec.record_words(2, N, rois.shape[-1], W * H)), host_upload_bytes=N * W * H)
    frame = 1000
    for sp in (False, True):
        t = {k: dict(device_ms=[], wall_ms=[]) for k in forms(sp)}
        for it in range(a.warmup + a.calls):
            for k, call in forms(sp).items():   # the forms take turns: what else the host and the GPU are doing is shared among them
                ef.sync()
                ef.stage_ms(reset=True)
                t0 = time.perf_counter()
                call(frame)
                ef.sync()
                t1 = time.perf_counter()
                frame += 3
                if it >= a.warmup:
                    t[k]["device_ms"].append(ef.stage_ms()["instance"])
                    t[k]["wall_ms"].append((t1 - t0) * 1e3)
        out["superpixels" if sp else "plain"] = {k: {q: dict(median=float(np.median(v)), min=float(np.min(v)), max=float(np.max(v))) for q, v in d.items()} for k, d in t.items()}
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    ef.close()


if __name__ == "__main__":
    main()
