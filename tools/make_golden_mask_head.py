#!/usr/bin/env python3
"""Writes tests/golden/mask_head_ref.npz: mask-head logits, boxes, scores and labels with what maskrcnn-benchmark's own Python makes of them between the mask
head's last convolution and the bridge -- the kept rows in order, the resized boxes, the pasted masks.

    python tools/make_golden_mask_head.py /path/to/maskrcnn-benchmark-master [--write-header]

Taken from that tree BY PATH AT RUN TIME and run on CPU torch; none of their text is in this repository:
  maskrcnn_benchmark/structures/bounding_box.py                  the module (it imports torch only): BoxList with resize and __getitem__
  maskrcnn_benchmark/modeling/roi_heads/mask_head/inference.py   the ast nodes of MaskPostProcessor, expand_boxes, expand_masks, paste_mask_in_image and Masker
  demo/predictor.py                                              the ast node of COCODemo.select_top_predictions, run as a function on an object that has
                                                                 confidence_threshold = 0.7
in the order of COCODemo.compute_prediction and the bridge: MaskPostProcessor.forward, prediction.resize((width, height)), the Masker, select_top_predictions.
A field "rows" (arange) rides along so that the file can say which input row each result came from.

Per case the file holds R, C, M, the frame size, in_size, boxes, scores, labels and the bytes q of each row's OWN channel (logit = (q - 128) / 16; the other
channels are made from q by mask_head_numpy.fixture_logits, which the reference is given too), then the reference's kept rows, resized boxes and bit-packed masks.
The tool also measures the largest difference between the rule's SIGMOID and torch's CPU sigmoid over the cases' samples (absolute and in ulp of torch's value),
stores both, and -- with --write-header -- writes them into include/ifx_c_api.h.  Before writing, the statement (tests/mask_head_numpy.py) is held against the
results with the conditions of tests/test_mask_head_cpu.py."""
import ast
import importlib.util
import os
import re
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
OUT = os.path.join(ROOT, "tests", "golden", "mask_head_ref.npz")
HEADER = os.path.join(ROOT, "include", "ifx_c_api.h")
FRAMES = ((160, 120), (320, 240))
IN_SIZES = ((800, 600), (801, 607))          # 800x600: equal ratios to both frames (0.2, 0.4); 801x607: unequal ones
MS, CS, RS = (7, 14, 28), (2, 81), (1, 5, 40)
THRESH = 0.7


def load_reference(tree):
    import torch

    p_box = os.path.join(tree, "maskrcnn_benchmark", "structures", "bounding_box.py")
    p_inf = os.path.join(tree, "maskrcnn_benchmark", "modeling", "roi_heads", "mask_head", "inference.py")
    p_demo = os.path.join(tree, "demo", "predictor.py")
    spec = importlib.util.spec_from_file_location("_ref_bounding_box", p_box)
    bb = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bb)
    with open(p_inf) as f:
        t = ast.parse(f.read())
    want = ("MaskPostProcessor", "expand_boxes", "expand_masks", "paste_mask_in_image", "Masker")
    nodes = [n for n in t.body if isinstance(n, (ast.FunctionDef, ast.ClassDef)) and n.name in want]
    assert sorted(n.name for n in nodes) == sorted(want), [n.name for n in nodes]
    ns = {"torch": torch, "nn": torch.nn, "np": np, "interpolate": torch.nn.functional.interpolate, "BoxList": bb.BoxList}
    exec(compile(ast.Module(body=nodes, type_ignores=[]), p_inf, "exec"), ns)
    with open(p_demo) as f:
        t = ast.parse(f.read())
    demo = [n for n in t.body if isinstance(n, ast.ClassDef) and n.name == "COCODemo"]
    assert len(demo) == 1
    sel = [n for n in demo[0].body if isinstance(n, ast.FunctionDef) and n.name == "select_top_predictions"]
    assert len(sel) == 1
    ns2 = {"torch": torch}
    exec(compile(ast.Module(body=sel, type_ignores=[]), p_demo, "exec"), ns2)
    return bb.BoxList, ns["MaskPostProcessor"](), ns["Masker"](threshold=0.5, padding=1), ns2["select_top_predictions"]


def smooth_q(rng, M):
    """A blob of logits with a few waves on it as bytes (logit = (q - 128) / 16 in [-8, 8)); never 128: a logit of 0 is a probability of exactly 0.5, and a
    plateau of those would be a plateau of ties at the Masker's threshold."""
    y, x = np.mgrid[0:M, 0:M].astype(np.float64) / max(M - 1, 1)
    cx, cy = rng.uniform(0.3, 0.7, 2)
    rad = rng.uniform(0.25, 0.6)
    v = (rad - np.hypot(x - cx, y - cy)) * rng.uniform(8, 30)
    for _ in range(3):
        fx, fy = rng.uniform(-9, 9, 2)
        v += rng.uniform(0.2, 1.0) * np.cos(fx * x + fy * y + rng.uniform(0, 6.28))
    q = np.clip(np.rint(v * 16.0) + 128, 0, 255).astype(np.uint8)
    q[q == 128] = 129
    return q


def make_case(rng, R, C, M, in_size):
    iw, ih = in_size
    x0 = rng.uniform(0, iw * 0.7, R); y0 = rng.uniform(0, ih * 0.7, R)
    w = rng.uniform(iw * 0.05, iw * 0.45, R); h = rng.uniform(ih * 0.05, ih * 0.45, R)
    boxes = np.stack([x0, y0, np.minimum(x0 + w, iw - 1), np.minimum(y0 + h, ih - 1)], axis=1).astype(np.float32)
    if R >= 5:
        boxes[1] = (0, 0, iw - 1, ih - 1)                      # the whole image
        boxes[2] = (10.5, 20.25, 14.0, 23.5)                   # less than a frame pixel at the smaller frame
    pool = np.asarray([0.7, 0.7000000476837158, 0.95, 0.95, 0.95, 0.81, 0.81, 0.3, 0.05, 0.999], np.float32)      # at the threshold, one ulp above it, ties
    scores = rng.uniform(0.02, 1.0, R).astype(np.float32)
    pick = rng.random(R) < 0.6
    scores[pick] = pool[rng.integers(0, len(pool), int(pick.sum()))]
    if R == 1:
        scores[0] = np.float32(0.9)
    if R >= 5:
        scores[0] = np.float32(0.7); scores[3] = scores[4] = np.float32(0.95)
    if R >= 40:
        scores[7] = np.nextafter(np.float32(0.7), np.float32(1)); scores[8] = np.float32(0.7)
    labels = rng.integers(0, C, R).astype(np.int64)
    labels[0] = C - 1
    if R >= 5:
        labels[3] = 0; labels[4] = C - 1
    q = np.stack([smooth_q(rng, M) for _ in range(R)])
    return boxes, scores, labels, q


def main():
    import torch

    import mask_head_numpy as mh
    import roi_paste_numpy as rp

    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    if len(args) != 1:
        sys.exit(__doc__)
    BoxList, post, masker, select_top = load_reference(args[0])
    demo = types.SimpleNamespace(confidence_threshold=THRESH)
    rng = np.random.default_rng(20261019)
    torch.set_num_threads(1)
    cases = []
    sig_abs = sig_ulp = 0.0
    k = 0
    for M in MS:
        for C in CS:
            for R in RS:
                (W, H), in_size = FRAMES[k % 2], IN_SIZES[(k // 2) % 2]
                k += 1
                boxes, scores, labels, q = make_case(rng, R, C, M, in_size)
                logits = mh.fixture_logits(q, labels, C)
                box = BoxList(torch.from_numpy(boxes), in_size, mode="xyxy")
                box.add_field("scores", torch.from_numpy(scores))
                box.add_field("labels", torch.from_numpy(labels))
                box.add_field("rows", torch.arange(R))
                pred = post(torch.from_numpy(logits), [box])[0]
                pred = pred.resize((W, H))
                pred.add_field("mask", masker([pred.get_field("mask")], [pred])[0])
                top = select_top(demo, pred)
                ref_rows = top.get_field("rows").numpy().astype(np.int32)
                ref_boxes = top.bbox.numpy().astype(np.float32)
                ref_masks = top.get_field("mask").numpy()[:, 0] != 0
                assert np.array_equal(top.get_field("labels").numpy(), labels[ref_rows])
                # the sigmoid of the reference on the samples the rule reads, against the rule's
                own = torch.from_numpy(logits[np.arange(R), labels]).sigmoid().numpy()
                mine = mh.sigmoid(logits[np.arange(R), labels])
                d = np.abs(mine.astype(np.float64) - own.astype(np.float64))
                sig_abs = max(sig_abs, float(d.max()))
                sig_ulp = max(sig_ulp, float((d / np.spacing(own).astype(np.float64)).max()))
                cases.append(dict(R=R, C=C, M=M, W=W, H=H, in_size=in_size, boxes=boxes, scores=scores, labels=labels, q=q, logits=logits,
                                  ref_rows=ref_rows, ref_boxes=ref_boxes, ref_masks=ref_masks))
    print(f"SIGMOID against torch's CPU sigmoid on the cases' samples: largest difference {sig_abs:.6e} ({sig_ulp:.3f} ulp)")
    band = mh.PASTE_BAND + sig_abs
    box_px = band_px = 0
    for c in cases:       # the conditions of tests/test_mask_head_cpu.py
        masks, bx, cls, rows = mh.mask_head_select(c["logits"], c["boxes"], c["scores"], c["labels"], c["in_size"], (c["W"], c["H"]), THRESH, True)
        assert sorted(rows.tolist()) == sorted(c["ref_rows"].tolist()), (rows, c["ref_rows"])
        assert np.array_equal(c["scores"][rows], c["scores"][c["ref_rows"]])
        at = {int(r): j for j, r in enumerate(c["ref_rows"])}
        for j, r in enumerate(rows):
            assert np.array_equal(bx[j].view(np.uint32), c["ref_boxes"][at[int(r)]].view(np.uint32)), (c["in_size"], c["W"], bx[j], c["ref_boxes"][at[int(r)]])
            rect, v = rp.paste_values(masks[j], bx[j], c["W"], c["H"])
            assert rect is not None
            X0, X1, Y0, Y1 = rect
            tie = np.zeros((c["H"], c["W"]), bool)
            tie[Y0:Y1, X0:X1] = np.abs(v.astype(np.float64) - 0.5) <= band
            mine = rp.paste_roi(masks[j], bx[j], c["W"], c["H"], 0.5) != 0
            box_px += (X1 - X0) * (Y1 - Y0)
            band_px += int(tie.sum())
            diff = (mine != c["ref_masks"][at[int(r)]]) & ~tie
            assert not diff.any(), (c["R"], c["C"], c["M"], int(r), np.argwhere(diff)[:4])
    print(f"{len(cases)} cases, {sum(len(c['ref_rows']) for c in cases)} kept rows, {box_px} box pixels, {band_px} within {band:.3e} of the threshold")
    assert band_px * 10000 <= box_px, (band_px, box_px)
    cat = lambda key, dt: np.concatenate([np.asarray(c[key], dt).reshape(-1) for c in cases]) if cases else np.zeros(0, dt)
    np.savez_compressed(
        OUT, r=np.asarray([c["R"] for c in cases], np.int32), c=np.asarray([c["C"] for c in cases], np.int32), m=np.asarray([c["M"] for c in cases], np.int32),
        w=np.asarray([c["W"] for c in cases], np.int32), h=np.asarray([c["H"] for c in cases], np.int32),
        in_w=np.asarray([c["in_size"][0] for c in cases], np.int32), in_h=np.asarray([c["in_size"][1] for c in cases], np.int32),
        kept=np.asarray([len(c["ref_rows"]) for c in cases], np.int32), q=cat("q", np.uint8), labels=cat("labels", np.int64),
        boxes=np.concatenate([c["boxes"] for c in cases]), scores=cat("scores", np.float32), ref_rows=cat("ref_rows", np.int32),
        ref_boxes=np.concatenate([c["ref_boxes"].reshape(-1, 4) for c in cases]),
        ref_bits=np.concatenate([np.packbits(m.reshape(-1)) for c in cases for m in c["ref_masks"]]),
        sigmoid_max_abs=np.float64(sig_abs), sigmoid_max_ulp=np.float64(sig_ulp))
    print(f"{OUT}: {os.path.getsize(OUT)} bytes")
    assert os.path.getsize(OUT) < 1000000
    if "--write-header" in sys.argv:
        src = open(HEADER).read()
        new, n = re.subn(r"differ by at most [0-9.e+-]+ \([0-9.]+ ulp of torch's value\)", f"differ by at most {sig_abs:.6e} ({sig_ulp:.3f} ulp of torch's value)", src)
        assert n == 1, "the sentence on the measured difference is not in the header"
        open(HEADER, "w").write(new)
        print(f"{HEADER}: updated")


if __name__ == "__main__":
    main()
