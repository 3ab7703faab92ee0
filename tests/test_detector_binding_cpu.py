"""The detector binding's refusals, pinned on the CPU against a table recorded from the commit before the binding moved into instancefusion_amd/detector.py.

Every argument check of the twelve detector operators of ElasticFusion and of the two *_image functions runs before the GPU is touched, and torch.device("cuda", 0)
can be made without one.  So the operators run here on a handle that never called ifx_create, with CPU tensors and with tensors that only report the handle's
device (a Tensor subclass; none of them reaches a kernel), and a stand-in for the stream.  Each case holds one fault; (exception type, message) must be the
table's, tests/golden/detector_binding_refusals.json.

The table is a record, never an output of the code under test.  It was written once by running this file as a program with the parent commit's package on the
import path:

    git worktree add ../parent <parent commit>
    PYTHONPATH=../parent python tests/test_detector_binding_cpu.py > tests/golden/detector_binding_refusals.json

(libifx.so is needed only by the `out` cases of the two *_image functions, for the host-only size rules.)  A case added later is recorded the same way, from a
commit whose wording is trusted."""
import json
import os
import re
import subprocess
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TABLE = os.path.join(ROOT, "tests", "golden", "detector_binding_refusals.json")
if __name__ == "__main__":
    sys.path.append(ROOT)      # (behind PYTHONPATH: the package recorded is the one the caller put first)

import instancefusion_amd as m  # noqa: E402

F32, I32, I64, U8 = torch.float32, torch.int32, torch.int64, torch.uint8
STREAM = types.SimpleNamespace(cuda_stream=0)      # given to every call, so that none asks torch for the current stream


class OnDevice(torch.Tensor):
    """a CPU tensor that reports the handle's device: it passes the device check, so the checks behind it are reached"""
    device = property(lambda self: torch.device("cuda", 0))


def dev(shape, dtype=F32):
    return torch.zeros(shape, dtype=dtype).as_subclass(OnDevice)


def handle():
    ef = object.__new__(m.ElasticFusion)     # no ifx_create: the checks read cfgd["device"] only
    ef.cfgd = {"device": 0}
    return ef


def image_handle():
    ef = handle()
    ef.L = m.lib()                           # detector_input_image asks the host-only ifx_detector_input_size before it looks at `out`
    return ef


def faults(t):
    """the single faults of one tensor argument whose good value is t"""
    f = {
        "not a tensor": np.zeros(tuple(t.shape), np.float32),
        "wrong dtype": torch.zeros(tuple(t.shape), dtype=torch.float64),
        "on the cpu": torch.zeros(tuple(t.shape), dtype=t.dtype),
        "wrong shape": dev((3, 3, 3, 3, 3), t.dtype),
    }
    if t.numel() > 1:                        # (one element is contiguous however it is strided)
        f["not contiguous"] = dev(tuple(t.shape) + (2,), t.dtype)[..., 0]
    return f


# name -> (function of (handle, **arguments), the good arguments, the handle's maker); every tensor among the arguments (lists included) gets each fault in turn
def operators():
    E = m.ElasticFusion
    img_out = m.detector_input_size(8, 6, 8)
    S = m.molded_input_size(8, 6, 8, 64)[2]
    pyr = [dev((1, 8 >> l, 8 >> l, 2)) for l in range(4)]
    return {
        "roi_align_forward": (E.roi_align_forward, dict(input=dev((1, 2, 4, 4)), rois=dev((3, 5)), spatial_scale=0.5, pooled_h=2, pooled_w=2, sampling_ratio=2,
                                                        out=dev((3, 2, 2, 2))), handle),
        "fpn_roi_align": (E.fpn_roi_align, dict(features=[dev((1, 2, 8, 8)), dev((1, 2, 4, 4))], rois=dev((3, 5)), scales=(0.25, 0.125), pooled_h=2, pooled_w=2,
                                                sampling_ratio=2, out=dev((3, 2, 2, 2)), levels_out=dev((3,), I32)), handle),
        "nms": (E.nms, dict(boxes=dev((3, 4)), scores=dev((3,)), threshold=0.5, groups=dev((3,), I32)), handle),
        "rpn_proposals": (E.rpn_proposals, dict(objectness=dev((2, 3, 3)), box_regression=dev((8, 3, 3)), anchors=dev((18, 4)), image_size=(32, 32)), handle),
        "rpn_proposals_fpn": (E.rpn_proposals_fpn, dict(objectness=[dev((2, 3, 3)), dev((1, 2, 2, 2))], box_regression=[dev((8, 3, 3)), dev((1, 8, 2, 2))],
                                                        anchors=[dev((18, 4)), dev((8, 4))], image_size=(32, 32)), handle),
        "box_decode": (E.box_decode, dict(codes=dev((3, 8)), boxes=dev((3, 4)), out=dev((3, 8))), handle),
        "box_detections": (E.box_detections, dict(class_logits=dev((3, 4)), box_regression=dev((3, 16)), proposals=dev((3, 4)), image_size=(32, 32)), handle),
        "mask_head_select": (E.mask_head_select, dict(mask_logits=dev((3, 4, 5, 5)), boxes=dev((3, 4)), scores=dev((3,)), labels=dev((3,), I64), in_size=(32, 32),
                                                      out_size=(32, 32), count=dev((1,), I32), class_map=dev((4,), I32)), handle),
        "unmold_detections": (E.unmold_detections, dict(detections=dev((3, 6)), mrcnn_mask=dev((3, 5, 5, 4)), window=(0, 0, 32, 32), out_size=(32, 32),
                                                        class_map=dev((4,), I32)), handle),
        "keras_proposals": (E.keras_proposals, dict(rpn_probs=dev((6, 2)), rpn_bbox=dev((6, 4)), anchors=dev((6, 4)), image_shape=(32, 32), proposal_count=5,
                                                    out=dev((5, 4))), handle),
        "pyramid_roi_align": (E.pyramid_roi_align, dict(features=pyr, boxes=dev((1, 3, 4)), image_shape=(32, 32), pool_shape=(2, 2), out=dev((1, 3, 2, 2, 2)),
                                                        levels_out=dev((1, 3), I32)), handle),
        "keras_detections": (E.keras_detections, dict(rois=dev((3, 4)), probs=dev((3, 4)), deltas=dev((3, 4, 4)), window=(0, 0, 32, 32), image_shape=(32, 32),
                                                      max_instances=5, out=dev((5, 6))), handle),
        "detector_input_image": (m.detector_input_image, dict(rgb=dev((6, 8, 3), U8), min_size=8, out=dev((1, 3, img_out[3], img_out[2]))), image_handle),
        "detector_input_molded_image": (m.detector_input_molded_image, dict(rgb=dev((6, 8, 3), U8), min_dim=8, max_dim=64, out=dev((1, S, S, 3))), image_handle),
    }


# the refusals that are plain Python: name -> (operator, the arguments that replace the good ones)
def plain_refusals():
    return {
        "pyramid_roi_align: three maps": ("pyramid_roi_align", dict(features=[dev((1, 8, 8, 2))] * 3)),
        "pyramid_roi_align: layout hwc": ("pyramid_roi_align", dict(layout="hwc")),
        "pyramid_roi_align: channels differ": ("pyramid_roi_align", dict(features=[dev((1, 8, 8, 2))] * 3 + [dev((1, 1, 1, 3))])),
        "pyramid_roi_align: boxes of two images": ("pyramid_roi_align", dict(boxes=dev((2, 3, 4)))),
        "fpn_roi_align: no features": ("fpn_roi_align", dict(features=[])),
        "fpn_roi_align: three scales": ("fpn_roi_align", dict(scales=(0.25, 0.125, 0.0625))),
        "fpn_roi_align: channels differ": ("fpn_roi_align", dict(features=[dev((1, 2, 8, 8)), dev((1, 3, 4, 4))])),
        "rpn_proposals_fpn: no levels": ("rpn_proposals_fpn", dict(objectness=[], box_regression=[], anchors=[])),
        "rpn_proposals_fpn: one level of anchors": ("rpn_proposals_fpn", dict(anchors=[dev((18, 4))])),
        "rpn_proposals_fpn: one level of box_regression": ("rpn_proposals_fpn", dict(box_regression=[dev((8, 3, 3))])),
        "rpn_proposals: anchors of another grid": ("rpn_proposals", dict(anchors=dev((17, 4)))),
        "rpn_proposals: box_regression of another grid": ("rpn_proposals", dict(box_regression=dev((8, 3, 2)))),
        "nms: scores of another length": ("nms", dict(scores=dev((4,)))),
        "box_decode: codes no multiple of four": ("box_decode", dict(codes=dev((3, 6)))),
        "box_detections: box_regression of two classes": ("box_detections", dict(box_regression=dev((3, 8)))),
        "mask_head_select: M of 65": ("mask_head_select", dict(mask_logits=dev((3, 4, 65, 65)))),
        "mask_head_select: count of two": ("mask_head_select", dict(count=dev((2,), I32))),
        "mask_head_select: class_map of five": ("mask_head_select", dict(class_map=dev((5,), I32))),
        "mask_head_select: NaN threshold": ("mask_head_select", dict(score_thresh=float("nan"))),
        "mask_head_select: empty in_size": ("mask_head_select", dict(in_size=(0, 32))),
        "unmold_detections: layout hwc": ("unmold_detections", dict(layout="hwc")),
        "unmold_detections: one class": ("unmold_detections", dict(mrcnn_mask=dev((3, 5, 5, 1)))),
        "unmold_detections: empty window": ("unmold_detections", dict(window=(0, 0, 0, 32))),
        "unmold_detections: empty out_size": ("unmold_detections", dict(out_size=(32, 0))),
        "unmold_detections: class_map of five": ("unmold_detections", dict(class_map=dev((5,), I32))),
        "keras_proposals: three columns": ("keras_proposals", dict(rpn_probs=dev((6, 3)))),
        "keras_proposals: anchors of another count": ("keras_proposals", dict(anchors=dev((5, 4)))),
        "keras_detections: window of three": ("keras_detections", dict(window=(0, 0, 32))),
        "keras_detections: deltas of another class count": ("keras_detections", dict(deltas=dev((3, 5, 4)))),
        "detector_input_image: two-entry mean": ("detector_input_image", dict(mean=(1.0, 2.0))),
        "detector_input_image: rgb of four channels": ("detector_input_image", dict(rgb=dev((6, 8, 4), U8))),
        "detector_input_molded_image: two-entry mean": ("detector_input_molded_image", dict(mean=(1.0, 2.0))),
        "detector_input_molded_image: out channels first": ("detector_input_molded_image", dict(out=dev((1, 3, 64, 64)))),
    }


def outcome(fn, *args, **kw):
    try:
        fn(*args, **kw)
    except Exception as e:          # (whatever it is: the comparison with the table says whether it is the right one)
        return [type(e).__name__, re.sub(r"np\.int32\((\d+)\)", r"\1", str(e))]    # (numpy 2 names the type of the scalars in a printed list, numpy 1 does not)
    return ["no exception", ""]


def table():
    out = {"detector_prep: two-entry mean": outcome(m.detector_prep, mean=(1.0, 2.0))}
    ops = operators()
    for name, (fn, good, make) in ops.items():
        for arg, value in good.items():
            slots = [(arg, None)] if isinstance(value, torch.Tensor) else [(f"{arg}[{i}]", i) for i in range(len(value))] if isinstance(value, list) else []
            for label, i in slots:
                for fault, bad in faults(value if i is None else value[i]).items():
                    kw = dict(good)
                    kw[arg] = bad if i is None else value[:i] + [bad] + value[i + 1:]
                    out[f"{name}: {label} {fault}"] = outcome(fn, make(), stream=STREAM, **kw)
    for label, (name, change) in plain_refusals().items():
        fn, good, make = ops[name]
        out[label] = outcome(fn, make(), stream=STREAM, **{**good, **change})
    return out


def test_refusals_are_the_recorded_ones():
    with open(TABLE) as f:
        want = json.load(f)
    assert {t for t, _ in want.values()} == {"TypeError", "ValueError"}, "the table holds refusals only: nothing in it reached the GPU runtime"
    got = table()
    assert sorted(got) == sorted(want), "the case list and the table differ: record new cases from a trusted commit, never from the code under test"
    wrong = {k: (got[k], want[k]) for k in want if got[k] != want[k]}
    assert not wrong, "\n".join(f"{k}: {g} instead of {w}" for k, (g, w) in wrong.items())


def test_the_example_of_the_stub_handle():
    """the unbound call on a namespace, as a user without a GPU would try it"""
    assert outcome(m.ElasticFusion.nms, types.SimpleNamespace(cfgd={"device": 0}), None, None, 0.5) == ["TypeError", "boxes must be a torch tensor on the handle's device"]


def test_import_leaves_torch_alone():
    code = "import sys; import instancefusion_amd, instancefusion_amd.sharded; assert 'torch' not in sys.modules, 'the package imported torch'"
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


PUBLIC = """DET_SWAP_RB DET_SCALE_255 UNMOLD_NHWC UNMOLD_NCHW MOLD_NHWC MOLD_NCHW MOLD_MEAN_PIXEL detector_prep detector_input_size detector_resize_taps
detector_input_image molded_input_size detector_input_molded_image fpn_level_thresholds pyramid_level_thresholds detector_ops rpn_post_processor box_post_processor
mask_post_processor pooler IfxError DetectorPrep RpnParams RpnLevel BoxDetParams KerasProposalParams KerasDetectionParams MaskHeadParams ElasticFusion InstanceFusion
lib exported_symbols""".split()
METHODS = """roi_align_forward fpn_roi_align nms rpn_proposals rpn_proposals_fpn box_decode box_detections mask_head_select unmold_detections keras_proposals
pyramid_roi_align keras_detections _mask_head_args _unmold_args""".split()


def test_the_package_still_offers_every_name():
    missing = [n for n in PUBLIC if not hasattr(m, n)] + [f"ElasticFusion.{n}" for n in METHODS if not callable(getattr(m.ElasticFusion, n, None))]
    assert not missing, missing
    assert isinstance(m._SIGS, dict) and sorted(m._SIGS) == m.exported_symbols()
    assert all(getattr(m.ElasticFusion, n).__doc__ for n in METHODS)


if __name__ == "__main__":
    t = table()
    odd = {k: v for k, v in t.items() if v[0] not in ("TypeError", "ValueError")}
    assert not odd, f"not a refusal (the case reached the GPU runtime, or passed): {odd}"
    json.dump(t, sys.stdout, indent=1, sort_keys=True)
    sys.stdout.write("\n")
