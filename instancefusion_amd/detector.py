"""The detector side of the binding: the detector-input calls, the stand-ins for maskrcnn-benchmark's modules and the twelve detector operators of
:class:`ElasticFusion` (_DetectorOperators, which it inherits).  None of them touches map state: caller's tensors, caller's stream.

The package imports this module once IfxError, the ctypes structures, lib() and _ptr exist, and re-exports its names; torch is imported on first use only.
Every operator goes through the same few helpers: _ops_tensor (the argument check), _stream_for (the stream default), _out_like / _empty_on (outputs made on
that stream), _dp / _sp (what the C call receives) and _cut (the padded / cut tail).
"""
from __future__ import annotations

import ctypes as C
import functools

import numpy as np

from . import BoxDetParams, DetectorPrep, IfxError, KerasDetectionParams, KerasProposalParams, MaskHeadParams, RpnLevel, RpnParams, _ptr, lib

# flags of ifx_detector_prep (include/ifx_c_api.h)
DET_SWAP_RB = 1      # output channel c reads source channel 2 - c
DET_SCALE_255 = 2    # ToTensor's [0, 1] back to [0, 255] before the normalisation


# -- the one argument path: pointers, the tensor check, the stream default, outputs, the padded / cut tail
def _dp(t, offset=0):
    """a tensor's device pointer for a C call, `offset` bytes in: NULL for None and for an empty tensor"""
    return None if t is None else C.c_void_p(t.data_ptr() + offset or None)


def _sp(stream):
    """a torch stream's handle for a C call"""
    return C.c_void_p(stream.cuda_stream or None)


def _device(ef):
    import torch

    return torch.device("cuda", int(ef.cfgd["device"]))


def _stream_for(ef, stream):
    """`stream`, or the current stream of the handle's device"""
    import torch

    return torch.cuda.current_stream(_device(ef)) if stream is None else stream


def _ops_tensor(ef, t, name, dtype, what, shape=None, expected=None, folded=False):
    """the argument checks of the detector operators, as detector_input_image's: TypeError for the dtype, ValueError for device / layout / shape.  shape: the
    extents, None for any; expected: how the message spells them (default: the list).  folded: a tensor that is not contiguous is reported with the shape, as
    "expected a contiguous ..." -- the wording of the detector-input calls."""
    import torch

    dev = _device(ef)
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{name} must be a torch tensor on the handle's device")
    if t.dtype != dtype:
        raise TypeError(f"{name}: dtype {t.dtype} is not supported ({what})")
    if t.device != dev:
        raise ValueError(f"{name} is on {t.device}, the handle on {dev}")
    if not folded and not t.is_contiguous():
        raise ValueError(f"{name}: not contiguous")
    if shape is not None and (t.dim() != len(shape) or any(e is not None and int(s) != e for s, e in zip(t.shape, shape)) or (folded and not t.is_contiguous())):
        raise ValueError(f"{name}: shape {tuple(t.shape)}, expected {'a contiguous ' if folded else ''}{list(shape) if expected is None else expected}")
    return t


def _empty_on(stream, dev, *specs):
    """one uninitialised tensor per (shape, dtype), made on `stream`"""
    import torch

    with torch.cuda.stream(stream):
        return [torch.empty(shape, dtype=dtype, device=dev) for shape, dtype in specs]


def _out_like(ef, out, shape, stream, folded=False):
    """the float32 output of an operator: made on `stream`, or the caller's `out` checked"""
    import torch

    if out is None:
        return _empty_on(stream, _device(ef), (shape, torch.float32))[0]
    return _ops_tensor(ef, out, "out", torch.float32, "float32", shape, folded=folded)


def _cut(stream, count, padded, tensors, extra=(), limit=None):
    """the tail of the operators that count their rows on the device.  padded: (*tensors, count, *extra) as they are, no synchronisation.  Otherwise the first
    count rows of each tensor: the 4-byte read of the count on `stream`, the only synchronisation; limit(count) may refuse or clamp it."""
    import torch

    if padded:
        return (*tensors, count, *extra)
    with torch.cuda.stream(stream):
        c = int(count.item())
        if limit is not None:
            c = limit(c)
        return tuple(t[:c] for t in tensors)


def detector_prep(min_size=800, max_size=None, size_divisible=0, mean=(102.9801, 115.9465, 122.7717), std=(1., 1., 1.), to_bgr255=True, swap_rb=False):
    """The ifx_detector_prep of the detector-input calls.  The defaults are maskrcnn-benchmark's (INPUT.MIN_SIZE_TEST, PIXEL_MEAN, PIXEL_STD, TO_BGR255,
    maskrcnn_benchmark/config/defaults.py:47-55; DATALOADER.SIZE_DIVISIBILITY is 0 there and 32 in the FPN configurations).  to_bgr255: multiply ToTensor's [0, 1]
    by 255 (IFX_DET_SCALE_255); swap_rb: output channel c reads source channel 2 - c (IFX_DET_SWAP_RB).  demo/predictor.py:142-145 on the RGB frame the map holds is
    to_bgr255=True, swap_rb=True (BGR x 255, what the released weights expect) or to_bgr255=False, swap_rb=False; max_size None or <= 0: no upper bound."""
    mean = [float(v) for v in mean]
    std = [float(v) for v in std]
    if len(mean) != 3 or len(std) != 3:
        raise ValueError("mean and std have three entries each")
    p = DetectorPrep()
    p.min_size, p.max_size, p.size_divisible = int(min_size), int(max_size) if max_size else 0, int(size_divisible)
    p.flags = (DET_SCALE_255 if to_bgr255 else 0) | (DET_SWAP_RB if swap_rb else 0)
    p.mean[:] = mean
    p.std[:] = std
    return p


def detector_input_size(width, height, min_size=800, max_size=None, size_divisible=0):
    """ifx_detector_input_size (host only, no GPU): (ow, oh, W', H') of a width x height frame -- the resized size by maskrcnn-benchmark's Resize.get_size and the
    size padded to a multiple of size_divisible."""
    out = np.zeros(4, np.int32)
    p = detector_prep(min_size, max_size, size_divisible)
    if lib().ifx_detector_input_size(int(width), int(height), C.byref(p), _ptr(out)) < 0:
        raise IfxError(f"ifx_detector_input_size: refused ({width} x {height}, min_size {min_size}, max_size {max_size}, size_divisible {size_divisible})")
    return tuple(int(v) for v in out)


def detector_resize_taps(in_size, out_size, max_ksize=None):
    """ifx_detector_resize_taps (host only): Pillow's 8-bit bilinear taps of one axis: (first [out], count [out], coeff [out, ksize] int32)"""
    ks = 2 * int(np.ceil(max(in_size / out_size, 1.0))) + 1 if max_ksize is None else int(max_ksize)
    first, count, coeff = np.zeros(out_size, np.int32), np.zeros(out_size, np.int32), np.zeros((out_size, ks), np.int32)
    r = lib().ifx_detector_resize_taps(int(in_size), int(out_size), _ptr(first), _ptr(count), _ptr(coeff), ks)
    if r < 0:
        raise IfxError(f"ifx_detector_resize_taps: refused ({in_size} -> {out_size}, max_ksize {ks})")
    return first, count, coeff.reshape(-1)[:out_size * r].reshape(out_size, r)


def _rgb_image(ef, rgb):
    """the checks of the frame the two *_image calls take: (height, width)"""
    import torch

    _ops_tensor(ef, rgb, "rgb", torch.uint8, "uint8", (None, None, 3), "[H,W,3]", folded=True)
    return int(rgb.shape[0]), int(rgb.shape[1])


def _detector_out(ef, size, out, stream):
    """the output tensor of the detector-input calls ([1,3,H',W'] float32 on the handle's device, made on the consumer's stream) and that stream"""
    stream = _stream_for(ef, stream)
    return _out_like(ef, out, (1, 3, size[3], size[2]), stream, folded=True), stream


def detector_input_image(ef, rgb, min_size=800, max_size=None, size_divisible=0, mean=(102.9801, 115.9465, 122.7717), std=(1., 1., 1.), to_bgr255=True, swap_rb=False,
                         out=None, stream=None):
    """ifx_detector_input_image: InstanceFusion.detector_input's kernel on any uint8 [H,W,3] torch tensor on the handle's device (the stage call).  `rgb` must be
    complete on `stream` (default: the current stream), the consumer's.  Returns (tensor [1,3,H',W'] float32, (oh, ow))."""
    hh, w = _rgb_image(ef, rgb)
    p = detector_prep(min_size, max_size, size_divisible, mean, std, to_bgr255, swap_rb)
    size = np.zeros(4, np.int32)
    if ef.L.ifx_detector_input_size(w, hh, C.byref(p), _ptr(size)) < 0:
        raise IfxError(f"ifx_detector_input_size: refused ({w} x {hh}, min_size {min_size}, max_size {max_size}, size_divisible {size_divisible}, std {tuple(std)})")
    out, stream = _detector_out(ef, size, out, stream)
    ef._chk(ef.L.ifx_detector_input_image(ef.handle, _dp(rgb), w, hh, C.byref(p), _dp(out), int(out.numel()), _sp(stream)), "ifx_detector_input_image")
    return out, (int(size[1]), int(size[0]))


# layouts of ifx_unmold_detections' mrcnn_mask and of ifx_detector_input_molded's output (include/ifx_c_api.h)
UNMOLD_NHWC = 0      # [R,M,M,C], as Keras emits it
UNMOLD_NCHW = 1      # [R,C,M,M], a torch port
MOLD_NHWC = 0        # [S,S,3], Keras
MOLD_NCHW = 1        # [3,S,S]
MOLD_MEAN_PIXEL = (123.7, 116.8, 103.9)   # Config.MEAN_PIXEL (deps/mask_rcnn/config.py)


def molded_input_size(width, height, min_dim=800, max_dim=1024):
    """ifx_molded_input_size (host only, no GPU): (nw, nh, S, S, top, left, top + nh, left + nw) of a width x height frame by utils.resize_image
    (deps/mask_rcnn/utils.py:384-432) with padding; the last four are the window unmold_detections needs."""
    out = np.zeros(8, np.int32)
    if lib().ifx_molded_input_size(int(width), int(height), int(min_dim), int(max_dim), _ptr(out)) < 0:
        raise IfxError(f"ifx_molded_input_size: refused ({width} x {height}, min_dim {min_dim}, max_dim {max_dim})")
    return tuple(int(v) for v in out)


def _molded_args(ef, w, hh, min_dim, max_dim, mean, channels_last, out, stream):
    """what the two molded-input calls share: (size8, mean as double[3], layout, out tensor, stream)"""
    mean = [float(v) for v in mean]
    if len(mean) != 3:
        raise ValueError("mean has three entries")
    size = molded_input_size(w, hh, min_dim, max_dim)
    S = size[2]
    stream = _stream_for(ef, stream)
    out = _out_like(ef, out, (1, S, S, 3) if channels_last else (1, 3, S, S), stream, folded=True)
    return size, (C.c_double * 3)(*mean), MOLD_NHWC if channels_last else MOLD_NCHW, out, stream


def _molded_result(size, out, w, hh, min_dim, max_dim):
    """(tensor, window (y1, x1, y2, x2), scale): the image, and what utils.resize_image returns beside it (the scale by its own two statements, utils.py:409-416)"""
    scale = max(1, min_dim / min(hh, w)) if min_dim else 1
    if round(max(hh, w) * scale) > max_dim:
        scale = max_dim / max(hh, w)
    return out, tuple(size[4:8]), scale


def detector_input_molded_image(ef, rgb, min_dim=800, max_dim=1024, mean=MOLD_MEAN_PIXEL, channels_last=True, out=None, stream=None):
    """ifx_detector_input_molded_image: InstanceFusion.detector_input_molded's kernel on any uint8 [H,W,3] torch tensor on the handle's device (the stage call);
    `rgb` must be complete on `stream` (default: the current stream), the consumer's.  Returns (tensor [1,S,S,3] or [1,3,S,S] float32, window (y1, x1, y2, x2), scale)."""
    hh, w = _rgb_image(ef, rgb)
    size, mean3, layout, out, stream = _molded_args(ef, w, hh, min_dim, max_dim, mean, channels_last, out, stream)
    ef._chk(ef.L.ifx_detector_input_molded_image(ef.handle, _dp(rgb), w, hh, int(min_dim), int(max_dim), mean3, layout, _dp(out), int(out.numel()), _sp(stream)),
            "ifx_detector_input_molded_image")
    return _molded_result(size, out, w, hh, int(min_dim), int(max_dim))


class _DetectorOps:
    """What detector_ops() returns: the two inference operators of maskrcnn_benchmark._C on this library's kernels, in _C's argument order."""
    def __init__(self, ef):
        self.ef = ef

    def nms(self, dets, scores, threshold):
        return self.ef.nms(dets, scores, threshold)

    def roi_align_forward(self, input, rois, spatial_scale, pooled_h, pooled_w, sampling_ratio):
        return self.ef.roi_align_forward(input, rois, spatial_scale, pooled_h, pooled_w, sampling_ratio)

    def __getattr__(self, name):
        if name.startswith(("roi_", "sigmoid_focal_loss_")):     # roi_align_backward, roi_pool_*, sigmoid_focal_loss_*: the rest of _C
            def refuse(*a, **k):
                raise NotImplementedError(f"{name}: this library provides the detector's operators for inference only (nms, roi_align_forward)")
            return refuse
        raise AttributeError(name)


@functools.lru_cache(maxsize=None)
def _rpn_post_processor_class():
    """the nn.Module behind rpn_post_processor, made on first use: the package imports torch lazily"""
    import torch

    class RpnPostProcessor(torch.nn.Module):
        def __init__(self, ef, pre_nms_top_n, post_nms_top_n, nms_thresh, min_size, fpn_post_nms_top_n):
            super().__init__()
            self.ef = ef
            self.pre_nms_top_n, self.post_nms_top_n, self.nms_thresh, self.min_size = int(pre_nms_top_n), int(post_nms_top_n), float(nms_thresh), float(min_size)
            self.fpn_post_nms_top_n = self.post_nms_top_n if fpn_post_nms_top_n is None else int(fpn_post_nms_top_n)

        def forward(self, anchors, objectness, box_regression, targets=None):
            if self.training:
                raise RuntimeError("rpn_post_processor: inference only (the module is in training mode)")
            out = []
            for img, per_level in enumerate(anchors):
                if len(per_level) == 1:
                    boxes, scores, _ = self.ef.rpn_proposals(objectness[0][img], box_regression[0][img], per_level[0].bbox.contiguous(), per_level[0].size,
                                                             self.pre_nms_top_n, self.post_nms_top_n, self.nms_thresh, self.min_size)
                else:
                    boxes, scores, _, _ = self.ef.rpn_proposals_fpn([o[img] for o in objectness], [b[img] for b in box_regression],
                                                                    [a.bbox.contiguous() for a in per_level], per_level[0].size, self.pre_nms_top_n,
                                                                    self.post_nms_top_n, self.nms_thresh, self.min_size, self.fpn_post_nms_top_n)
                r = type(per_level[0])(boxes, per_level[0].size, mode="xyxy")
                r.add_field("objectness", scores)
                out.append(r)
            return out

    return RpnPostProcessor


def rpn_post_processor(ef, pre_nms_top_n, post_nms_top_n, nms_thresh, min_size, fpn_post_nms_top_n=None):
    """An nn.Module that stands in for maskrcnn-benchmark's RPNPostProcessor (modeling/rpn/inference.py) at inference time: forward(anchors, objectness,
    box_regression, targets=None) with anchors a list (per image) of lists (per level) of box lists, objectness / box_regression lists (per level) of [N,A,H,W] /
    [N,4A,H,W], makes one call per image -- ElasticFusion.rpn_proposals for one level, ElasticFusion.rpn_proposals_fpn for several -- and returns one box list
    per image with the field "objectness".  The result is built with the class of the anchor lists it is given -- type(anchors[0][0])(bbox, size, mode="xyxy")
    and add_field -- so nothing of the reference is imported.  Several levels: the best fpn_post_nms_top_n (default: post_nms_top_n) of an image over all its
    levels, selected on the device by the rule of include/ifx_c_api.h (select_over_all_levels when not training; equal logits by level, then by row).  Box
    weights are RPNPostProcessor's default (1, 1, 1, 1).  It raises in training mode."""
    return _rpn_post_processor_class()(ef, pre_nms_top_n, post_nms_top_n, nms_thresh, min_size, fpn_post_nms_top_n)


@functools.lru_cache(maxsize=None)
def _box_post_processor_class():
    """the nn.Module behind box_post_processor, made on first use: the package imports torch lazily"""
    import torch

    class PostProcessor(torch.nn.Module):
        def __init__(self, ef, score_thresh, nms, detections_per_img, weights, cls_agnostic_bbox_reg):
            super().__init__()
            self.ef = ef
            self.score_thresh, self.nms, self.detections_per_img = float(score_thresh), float(nms), int(detections_per_img)
            self.weights, self.cls_agnostic_bbox_reg = tuple(float(v) for v in weights), bool(cls_agnostic_bbox_reg)

        def forward(self, x, boxes):
            if self.training:
                raise RuntimeError("box_post_processor: inference only (the module is in training mode)")
            class_logits, box_regression = x
            if self.cls_agnostic_bbox_reg:
                box_regression = box_regression[:, -4:]
            out, first = [], 0
            for box in boxes:
                rows = slice(first, first + len(box))
                first += len(box)
                b, s, l, _ = self.ef.box_detections(class_logits[rows].contiguous(), box_regression[rows].contiguous(), box.bbox.contiguous(), box.size,
                                                    self.score_thresh, self.nms, self.detections_per_img, self.weights)
                r = type(box)(b, box.size, mode="xyxy")
                r.add_field("scores", s)
                r.add_field("labels", l)
                out.append(r)
            return out

    return PostProcessor


def box_post_processor(ef, score_thresh, nms, detections_per_img, weights=(10, 10, 5, 5), cls_agnostic_bbox_reg=False):
    """An nn.Module that stands in for maskrcnn-benchmark's box-head PostProcessor (modeling/roi_heads/box_head/inference.py) at inference time:
    forward((class_logits, box_regression), boxes) with class_logits [sum R, C], box_regression [sum R, 4C] and boxes a list of box lists, one per image, splits the
    rows by len(box), makes one ElasticFusion.box_detections call per image and returns one box list per image in mode "xyxy" with the image's size and the fields
    "scores" and "labels" (int64).  The result is built with the class of the box lists it is given -- type(boxes[0])(bbox, size, mode="xyxy") and add_field -- so
    nothing of the reference is imported.  cls_agnostic_bbox_reg: the last four columns of box_regression are every class's code.  It raises in training mode."""
    return _box_post_processor_class()(ef, score_thresh, nms, detections_per_img, weights, cls_agnostic_bbox_reg)


@functools.lru_cache(maxsize=None)
def _mask_post_processor_class():
    """the nn.Module behind mask_post_processor, made on first use: the package imports torch lazily"""
    import torch

    class MaskPostProcessor(torch.nn.Module):
        def __init__(self, ef):
            super().__init__()
            self.ef = ef
            self.masker = None

        def forward(self, x, boxes):
            out, first = [], 0
            for box in boxes:
                n = len(box)
                rows = slice(first, first + n)
                first += n
                labels = box.get_field("labels")
                scores = torch.zeros(n, dtype=torch.float32, device=x.device)      # (score_thresh = -inf: the scores are not examined)
                masks, _, _, _, _ = self.ef.mask_head_select(x[rows].contiguous(), box.bbox.contiguous(), scores, labels.to(torch.int64).contiguous(), box.size, box.size,
                                                                score_thresh=float("-inf"), sort_by_score=False, padded=True)
                r = type(box)(box.bbox, box.size, mode="xyxy")
                for field in box.fields():
                    r.add_field(field, box.get_field(field))
                r.add_field("mask", masks[:, None])
                out.append(r)
            return out

    return MaskPostProcessor


def mask_post_processor(ef):
    """An nn.Module that stands in for maskrcnn-benchmark's MaskPostProcessor (modeling/roi_heads/mask_head/inference.py) with masker=None: forward(x, boxes) with
    x the mask logits [sum R, C, M, M] and boxes a list of box lists with the field "labels", one per image, splits the rows by len(box), makes one
    ElasticFusion.mask_head_select call per image (score_thresh=-inf, no sort, out_size == in_size: every row in its own place, nothing read back) and returns one
    box list per image with the given boxes, every field copied and the field "mask" [n,1,M,M]: the sigmoid of each row's own channel by the rule of
    include/ifx_c_api.h.  A row whose label is outside 0 .. C - 1 -- the reference raises there -- leaves the rows behind it one place up and zeros at the end.
    The result is built with the class of the box lists it is given, as box_post_processor does, so nothing of the reference is imported."""
    return _mask_post_processor_class()(ef)


@functools.lru_cache(maxsize=None)
def _pooler_class():
    """the nn.Module behind pooler, made on first use: the package imports torch lazily"""
    import torch

    class Pooler(torch.nn.Module):
        def __init__(self, ef, output_size, scales, sampling_ratio):
            super().__init__()
            self.ef = ef
            self.output_size = (int(output_size), int(output_size)) if isinstance(output_size, int) else (int(output_size[0]), int(output_size[1]))
            self.scales, self.sampling_ratio = tuple(float(s) for s in scales), int(sampling_ratio)

        def convert_to_roi_format(self, boxes):
            bbox = [b.bbox for b in boxes]
            ids = [torch.full((len(b), 1), i, dtype=b.bbox.dtype, device=b.bbox.device) for i, b in enumerate(boxes)]
            return torch.cat([torch.cat(ids, dim=0), torch.cat(bbox, dim=0)], dim=1)

        def forward(self, x, boxes):
            rois = self.convert_to_roi_format(boxes)
            return self.ef.fpn_roi_align([f.contiguous() for f in x], rois, self.scales, self.output_size[0], self.output_size[1], self.sampling_ratio)

    return Pooler


def pooler(ef, output_size, scales, sampling_ratio):
    """An nn.Module that stands in for maskrcnn-benchmark's Pooler (modeling/poolers.py) at inference time: forward(x, boxes) with x a list (per level) of
    [N,C,H_l,W_l] feature maps and boxes a list (per image) of box lists does convert_to_roi_format (the image's position in the list as the batch index in front of
    .bbox) and ONE ElasticFusion.fpn_roi_align call -- LevelMapper with its defaults (224, 4, 1e-6) and ROIAlign on the chosen level -- and returns
    [sum R, C, output_size[0], output_size[1]].  The box lists are duck-typed (.bbox, len), so nothing of the reference is imported.  scales must be the ladder
    2^-k_min, 2^-(k_min + 1), ... the Pooler itself assumes."""
    return _pooler_class()(ef, output_size, scales, sampling_ratio)


def fpn_level_thresholds(scales, canonical_level=4):
    """ifx_fpn_level_thresholds (host only, no GPU): (k_min, T) with T[j - 1] the smallest float32 v = sqrt(area) / canonical_scale + eps that ifx_fpn_roi_align
    maps to level j, j = 1 .. len(scales) - 1."""
    sc = np.ascontiguousarray(scales, np.float32).reshape(-1)
    out = np.zeros(max(sc.size - 1, 0), np.float32)
    r = lib().ifx_fpn_level_thresholds(_ptr(sc), int(sc.size), int(canonical_level), _ptr(np.zeros(1, np.float32)) if out.size == 0 else _ptr(out))
    if r < 0:
        raise IfxError(f"ifx_fpn_level_thresholds: refused (scales {[float(v) for v in sc]})")
    return r, out


def pyramid_level_thresholds(image_h, image_w):
    """ifx_pyramid_level_thresholds (host only, no GPU): float32 [3], T0, T1, T2 of ifx_pyramid_roi_align's level rule, level = 2 + (s > T0) + (s >= T1) +
    (s > T2) for s = sqrt(h * w) of a normalised box."""
    out = np.zeros(3, np.float32)
    if lib().ifx_pyramid_level_thresholds(int(image_h), int(image_w), _ptr(out)) < 0:
        raise IfxError(f"ifx_pyramid_level_thresholds: refused (image {image_h} x {image_w})")
    return out


def detector_ops(ef):
    """An object that stands in for maskrcnn_benchmark._C at inference time: nms(dets, scores, threshold) and roi_align_forward(input, rois, spatial_scale,
    pooled_h, pooled_w, sampling_ratio) run ifx_nms / ifx_roi_align_forward on `ef`'s device and the current stream; every other _C name (roi_align_backward,
    roi_pool_*, sigmoid_focal_loss_*) raises NotImplementedError."""
    return _DetectorOps(ef)


def _rpn_level(ef, o, r, a, at=""):
    """the checks of one level of the proposal stage, objectness [A,H,W] / box_regression [4A,H,W] (each with or without a leading 1) / anchors [H*W*A,4]:
    (objectness and box_regression without the leading 1, A, H, W).  at: "[l]" behind the names in the messages."""
    import torch

    for name, t in (("objectness", o), ("box_regression", r), ("anchors", a)):
        _ops_tensor(ef, t, name + at, torch.float32, "float32")
    if o.dim() == 4 and o.shape[0] == 1:
        o = o[0]
    if r.dim() == 4 and r.shape[0] == 1:
        r = r[0]
    if o.dim() != 3:
        raise ValueError(f"objectness{at}: shape {tuple(o.shape)}, expected [A,H,W] or [1,A,H,W]")
    A, H, W = (int(v) for v in o.shape)
    if tuple(r.shape) != (4 * A, H, W):
        raise ValueError(f"box_regression{at}: shape {tuple(r.shape)}, expected [{4 * A},{H},{W}]")
    if tuple(a.shape) != (A * H * W, 4):
        raise ValueError(f"anchors{at}: shape {tuple(a.shape)}, expected [{A * H * W},4]")
    return o, r, A, H, W


def _rpn_params(pre_nms_top_n, post_nms_top_n, nms_thresh, min_size, weights, image_size):
    p = RpnParams()
    p.pre_nms_top_n, p.post_nms_top_n, p.nms_thresh, p.min_size = int(pre_nms_top_n), int(post_nms_top_n), float(nms_thresh), float(min_size)
    p.weights[:] = [float(v) for v in weights]
    p.xform_clip = 0.0
    p.image_w, p.image_h = int(image_size[0]), int(image_size[1])
    return p


def _rpn_result(stream, count, padded, tensors, extra=()):
    """_cut for the proposal stage, whose second tensor holds logits: their torch.sigmoid, of the rows returned, on `stream`"""
    import torch

    boxes, logits, *rest = _cut(stream, count, padded, tensors, extra)
    with torch.cuda.stream(stream):
        return (boxes, torch.sigmoid(logits), *rest)


class _DetectorOperators:
    """The detector's operators as methods of ElasticFusion, which inherits this class: they use the handle (self.handle, self.L, self._chk, self.cfgd) and no
    frame or map state."""

    # -- maskrcnn_benchmark._C.roi_align_forward / _C.nms
    def roi_align_forward(self, input, rois, spatial_scale, pooled_h, pooled_w, sampling_ratio, out=None, stream=None):
        """ifx_roi_align_forward: input [B,C,H,W] float32, rois [n,5] float32 (batch index, x0, y0, x1, y1) -> [n,C,pooled_h,pooled_w] float32, bit for bit the
        rule of include/ifx_c_api.h.  Enqueue-only on `stream` (default: the current stream)."""
        import torch

        _ops_tensor(self, input, "input", torch.float32, "float32", (None,) * 4, "[B,C,H,W]")
        _ops_tensor(self, rois, "rois", torch.float32, "float32", (None, 5), "[n,5]")
        B, Cn, H, W = (int(v) for v in input.shape)
        n, ph, pw = int(rois.shape[0]), int(pooled_h), int(pooled_w)
        stream = _stream_for(self, stream)
        out = _out_like(self, out, (n, Cn, max(ph, 0), max(pw, 0)), stream)
        self._chk(self.L.ifx_roi_align_forward(self.handle, _dp(input), B, Cn, H, W, _dp(rois), n, float(spatial_scale), ph, pw, int(sampling_ratio), _dp(out),
                                               _sp(stream)), "ifx_roi_align_forward")
        return out

    def fpn_roi_align(self, features, rois, scales, pooled_h, pooled_w, sampling_ratio, canonical_scale=224, canonical_level=4, eps=1e-6, out=None, levels_out=None,
                      stream=None):
        """ifx_fpn_roi_align, the FPN Pooler in one launch: features a list of contiguous [B,C,H_l,W_l] float32 maps, rois [n,5] float32 (batch index, x0, y0, x1,
        y1), scales[l] == 2^-(k_min + l) -> [n,C,pooled_h,pooled_w] float32: every ROI pooled from the level LevelMapper gives it, bit for bit the rule of
        include/ifx_c_api.h.  levels_out: an int32 [n] tensor that receives each ROI's level index (-1: no level, a row of zeros).  Enqueue-only on `stream`
        (default: the current stream)."""
        import torch

        features = list(features)
        if not features:
            raise ValueError("features: an empty list")
        for l, f in enumerate(features):
            _ops_tensor(self, f, f"features[{l}]", torch.float32, "float32", (None,) * 4, "[B,C,H,W]")
            if tuple(f.shape[:2]) != tuple(features[0].shape[:2]):
                raise ValueError(f"features[{l}]: shape {tuple(f.shape)}, expected the batch and channels of features[0], {list(features[0].shape[:2])}")
        _ops_tensor(self, rois, "rois", torch.float32, "float32", (None, 5), "[n,5]")
        scales = [float(s) for s in scales]
        if len(scales) != len(features):
            raise ValueError(f"scales: {len(scales)} entries for {len(features)} feature maps")
        nl = len(features)
        B, Cn = int(features[0].shape[0]), int(features[0].shape[1])
        n, ph, pw = int(rois.shape[0]), int(pooled_h), int(pooled_w)
        stream = _stream_for(self, stream)
        out = _out_like(self, out, (n, Cn, max(ph, 0), max(pw, 0)), stream)
        if levels_out is not None:
            _ops_tensor(self, levels_out, "levels_out", torch.int32, "int32", (n,), f"[{n}]")
        ptrs = (C.c_void_p * nl)(*[f.data_ptr() for f in features])
        hs = (C.c_int32 * nl)(*[int(f.shape[2]) for f in features])
        ws = (C.c_int32 * nl)(*[int(f.shape[3]) for f in features])
        sc = (C.c_float * nl)(*scales)
        self._chk(self.L.ifx_fpn_roi_align(self.handle, ptrs, hs, ws, sc, nl, B, Cn, _dp(rois), n, float(canonical_scale), int(canonical_level), float(eps), ph, pw,
                                           int(sampling_ratio), _dp(out), _dp(levels_out), _sp(stream)), "ifx_fpn_roi_align")
        return out

    def nms(self, boxes, scores, threshold, groups=None, stream=None, padded=False):
        """ifx_nms: boxes [n,4] float32 (x0, y0, x1, y1), scores [n] float32, groups None or [n] int32 -> the kept indices, ascending (int64 tensor); a box
        suppresses the later boxes of its own group whose IoU is > threshold.  Order, pair mask and reduction run on the device; the 4-byte read of the count is
        this method's only synchronisation, and padded=True returns (keep [n] with -1 behind the kept indices, count [1] int32) without it."""
        import torch

        _ops_tensor(self, boxes, "boxes", torch.float32, "float32", (None, 4), "[n,4]")
        n = int(boxes.shape[0])
        _ops_tensor(self, scores, "scores", torch.float32, "float32", (n,), f"[{n}]")
        if groups is not None:
            _ops_tensor(self, groups, "groups", torch.int32, "int32", (n,), f"[{n}]")
        stream = _stream_for(self, stream)
        keep, count = _empty_on(stream, _device(self), ((n,), torch.int64), ((1,), torch.int32))
        self._chk(self.L.ifx_nms(self.handle, _dp(boxes), _dp(scores), _dp(groups), n, float(threshold), _dp(keep), _dp(count), _sp(stream)), "ifx_nms")
        r = _cut(stream, count, padded, (keep,))
        return r if padded else r[0]

    # -- the RPN's proposal stage and box decoding (RPNPostProcessor.forward_for_single_feature_map / BoxCoder.decode): caller's tensors, caller's stream
    def rpn_proposals(self, objectness, box_regression, anchors, image_size, pre_nms_top_n=6000, post_nms_top_n=1000, nms_thresh=0.7, min_size=0, weights=(1, 1, 1, 1),
                      padded=False, stream=None):
        """ifx_rpn_proposals, one level of one image: objectness [A,H,W] (or [1,A,H,W]), box_regression [4A,H,W] (or [1,4A,H,W]), anchors [H*W*A,4] in the
        reference's order, image_size (width, height) -> (boxes [c,4], objectness [c], index [c] int64): the proposals in descending objectness, torch.sigmoid of
        their logits, and their flat anchor indices, by the rule of include/ifx_c_api.h.  Everything runs on the device; the 4-byte read of the count is this
        method's only synchronisation, and padded=True returns the uncut [post_nms_top_n] tensors and a fourth value count [1] int32 without it."""
        import torch

        objectness, box_regression, A, H, W = _rpn_level(self, objectness, box_regression, anchors)
        p = _rpn_params(pre_nms_top_n, post_nms_top_n, nms_thresh, min_size, weights, image_size)
        post = max(p.post_nms_top_n, 0)
        stream = _stream_for(self, stream)
        boxes, logits, index, count = _empty_on(stream, _device(self), ((post, 4), torch.float32), ((post,), torch.float32), ((post,), torch.int64), ((1,), torch.int32))
        self._chk(self.L.ifx_rpn_proposals(self.handle, _dp(objectness), _dp(box_regression), _dp(anchors), A, H, W, C.byref(p), _dp(boxes), _dp(logits), _dp(index),
                                           _dp(count), _sp(stream)), "ifx_rpn_proposals")
        return _rpn_result(stream, count, padded, (boxes, logits, index))

    def rpn_proposals_fpn(self, objectness, box_regression, anchors, image_size, pre_nms_top_n=1000, post_nms_top_n=1000, nms_thresh=0.7, min_size=0,
                          fpn_post_nms_top_n=None, weights=(1, 1, 1, 1), padded=False, stream=None):
        """ifx_rpn_proposals_fpn, all levels of one image: objectness, box_regression and anchors are lists with one entry per level, each entry shaped as
        rpn_proposals' argument ([A,H,W] or [1,A,H,W], [4A,H,W] or [1,4A,H,W], [H*W*A,4]); image_size (width, height) -> (boxes [c,4], objectness [c], level [c]
        int32, index [c] int64): per level what rpn_proposals gives, then the best fpn_post_nms_top_n (None: post_nms_top_n) over all levels in descending
        objectness, torch.sigmoid of their logits, each one's level and its flat anchor index inside that level, by the rule of include/ifx_c_api.h.  One memset
        and at most nine launches whatever the number of levels; the 4-byte read of the count is this method's only synchronisation, and padded=True returns the
        uncut [fpn_post_nms_top_n] tensors and count [1] int32, level_counts [L] int32 (the proposals each level contributed to the selection) without it."""
        import torch

        objectness, box_regression, anchors = list(objectness), list(box_regression), list(anchors)
        nl = len(objectness)
        if nl == 0:
            raise ValueError("objectness: an empty list")
        if len(box_regression) != nl or len(anchors) != nl:
            raise ValueError(f"{nl} levels of objectness, {len(box_regression)} of box_regression, {len(anchors)} of anchors")
        lv = (RpnLevel * nl)()
        for l in range(nl):
            o, r, A, H, W = _rpn_level(self, objectness[l], box_regression[l], anchors[l], f"[{l}]")
            lv[l].objectness, lv[l].regression, lv[l].anchors = o.data_ptr() or None, r.data_ptr() or None, anchors[l].data_ptr() or None
            lv[l].A, lv[l].H, lv[l].W = A, H, W
        p = _rpn_params(pre_nms_top_n, post_nms_top_n, nms_thresh, min_size, weights, image_size)
        F = p.post_nms_top_n if fpn_post_nms_top_n is None else int(fpn_post_nms_top_n)
        rows = max(F, 0)
        stream = _stream_for(self, stream)
        boxes, logits, level, index, count, level_counts = _empty_on(stream, _device(self), ((rows, 4), torch.float32), ((rows,), torch.float32), ((rows,), torch.int32),
                                                                     ((rows,), torch.int64), ((1,), torch.int32), ((nl,), torch.int32))
        self._chk(self.L.ifx_rpn_proposals_fpn(self.handle, lv, nl, C.byref(p), F, _dp(boxes), _dp(logits), _dp(level), _dp(index), _dp(count), _dp(level_counts),
                                               _sp(stream)), "ifx_rpn_proposals_fpn")
        return _rpn_result(stream, count, padded, (boxes, logits, level, index), (level_counts,))

    def box_decode(self, codes, boxes, weights=(1, 1, 1, 1), clip_to=None, out=None, stream=None):
        """ifx_box_decode: codes [n,4k] float32 against boxes [n,4] float32 -> [n,4k] float32, BoxCoder.decode by the rule of include/ifx_c_api.h (k = 81 and
        weights (10, 10, 5, 5): the box head).  clip_to (width, height): BoxList.clip_to_image on top.  Enqueue-only on `stream` (default: the current stream)."""
        import torch

        _ops_tensor(self, codes, "codes", torch.float32, "float32")
        _ops_tensor(self, boxes, "boxes", torch.float32, "float32", (None, 4), "[n,4]")
        n = int(boxes.shape[0])
        if codes.dim() != 2 or int(codes.shape[0]) != n or codes.shape[1] % 4 or codes.shape[1] == 0:
            raise ValueError(f"codes: shape {tuple(codes.shape)}, expected [{n},4k]")
        stream = _stream_for(self, stream)
        out = _out_like(self, out, tuple(codes.shape), stream)
        w = (C.c_float * 4)(*[float(v) for v in weights])
        cw, ch = (0, 0) if clip_to is None else (int(clip_to[0]), int(clip_to[1]))
        self._chk(self.L.ifx_box_decode(self.handle, _dp(codes), _dp(boxes), n, int(codes.shape[1]) // 4, C.byref(w), 0.0, cw, ch, _dp(out), _sp(stream)), "ifx_box_decode")
        return out

    # -- the box head's post-processing (PostProcessor.forward / filter_results): caller's tensors, caller's stream
    def box_detections(self, class_logits, box_regression, proposals, image_size, score_thresh=0.05, nms=0.5, detections_per_img=100, weights=(10, 10, 5, 5),
                       max_out=None, padded=False, stream=None):
        """ifx_box_detections, one image: class_logits [R,C], box_regression [R,4C] (or [R,4]: one class-agnostic code per row), proposals [R,4], image_size
        (width, height) -> (boxes [c,4], scores [c], labels [c] int64, index [c] int64): the detections in class-major order, their softmax probabilities, classes
        and proposal rows, by the rule of include/ifx_c_api.h.  Everything runs on the device; the 4-byte read of the count is this method's only synchronisation,
        and padded=True returns the uncut [max_out] tensors plus count [1] int32 and stats [2] int32 (K candidates, D kept) without it.  max_out defaults to
        detections_per_img when that is > 0, else 8192; ties at the limit beyond max_out are counted, not written.  More than 8192 candidates: IfxError in the cut
        form, count -1 in the padded form (raise score_thresh)."""
        import torch

        _ops_tensor(self, class_logits, "class_logits", torch.float32, "float32", (None, None), "[R,C]")
        _ops_tensor(self, box_regression, "box_regression", torch.float32, "float32")
        R, Cn = (int(v) for v in class_logits.shape)
        if box_regression.dim() != 2 or int(box_regression.shape[0]) != R or int(box_regression.shape[1]) not in (4, 4 * Cn):
            raise ValueError(f"box_regression: shape {tuple(box_regression.shape)}, expected [{R},{4 * Cn}] or [{R},4]")
        _ops_tensor(self, proposals, "proposals", torch.float32, "float32", (R, 4), f"[{R},4]")
        p = BoxDetParams()
        p.score_thresh, p.nms, p.detections_per_img = float(score_thresh), float(nms), int(detections_per_img)
        p.max_out = int(max_out) if max_out is not None else (p.detections_per_img if p.detections_per_img > 0 else 8192)
        p.weights[:] = [float(v) for v in weights]
        p.xform_clip = 0.0
        p.image_w, p.image_h = int(image_size[0]), int(image_size[1])
        rows = max(p.max_out, 0)
        stream = _stream_for(self, stream)
        boxes, scores, labels, index, count, stats = _empty_on(stream, _device(self), ((rows, 4), torch.float32), ((rows,), torch.float32), ((rows,), torch.int64),
                                                               ((rows,), torch.int64), ((1,), torch.int32), ((2,), torch.int32))
        self._chk(self.L.ifx_box_detections(self.handle, _dp(class_logits), _dp(box_regression), _dp(proposals), R, Cn, int(box_regression.shape[1]) // 4, C.byref(p),
                                            _dp(boxes), _dp(scores), _dp(labels), _dp(index), _dp(count), _dp(stats), _sp(stream)), "ifx_box_detections")

        def limit(c):
            if c < 0:
                raise IfxError(f"ifx_box_detections: {int(stats[0].item())} candidates, above the cap of 8192: raise score_thresh")
            return min(c, rows)

        return _cut(stream, count, padded, (boxes, scores, labels, index), (stats,), limit)

    # -- the mask head's logits to ROI masks, resized boxes and class ids (MaskPostProcessor.forward, BoxList.resize, select_top_predictions)
    def _mask_head_args(self, mask_logits, boxes, scores, labels, in_size, out_size, score_thresh, sort_by_score, count, class_map, stream):
        """validates the mask head's tensors and parameters: (R, C, M, ifx_mask_head_params, stream)"""
        import torch

        _ops_tensor(self, mask_logits, "mask_logits", torch.float32, "float32")
        if mask_logits.dim() != 4 or mask_logits.shape[2] != mask_logits.shape[3]:
            raise ValueError(f"mask_logits: shape {tuple(mask_logits.shape)}, expected [R,C,M,M]")
        R, Cn, M = int(mask_logits.shape[0]), int(mask_logits.shape[1]), int(mask_logits.shape[3])
        if not (1 <= M <= 64 and 1 <= Cn <= 1024 and R <= 1024):
            raise ValueError(f"mask_logits: shape {tuple(mask_logits.shape)}, expected R <= 1024, C in 1 .. 1024, M in 1 .. 64")
        _ops_tensor(self, boxes, "boxes", torch.float32, "float32", (R, 4), f"[{R},4]")
        _ops_tensor(self, scores, "scores", torch.float32, "float32", (R,), f"[{R}]")
        _ops_tensor(self, labels, "labels", torch.int64, "int64, as box_detections returns them", (R,), f"[{R}]")
        if count is not None:
            _ops_tensor(self, count, "count", torch.int32, "int32, as box_detections(padded=True) returns it")
            if int(count.numel()) != 1:
                raise ValueError(f"count: shape {tuple(count.shape)}, expected one element")
        if class_map is not None:
            _ops_tensor(self, class_map, "class_map", torch.int32, "int32", (Cn,), f"[{Cn}]")
        p = MaskHeadParams()
        p.score_thresh = float(score_thresh)
        if p.score_thresh != p.score_thresh:
            raise ValueError("score_thresh is NaN")
        p.in_w, p.in_h, p.out_w, p.out_h = int(in_size[0]), int(in_size[1]), int(out_size[0]), int(out_size[1])
        if min(p.in_w, p.in_h, p.out_w, p.out_h) < 1:
            raise ValueError(f"in_size {tuple(in_size)}, out_size {tuple(out_size)}: a size < 1")
        p.sort_by_score = 1 if sort_by_score else 0
        return R, Cn, M, p, _stream_for(self, stream)

    def mask_head_select(self, mask_logits, boxes, scores, labels, in_size, out_size, score_thresh=0.7, sort_by_score=True, count=None, class_map=None, padded=False,
                         stream=None):
        """ifx_mask_head_select, one image: mask_logits [R,C,M,M], boxes [R,4] in the coordinates of in_size = (width, height), scores [R], labels [R] int64 ->
        (roi_masks [k,M,M] probabilities of each kept row's own channel, boxes [k,4] resized to out_size, class_ids [k] int32, rows [k] int32): the rows with
        score > score_thresh and a label in 0 .. C - 1, by descending score (sort_by_score) or in their own order, by the rule of include/ifx_c_api.h.  count: an
        int32 device tensor of one element -- only the first count rows are valid (box_detections(padded=True)'s count goes in as it is); class_map: an int32 device
        tensor [C], class id per label.  Everything runs on the device; the 4-byte read of kept is this method's only synchronisation, and padded=True returns the
        uncut [R] tensors plus kept [1] int32 without it (zeros and -1 behind kept)."""
        import torch

        R, Cn, M, p, stream = self._mask_head_args(mask_logits, boxes, scores, labels, in_size, out_size, score_thresh, sort_by_score, count, class_map, stream)
        masks, bout, cls, rows, kept = _empty_on(stream, _device(self), ((R, M, M), torch.float32), ((R, 4), torch.float32), ((R,), torch.int32), ((R,), torch.int32),
                                                 ((1,), torch.int32))
        self._chk(self.L.ifx_mask_head_select(self.handle, _dp(mask_logits), _dp(boxes), _dp(scores), _dp(labels), _dp(count), _dp(class_map), R, Cn, M, C.byref(p),
                                              _dp(masks), _dp(bout), _dp(cls), _dp(rows), _dp(kept), _sp(stream)), "ifx_mask_head_select")
        return _cut(stream, kept, padded, (masks, bout, cls, rows))

    # -- the reference's default detector: detections [R,6] and mrcnn_mask to image-sized masks (MaskRCNN.unmold_detections, deps/mask_rcnn/model.py:2285-2344)
    def _unmold_args(self, detections, mrcnn_mask, window, layout, class_map, stream):
        """validates the default detector's tensors: (R, M, C, layout flag, window as int32[4], stream)"""
        import torch

        _ops_tensor(self, detections, "detections", torch.float32, "float32")
        _ops_tensor(self, mrcnn_mask, "mrcnn_mask", torch.float32, "float32")
        if layout in ("nhwc", UNMOLD_NHWC):
            flag = UNMOLD_NHWC
        elif layout in ("nchw", UNMOLD_NCHW):
            flag = UNMOLD_NCHW
        else:
            raise ValueError(f"layout {layout!r}: 'nhwc' ([R,M,M,C]) or 'nchw' ([R,C,M,M])")
        sh = tuple(mrcnn_mask.shape)
        if len(sh) != 4 or (sh[1] != sh[2] if flag == UNMOLD_NHWC else sh[2] != sh[3]):
            raise ValueError(f"mrcnn_mask: shape {sh}, expected [R,M,M,C] ('nhwc') or [R,C,M,M] ('nchw')")
        R, M, Cn = (sh[0], sh[1], sh[3]) if flag == UNMOLD_NHWC else (sh[0], sh[2], sh[1])
        if not (1 <= M <= 64 and 2 <= Cn <= 1024 and R <= 1024):
            raise ValueError(f"mrcnn_mask: shape {sh}, expected R <= 1024, C in 2 .. 1024, M in 1 .. 64")
        if tuple(detections.shape) != (R, 6):
            raise ValueError(f"detections: shape {tuple(detections.shape)}, expected [{R},6]")
        if class_map is not None:
            _ops_tensor(self, class_map, "class_map", torch.int32, "int32", (Cn,), f"[{Cn}]")
        win = np.ascontiguousarray([int(v) for v in window], np.int32)
        if win.shape != (4,) or win[2] <= win[0] or win[3] <= win[1]:
            raise ValueError(f"window {tuple(window)}: four integers (y1, x1, y2, x2) with y2 > y1 and x2 > x1")
        return R, M, Cn, flag, win, _stream_for(self, stream)

    def unmold_detections(self, detections, mrcnn_mask, window, out_size, layout="nhwc", class_map=None, padded=False, stream=None):
        """ifx_unmold_detections, one image: detections [R,6] float32 (y1, x1, y2, x2, class_id, score) in molded-image pixels, mrcnn_mask [R,M,M,C] ('nhwc') or
        [R,C,M,M] ('nchw') float32, window (y1, x1, y2, x2) of the image in the molded input, out_size = (width, height) ->
        (masks [k,H,W] uint8 0/1, class_ids [k] int32, boxes [k,4] int32 (y1, x1, y2, x2), scores [k], rows [k] int32) by the rule of include/ifx_c_api.h:
        MaskRCNN.unmold_detections with utils.unmold_mask.  class_map: an int32 device tensor [C], class id per class.  Everything runs on the device; the 4-byte
        read of kept is this method's only synchronisation, and padded=True returns the uncut [R] tensors plus kept [1] int32 without it."""
        import torch

        R, M, Cn, flag, win, stream = self._unmold_args(detections, mrcnn_mask, window, layout, class_map, stream)
        W, H = int(out_size[0]), int(out_size[1])
        if W < 1 or H < 1:
            raise ValueError(f"out_size {tuple(out_size)}: a size < 1")
        masks, cls, boxes, scores, rows, kept = _empty_on(stream, _device(self), ((R, H, W), torch.uint8), ((R,), torch.int32), ((R, 4), torch.int32),
                                                          ((R,), torch.float32), ((R,), torch.int32), ((1,), torch.int32))
        self._chk(self.L.ifx_unmold_detections(self.handle, _dp(detections), _dp(mrcnn_mask), _ptr(win), _dp(class_map), R, M, Cn, flag, W, H, _dp(masks), _dp(cls),
                                               _dp(boxes), _dp(scores), _dp(rows), _dp(kept), _sp(stream)), "ifx_unmold_detections")
        return _cut(stream, kept, padded, (masks, cls, boxes, scores, rows))

    # -- the default detector's three layers that are no convolutions (deps/mask_rcnn/model.py: ProposalLayer, PyramidROIAlign, DetectionLayer)
    def keras_proposals(self, rpn_probs, rpn_bbox, anchors, image_shape, pre_nms_limit=6000, proposal_count=1000, nms_threshold=0.7, std_dev=(0.1, 0.1, 0.2, 0.2),
                        out=None, padded=False, stream=None):
        """ifx_keras_proposals, ProposalLayer.call: rpn_probs [n,2] (background, foreground), rpn_bbox [n,4], anchors [n,4] in pixels (y1, x1, y2, x2), image_shape
        (height, width) -> (proposals [c,4] normalised, index [c] int64 anchor indices) by the rule of include/ifx_c_api.h.  Everything runs on the device; the
        4-byte read of the count is this method's only synchronisation, and padded=True returns (proposals [proposal_count,4] with zero rows behind the kept ones
        -- the layer's own output --, index with -1 behind them, count [1] int32) without it.  With a batch dimension (rpn_probs [B,n,2], rpn_bbox [B,n,4]; the
        anchors are shared) the images are enqueued one after the other and the result is always the padded form: [B,proposal_count,4], [B,proposal_count],
        count [B].  out: the proposals tensor to write into.  Enqueue-only on `stream` (default: the current stream)."""
        import torch

        _ops_tensor(self, rpn_probs, "rpn_probs", torch.float32, "float32")
        batched = rpn_probs.dim() == 3
        if rpn_probs.dim() not in (2, 3) or rpn_probs.shape[-1] != 2:
            raise ValueError(f"rpn_probs: shape {tuple(rpn_probs.shape)}, expected [n,2] or [B,n,2]")
        n = int(rpn_probs.shape[-2])
        lead = tuple(rpn_probs.shape[:-2])
        _ops_tensor(self, rpn_bbox, "rpn_bbox", torch.float32, "float32", lead + (n, 4))
        _ops_tensor(self, anchors, "anchors", torch.float32, "float32", (n, 4), f"[{n},4]")
        p = KerasProposalParams()
        p.pre_nms_limit, p.proposal_count, p.nms_threshold = int(pre_nms_limit), int(proposal_count), float(nms_threshold)
        p.std_dev[:] = [float(v) for v in std_dev]
        p.image_h, p.image_w = int(image_shape[0]), int(image_shape[1])
        rows = max(p.proposal_count, 0)
        B = int(lead[0]) if batched else 1
        stream = _stream_for(self, stream)
        out = _out_like(self, out, lead + (rows, 4), stream)
        index, count = _empty_on(stream, _device(self), (lead + (rows,), torch.int64), ((B,), torch.int32))
        e = 4                                       # bytes of a float32 / int32
        for b in range(B):
            self._chk(self.L.ifx_keras_proposals(self.handle, _dp(rpn_probs, b * n * 2 * e), _dp(rpn_bbox, b * n * 4 * e), _dp(anchors), n, C.byref(p),
                                                 _dp(out, b * rows * 4 * e), _dp(index, b * rows * 8), _dp(count, b * e), _sp(stream)), "ifx_keras_proposals")
        return _cut(stream, count, padded or batched, (out, index))

    def pyramid_roi_align(self, features, boxes, image_shape, pool_shape, layout="nhwc", out=None, levels_out=None, stream=None):
        """ifx_pyramid_roi_align, PyramidROIAlign.call in one launch: features, the four maps P2 .. P5, each [B,H_l,W_l,C] ('nhwc', as Keras holds them) or
        [B,C,H_l,W_l] ('nchw'); boxes [B,n,4] (or [n,4] with B == 1) normalised y1, x1, y2, x2; image_shape (height, width); pool_shape (pool_h, pool_w) ->
        [B,n,pool_h,pool_w,C] or [B,n,C,pool_h,pool_w] ([n,...] for boxes [n,4]) float32: every box sampled from the level the reference gives it, by the rule of
        include/ifx_c_api.h.  levels_out: an int32 tensor shaped as the boxes' leading dimensions that receives each box's level 2 .. 5.  Enqueue-only on `stream`
        (default: the current stream)."""
        import torch

        features = list(features)
        if len(features) != 4:
            raise ValueError(f"features: {len(features)} maps, expected the four P2 .. P5")
        if layout not in ("nhwc", "nchw"):
            raise ValueError(f"layout {layout!r}: 'nhwc' ([B,H,W,C]) or 'nchw' ([B,C,H,W])")
        nhwc = layout == "nhwc"
        for l, f in enumerate(features):
            _ops_tensor(self, f, f"features[{l}]", torch.float32, "float32", (None,) * 4, "four dimensions")
        B = int(features[0].shape[0])
        Cn = int(features[0].shape[3 if nhwc else 1])
        for l, f in enumerate(features):
            if int(f.shape[0]) != B or int(f.shape[3 if nhwc else 1]) != Cn:
                raise ValueError(f"features[{l}]: shape {tuple(f.shape)}, expected the batch {B} and the {Cn} channels of features[0]")
        _ops_tensor(self, boxes, "boxes", torch.float32, "float32")
        if boxes.dim() not in (2, 3) or boxes.shape[-1] != 4 or (boxes.dim() == 2 and B != 1) or (boxes.dim() == 3 and int(boxes.shape[0]) != B):
            raise ValueError(f"boxes: shape {tuple(boxes.shape)}, expected [{B},n,4]" + (" or [n,4]" if B == 1 else ""))
        lead = tuple(int(v) for v in boxes.shape[:-1])
        n = lead[-1]
        ph, pw = int(pool_shape[0]), int(pool_shape[1])
        stream = _stream_for(self, stream)
        out = _out_like(self, out, lead + ((max(ph, 0), max(pw, 0), Cn) if nhwc else (Cn, max(ph, 0), max(pw, 0))), stream)
        if levels_out is not None:
            _ops_tensor(self, levels_out, "levels_out", torch.int32, "int32", lead)
        if n == 0:
            return out
        hw = (1, 2) if nhwc else (2, 3)
        ptrs = (C.c_void_p * 4)(*[f.data_ptr() for f in features])
        hs = (C.c_int32 * 4)(*[int(f.shape[hw[0]]) for f in features])
        ws = (C.c_int32 * 4)(*[int(f.shape[hw[1]]) for f in features])
        self._chk(self.L.ifx_pyramid_roi_align(self.handle, ptrs, hs, ws, B, Cn, 1 if nhwc else 0, _dp(boxes), n, int(image_shape[0]), int(image_shape[1]), ph, pw,
                                               _dp(out), _dp(levels_out), _sp(stream)), "ifx_pyramid_roi_align")
        return out

    def keras_detections(self, rois, probs, deltas, window, image_shape, min_confidence=0.7, nms_threshold=0.3, max_instances=100, std_dev=(0.1, 0.1, 0.2, 0.2),
                         out=None, padded=False, stream=None):
        """ifx_keras_detections, refine_detections_graph: rois [R,4] normalised, probs [R,C], deltas [R,C,4], window (y1, x1, y2, x2) in pixels (numbers on the
        host), image_shape (height, width) -> (detections [c,6]: y1, x1, y2, x2, class, score; boxes_norm [c,4]: the boxes normalised for the mask branch's
        pyramid_roi_align; index [c] int64: each detection's ROI row) by the rule of include/ifx_c_api.h.  Everything runs on the device; the 4-byte read of the
        count is this method's only synchronisation, and padded=True returns the [max_instances] tensors (zero rows behind the detections -- the layer's own output,
        what unmold_detections and process_segmentation_unmolded take --, -1 in index) and count [1] int32 without it.  With a batch dimension (rois [B,R,4], probs
        [B,R,C], deltas [B,R,C,4], window [B][4]) the images are enqueued one after the other and the result is always the padded form with a leading B.  out: the
        detections tensor to write into.  Enqueue-only on `stream` (default: the current stream)."""
        import torch

        _ops_tensor(self, probs, "probs", torch.float32, "float32")
        batched = probs.dim() == 3
        if probs.dim() not in (2, 3):
            raise ValueError(f"probs: shape {tuple(probs.shape)}, expected [R,C] or [B,R,C]")
        lead = tuple(int(v) for v in probs.shape[:-2])
        R, Cn = int(probs.shape[-2]), int(probs.shape[-1])
        _ops_tensor(self, rois, "rois", torch.float32, "float32", lead + (R, 4))
        _ops_tensor(self, deltas, "deltas", torch.float32, "float32", lead + (R, Cn, 4))
        B = lead[0] if batched else 1
        win = np.ascontiguousarray(window, np.float32)
        if win.shape != ((B, 4) if batched else (4,)):
            raise ValueError(f"window: shape {win.shape}, expected {[B, 4] if batched else [4]}")
        win = win.reshape(B, 4)
        p = KerasDetectionParams()
        p.std_dev[:] = [float(v) for v in std_dev]
        p.min_confidence, p.nms_threshold, p.max_instances = float(min_confidence), float(nms_threshold), int(max_instances)
        p.image_h, p.image_w = int(image_shape[0]), int(image_shape[1])
        rows = max(p.max_instances, 0)
        stream = _stream_for(self, stream)
        out = _out_like(self, out, lead + (rows, 6), stream)
        norm, index, count = _empty_on(stream, _device(self), (lead + (rows, 4), torch.float32), (lead + (rows,), torch.int64), ((B,), torch.int32))
        e = 4
        for b in range(B):
            p.window[:] = [float(v) for v in win[b]]
            self._chk(self.L.ifx_keras_detections(self.handle, _dp(rois, b * R * 4 * e), _dp(probs, b * R * Cn * e), _dp(deltas, b * R * Cn * 4 * e), R, Cn, C.byref(p),
                                                  _dp(out, b * rows * 6 * e), _dp(norm, b * rows * 4 * e), _dp(index, b * rows * 8), _dp(count, b * e), _sp(stream)),
                      "ifx_keras_detections")
        return _cut(stream, count, padded or batched, (out, norm, index))
