"""instancefusion_amd -- host-side Python mirror of the reference's interface over libifx.so.

The product is the C-ABI shared library ``instancefusion_amd/libifx.so`` (HIP kernels for gfx950,
declared in ``include/ifx_c_api.h``).  This package only binds it with ctypes and mirrors the
reference's classes for the hot path:

* :class:`ElasticFusion`  -- ``ElasticFusion::processFrame`` / ``ElasticFusionInterface``
  (elasticfusionpublic/Core/src/ElasticFusion.h:75-82, src/map_interface/ElasticFusionInterface.h:55-130)
* :class:`InstanceFusion` -- ``InstanceFusion::whetherDoSegmentation`` / ``ProcessSegmentation``
  (src/Core/InstanceFusion.h:72-107) with the Mask-RCNN bridge replaced by replayed masks.

There is no CPU fallback: importing works anywhere (so the symbols can be checked), but creating a
handle without a MI355X raises :class:`IfxError`.
"""
from __future__ import annotations

import ctypes as C
import functools
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("IFX_LIB") or os.path.join(_HERE, "libifx.so")   # IFX_LIB: an experimental build of the same library (tools/bench_variants.sh)
HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "ifx_c_api.h")

NUM_INSTANCES = 96
VOTE_FLOATS = 48


class IfxError(RuntimeError):
    pass


class IfxConfig(C.Structure):
    _fields_ = [
        ("width", C.c_int32), ("height", C.c_int32),
        ("fx", C.c_float), ("fy", C.c_float), ("cx", C.c_float), ("cy", C.c_float),
        ("time_delta", C.c_int32), ("confidence", C.c_float), ("depth_cut", C.c_float),
        ("max_depth_processed", C.c_float), ("icp_weight", C.c_float),
        ("pyramid", C.c_int32), ("fast_odom", C.c_int32), ("so3", C.c_int32),
        ("max_surfels", C.c_int32), ("device", C.c_int32), ("n_ranks", C.c_int32), ("rank", C.c_int32),
    ]


class Pyramids(C.Structure):
    """ifx_pyramids: device pointers of the caller's output buffers, three levels each (0 = skipped)"""
    _fields_ = [(n, C.c_void_p * 3) for n in ("depth", "vmap_curr", "nmap_curr", "next_img", "didx", "didy", "vmap_g_prev", "nmap_g_prev", "last_depth", "last_img", "cloud")]


class DetectorPrep(C.Structure):
    """ifx_detector_prep: the parameters of the detector-input stage (include/ifx_c_api.h)"""
    _fields_ = [("min_size", C.c_int32), ("max_size", C.c_int32), ("size_divisible", C.c_int32), ("flags", C.c_int32), ("mean", C.c_float * 3), ("std", C.c_float * 3)]


class RpnParams(C.Structure):
    """ifx_rpn_params: the parameters of the proposal stage (include/ifx_c_api.h)"""
    _fields_ = [("pre_nms_top_n", C.c_int32), ("post_nms_top_n", C.c_int32), ("nms_thresh", C.c_float), ("min_size", C.c_float), ("weights", C.c_float * 4),
                ("xform_clip", C.c_float), ("image_w", C.c_int32), ("image_h", C.c_int32)]


class RpnLevel(C.Structure):
    """ifx_rpn_level: one level's inputs of ifx_rpn_proposals_fpn (include/ifx_c_api.h)"""
    _fields_ = [("objectness", C.c_void_p), ("regression", C.c_void_p), ("anchors", C.c_void_p), ("A", C.c_int32), ("H", C.c_int32), ("W", C.c_int32)]


class BoxDetParams(C.Structure):
    """ifx_box_det_params: the parameters of the box head's post-processing (include/ifx_c_api.h)"""
    _fields_ = [("score_thresh", C.c_float), ("nms", C.c_float), ("detections_per_img", C.c_int32), ("max_out", C.c_int32), ("weights", C.c_float * 4),
                ("xform_clip", C.c_float), ("image_w", C.c_int32), ("image_h", C.c_int32)]


class KerasProposalParams(C.Structure):
    """ifx_keras_proposal_params: the parameters of the Keras detector's proposal layer (include/ifx_c_api.h)"""
    _fields_ = [("pre_nms_limit", C.c_int32), ("proposal_count", C.c_int32), ("nms_threshold", C.c_float), ("std_dev", C.c_float * 4), ("image_h", C.c_int32),
                ("image_w", C.c_int32)]


class KerasDetectionParams(C.Structure):
    """ifx_keras_detection_params: the parameters of the Keras detector's detection layer (include/ifx_c_api.h)"""
    _fields_ = [("std_dev", C.c_float * 4), ("min_confidence", C.c_float), ("nms_threshold", C.c_float), ("max_instances", C.c_int32), ("image_h", C.c_int32),
                ("image_w", C.c_int32), ("window", C.c_float * 4)]


class MaskHeadParams(C.Structure):
    """ifx_mask_head_params: the parameters of the mask head's select / sigmoid stage (include/ifx_c_api.h)"""
    _fields_ = [("score_thresh", C.c_float), ("in_w", C.c_int32), ("in_h", C.c_int32), ("out_w", C.c_int32), ("out_h", C.c_int32), ("sort_by_score", C.c_int32)]


class SoaView(C.Structure):
    _fields_ = [("count", C.c_int32), ("capacity", C.c_int32), ("d_pos_conf", C.c_void_p), ("d_norm_rad", C.c_void_p),
                ("d_color", C.c_void_p), ("d_times", C.c_void_p), ("d_img_corr", C.c_void_p), ("d_votes", C.c_void_p)]


def default_config(w=640, h=480, fx=528.0, fy=528.0, cx=320.0, cy=240.0, max_surfels=1 << 20, **kw):
    """The constants the reference runs with (src/map_interface/ElasticFusionInterface.cpp:43-45, src/main.cpp:46-47)."""
    d = dict(width=w, height=h, fx=fx, fy=fy, cx=cx, cy=cy, time_delta=200, confidence=10.0, depth_cut=12.0,
             max_depth_processed=20.0, icp_weight=10.0, pyramid=1, fast_odom=0, so3=1, max_surfels=max_surfels,
             device=0, n_ranks=1, rank=0)
    d.update(kw)
    return d


_lib = None

_P = C.c_void_p
_SIGS = {
    "ifx_create": (C.c_int, [C.POINTER(IfxConfig), C.POINTER(_P)]),
    "ifx_destroy": (None, [_P]),
    "ifx_last_error": (C.c_char_p, [_P]),
    "ifx_global_error": (C.c_char_p, []),
    "ifx_process_frame": (C.c_int, [_P, _P, _P, C.c_int64, _P, C.c_float, _P]),
    "ifx_process_frame_ex": (C.c_int, [_P, _P, _P, C.c_int64, _P, _P, C.c_float, C.c_int, _P]),
    "ifx_enqueue_frame_device": (C.c_int, [_P, _P, _P, C.c_int64, _P, C.c_float]),
    "ifx_set_shard": (C.c_int, [_P, C.c_int, C.c_int]),
    "ifx_sharded_frame_phase": (C.c_int, [_P, C.c_int, _P, _P]),
    "ifx_key_images": (C.c_int, [_P, _P, _P, _P, _P, _P]),
    "ifx_stream_handles": (C.c_int, [_P, _P, _P]),
    "ifx_owner_frame_phase": (C.c_int, [_P, C.c_int, _P, _P]),
    "ifx_owner_exchange": (C.c_int, [_P, C.c_int, _P, _P, _P, C.c_int]),
    "ifx_owner_of": (C.c_int, [_P, C.c_int, C.c_int, _P]),
    "ifx_owner_segmentation_begin": (C.c_int, [_P, _P, _P, _P, _P, C.c_int, C.c_int, C.c_int]),
    "ifx_owner_segmentation_resume": (C.c_int, [_P]),
    "ifx_owner_segmentation_abort": (C.c_int, [_P]),
    "ifx_owner_ids_begin": (C.c_int, [_P]),
    "ifx_owner_ids_resume": (C.c_int, [_P]),
    "ifx_owner_knn_export": (C.c_int, [_P, _P, _P, _P]),
    "ifx_owner_knn_vote": (C.c_int, [_P, _P, _P, C.c_int, C.c_int]),
    "ifx_owner_predict_phase": (C.c_int, [_P, C.c_int]),
    "ifx_camera_count": (C.c_int, [_P, C.c_int]),
    "ifx_camera_select": (C.c_int, [_P, C.c_int]),
    "ifx_owner_set_frame_pose": (C.c_int, [_P, _P]),
    "ifx_owner_set_tracking_rank": (C.c_int, [_P, C.c_int]),
    "ifx_owner_track_ahead": (C.c_int, [_P, C.c_int, C.c_int, _P, _P]),
    "ifx_comm_unique_id": (C.c_int, [_P]),
    "ifx_owner_init_comm": (C.c_int, [_P, _P]),
    "ifx_owner_set_comm": (C.c_int, [_P, _P]),
    "ifx_owner_process_frame_device": (C.c_int, [_P, _P, _P, C.c_int64]),
    "ifx_owner_process_frame": (C.c_int, [_P, _P, _P, C.c_int64, _P]),
    "ifx_owner_predict": (C.c_int, [_P]),
    "ifx_owner_process_segmentation": (C.c_int, [_P, _P, _P, _P, _P, C.c_int, C.c_int, C.c_int]),
    "ifx_owner_knn_vote_colour": (C.c_int, [_P]),
    "ifx_owner_exchange_stats": (C.c_int, [_P, _P, C.c_int]),
    "ifx_owner_comm_ranks": (C.c_int, [_P]),
    "ifx_map_seq": (C.c_int, [_P, _P, C.c_int]),
    "ifx_prefetch_frame_device": (C.c_int, [_P, _P, _P]),
    "ifx_hint_next_frame_device": (C.c_int, [_P, _P, _P]),
    "ifx_hint_next_frame": (C.c_int, [_P, _P, _P]),
    "ifx_lookahead_stats": (C.c_int, [_P, _P, C.c_int]),
    "ifx_view_list_stats": (C.c_int, [_P, _P]),
    "ifx_map_bounding_boxes": (C.c_int, [_P, C.c_int, C.c_float, _P, _P, _P, _P, _P]),
    "ifx_instance_point_cloud": (C.c_int, [_P, C.c_int, _P, C.c_int, _P, C.c_int]),
    "ifx_sync": (C.c_int, [_P]),
    "ifx_get_pose": (C.c_int, [_P, _P]),
    "ifx_tick": (C.c_int, [_P]),
    "ifx_trajectory": (C.c_int, [_P, _P, C.c_int]),
    "ifx_tracker_diag": (C.c_int, [_P, _P]),
    "ifx_tracker_fallbacks": (C.c_int, [_P]),
    "ifx_build_pyramids": (C.c_int, [_P, _P, _P, _P, _P, _P, _P, C.POINTER(Pyramids)]),
    "ifx_tracker_range_exceeded": (C.c_int, [_P]),
    "ifx_tracker_meet_giveups": (C.c_int, [_P]),
    "ifx_hot_records_stale": (C.c_int, [_P]),
    "ifx_set_loop_closure": (C.c_int, [_P, C.c_int, C.c_int, C.c_float, C.c_float]),
    "ifx_loop_closure_diag": (C.c_int, [_P, _P]),
    "ifx_set_loop_closure_callback": (C.c_int, [_P, _P, _P]),
    "ifx_sample_graph_model": (C.c_int, [_P, _P, C.c_int]),
    "ifx_loop_closure_constraints": (C.c_int, [_P, _P, _P, _P, C.c_int]),
    "ifx_set_deformation": (C.c_int, [_P, _P, C.c_int, C.c_int]),
    "ifx_adopt_estimated_pose": (C.c_int, [_P]),
    "ifx_set_fern_callback": (C.c_int, [_P, _P, _P]),
    "ifx_adopt_pose": (C.c_int, [_P, _P]),
    "ifx_fern_frame": (C.c_int, [_P, _P, _P, _P, _P]),
    "ifx_fern_frame_async": (C.c_int, [_P]),
    "ifx_fern_frame_fetch": (C.c_int, [_P, _P, _P, _P, _P]),
    "ifx_track_maps": (C.c_int, [_P, _P, _P, _P, _P, _P, _P, _P, _P]),
    "ifx_map_view": (C.c_int, [_P, C.POINTER(SoaView)]),
    "ifx_map_count": (C.c_int, [_P]),
    "ifx_map_slots": (C.c_int, [_P]),
    "ifx_map_download": (C.c_int, [_P, C.c_int] + [_P] * 6),
    "ifx_map_upload": (C.c_int, [_P, C.c_int] + [_P] * 6),
    "ifx_set_pose": (C.c_int, [_P, _P, C.c_int]),
    "ifx_compact": (C.c_int, [_P]),
    "ifx_set_option": (C.c_int, [_P, C.c_char_p, C.c_int]),
    "ifx_ids_after": (_P, [_P]),
    "ifx_image_download": (C.c_int, [_P, C.c_char_p, _P, C.c_int64]),
    "ifx_predict_indices": (C.c_int, [_P, _P, C.c_int]),
    "ifx_combined_predict": (C.c_int, [_P, _P, C.c_int, C.c_int]),
    "ifx_fuse": (C.c_int, [_P, _P, C.c_int, C.c_float]),
    "ifx_clean": (C.c_int, [_P, _P, C.c_int]),
    "ifx_render_ids": (C.c_int, [_P, _P, C.c_int]),
    "ifx_set_frame": (C.c_int, [_P, _P, _P]),
    "ifx_icp_step": (C.c_int, [_P, _P, _P, _P, _P, _P, _P, C.c_float, C.c_float, C.c_float, C.c_float, _P, _P, C.c_float, C.c_float, C.c_int, C.c_int, _P]),
    "ifx_rgb_residual": (C.c_int, [_P, C.c_float, _P, _P, _P, _P, _P, _P, _P, C.c_float, _P, _P, C.c_int, C.c_int, _P, _P]),
    "ifx_rgb_step": (C.c_int, [_P, _P, C.c_float, _P, C.c_float, C.c_float, _P, _P, C.c_float, C.c_int, C.c_int, _P]),
    "ifx_so3_step": (C.c_int, [_P, _P, _P, _P, _P, _P, C.c_int, C.c_int, _P]),
    "ifx_track_pair": (C.c_int, [_P] * 9),
    "ifx_tracker_buffer_download": (C.c_int, [_P, C.c_char_p, C.c_int, _P, C.c_int64]),
    "ifx_should_segment": (C.c_int, [_P, C.c_int]),
    "ifx_process_segmentation": (C.c_int, [_P, _P, _P, _P, _P, C.c_int, C.c_int, C.c_int]),
    "ifx_process_segmentation_device": (C.c_int, [_P, _P, C.c_int, C.c_float, _P, C.c_int, C.c_int, C.c_int, _P]),
    "ifx_segmentation_snapshot": (C.c_int, [_P, C.c_int]),
    "ifx_process_segmentation_deferred": (C.c_int, [_P, C.c_int, _P, _P, C.c_int, C.c_int, C.c_int]),
    "ifx_process_segmentation_deferred_device": (C.c_int, [_P, C.c_int, _P, C.c_int, C.c_float, _P, C.c_int, C.c_int, C.c_int, _P]),
    "ifx_process_segmentation_rois": (C.c_int, [_P, _P, C.c_int, _P, C.c_float, _P, C.c_int, C.c_int, C.c_int, _P]),
    "ifx_process_segmentation_deferred_rois": (C.c_int, [_P, C.c_int, _P, C.c_int, _P, C.c_float, _P, C.c_int, C.c_int, C.c_int, _P]),
    "ifx_ingest_masks": (C.c_int, [_P, _P, C.c_int, C.c_float, _P, C.c_int, _P, _P, _P, _P, _P]),
    "ifx_paste_roi_masks": (C.c_int, [_P, _P, C.c_int, _P, C.c_float, _P, C.c_int, _P, _P, _P, _P, _P]),
    "ifx_detector_input_size": (C.c_int, [C.c_int, C.c_int, C.POINTER(DetectorPrep), _P]),
    "ifx_detector_resize_taps": (C.c_int, [C.c_int, C.c_int, _P, _P, _P, C.c_int]),
    "ifx_detector_input": (C.c_int, [_P, C.c_int, C.POINTER(DetectorPrep), _P, C.c_int64, _P]),
    "ifx_detector_input_image": (C.c_int, [_P, _P, C.c_int, C.c_int, C.POINTER(DetectorPrep), _P, C.c_int64, _P]),
    "ifx_roi_align_forward": (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int, C.c_int, _P, C.c_int, C.c_float, C.c_int, C.c_int, C.c_int, _P, _P]),
    "ifx_nms": (C.c_int, [_P, _P, _P, _P, C.c_int, C.c_float, _P, _P, _P]),
    "ifx_fpn_level_thresholds": (C.c_int, [_P, C.c_int, C.c_int, _P]),
    "ifx_fpn_roi_align": (C.c_int, [_P, _P, _P, _P, _P, C.c_int, C.c_int, C.c_int, _P, C.c_int, C.c_float, C.c_int, C.c_float, C.c_int, C.c_int, C.c_int, _P, _P, _P]),
    "ifx_rpn_proposals": (C.c_int, [_P, _P, _P, _P, C.c_int, C.c_int, C.c_int, C.POINTER(RpnParams), _P, _P, _P, _P, _P]),
    "ifx_rpn_proposals_fpn": (C.c_int, [_P, C.POINTER(RpnLevel), C.c_int, C.POINTER(RpnParams), C.c_int, _P, _P, _P, _P, _P, _P, _P]),
    "ifx_box_decode": (C.c_int, [_P, _P, _P, C.c_int, C.c_int, C.POINTER(C.c_float * 4), C.c_float, C.c_int, C.c_int, _P, _P]),
    "ifx_box_detections": (C.c_int, [_P, _P, _P, _P, C.c_int, C.c_int, C.c_int, C.POINTER(BoxDetParams), _P, _P, _P, _P, _P, _P, _P]),
    "ifx_mask_head_select": (C.c_int, [_P, _P, _P, _P, _P, _P, _P, C.c_int, C.c_int, C.c_int, C.POINTER(MaskHeadParams), _P, _P, _P, _P, _P, _P]),
    "ifx_process_segmentation_detections": (C.c_int, [_P, _P, _P, _P, _P, _P, _P, C.c_int, C.c_int, C.c_int, C.POINTER(MaskHeadParams), C.c_float, C.c_int, C.c_int, _P, _P]),
    "ifx_process_segmentation_deferred_detections": (C.c_int, [_P, C.c_int, _P, _P, _P, _P, _P, _P, C.c_int, C.c_int, C.c_int, C.POINTER(MaskHeadParams), C.c_float, C.c_int,
                                                               C.c_int, _P, _P]),
    "ifx_unmold_detections": (C.c_int, [_P, _P, _P, _P, _P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _P, _P, _P, _P, _P, _P, _P]),
    "ifx_process_segmentation_unmolded": (C.c_int, [_P, _P, _P, _P, _P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _P, _P]),
    "ifx_process_segmentation_deferred_unmolded": (C.c_int, [_P, C.c_int, _P, _P, _P, _P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _P, _P]),
    "ifx_molded_input_size": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, _P]),
    "ifx_detector_input_molded": (C.c_int, [_P, C.c_int, C.c_int, C.c_int, _P, C.c_int, _P, C.c_int64, _P]),
    "ifx_detector_input_molded_image": (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int, C.c_int, _P, C.c_int, _P, C.c_int64, _P]),
    "ifx_keras_proposals": (C.c_int, [_P, _P, _P, _P, C.c_int, C.POINTER(KerasProposalParams), _P, _P, _P, _P]),
    "ifx_pyramid_level_thresholds": (C.c_int, [C.c_int, C.c_int, _P]),
    "ifx_pyramid_roi_align": (C.c_int, [_P, _P, _P, _P, C.c_int, C.c_int, C.c_int, _P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _P, _P, _P]),
    "ifx_keras_detections": (C.c_int, [_P, _P, _P, _P, C.c_int, C.c_int, C.POINTER(KerasDetectionParams), _P, _P, _P, _P, _P]),
    # the device forms on a sharded map: (h, root, max_n, rgb, depth) in front of the unsharded entry's arguments
    "ifx_owner_segmentation_begin_device": (C.c_int, [_P, C.c_int, C.c_int, _P, _P, _P, C.c_int, C.c_float, _P, C.c_int, C.c_int, C.c_int, _P]),
    "ifx_owner_segmentation_begin_rois": (C.c_int, [_P, C.c_int, C.c_int, _P, _P, _P, C.c_int, _P, C.c_float, _P, C.c_int, C.c_int, C.c_int, _P]),
    "ifx_owner_segmentation_begin_detections": (C.c_int, [_P, C.c_int, C.c_int, _P, _P, _P, _P, _P, _P, _P, _P, C.c_int, C.c_int, C.c_int, C.POINTER(MaskHeadParams), C.c_float,
                                                          C.c_int, C.c_int, _P, _P]),
    "ifx_owner_process_segmentation_device": (C.c_int, [_P, C.c_int, C.c_int, _P, _P, _P, C.c_int, C.c_float, _P, C.c_int, C.c_int, C.c_int, _P]),
    "ifx_owner_process_segmentation_rois": (C.c_int, [_P, C.c_int, C.c_int, _P, _P, _P, C.c_int, _P, C.c_float, _P, C.c_int, C.c_int, C.c_int, _P]),
    "ifx_owner_process_segmentation_detections": (C.c_int, [_P, C.c_int, C.c_int, _P, _P, _P, _P, _P, _P, _P, _P, C.c_int, C.c_int, C.c_int, C.POINTER(MaskHeadParams), C.c_float,
                                                          C.c_int, C.c_int, _P, _P]),
    "ifx_segmentation_snapshot_release": (C.c_int, [_P, C.c_int]),
    "ifx_segmentation_snapshot_stats": (C.c_int, [_P, C.c_int, _P]),
    "ifx_labels": (C.c_int, [_P, _P, C.c_int]),
    "ifx_render_project_map": (C.c_int, [_P, _P, _P]),
    "ifx_set_instance_gt": (C.c_int, [_P, _P]),
    "ifx_precision_recall": (C.c_int, [_P, _P, _P, _P]),
    "ifx_instance_table": (C.c_int, [_P, _P]),
    "ifx_loop_closure_instance_table": (C.c_int, [_P, _P]),
    "ifx_mask_clean_overlap": (C.c_int, [_P, _P, C.c_int]),
    "ifx_mask_geometric_filter": (C.c_int, [_P, _P, _P, _P, C.c_int, _P]),
    "ifx_mask_compare_map": (C.c_int, [_P, _P, _P, C.c_int, _P, _P, _P, _P]),
    "ifx_segmentation_matches": (C.c_int, [_P, _P, _P, C.c_int]),
    "ifx_knn_vote_colour": (C.c_int, [_P, _P, C.c_int]),
    "ifx_slic_segment": (C.c_int, [_P, _P, _P]),
    "ifx_merge_superpixels": (C.c_int, [_P, _P, _P, _P, _P]),
    "ifx_mask_superpixel_filter": (C.c_int, [_P, _P, _P, C.c_int]),
    "ifx_stage_ms": (C.c_int, [_P, _P, C.c_int]),
    "ifx_superpixel_ahead_stats": (C.c_int, [_P, _P, _P, _P, C.c_int]),
    "ifx_kernel_ms": (C.c_int, [_P, C.c_char_p, _P, _P]),
}


def lib():
    """Loads libifx.so (built by ``__graft_entry__.build()`` / ``make -C instancefusion_amd/csrc``)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise IfxError(f"{LIB_PATH} is missing: build it with `make -C instancefusion_amd/csrc` "
                           "(there is no CPU fallback)")
        L = C.CDLL(LIB_PATH)
        for name, (res, args) in _SIGS.items():
            f = getattr(L, name)  # raises AttributeError when a declared symbol is not exported
            f.restype = res
            f.argtypes = args
        _lib = L
    return _lib


def exported_symbols():
    return sorted(_SIGS)


def _ptr(a):
    if a is None:
        return None
    assert a.flags["C_CONTIGUOUS"]
    return a.ctypes.data_as(C.c_void_p)


_IMG_SPECS = {
    "ids_after": (np.int32, 1), "ids_tmp": (np.int32, 1), "index": (np.uint32, 1), "index_vc": (np.float32, 4),
    "index_ct": (np.float32, 4), "index_nr": (np.float32, 4), "pred_vertex": (np.float32, 4),
    "pred_normal": (np.float32, 4), "pred_image": (np.uint8, 4), "pred_inst": (np.uint8, 4), "pred_time": (np.uint16, 1),
    "fill_vertex": (np.float32, 4), "fill_normal": (np.float32, 4), "fill_image": (np.uint8, 4),
    "depth_filtered": (np.uint16, 1), "depth_metric": (np.float32, 1), "depth_metric_filtered": (np.float32, 1),
    "old_vertex": (np.float32, 4), "old_normal": (np.float32, 4), "old_image": (np.uint8, 4), "old_time": (np.uint16, 1),
    "act_vertex": (np.float32, 4), "act_normal": (np.float32, 4), "act_image": (np.uint8, 4),
}
_TRK_SPECS = {
    "vmap_curr": (np.float32, 3, True), "nmap_curr": (np.float32, 3, True), "vmap_prev": (np.float32, 3, True),
    "nmap_prev": (np.float32, 3, True), "last_depth": (np.float32, 1, False), "next_depth": (np.float32, 1, False),
    "last_img": (np.uint8, 1, False), "next_img": (np.uint8, 1, False), "lastnext_img": (np.uint8, 1, False),
    "didx": (np.int16, 1, False), "didy": (np.int16, 1, False), "cloud": (np.float32, 3, False),
    "depth_tmp": (np.uint16, 1, False),
}
CORRES_DTYPE = np.dtype([("zx", np.int16), ("zy", np.int16), ("diff", np.float32)])
CAND_DTYPE = np.dtype([("pixel", np.uint32), ("gx", np.int16), ("gy", np.int16)])   # an entry of a frame slot's candidate list (ifx_ctx.h CandEntry)


# mask formats of ifx_process_segmentation_device (include/ifx_c_api.h)
MASK_U8 = 0     # inside iff the byte is non-zero (torch bool / uint8, the host entry's 0/255)
MASK_F32 = 1    # inside iff the value is > threshold (mask probabilities; NaN is outside)

# flags of ifx_detector_prep (include/ifx_c_api.h)
DET_SWAP_RB = 1      # output channel c reads source channel 2 - c
DET_SCALE_255 = 2    # ToTensor's [0, 1] back to [0, 255] before the normalisation

# option "id_rule" (include/ifx_c_api.h): which rule draws the surfel-id images
ID_RULE_RAY_DISC = 0     # default: a ray through each pixel centre against the disc, f32 depth keys
ID_RULE_REFERENCE = 1    # the reference's surfel_ids.geom / .frag: screen-space quads, 24-bit depth


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


def _detector_out(ef, size, out, stream):
    """the output tensor of the detector-input calls ([1,3,H',W'] float32 on the handle's device, made on the consumer's stream) and that stream"""
    import torch

    dev = torch.device("cuda", int(ef.cfgd["device"]))
    if stream is None:
        stream = torch.cuda.current_stream(dev)
    shape = (1, 3, size[3], size[2])
    if out is None:
        with torch.cuda.stream(stream):
            out = torch.empty(shape, dtype=torch.float32, device=dev)
    else:
        if not isinstance(out, torch.Tensor):
            raise TypeError("out must be a torch tensor on the handle's device")
        if out.dtype != torch.float32:
            raise TypeError(f"out: dtype {out.dtype} is not supported (float32)")
        if out.device != dev:
            raise ValueError(f"out is on {out.device}, the handle on {dev}")
        if tuple(out.shape) != shape or not out.is_contiguous():
            raise ValueError(f"out: shape {tuple(out.shape)}, expected a contiguous {list(shape)}")
    return out, stream


def detector_input_image(ef, rgb, min_size=800, max_size=None, size_divisible=0, mean=(102.9801, 115.9465, 122.7717), std=(1., 1., 1.), to_bgr255=True, swap_rb=False,
                         out=None, stream=None):
    """ifx_detector_input_image: InstanceFusion.detector_input's kernel on any uint8 [H,W,3] torch tensor on the handle's device (the stage call).  `rgb` must be
    complete on `stream` (default: the current stream), the consumer's.  Returns (tensor [1,3,H',W'] float32, (oh, ow))."""
    import torch

    dev = torch.device("cuda", int(ef.cfgd["device"]))
    if not isinstance(rgb, torch.Tensor):
        raise TypeError("rgb must be a torch tensor on the handle's device")
    if rgb.dtype != torch.uint8:
        raise TypeError(f"rgb: dtype {rgb.dtype} is not supported (uint8)")
    if rgb.device != dev:
        raise ValueError(f"rgb is on {rgb.device}, the handle on {dev}")
    if rgb.dim() != 3 or rgb.shape[2] != 3 or not rgb.is_contiguous():
        raise ValueError(f"rgb: shape {tuple(rgb.shape)}, expected a contiguous [H,W,3]")
    hh, w = int(rgb.shape[0]), int(rgb.shape[1])
    p = detector_prep(min_size, max_size, size_divisible, mean, std, to_bgr255, swap_rb)
    size = np.zeros(4, np.int32)
    if ef.L.ifx_detector_input_size(w, hh, C.byref(p), _ptr(size)) < 0:
        raise IfxError(f"ifx_detector_input_size: refused ({w} x {hh}, min_size {min_size}, max_size {max_size}, size_divisible {size_divisible}, std {tuple(std)})")
    out, stream = _detector_out(ef, size, out, stream)
    ef._chk(ef.L.ifx_detector_input_image(ef.handle, C.c_void_p(rgb.data_ptr()), w, hh, C.byref(p), C.c_void_p(out.data_ptr()), int(out.numel()),
                                          C.c_void_p(stream.cuda_stream or None)), "ifx_detector_input_image")
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
    import torch

    mean = [float(v) for v in mean]
    if len(mean) != 3:
        raise ValueError("mean has three entries")
    size = molded_input_size(w, hh, min_dim, max_dim)
    S = size[2]
    dev = torch.device("cuda", int(ef.cfgd["device"]))
    if stream is None:
        stream = torch.cuda.current_stream(dev)
    shape = (1, S, S, 3) if channels_last else (1, 3, S, S)
    if out is None:
        with torch.cuda.stream(stream):
            out = torch.empty(shape, dtype=torch.float32, device=dev)
    else:
        if not isinstance(out, torch.Tensor):
            raise TypeError("out must be a torch tensor on the handle's device")
        if out.dtype != torch.float32:
            raise TypeError(f"out: dtype {out.dtype} is not supported (float32)")
        if out.device != dev:
            raise ValueError(f"out is on {out.device}, the handle on {dev}")
        if tuple(out.shape) != shape or not out.is_contiguous():
            raise ValueError(f"out: shape {tuple(out.shape)}, expected a contiguous {list(shape)}")
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
    import torch

    dev = torch.device("cuda", int(ef.cfgd["device"]))
    if not isinstance(rgb, torch.Tensor):
        raise TypeError("rgb must be a torch tensor on the handle's device")
    if rgb.dtype != torch.uint8:
        raise TypeError(f"rgb: dtype {rgb.dtype} is not supported (uint8)")
    if rgb.device != dev:
        raise ValueError(f"rgb is on {rgb.device}, the handle on {dev}")
    if rgb.dim() != 3 or rgb.shape[2] != 3 or not rgb.is_contiguous():
        raise ValueError(f"rgb: shape {tuple(rgb.shape)}, expected a contiguous [H,W,3]")
    hh, w = int(rgb.shape[0]), int(rgb.shape[1])
    size, mean3, layout, out, stream = _molded_args(ef, w, hh, min_dim, max_dim, mean, channels_last, out, stream)
    ef._chk(ef.L.ifx_detector_input_molded_image(ef.handle, C.c_void_p(rgb.data_ptr()), w, hh, int(min_dim), int(max_dim), mean3, layout, C.c_void_p(out.data_ptr()),
                                                 int(out.numel()), C.c_void_p(stream.cuda_stream or None)), "ifx_detector_input_molded_image")
    return _molded_result(size, out, w, hh, int(min_dim), int(max_dim))


def _ops_tensor(ef, t, name, dtype, what):
    """the argument checks of the detector operators, as detector_input_image's: TypeError for the dtype, ValueError for device / layout"""
    import torch

    dev = torch.device("cuda", int(ef.cfgd["device"]))
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{name} must be a torch tensor on the handle's device")
    if t.dtype != dtype:
        raise TypeError(f"{name}: dtype {t.dtype} is not supported ({what})")
    if t.device != dev:
        raise ValueError(f"{name} is on {t.device}, the handle on {dev}")
    if not t.is_contiguous():
        raise ValueError(f"{name}: not contiguous")
    return t


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


class ElasticFusion:
    """Mirror of ``ElasticFusion`` / ``ElasticFusionInterface`` for the hot path.  ``id_rule``: ID_RULE_REFERENCE draws the id images with the reference's
    screen-space quad rule (option "id_rule"); None leaves the library's default."""

    def __init__(self, id_rule=None, **cfg):
        self.cfgd = default_config(**cfg)
        self.cfg = IfxConfig(**self.cfgd)
        self.L = lib()
        self.w, self.h = self.cfgd["width"], self.cfgd["height"]
        hp = _P()
        r = self.L.ifx_create(C.byref(self.cfg), C.byref(hp))
        if r != 0:
            raise IfxError(f"ifx_create failed ({r}): {self.L.ifx_global_error().decode()}")
        self.handle = hp
        if id_rule is not None:
            self.set_option("id_rule", id_rule)

    # -- life cycle
    def close(self):
        if getattr(self, "handle", None):
            self.L.ifx_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _chk(self, r, what):
        if r < 0:
            raise IfxError(f"{what} failed ({r}): {self.L.ifx_last_error(self.handle).decode()}")
        return r

    def set_option(self, name, value):
        self._chk(self.L.ifx_set_option(self.handle, name.encode(), int(value)), "ifx_set_option")

    # -- the detector's operators (maskrcnn_benchmark._C.roi_align_forward / _C.nms): caller's tensors, caller's stream, no frame or map state
    def roi_align_forward(self, input, rois, spatial_scale, pooled_h, pooled_w, sampling_ratio, out=None, stream=None):
        """ifx_roi_align_forward: input [B,C,H,W] float32, rois [n,5] float32 (batch index, x0, y0, x1, y1) -> [n,C,pooled_h,pooled_w] float32, bit for bit the
        rule of include/ifx_c_api.h.  Enqueue-only on `stream` (default: the current stream)."""
        import torch

        _ops_tensor(self, input, "input", torch.float32, "float32")
        _ops_tensor(self, rois, "rois", torch.float32, "float32")
        if input.dim() != 4:
            raise ValueError(f"input: shape {tuple(input.shape)}, expected [B,C,H,W]")
        if rois.dim() != 2 or rois.shape[1] != 5:
            raise ValueError(f"rois: shape {tuple(rois.shape)}, expected [n,5]")
        B, Cn, H, W = (int(v) for v in input.shape)
        n, ph, pw = int(rois.shape[0]), int(pooled_h), int(pooled_w)
        if stream is None:
            stream = torch.cuda.current_stream(input.device)
        shape = (n, Cn, max(ph, 0), max(pw, 0))
        if out is None:
            with torch.cuda.stream(stream):
                out = torch.empty(shape, dtype=torch.float32, device=input.device)
        else:
            _ops_tensor(self, out, "out", torch.float32, "float32")
            if tuple(out.shape) != shape:
                raise ValueError(f"out: shape {tuple(out.shape)}, expected {list(shape)}")
        self._chk(self.L.ifx_roi_align_forward(self.handle, C.c_void_p(input.data_ptr()), B, Cn, H, W, C.c_void_p(rois.data_ptr()), n, float(spatial_scale), ph, pw,
                                               int(sampling_ratio), C.c_void_p(out.data_ptr()), C.c_void_p(stream.cuda_stream or None)), "ifx_roi_align_forward")
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
            _ops_tensor(self, f, f"features[{l}]", torch.float32, "float32")
            if f.dim() != 4:
                raise ValueError(f"features[{l}]: shape {tuple(f.shape)}, expected [B,C,H,W]")
            if tuple(f.shape[:2]) != tuple(features[0].shape[:2]):
                raise ValueError(f"features[{l}]: shape {tuple(f.shape)}, expected the batch and channels of features[0], {list(features[0].shape[:2])}")
        _ops_tensor(self, rois, "rois", torch.float32, "float32")
        if rois.dim() != 2 or rois.shape[1] != 5:
            raise ValueError(f"rois: shape {tuple(rois.shape)}, expected [n,5]")
        scales = [float(s) for s in scales]
        if len(scales) != len(features):
            raise ValueError(f"scales: {len(scales)} entries for {len(features)} feature maps")
        nl = len(features)
        B, Cn = int(features[0].shape[0]), int(features[0].shape[1])
        n, ph, pw = int(rois.shape[0]), int(pooled_h), int(pooled_w)
        dev = features[0].device
        if stream is None:
            stream = torch.cuda.current_stream(dev)
        shape = (n, Cn, max(ph, 0), max(pw, 0))
        if out is None:
            with torch.cuda.stream(stream):
                out = torch.empty(shape, dtype=torch.float32, device=dev)
        else:
            _ops_tensor(self, out, "out", torch.float32, "float32")
            if tuple(out.shape) != shape:
                raise ValueError(f"out: shape {tuple(out.shape)}, expected {list(shape)}")
        if levels_out is not None:
            _ops_tensor(self, levels_out, "levels_out", torch.int32, "int32")
            if tuple(levels_out.shape) != (n,):
                raise ValueError(f"levels_out: shape {tuple(levels_out.shape)}, expected [{n}]")
        ptrs = (C.c_void_p * nl)(*[f.data_ptr() for f in features])
        hs = (C.c_int32 * nl)(*[int(f.shape[2]) for f in features])
        ws = (C.c_int32 * nl)(*[int(f.shape[3]) for f in features])
        sc = (C.c_float * nl)(*scales)
        self._chk(self.L.ifx_fpn_roi_align(self.handle, ptrs, hs, ws, sc, nl, B, Cn, C.c_void_p(rois.data_ptr()), n, float(canonical_scale), int(canonical_level),
                                           float(eps), ph, pw, int(sampling_ratio), C.c_void_p(out.data_ptr()),
                                           None if levels_out is None else C.c_void_p(levels_out.data_ptr()), C.c_void_p(stream.cuda_stream or None)),
                  "ifx_fpn_roi_align")
        return out

    def nms(self, boxes, scores, threshold, groups=None, stream=None, padded=False):
        """ifx_nms: boxes [n,4] float32 (x0, y0, x1, y1), scores [n] float32, groups None or [n] int32 -> the kept indices, ascending (int64 tensor); a box
        suppresses the later boxes of its own group whose IoU is > threshold.  Order, pair mask and reduction run on the device; the 4-byte read of the count is
        this method's only synchronisation, and padded=True returns (keep [n] with -1 behind the kept indices, count [1] int32) without it."""
        import torch

        _ops_tensor(self, boxes, "boxes", torch.float32, "float32")
        _ops_tensor(self, scores, "scores", torch.float32, "float32")
        if boxes.dim() != 2 or boxes.shape[1] != 4:
            raise ValueError(f"boxes: shape {tuple(boxes.shape)}, expected [n,4]")
        n = int(boxes.shape[0])
        if scores.dim() != 1 or int(scores.shape[0]) != n:
            raise ValueError(f"scores: shape {tuple(scores.shape)}, expected [{n}]")
        if groups is not None:
            _ops_tensor(self, groups, "groups", torch.int32, "int32")
            if groups.dim() != 1 or int(groups.shape[0]) != n:
                raise ValueError(f"groups: shape {tuple(groups.shape)}, expected [{n}]")
        if stream is None:
            stream = torch.cuda.current_stream(boxes.device)
        with torch.cuda.stream(stream):
            keep = torch.empty(n, dtype=torch.int64, device=boxes.device)
            count = torch.empty(1, dtype=torch.int32, device=boxes.device)
        self._chk(self.L.ifx_nms(self.handle, C.c_void_p(boxes.data_ptr()), C.c_void_p(scores.data_ptr()), None if groups is None else C.c_void_p(groups.data_ptr()), n,
                                 float(threshold), C.c_void_p(keep.data_ptr()), C.c_void_p(count.data_ptr()), C.c_void_p(stream.cuda_stream or None)), "ifx_nms")
        if padded:
            return keep, count
        with torch.cuda.stream(stream):
            return keep[:int(count.item())]

    # -- the RPN's proposal stage and box decoding (RPNPostProcessor.forward_for_single_feature_map / BoxCoder.decode): caller's tensors, caller's stream
    def rpn_proposals(self, objectness, box_regression, anchors, image_size, pre_nms_top_n=6000, post_nms_top_n=1000, nms_thresh=0.7, min_size=0, weights=(1, 1, 1, 1),
                      padded=False, stream=None):
        """ifx_rpn_proposals, one level of one image: objectness [A,H,W] (or [1,A,H,W]), box_regression [4A,H,W] (or [1,4A,H,W]), anchors [H*W*A,4] in the
        reference's order, image_size (width, height) -> (boxes [c,4], objectness [c], index [c] int64): the proposals in descending objectness, torch.sigmoid of
        their logits, and their flat anchor indices, by the rule of include/ifx_c_api.h.  Everything runs on the device; the 4-byte read of the count is this
        method's only synchronisation, and padded=True returns the uncut [post_nms_top_n] tensors and a fourth value count [1] int32 without it."""
        import torch

        _ops_tensor(self, objectness, "objectness", torch.float32, "float32")
        _ops_tensor(self, box_regression, "box_regression", torch.float32, "float32")
        _ops_tensor(self, anchors, "anchors", torch.float32, "float32")
        if objectness.dim() == 4 and objectness.shape[0] == 1:
            objectness = objectness[0]
        if box_regression.dim() == 4 and box_regression.shape[0] == 1:
            box_regression = box_regression[0]
        if objectness.dim() != 3:
            raise ValueError(f"objectness: shape {tuple(objectness.shape)}, expected [A,H,W] or [1,A,H,W]")
        A, H, W = (int(v) for v in objectness.shape)
        if tuple(box_regression.shape) != (4 * A, H, W):
            raise ValueError(f"box_regression: shape {tuple(box_regression.shape)}, expected [{4 * A},{H},{W}]")
        if tuple(anchors.shape) != (A * H * W, 4):
            raise ValueError(f"anchors: shape {tuple(anchors.shape)}, expected [{A * H * W},4]")
        p = RpnParams()
        p.pre_nms_top_n, p.post_nms_top_n, p.nms_thresh, p.min_size = int(pre_nms_top_n), int(post_nms_top_n), float(nms_thresh), float(min_size)
        p.weights[:] = [float(v) for v in weights]
        p.xform_clip = 0.0
        p.image_w, p.image_h = int(image_size[0]), int(image_size[1])
        post = max(p.post_nms_top_n, 0)
        if stream is None:
            stream = torch.cuda.current_stream(objectness.device)
        with torch.cuda.stream(stream):
            boxes = torch.empty((post, 4), dtype=torch.float32, device=objectness.device)
            logits = torch.empty(post, dtype=torch.float32, device=objectness.device)
            index = torch.empty(post, dtype=torch.int64, device=objectness.device)
            count = torch.empty(1, dtype=torch.int32, device=objectness.device)
        self._chk(self.L.ifx_rpn_proposals(self.handle, C.c_void_p(objectness.data_ptr()), C.c_void_p(box_regression.data_ptr()), C.c_void_p(anchors.data_ptr()), A, H, W,
                                           C.byref(p), C.c_void_p(boxes.data_ptr()), C.c_void_p(logits.data_ptr()), C.c_void_p(index.data_ptr()),
                                           C.c_void_p(count.data_ptr()), C.c_void_p(stream.cuda_stream or None)), "ifx_rpn_proposals")
        with torch.cuda.stream(stream):
            if padded:
                return boxes, torch.sigmoid(logits), index, count
            c = int(count.item())
            return boxes[:c], torch.sigmoid(logits[:c]), index[:c]

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
            o, r, a = objectness[l], box_regression[l], anchors[l]
            _ops_tensor(self, o, f"objectness[{l}]", torch.float32, "float32")
            _ops_tensor(self, r, f"box_regression[{l}]", torch.float32, "float32")
            _ops_tensor(self, a, f"anchors[{l}]", torch.float32, "float32")
            if o.dim() == 4 and o.shape[0] == 1:
                o = o[0]
            if r.dim() == 4 and r.shape[0] == 1:
                r = r[0]
            if o.dim() != 3:
                raise ValueError(f"objectness[{l}]: shape {tuple(o.shape)}, expected [A,H,W] or [1,A,H,W]")
            A, H, W = (int(v) for v in o.shape)
            if tuple(r.shape) != (4 * A, H, W):
                raise ValueError(f"box_regression[{l}]: shape {tuple(r.shape)}, expected [{4 * A},{H},{W}]")
            if tuple(a.shape) != (A * H * W, 4):
                raise ValueError(f"anchors[{l}]: shape {tuple(a.shape)}, expected [{A * H * W},4]")
            lv[l].objectness, lv[l].regression, lv[l].anchors = o.data_ptr() or None, r.data_ptr() or None, a.data_ptr() or None
            lv[l].A, lv[l].H, lv[l].W = A, H, W
        p = RpnParams()
        p.pre_nms_top_n, p.post_nms_top_n, p.nms_thresh, p.min_size = int(pre_nms_top_n), int(post_nms_top_n), float(nms_thresh), float(min_size)
        p.weights[:] = [float(v) for v in weights]
        p.xform_clip = 0.0
        p.image_w, p.image_h = int(image_size[0]), int(image_size[1])
        F = p.post_nms_top_n if fpn_post_nms_top_n is None else int(fpn_post_nms_top_n)
        rows = max(F, 0)
        dev = objectness[0].device
        if stream is None:
            stream = torch.cuda.current_stream(dev)
        with torch.cuda.stream(stream):
            boxes = torch.empty((rows, 4), dtype=torch.float32, device=dev)
            logits = torch.empty(rows, dtype=torch.float32, device=dev)
            level = torch.empty(rows, dtype=torch.int32, device=dev)
            index = torch.empty(rows, dtype=torch.int64, device=dev)
            count = torch.empty(1, dtype=torch.int32, device=dev)
            level_counts = torch.empty(nl, dtype=torch.int32, device=dev)
        self._chk(self.L.ifx_rpn_proposals_fpn(self.handle, lv, nl, C.byref(p), F, C.c_void_p(boxes.data_ptr()), C.c_void_p(logits.data_ptr()),
                                               C.c_void_p(level.data_ptr()), C.c_void_p(index.data_ptr()), C.c_void_p(count.data_ptr()),
                                               C.c_void_p(level_counts.data_ptr()), C.c_void_p(stream.cuda_stream or None)), "ifx_rpn_proposals_fpn")
        with torch.cuda.stream(stream):
            if padded:
                return boxes, torch.sigmoid(logits), level, index, count, level_counts
            c = int(count.item())
            return boxes[:c], torch.sigmoid(logits[:c]), level[:c], index[:c]

    def box_decode(self, codes, boxes, weights=(1, 1, 1, 1), clip_to=None, out=None, stream=None):
        """ifx_box_decode: codes [n,4k] float32 against boxes [n,4] float32 -> [n,4k] float32, BoxCoder.decode by the rule of include/ifx_c_api.h (k = 81 and
        weights (10, 10, 5, 5): the box head).  clip_to (width, height): BoxList.clip_to_image on top.  Enqueue-only on `stream` (default: the current stream)."""
        import torch

        _ops_tensor(self, codes, "codes", torch.float32, "float32")
        _ops_tensor(self, boxes, "boxes", torch.float32, "float32")
        if boxes.dim() != 2 or boxes.shape[1] != 4:
            raise ValueError(f"boxes: shape {tuple(boxes.shape)}, expected [n,4]")
        n = int(boxes.shape[0])
        if codes.dim() != 2 or int(codes.shape[0]) != n or codes.shape[1] % 4 or codes.shape[1] == 0:
            raise ValueError(f"codes: shape {tuple(codes.shape)}, expected [{n},4k]")
        if stream is None:
            stream = torch.cuda.current_stream(codes.device)
        if out is None:
            with torch.cuda.stream(stream):
                out = torch.empty_like(codes)
        else:
            _ops_tensor(self, out, "out", torch.float32, "float32")
            if tuple(out.shape) != tuple(codes.shape):
                raise ValueError(f"out: shape {tuple(out.shape)}, expected {list(codes.shape)}")
        w = (C.c_float * 4)(*[float(v) for v in weights])
        cw, ch = (0, 0) if clip_to is None else (int(clip_to[0]), int(clip_to[1]))
        self._chk(self.L.ifx_box_decode(self.handle, C.c_void_p(codes.data_ptr()), C.c_void_p(boxes.data_ptr()), n, int(codes.shape[1]) // 4, C.byref(w), 0.0, cw, ch,
                                        C.c_void_p(out.data_ptr()), C.c_void_p(stream.cuda_stream or None)), "ifx_box_decode")
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

        _ops_tensor(self, class_logits, "class_logits", torch.float32, "float32")
        _ops_tensor(self, box_regression, "box_regression", torch.float32, "float32")
        _ops_tensor(self, proposals, "proposals", torch.float32, "float32")
        if class_logits.dim() != 2:
            raise ValueError(f"class_logits: shape {tuple(class_logits.shape)}, expected [R,C]")
        R, Cn = (int(v) for v in class_logits.shape)
        if box_regression.dim() != 2 or int(box_regression.shape[0]) != R or int(box_regression.shape[1]) not in (4, 4 * Cn):
            raise ValueError(f"box_regression: shape {tuple(box_regression.shape)}, expected [{R},{4 * Cn}] or [{R},4]")
        if tuple(proposals.shape) != (R, 4):
            raise ValueError(f"proposals: shape {tuple(proposals.shape)}, expected [{R},4]")
        p = BoxDetParams()
        p.score_thresh, p.nms, p.detections_per_img = float(score_thresh), float(nms), int(detections_per_img)
        p.max_out = int(max_out) if max_out is not None else (p.detections_per_img if p.detections_per_img > 0 else 8192)
        p.weights[:] = [float(v) for v in weights]
        p.xform_clip = 0.0
        p.image_w, p.image_h = int(image_size[0]), int(image_size[1])
        rows = max(p.max_out, 0)
        if stream is None:
            stream = torch.cuda.current_stream(class_logits.device)
        with torch.cuda.stream(stream):
            dev = class_logits.device
            boxes = torch.empty((rows, 4), dtype=torch.float32, device=dev)
            scores = torch.empty(rows, dtype=torch.float32, device=dev)
            labels = torch.empty(rows, dtype=torch.int64, device=dev)
            index = torch.empty(rows, dtype=torch.int64, device=dev)
            count = torch.empty(1, dtype=torch.int32, device=dev)
            stats = torch.empty(2, dtype=torch.int32, device=dev)
        self._chk(self.L.ifx_box_detections(self.handle, C.c_void_p(class_logits.data_ptr()), C.c_void_p(box_regression.data_ptr()), C.c_void_p(proposals.data_ptr()),
                                            R, Cn, int(box_regression.shape[1]) // 4, C.byref(p), C.c_void_p(boxes.data_ptr()), C.c_void_p(scores.data_ptr()),
                                            C.c_void_p(labels.data_ptr()), C.c_void_p(index.data_ptr()), C.c_void_p(count.data_ptr()), C.c_void_p(stats.data_ptr()),
                                            C.c_void_p(stream.cuda_stream or None)), "ifx_box_detections")
        if padded:
            return boxes, scores, labels, index, count, stats
        with torch.cuda.stream(stream):
            c = int(count.item())
            if c < 0:
                raise IfxError(f"ifx_box_detections: {int(stats[0].item())} candidates, above the cap of 8192: raise score_thresh")
            c = min(c, rows)
            return boxes[:c], scores[:c], labels[:c], index[:c]

    # -- the mask head's logits to ROI masks, resized boxes and class ids (MaskPostProcessor.forward, BoxList.resize, select_top_predictions)
    def _mask_head_args(self, mask_logits, boxes, scores, labels, in_size, out_size, score_thresh, sort_by_score, count, class_map, stream):
        """validates the mask head's tensors and parameters: (R, C, M, ifx_mask_head_params, stream)"""
        import torch

        _ops_tensor(self, mask_logits, "mask_logits", torch.float32, "float32")
        _ops_tensor(self, boxes, "boxes", torch.float32, "float32")
        _ops_tensor(self, scores, "scores", torch.float32, "float32")
        _ops_tensor(self, labels, "labels", torch.int64, "int64, as box_detections returns them")
        if mask_logits.dim() != 4 or mask_logits.shape[2] != mask_logits.shape[3]:
            raise ValueError(f"mask_logits: shape {tuple(mask_logits.shape)}, expected [R,C,M,M]")
        R, Cn, M = int(mask_logits.shape[0]), int(mask_logits.shape[1]), int(mask_logits.shape[3])
        if not (1 <= M <= 64 and 1 <= Cn <= 1024 and R <= 1024):
            raise ValueError(f"mask_logits: shape {tuple(mask_logits.shape)}, expected R <= 1024, C in 1 .. 1024, M in 1 .. 64")
        if tuple(boxes.shape) != (R, 4):
            raise ValueError(f"boxes: shape {tuple(boxes.shape)}, expected [{R},4]")
        if tuple(scores.shape) != (R,):
            raise ValueError(f"scores: shape {tuple(scores.shape)}, expected [{R}]")
        if tuple(labels.shape) != (R,):
            raise ValueError(f"labels: shape {tuple(labels.shape)}, expected [{R}]")
        if count is not None:
            _ops_tensor(self, count, "count", torch.int32, "int32, as box_detections(padded=True) returns it")
            if int(count.numel()) != 1:
                raise ValueError(f"count: shape {tuple(count.shape)}, expected one element")
        if class_map is not None:
            _ops_tensor(self, class_map, "class_map", torch.int32, "int32")
            if tuple(class_map.shape) != (Cn,):
                raise ValueError(f"class_map: shape {tuple(class_map.shape)}, expected [{Cn}]")
        p = MaskHeadParams()
        p.score_thresh = float(score_thresh)
        if p.score_thresh != p.score_thresh:
            raise ValueError("score_thresh is NaN")
        p.in_w, p.in_h, p.out_w, p.out_h = int(in_size[0]), int(in_size[1]), int(out_size[0]), int(out_size[1])
        if min(p.in_w, p.in_h, p.out_w, p.out_h) < 1:
            raise ValueError(f"in_size {tuple(in_size)}, out_size {tuple(out_size)}: a size < 1")
        p.sort_by_score = 1 if sort_by_score else 0
        if stream is None:
            stream = torch.cuda.current_stream(mask_logits.device)
        return R, Cn, M, p, stream

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
        with torch.cuda.stream(stream):
            dev = mask_logits.device
            masks = torch.empty((R, M, M), dtype=torch.float32, device=dev)
            bout = torch.empty((R, 4), dtype=torch.float32, device=dev)
            cls = torch.empty(R, dtype=torch.int32, device=dev)
            rows = torch.empty(R, dtype=torch.int32, device=dev)
            kept = torch.empty(1, dtype=torch.int32, device=dev)
        self._chk(self.L.ifx_mask_head_select(self.handle, C.c_void_p(mask_logits.data_ptr() or None), C.c_void_p(boxes.data_ptr() or None),
                                              C.c_void_p(scores.data_ptr() or None), C.c_void_p(labels.data_ptr() or None),
                                              None if count is None else C.c_void_p(count.data_ptr()), None if class_map is None else C.c_void_p(class_map.data_ptr()),
                                              R, Cn, M, C.byref(p), C.c_void_p(masks.data_ptr() or None), C.c_void_p(bout.data_ptr() or None),
                                              C.c_void_p(cls.data_ptr() or None), C.c_void_p(rows.data_ptr() or None), C.c_void_p(kept.data_ptr()),
                                              C.c_void_p(stream.cuda_stream or None)), "ifx_mask_head_select")
        if padded:
            return masks, bout, cls, rows, kept
        with torch.cuda.stream(stream):
            k = int(kept.item())
            return masks[:k], bout[:k], cls[:k], rows[:k]

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
            _ops_tensor(self, class_map, "class_map", torch.int32, "int32")
            if tuple(class_map.shape) != (Cn,):
                raise ValueError(f"class_map: shape {tuple(class_map.shape)}, expected [{Cn}]")
        win = np.ascontiguousarray([int(v) for v in window], np.int32)
        if win.shape != (4,) or win[2] <= win[0] or win[3] <= win[1]:
            raise ValueError(f"window {tuple(window)}: four integers (y1, x1, y2, x2) with y2 > y1 and x2 > x1")
        if stream is None:
            stream = torch.cuda.current_stream(mrcnn_mask.device)
        return R, M, Cn, flag, win, stream

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
        with torch.cuda.stream(stream):
            dev = mrcnn_mask.device
            masks = torch.empty((R, H, W), dtype=torch.uint8, device=dev)
            cls = torch.empty(R, dtype=torch.int32, device=dev)
            boxes = torch.empty((R, 4), dtype=torch.int32, device=dev)
            scores = torch.empty(R, dtype=torch.float32, device=dev)
            rows = torch.empty(R, dtype=torch.int32, device=dev)
            kept = torch.empty(1, dtype=torch.int32, device=dev)
        self._chk(self.L.ifx_unmold_detections(self.handle, C.c_void_p(detections.data_ptr() or None), C.c_void_p(mrcnn_mask.data_ptr() or None), _ptr(win),
                                               None if class_map is None else C.c_void_p(class_map.data_ptr()), R, M, Cn, flag, W, H,
                                               C.c_void_p(masks.data_ptr() or None), C.c_void_p(cls.data_ptr() or None), C.c_void_p(boxes.data_ptr() or None),
                                               C.c_void_p(scores.data_ptr() or None), C.c_void_p(rows.data_ptr() or None), C.c_void_p(kept.data_ptr()),
                                               C.c_void_p(stream.cuda_stream or None)), "ifx_unmold_detections")
        if padded:
            return masks, cls, boxes, scores, rows, kept
        with torch.cuda.stream(stream):
            k = int(kept.item())
            return masks[:k], cls[:k], boxes[:k], scores[:k], rows[:k]

    # -- the default detector's three layers that are no convolutions (deps/mask_rcnn/model.py: ProposalLayer, PyramidROIAlign, DetectionLayer)
    def _keras_stream(self, t, stream):
        import torch

        return torch.cuda.current_stream(t.device) if stream is None else stream

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
        _ops_tensor(self, rpn_bbox, "rpn_bbox", torch.float32, "float32")
        _ops_tensor(self, anchors, "anchors", torch.float32, "float32")
        batched = rpn_probs.dim() == 3
        if rpn_probs.dim() not in (2, 3) or rpn_probs.shape[-1] != 2:
            raise ValueError(f"rpn_probs: shape {tuple(rpn_probs.shape)}, expected [n,2] or [B,n,2]")
        n = int(rpn_probs.shape[-2])
        lead = tuple(rpn_probs.shape[:-2])
        if tuple(rpn_bbox.shape) != lead + (n, 4):
            raise ValueError(f"rpn_bbox: shape {tuple(rpn_bbox.shape)}, expected {list(lead + (n, 4))}")
        if tuple(anchors.shape) != (n, 4):
            raise ValueError(f"anchors: shape {tuple(anchors.shape)}, expected [{n},4]")
        p = KerasProposalParams()
        p.pre_nms_limit, p.proposal_count, p.nms_threshold = int(pre_nms_limit), int(proposal_count), float(nms_threshold)
        p.std_dev[:] = [float(v) for v in std_dev]
        p.image_h, p.image_w = int(image_shape[0]), int(image_shape[1])
        rows = max(p.proposal_count, 0)
        B = int(lead[0]) if batched else 1
        stream = self._keras_stream(rpn_probs, stream)
        dev = rpn_probs.device
        if out is None:
            with torch.cuda.stream(stream):
                out = torch.empty(lead + (rows, 4), dtype=torch.float32, device=dev)
        else:
            _ops_tensor(self, out, "out", torch.float32, "float32")
            if tuple(out.shape) != lead + (rows, 4):
                raise ValueError(f"out: shape {tuple(out.shape)}, expected {list(lead + (rows, 4))}")
        with torch.cuda.stream(stream):
            index = torch.empty(lead + (rows,), dtype=torch.int64, device=dev)
            count = torch.empty(B, dtype=torch.int32, device=dev)
        e = 4                                       # bytes of a float32 / int32
        for b in range(B):
            self._chk(self.L.ifx_keras_proposals(self.handle, C.c_void_p(rpn_probs.data_ptr() + b * n * 2 * e), C.c_void_p(rpn_bbox.data_ptr() + b * n * 4 * e),
                                                 C.c_void_p(anchors.data_ptr()), n, C.byref(p), C.c_void_p(out.data_ptr() + b * rows * 4 * e),
                                                 C.c_void_p(index.data_ptr() + b * rows * 8), C.c_void_p(count.data_ptr() + b * e),
                                                 C.c_void_p(stream.cuda_stream or None)), "ifx_keras_proposals")
        if padded or batched:
            return out, index, count
        with torch.cuda.stream(stream):
            c = int(count.item())
            return out[:c], index[:c]

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
            _ops_tensor(self, f, f"features[{l}]", torch.float32, "float32")
            if f.dim() != 4:
                raise ValueError(f"features[{l}]: shape {tuple(f.shape)}, expected four dimensions")
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
        shape = lead + ((max(ph, 0), max(pw, 0), Cn) if nhwc else (Cn, max(ph, 0), max(pw, 0)))
        stream = self._keras_stream(boxes, stream)
        if out is None:
            with torch.cuda.stream(stream):
                out = torch.empty(shape, dtype=torch.float32, device=boxes.device)
        else:
            _ops_tensor(self, out, "out", torch.float32, "float32")
            if tuple(out.shape) != shape:
                raise ValueError(f"out: shape {tuple(out.shape)}, expected {list(shape)}")
        if levels_out is not None:
            _ops_tensor(self, levels_out, "levels_out", torch.int32, "int32")
            if tuple(levels_out.shape) != lead:
                raise ValueError(f"levels_out: shape {tuple(levels_out.shape)}, expected {list(lead)}")
        if n == 0:
            return out
        hw = (1, 2) if nhwc else (2, 3)
        ptrs = (C.c_void_p * 4)(*[f.data_ptr() for f in features])
        hs = (C.c_int32 * 4)(*[int(f.shape[hw[0]]) for f in features])
        ws = (C.c_int32 * 4)(*[int(f.shape[hw[1]]) for f in features])
        self._chk(self.L.ifx_pyramid_roi_align(self.handle, ptrs, hs, ws, B, Cn, 1 if nhwc else 0, C.c_void_p(boxes.data_ptr()), n, int(image_shape[0]),
                                               int(image_shape[1]), ph, pw, C.c_void_p(out.data_ptr() or None),
                                               None if levels_out is None else C.c_void_p(levels_out.data_ptr()), C.c_void_p(stream.cuda_stream or None)),
                  "ifx_pyramid_roi_align")
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

        _ops_tensor(self, rois, "rois", torch.float32, "float32")
        _ops_tensor(self, probs, "probs", torch.float32, "float32")
        _ops_tensor(self, deltas, "deltas", torch.float32, "float32")
        batched = probs.dim() == 3
        if probs.dim() not in (2, 3):
            raise ValueError(f"probs: shape {tuple(probs.shape)}, expected [R,C] or [B,R,C]")
        lead = tuple(int(v) for v in probs.shape[:-2])
        R, Cn = int(probs.shape[-2]), int(probs.shape[-1])
        if tuple(rois.shape) != lead + (R, 4):
            raise ValueError(f"rois: shape {tuple(rois.shape)}, expected {list(lead + (R, 4))}")
        if tuple(deltas.shape) != lead + (R, Cn, 4):
            raise ValueError(f"deltas: shape {tuple(deltas.shape)}, expected {list(lead + (R, Cn, 4))}")
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
        stream = self._keras_stream(probs, stream)
        dev = probs.device
        if out is None:
            with torch.cuda.stream(stream):
                out = torch.empty(lead + (rows, 6), dtype=torch.float32, device=dev)
        else:
            _ops_tensor(self, out, "out", torch.float32, "float32")
            if tuple(out.shape) != lead + (rows, 6):
                raise ValueError(f"out: shape {tuple(out.shape)}, expected {list(lead + (rows, 6))}")
        with torch.cuda.stream(stream):
            norm = torch.empty(lead + (rows, 4), dtype=torch.float32, device=dev)
            index = torch.empty(lead + (rows,), dtype=torch.int64, device=dev)
            count = torch.empty(B, dtype=torch.int32, device=dev)
        e = 4
        for b in range(B):
            p.window[:] = [float(v) for v in win[b]]
            self._chk(self.L.ifx_keras_detections(self.handle, C.c_void_p(rois.data_ptr() + b * R * 4 * e), C.c_void_p(probs.data_ptr() + b * R * Cn * e),
                                                  C.c_void_p(deltas.data_ptr() + b * R * Cn * 4 * e), R, Cn, C.byref(p), C.c_void_p(out.data_ptr() + b * rows * 6 * e),
                                                  C.c_void_p(norm.data_ptr() + b * rows * 4 * e), C.c_void_p(index.data_ptr() + b * rows * 8),
                                                  C.c_void_p(count.data_ptr() + b * e), C.c_void_p(stream.cuda_stream or None)), "ifx_keras_detections")
        if padded or batched:
            return out, norm, index, count
        with torch.cuda.stream(stream):
            c = int(count.item())
            return out[:c], norm[:c], index[:c]

    # -- frame entry (ElasticFusion::processFrame)
    def set_instance_gt(self, gt):
        """instanceGT of ElasticFusion::processFrame for the frames that follow (H x W uint8, None: off)."""
        self._chk(self.L.ifx_set_instance_gt(self.handle, None if gt is None else _ptr(np.ascontiguousarray(gt, np.uint8))), "ifx_set_instance_gt")

    def processFrame(self, rgb, depth, timestamp=0, smallInstanceTable=None, instanceGT=None, inPose=None, weightMultiplier=1.0, bootstrap=False):
        """ElasticFusion::processFrame (EF/ElasticFusion.h:75-82), same argument order and meaning."""
        rgb = np.ascontiguousarray(rgb, np.uint8)
        depth = np.ascontiguousarray(depth, np.uint16)
        assert rgb.size == self.w * self.h * 3 and depth.size == self.w * self.h
        if instanceGT is not None:
            self.set_instance_gt(instanceGT)
        out = np.zeros(16, np.float32)
        ip = None if inPose is None else np.ascontiguousarray(inPose, np.float32).reshape(16)
        tab = None if smallInstanceTable is None else np.ascontiguousarray(smallInstanceTable, np.int32)
        self._chk(self.L.ifx_process_frame_ex(self.handle, _ptr(rgb), _ptr(depth), int(timestamp), _ptr(tab), _ptr(ip), float(weightMultiplier), int(bool(bootstrap)), _ptr(out)),
                  "ifx_process_frame_ex")
        return out.reshape(4, 4)

    process_frame = processFrame

    def hint_next_frame(self, rgb, depth):
        """Announce the frame after the one about to be processed, host arrays (see ifx_hint_next_frame): pass the SAME arrays to the next processFrame."""
        rgb = np.ascontiguousarray(rgb, np.uint8)
        depth = np.ascontiguousarray(depth, np.uint16)
        assert rgb.size == self.w * self.h * 3 and depth.size == self.w * self.h
        self._chk(self.L.ifx_hint_next_frame(self.handle, _ptr(rgb), _ptr(depth)), "ifx_hint_next_frame")

    def enqueue_frame_device(self, d_rgb_ptr: int, d_depth_ptr: int, timestamp=0):
        self._chk(self.L.ifx_enqueue_frame_device(self.handle, C.c_void_p(d_rgb_ptr), C.c_void_p(d_depth_ptr), int(timestamp), None, 1.0),
                  "ifx_enqueue_frame_device")

    def prefetch_frame_device(self, d_rgb_ptr: int, d_depth_ptr: int):
        """One-frame look-ahead: frame side of the NEXT frame on the side stream (see ifx_prefetch_frame_device)."""
        self._chk(self.L.ifx_prefetch_frame_device(self.handle, C.c_void_p(d_rgb_ptr), C.c_void_p(d_depth_ptr)), "ifx_prefetch_frame_device")

    def hint_next_frame_device(self, d_rgb_ptr: int, d_depth_ptr: int):
        """Announce the frame after the one about to be enqueued (see ifx_hint_next_frame_device)."""
        self._chk(self.L.ifx_hint_next_frame_device(self.handle, C.c_void_p(d_rgb_ptr), C.c_void_p(d_depth_ptr)), "ifx_hint_next_frame_device")

    def camera_count(self, k):
        self._chk(self.L.ifx_camera_count(self.handle, int(k)), "ifx_camera_count")

    def camera_select(self, c):
        self._chk(self.L.ifx_camera_select(self.handle, int(c)), "ifx_camera_select")

    def owner_set_frame_pose(self, pose):
        p = None if pose is None else np.ascontiguousarray(pose, np.float32).reshape(16)
        self._chk(self.L.ifx_owner_set_frame_pose(self.handle, _ptr(p)), "ifx_owner_set_frame_pose")

    def owner_track_ahead(self, cam, tracking_rank, d_rgb_ptr=0, d_depth_ptr=0):
        """ifx_owner_track_ahead: rank `tracking_rank` runs the tracker of camera cam's NEXT frame now, from the camera's parked context (cam = -1: frames served that way so far)"""
        return self._chk(self.L.ifx_owner_track_ahead(self.handle, int(cam), int(tracking_rank), C.c_void_p(d_rgb_ptr), C.c_void_p(d_depth_ptr)), "ifx_owner_track_ahead")

    def owner_frame_phase(self, phase, d_rgb_ptr=0, d_depth_ptr=0):
        """ifx_owner_frame_phase: one phase of a sharded map's frame (the exchanges between the phases are the caller's, or ifx_comm.hip's)"""
        return self._chk(self.L.ifx_owner_frame_phase(self.handle, int(phase), C.c_void_p(d_rgb_ptr), C.c_void_p(d_depth_ptr)), "ifx_owner_frame_phase")

    def owner_set_tracking_rank(self, r):
        self._chk(self.L.ifx_owner_set_tracking_rank(self.handle, int(r)), "ifx_owner_set_tracking_rank")

    def view_list_stats(self):
        out = np.zeros(4, np.int32)
        self._chk(self.L.ifx_view_list_stats(self.handle, _ptr(out)), "ifx_view_list_stats")
        return dict(window=int(out[0]), outside=int(out[1]), scans=int(out[2]), age=int(out[3]))

    def sync(self):
        self._chk(self.L.ifx_sync(self.handle), "ifx_sync")

    def getCurrPose(self):
        out = np.zeros(16, np.float32)
        self._chk(self.L.ifx_get_pose(self.handle, _ptr(out)), "ifx_get_pose")
        return out.reshape(4, 4)

    @property
    def tick(self):
        return self.L.ifx_tick(self.handle)

    def trajectory(self, max_frames=1 << 16):
        out = np.zeros((max_frames, 16), np.float32)
        n = self._chk(self.L.ifx_trajectory(self.handle, _ptr(out), max_frames), "ifx_trajectory")
        return out[:n].reshape(n, 4, 4).copy()

    def tracker_diag(self):
        out = np.zeros(8, np.float32)
        self._chk(self.L.ifx_tracker_diag(self.handle, _ptr(out)), "ifx_tracker_diag")
        return out

    def tracker_fallbacks(self):
        """pyramid levels the persistent Gauss-Newton kernel handed to its one-workgroup fallback so far (0 in a healthy run)"""
        return self._chk(self.L.ifx_tracker_fallbacks(self.handle), "ifx_tracker_fallbacks")

    def tracker_range_exceeded(self):
        """reductions whose totals left the exact range of the tracker's sums so far (0: every pose is order-independent and equals the oracle's)"""
        return self._chk(self.L.ifx_tracker_range_exceeded(self.handle), "ifx_tracker_range_exceeded")

    def tracker_meet_giveups(self):
        """photometric blocks of fused tracker iterations (option rgb_fuse) that stopped waiting at their bounded meeting so far (0 in a healthy run)"""
        return self._chk(self.L.ifx_tracker_meet_giveups(self.handle), "ifx_tracker_meet_giveups")

    # -- local loop-closure detection (closeLoops, countThresh, errThresh, covThresh of the reference constructor)
    def set_loop_closure(self, enable=True, count_thresh=35000, err_thresh=5e-5, cov_thresh=1e-5):
        self._chk(self.L.ifx_set_loop_closure(self.handle, int(enable), int(count_thresh), err_thresh, cov_thresh), "ifx_set_loop_closure")

    def loop_closure_diag(self):
        out = np.zeros(24, np.float32)
        self._chk(self.L.ifx_loop_closure_diag(self.handle, _ptr(out)), "ifx_loop_closure_diag")
        return dict(ran=bool(out[0]), inactive_pixels=int(out[1]), icp_error=float(out[2]), icp_count=float(out[3]), cov_ok=bool(out[4]),
                    accepted=bool(out[5]), est_pose=out[6:22].reshape(4, 4).copy(), cov_max=float(out[22]), candidates=int(out[23]))

    # -- hooks of the deformation an accepted candidate triggers (the graph optimisation itself is the caller's)
    def set_loop_closure_callback(self, fn):
        """fn(ef, lc24) runs inside processFrame when the frame's candidate was accepted (None removes it)."""
        if fn is None:
            self._lc_cb = None
            self._chk(self.L.ifx_set_loop_closure_callback(self.handle, None, None), "ifx_set_loop_closure_callback")
            return

        def tramp(_h, lc, _user):
            try:
                fn(self, np.ctypeslib.as_array(lc, shape=(24,)).copy())
                return 0
            except Exception:      # never unwind through the C frames
                import traceback

                traceback.print_exc()
                return -1

        self._lc_cb = C.CFUNCTYPE(C.c_int, C.c_void_p, C.POINTER(C.c_float), C.c_void_p)(tramp)
        self._chk(self.L.ifx_set_loop_closure_callback(self.handle, C.cast(self._lc_cb, C.c_void_p), None), "ifx_set_loop_closure_callback")

    def sample_graph_model(self, max_n=4096):
        out = np.zeros((max_n, 4), np.float32)
        n = self._chk(self.L.ifx_sample_graph_model(self.handle, _ptr(out), max_n), "ifx_sample_graph_model")
        return out[:n].copy()

    def loop_closure_constraints(self, max_n=4096):
        src, dst, tm = np.zeros((max_n, 3), np.float32), np.zeros((max_n, 3), np.float32), np.zeros(max_n, np.int32)
        n = self._chk(self.L.ifx_loop_closure_constraints(self.handle, _ptr(src), _ptr(dst), _ptr(tm), max_n), "ifx_loop_closure_constraints")
        return src[:n].copy(), dst[:n].copy(), tm[:n].copy()

    def set_deformation(self, graph16, is_fern=False):
        g = np.ascontiguousarray(graph16, np.float32).reshape(-1, 16)
        self._chk(self.L.ifx_set_deformation(self.handle, _ptr(g), g.shape[0], int(is_fern)), "ifx_set_deformation")

    def adopt_estimated_pose(self):
        self._chk(self.L.ifx_adopt_estimated_pose(self.handle), "ifx_adopt_estimated_pose")

    # -- GPU contacts of the fern data base (EF/Ferns.cpp)
    def set_fern_callback(self, fn):
        """fn(ef) -> truthy when a graph was produced; runs inside processFrame every frame after predict() at the tracked pose
        (Ferns::findFrame + global deformation, EF/ElasticFusion.cpp:457-514).  None removes it."""
        if fn is None:
            self._fern_cb = None
            self._chk(self.L.ifx_set_fern_callback(self.handle, None, None), "ifx_set_fern_callback")
            return

        def tramp(_h, _user):
            try:
                return 1 if fn(self) else 0
            except Exception:      # never unwind through the C frames
                import traceback

                traceback.print_exc()
                return -1

        self._fern_cb = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p)(tramp)
        self._chk(self.L.ifx_set_fern_callback(self.handle, C.cast(self._fern_cb, C.c_void_p), None), "ifx_set_fern_callback")

    def adopt_pose(self, pose):
        p = np.ascontiguousarray(pose, np.float32).reshape(16)
        self._chk(self.L.ifx_adopt_pose(self.handle, _ptr(p)), "ifx_adopt_pose")

    def fern_frame(self):
        """fill-in image / vertex / normal and instance render at (w/8) x (h/8): what Ferns::addFrame / findFrame read back"""
        rw, rh = self.w // 8, self.h // 8
        img, inst = np.zeros((rh, rw, 3), np.uint8), np.zeros((rh, rw, 3), np.uint8)
        v, n = np.zeros((rh, rw, 4), np.float32), np.zeros((rh, rw, 4), np.float32)
        self._chk(self.L.ifx_fern_frame(self.handle, _ptr(img), _ptr(v), _ptr(n), _ptr(inst)), "ifx_fern_frame")
        return img, v, n, inst

    def fern_frame_async(self):
        self._chk(self.L.ifx_fern_frame_async(self.handle), "ifx_fern_frame_async")

    def fern_frame_fetch(self):
        rw, rh = self.w // 8, self.h // 8
        img, inst = np.zeros((rh, rw, 3), np.uint8), np.zeros((rh, rw, 3), np.uint8)
        v, n = np.zeros((rh, rw, 4), np.float32), np.zeros((rh, rw, 4), np.float32)
        self._chk(self.L.ifx_fern_frame_fetch(self.handle, _ptr(img), _ptr(v), _ptr(n), _ptr(inst)), "ifx_fern_frame_fetch")
        return img, v, n, inst

    def track_maps(self, model_v4, model_n4, cur_v4, cur_n4, pose, model_rgba=None, cur_rgba=None):
        a = [np.ascontiguousarray(x, np.float32) for x in (model_v4, model_n4, cur_v4, cur_n4)]
        im = [None if x is None else np.ascontiguousarray(x, np.uint8) for x in (model_rgba, cur_rgba)]
        p = np.ascontiguousarray(pose, np.float32).reshape(16).copy()
        diag = np.zeros(8, np.float32)
        self._chk(self.L.ifx_track_maps(self.handle, _ptr(a[0]), _ptr(a[1]), _ptr(im[0]), _ptr(a[2]), _ptr(a[3]), _ptr(im[1]), _ptr(p), _ptr(diag)), "ifx_track_maps")
        return p.reshape(4, 4), diag

    def mask_compare_map(self, masks, class_ids, unavailable=None):
        """ifx_mask_compare_map: the mask rule of the compare map (the reference's compareMapType 2) as a stage, whatever option compare_map says.
        masks n x H x W uint8 (used as given), class_ids n -> (I, U, best): n x 96 int32 tables and the matched instance per mask (-1: none)."""
        masks = np.ascontiguousarray(masks, np.uint8).reshape(-1, self.h, self.w)
        n = int(masks.shape[0])
        cls = np.ascontiguousarray(class_ids, np.int32)
        un = None if unavailable is None else np.ascontiguousarray(unavailable, np.uint8)
        I, U, best = np.zeros((n, 96), np.int32), np.zeros((n, 96), np.int32), np.full(n, -1, np.int32)
        self._chk(self.L.ifx_mask_compare_map(self.handle, _ptr(masks) if n else None, _ptr(cls) if n else None, n, None if un is None else _ptr(un), _ptr(I), _ptr(U), _ptr(best)),
                  "ifx_mask_compare_map")
        return I, U, best

    # -- map access (getMapSurfelCount / getMapSurfelsGpu / id textures)
    def getMapSurfelCount(self):
        return self._chk(self.L.ifx_map_count(self.handle), "ifx_map_count")

    count = property(getMapSurfelCount)

    @property
    def slots(self):
        return self._chk(self.L.ifx_map_slots(self.handle), "ifx_map_slots")

    def map_view(self):
        v = SoaView()
        self._chk(self.L.ifx_map_view(self.handle, C.byref(v)), "ifx_map_view")
        return v

    def hot_records_stale(self):
        """slots whose gathered copy differed from the store when a frame was about to read it (option hot_verify; 0 unless a kept map_view pointer was written past a frame call)"""
        return self._chk(self.L.ifx_hot_records_stale(self.handle), "ifx_hot_records_stale")

    def download(self, fields=None):
        """the live surfels in map order; `fields`: a subset of (pc, nr, col, tm, ic, votes) -- a 50M-surfel map is 12.8 GB on the host, 9.6 of them votes"""
        n = self.getMapSurfelCount()
        width = dict(pc=4, nr=4, col=2, tm=2, ic=4, votes=48)
        want = tuple(width) if fields is None else tuple(fields)
        d = {k: np.zeros((n, width[k]), np.float32) for k in want}
        args = [(_ptr(d[k]) if k in d else C.c_void_p(None)) for k in ("pc", "nr", "col", "tm", "ic", "votes")]
        m = self._chk(self.L.ifx_map_download(self.handle, n, *args), "ifx_map_download")
        assert m == n
        return d

    def upload(self, m):
        n = m["pc"].shape[0]
        a = {k: np.ascontiguousarray(m[k], np.float32) for k in ("pc", "nr", "col", "tm", "ic", "votes")}
        self._chk(self.L.ifx_map_upload(self.handle, n, _ptr(a["pc"]), _ptr(a["nr"]), _ptr(a["col"]), _ptr(a["tm"]), _ptr(a["ic"]), _ptr(a["votes"])),
                  "ifx_map_upload")

    def set_pose(self, pose, tick):
        p = np.ascontiguousarray(pose, np.float32).reshape(16)
        self._chk(self.L.ifx_set_pose(self.handle, _ptr(p), int(tick)), "ifx_set_pose")

    def seq(self):
        """creation numbers of the live surfels in download() order (a sharded map's shards merge by them into the unsharded map)"""
        n = self.count
        out = np.zeros(max(n, 1), np.uint32)
        m = self._chk(self.L.ifx_map_seq(self.handle, _ptr(out), n), "ifx_map_seq")
        return out[:m]

    def compact(self):
        self._chk(self.L.ifx_compact(self.handle), "ifx_compact")

    def image(self, name):
        dt, ch = _IMG_SPECS[name]
        a = np.zeros((self.h, self.w, ch) if ch > 1 else (self.h, self.w), dt)
        self._chk(self.L.ifx_image_download(self.handle, name.encode(), _ptr(a), a.nbytes), "ifx_image_download")
        return a

    def getSurfelIdsAfterFusion(self):
        return self.image("ids_after")

    # -- map stage API
    def _pose(self, pose):
        return np.ascontiguousarray(pose, np.float32).reshape(16)

    def set_frame(self, rgb, depth):
        rgb = np.ascontiguousarray(rgb, np.uint8)
        depth = np.ascontiguousarray(depth, np.uint16)
        self._chk(self.L.ifx_set_frame(self.handle, _ptr(rgb), _ptr(depth)), "ifx_set_frame")

    def predict_indices(self, pose, time):
        self._chk(self.L.ifx_predict_indices(self.handle, _ptr(self._pose(pose)), int(time)), "ifx_predict_indices")

    def combined_predict(self, pose, time, max_time):
        self._chk(self.L.ifx_combined_predict(self.handle, _ptr(self._pose(pose)), int(time), int(max_time)), "ifx_combined_predict")

    def fuse(self, pose, time, weighting):
        self._chk(self.L.ifx_fuse(self.handle, _ptr(self._pose(pose)), int(time), float(weighting)), "ifx_fuse")

    def clean(self, pose, time):
        self._chk(self.L.ifx_clean(self.handle, _ptr(self._pose(pose)), int(time)), "ifx_clean")

    def render_ids(self, pose, mode=0):
        self._chk(self.L.ifx_render_ids(self.handle, _ptr(self._pose(pose)), int(mode)), "ifx_render_ids")
        return self.image("ids_tmp")

    # -- tracker
    def track_pair(self, model_v4, model_n4, model_rgba, prev_rgb, depth_filtered, rgb, pose):
        p = np.ascontiguousarray(pose, np.float32).reshape(16).copy()
        diag = np.zeros(8, np.float32)
        args = [np.ascontiguousarray(model_v4, np.float32), np.ascontiguousarray(model_n4, np.float32), np.ascontiguousarray(model_rgba, np.uint8),
                None if prev_rgb is None else np.ascontiguousarray(prev_rgb, np.uint8), np.ascontiguousarray(depth_filtered, np.uint16),
                np.ascontiguousarray(rgb, np.uint8)]
        self._chk(self.L.ifx_track_pair(self.handle, *[_ptr(a) for a in args], _ptr(p), _ptr(diag)), "ifx_track_pair")
        return p.reshape(4, 4), diag

    def build_pyramids(self, d_depth_filtered=0, d_rgb=0, d_model_v4=0, d_model_n4=0, d_model_rgba=0, model_pose=None, **out_ptrs):
        """ifx_build_pyramids: device pointers in; out_ptrs: name -> three device pointers (one per level) of caller-allocated dense buffers"""
        pyr = Pyramids()
        for name, ptrs in out_ptrs.items():
            getattr(pyr, name)[:] = [int(x) for x in ptrs]
        pose = None if model_pose is None else np.ascontiguousarray(model_pose, np.float32).reshape(16)
        self._chk(self.L.ifx_build_pyramids(self.handle, C.c_void_p(d_depth_filtered or None), C.c_void_p(d_rgb or None), C.c_void_p(d_model_v4 or None),
                                            C.c_void_p(d_model_n4 or None), C.c_void_p(d_model_rgba or None), None if pose is None else _ptr(pose), C.byref(pyr)), "ifx_build_pyramids")

    def tracker_buffer(self, name, level, m2m=False):
        if m2m:
            dt, ch, planar = _TRK_SPECS[name]
            w, h = self.w >> level, self.h >> level
            a = np.zeros((ch, h, w) if planar else ((h, w, ch) if ch > 1 else (h, w)), dt)
            self._chk(self.L.ifx_tracker_buffer_download(self.handle, ("m2m:" + name).encode(), level, _ptr(a), a.nbytes), "ifx_tracker_buffer_download")
            return a
        return self._tracker_buffer(name, level)

    def _tracker_buffer(self, name, level):
        w, h = self.w >> level, self.h >> level
        if name == "corres":
            a = np.zeros((h, w), CORRES_DTYPE)
        elif name == "cand_n":     # number of valid entries of the bound frame slot's candidate list at this level
            a = np.zeros(1, np.uint32)
        elif name == "cand":       # the valid entries, in the order the device appended them (none in particular)
            a = np.zeros(h * w, CAND_DTYPE)
            self._chk(self.L.ifx_tracker_buffer_download(self.handle, name.encode(), level, _ptr(a), a.nbytes), "ifx_tracker_buffer_download")
            return a[: int(self._tracker_buffer("cand_n", level)[0])].copy()
        else:
            dt, ch, planar = _TRK_SPECS[name]
            a = np.zeros((ch, h, w) if planar else ((h, w, ch) if ch > 1 else (h, w)), dt)
        self._chk(self.L.ifx_tracker_buffer_download(self.handle, name.encode(), level, _ptr(a), a.nbytes), "ifx_tracker_buffer_download")
        return a

    # -- measurement
    def stage_ms(self, reset=False):
        out = np.zeros(4, np.float32)
        self._chk(self.L.ifx_stage_ms(self.handle, _ptr(out), int(reset)), "ifx_stage_ms")
        return dict(track=float(out[0]), fuse=float(out[1]), instance=float(out[2]), preprocess=float(out[3]))

    def lookahead_stats(self, reset=False):
        """ifx_lookahead_stats: frames that found their frame side done / their tracker run ahead / came through ifx_hint_next_frame."""
        out = np.zeros(3, np.int32)
        self._chk(self.L.ifx_lookahead_stats(self.handle, _ptr(out), int(reset)), "ifx_lookahead_stats")
        return dict(side_prepared=int(out[0]), tracked_ahead=int(out[1]), host_hinted=int(out[2]))

    def superpixel_ahead_stats(self, reset=False):
        """Superpixels run ahead of segmentation calls on the side stream (ifx_superpixel_ahead_stats): device ms, runs enqueued, runs a call used."""
        ms = C.c_float(0)
        runs = C.c_int32(0)
        used = C.c_int32(0)
        self._chk(self.L.ifx_superpixel_ahead_stats(self.handle, C.byref(ms), C.byref(runs), C.byref(used), int(reset)), "ifx_superpixel_ahead_stats")
        return dict(ms=float(ms.value), runs=int(runs.value), used=int(used.value))

    def kernel_ms(self, name):
        avg = C.c_float(0)
        n = C.c_int(0)
        self._chk(self.L.ifx_kernel_ms(self.handle, name.encode(), C.byref(avg), C.byref(n)), "ifx_kernel_ms")
        return float(avg.value), int(n.value)


class InstanceFusion:
    """Mirror of the ``InstanceFusion`` class for the hot path; masks come from the caller (replay)."""

    def __init__(self, ef: ElasticFusion):
        self.ef = ef
        self.L = ef.L

    def whetherDoSegmentation(self, frame):
        return bool(self.ef._chk(self.L.ifx_should_segment(self.ef.handle, int(frame)), "ifx_should_segment"))

    def ProcessSegmentation(self, rgb, depth, masks, class_ids, frame, isflann=False, superpixels=False):
        """InstanceFusion::ProcessSegmentation.  rgb = depth = None: the frame most recently processed (still resident on the device) instead of host copies."""
        rgb = None if rgb is None else np.ascontiguousarray(rgb, np.uint8)
        depth = None if depth is None else np.ascontiguousarray(depth, np.uint16)
        self._host_call("ifx_process_segmentation", (_ptr(rgb), _ptr(depth)), masks, class_ids, frame, isflann, superpixels)

    # -- what the entries share: one call shape (a deferred wrapper is its twin with lead=(int(ticket),)), the flags, the producer's stream, class ids on the device
    def _seg_call(self, name, lead, *args):
        return self.ef._chk(getattr(self.L, name)(self.ef.handle, *lead, *args), name)

    @staticmethod
    def _seg_flags(isflann, superpixels):
        return (1 if isflann else 0) | (2 if superpixels else 0)

    def _host_call(self, name, lead, masks, class_ids, frame, isflann, superpixels):
        masks = np.ascontiguousarray(masks, np.uint8)
        cls = np.ascontiguousarray(class_ids, np.int32)
        self._seg_call(name, lead, _ptr(masks), _ptr(cls), int(masks.shape[0]), int(frame), self._seg_flags(isflann, superpixels))

    def _image_call(self, name, lead, masks, class_ids, frame, isflann, superpixels, threshold, stream):
        m, cls, fmt, n, stream = self._device_masks(masks, class_ids, stream)
        self._seg_call(name, lead, C.c_void_p(m.data_ptr() or None), fmt, float(threshold), C.c_void_p(cls.data_ptr() or None), n, int(frame),
                       self._seg_flags(isflann, superpixels), C.c_void_p(stream.cuda_stream or None))
        # (the call returned after its work finished: m and cls may go; they were used on the handle's streams only behind `stream`)

    def _rois_call(self, name, lead, roi_masks, boxes, class_ids, frame, isflann, superpixels, threshold, stream):
        m, M, bx, cls, n, stream = self._device_rois(roi_masks, boxes, class_ids, stream)
        self._seg_call(name, lead, C.c_void_p(m.data_ptr() or None), M, C.c_void_p(bx.data_ptr() or None), float(threshold), C.c_void_p(cls.data_ptr() or None), n, int(frame),
                       self._seg_flags(isflann, superpixels), C.c_void_p(stream.cuda_stream or None))

    def _stage_call(self, name, n, stream, *args):
        """the ingestion alone: (masks in the bridge's order, the same after the overlap clean, the order as input indices, the class ids in that order)"""
        ori = np.zeros((n, self.ef.h, self.ef.w), np.uint8)
        clean = np.zeros_like(ori)
        order, out_cls = np.zeros(n, np.int32), np.zeros(n, np.int32)
        self._seg_call(name, (), *args, n, C.c_void_p(stream.cuda_stream or None), _ptr(ori), _ptr(clean), _ptr(order), _ptr(out_cls))
        return ori, clean, order, out_cls

    def _producer_stream(self, stream):
        """(the handle's torch device, the stream the caller's tensors were written on: the current one by default)"""
        import torch

        dev = torch.device("cuda", int(self.ef.cfgd["device"]))
        return dev, torch.cuda.current_stream(dev) if stream is None else stream

    @staticmethod
    def _device_class_ids(class_ids, dev, n, what):
        """class ids (tensor or sequence) as an int32 [n] tensor on the device; made on the current stream, which the caller has set to the producer's"""
        import torch

        if isinstance(class_ids, torch.Tensor):
            if class_ids.dtype.is_floating_point or class_ids.dtype.is_complex or class_ids.dtype == torch.bool:
                raise TypeError(f"class_ids: dtype {class_ids.dtype} is not an integer type")
            cls = class_ids.to(device=dev, dtype=torch.int32).reshape(-1).contiguous()
        else:
            a = np.asarray(class_ids)
            if a.size and not np.issubdtype(a.dtype, np.integer):
                raise TypeError(f"class_ids: {a.dtype} is not an integer type")
            cls = torch.from_numpy(np.ascontiguousarray(a, np.int32).reshape(-1)).pin_memory().to(dev, non_blocking=True)   # (no host synchronisation on the stream)
        if int(cls.numel()) != n:
            raise ValueError(f"class_ids: {int(cls.numel())} entries for {n} {what}")
        return cls

    def _device_masks(self, masks, class_ids, stream):
        """validates a detector's tensors for the image-mask entries: (contiguous masks, int32 class ids on the device, format, n, stream)"""
        import torch

        dev, stream = self._producer_stream(stream)
        if not isinstance(masks, torch.Tensor):
            raise TypeError("masks must be a torch tensor on the handle's device")
        if masks.dtype in (torch.bool, torch.uint8):
            fmt = MASK_U8
        elif masks.dtype == torch.float32:
            fmt = MASK_F32
        else:
            raise TypeError(f"masks: dtype {masks.dtype} is not supported (bool, uint8 or float32)")
        if masks.device != dev:
            raise ValueError(f"masks are on {masks.device}, the handle on {dev}")
        hw = (self.ef.h, self.ef.w)
        if not ((masks.dim() == 3 and tuple(masks.shape[1:]) == hw) or (masks.dim() == 4 and masks.shape[1] == 1 and tuple(masks.shape[2:]) == hw)):
            raise ValueError(f"masks: shape {tuple(masks.shape)}, expected [N,{hw[0]},{hw[1]}] or [N,1,{hw[0]},{hw[1]}]")
        n = int(masks.shape[0])
        with torch.cuda.stream(stream):          # whatever has to be made on the way is made on the producer's stream
            m = masks.contiguous()
            cls = self._device_class_ids(class_ids, dev, n, "masks")
        return m, cls, fmt, n, stream

    def process_segmentation_device(self, masks, class_ids, frame, isflann=False, superpixels=False, threshold=0.5, stream=None):
        """ProcessSegmentation on a detector's raw output already on the handle's GPU (ifx_process_segmentation_device): no download, no host sort.
        masks: torch tensor [N,H,W] or [N,1,H,W] on the handle's device, in any order; bool / uint8 (inside iff non-zero) or float32 (inside iff > threshold).
        class_ids: N integers (tensor or sequence), each following its mask.  The library applies the bridge's binarisation and stable area sort itself.
        stream: the torch stream the masks were written on (default: the current stream); the call waits for it on the device.  Always the resident frame."""
        self._image_call("ifx_process_segmentation_device", (), masks, class_ids, frame, isflann, superpixels, threshold, stream)

    def ingest_masks(self, masks, class_ids, threshold=0.5, stream=None):
        """The ingestion of process_segmentation_device alone (ifx_ingest_masks): (the 0/255 masks [N,H,W] in the bridge's order, the same after the overlap
        clean, the order as input indices, the class ids in that order), as numpy arrays."""
        m, cls, fmt, n, stream = self._device_masks(masks, class_ids, stream)
        return self._stage_call("ifx_ingest_masks", n, stream, C.c_void_p(m.data_ptr() or None), fmt, float(threshold), C.c_void_p(cls.data_ptr() or None))

    # -- a detector slower than the frame loop: snapshot at the frame the masks belong to, deferred call when they arrive (include/ifx_c_api.h)
    def snapshot(self, superpixels=False):
        """ifx_segmentation_snapshot: pins the id image (as creation numbers), the pose and -- superpixels=True -- the raw frame of the frame just processed, without
        synchronising; returns a ticket for process_segmentation_deferred[_device] / release_snapshot."""
        return self.ef._chk(self.L.ifx_segmentation_snapshot(self.ef.handle, 2 if superpixels else 0), "ifx_segmentation_snapshot")

    def process_segmentation_deferred(self, ticket, masks, class_ids, frame, isflann=False, superpixels=False):
        """ProcessSegmentation of the masks a detector made of the snapshot's frame, on the map as it is now (ifx_process_segmentation_deferred); releases the ticket."""
        self._host_call("ifx_process_segmentation_deferred", (int(ticket),), masks, class_ids, frame, isflann, superpixels)

    def process_segmentation_deferred_device(self, ticket, masks, class_ids, frame, isflann=False, superpixels=False, threshold=0.5, stream=None):
        """The deferred call on a detector's raw output on the handle's GPU: tensors and stream exactly as for process_segmentation_device."""
        self._image_call("ifx_process_segmentation_deferred_device", (int(ticket),), masks, class_ids, frame, isflann, superpixels, threshold, stream)

    # -- the mask head's own output: [N,1,M,M] probabilities and N boxes, pasted on the GPU as maskrcnn-benchmark's Masker does on the CPU (include/ifx_c_api.h)
    def _device_rois(self, roi_masks, boxes, class_ids, stream):
        """validates a mask head's tensors for the ROI entries: (contiguous ROI masks, M, contiguous boxes, int32 class ids on the device, n, stream)"""
        import torch

        dev, stream = self._producer_stream(stream)
        for name, t in (("roi_masks", roi_masks), ("boxes", boxes)):
            if not isinstance(t, torch.Tensor):
                raise TypeError(f"{name} must be a torch tensor on the handle's device")
            if t.dtype != torch.float32:
                raise TypeError(f"{name}: dtype {t.dtype} is not supported (float32)")
            if t.device != dev:
                raise ValueError(f"{name} are on {t.device}, the handle on {dev}")
        sh = tuple(roi_masks.shape)
        if not ((len(sh) == 3 and sh[1] == sh[2]) or (len(sh) == 4 and sh[1] == 1 and sh[2] == sh[3])):
            raise ValueError(f"roi_masks: shape {sh}, expected [N,M,M] or [N,1,M,M]")
        n, M = int(sh[0]), int(sh[-1])
        if not 1 <= M <= 64:
            raise ValueError(f"roi_masks: M = {M}, expected 1 .. 64")
        if tuple(boxes.shape) != (n, 4):
            raise ValueError(f"boxes: shape {tuple(boxes.shape)}, expected [{n},4]")
        with torch.cuda.stream(stream):          # whatever has to be made on the way is made on the producer's stream
            m = roi_masks.contiguous()
            bx = boxes.contiguous()
            cls = self._device_class_ids(class_ids, dev, n, "ROI masks")
        return m, M, bx, cls, n, stream

    def process_segmentation_rois(self, roi_masks, boxes, class_ids, frame, isflann=False, superpixels=False, threshold=0.5, stream=None):
        """ProcessSegmentation on a mask head's own output on the handle's GPU (ifx_process_segmentation_rois): the Masker's paste, the bridge's binarisation and
        its stable area sort all run there.  roi_masks: float32 [N,M,M] or [N,1,M,M] probabilities, M in 1 .. 64; boxes: float32 [N,4] (x0, y0, x1, y1) in frame
        pixel coordinates; class_ids, stream and the resident frame as for process_segmentation_device."""
        self._rois_call("ifx_process_segmentation_rois", (), roi_masks, boxes, class_ids, frame, isflann, superpixels, threshold, stream)

    def process_segmentation_deferred_rois(self, ticket, roi_masks, boxes, class_ids, frame, isflann=False, superpixels=False, threshold=0.5, stream=None):
        """The deferred call on a mask head's own output: tensors and stream exactly as for process_segmentation_rois."""
        self._rois_call("ifx_process_segmentation_deferred_rois", (int(ticket),), roi_masks, boxes, class_ids, frame, isflann, superpixels, threshold, stream)

    # -- the mask head's logits and the box head's detections: select, sigmoid, paste, votes in one call (include/ifx_c_api.h)
    def _detections_call(self, name, lead, mask_logits, boxes, scores, labels, in_size, frame, score_thresh, class_map, count, isflann, superpixels, threshold, stream):
        ef = self.ef
        R, Cn, M, p, stream = ef._mask_head_args(mask_logits, boxes, scores, labels, in_size, (ef.w, ef.h), score_thresh, True, count, class_map, stream)
        kept = C.c_int32(0)
        self._seg_call(name, lead, C.c_void_p(mask_logits.data_ptr() or None), C.c_void_p(boxes.data_ptr() or None), C.c_void_p(scores.data_ptr() or None),
                       C.c_void_p(labels.data_ptr() or None), None if count is None else C.c_void_p(count.data_ptr()),
                       None if class_map is None else C.c_void_p(class_map.data_ptr()), R, Cn, M, C.byref(p), float(threshold), int(frame),
                       self._seg_flags(isflann, superpixels), C.c_void_p(stream.cuda_stream or None), C.byref(kept))
        return int(kept.value)

    def process_segmentation_detections(self, mask_logits, boxes, scores, labels, in_size, frame, score_thresh=0.7, class_map=None, count=None, isflann=False,
                                        superpixels=False, threshold=0.5, stream=None):
        """ProcessSegmentation on the mask head's logits and the box head's detections on the handle's GPU (ifx_process_segmentation_detections):
        ElasticFusion.mask_head_select with sort_by_score and out_size = the frame's size, then process_segmentation_rois on what it keeps -- the reference's
        MaskPostProcessor, resize, select_top_predictions, Masker and bridge.  Tensors as for mask_head_select, written on `stream` (default: the current one);
        threshold is the Masker's.  Returns kept, the number of detections that reached the map; more than 256 raise IfxError (IFX_E_CAPACITY)."""
        return self._detections_call("ifx_process_segmentation_detections", (), mask_logits, boxes, scores, labels, in_size, frame, score_thresh, class_map, count,
                                     isflann, superpixels, threshold, stream)

    def process_segmentation_deferred_detections(self, ticket, mask_logits, boxes, scores, labels, in_size, frame, score_thresh=0.7, class_map=None, count=None,
                                                 isflann=False, superpixels=False, threshold=0.5, stream=None):
        """The deferred call on the mask head's logits: tensors and stream exactly as for process_segmentation_detections; releases the ticket."""
        return self._detections_call("ifx_process_segmentation_deferred_detections", (int(ticket),), mask_logits, boxes, scores, labels, in_size, frame, score_thresh,
                                     class_map, count, isflann, superpixels, threshold, stream)

    # -- the reference's default detector (Keras Mask R-CNN): unmold_detections, the bridge and the votes in one call (include/ifx_c_api.h)
    def _unmolded_call(self, name, lead, detections, mrcnn_mask, window, frame, layout, class_map, isflann, superpixels, stream):
        R, M, Cn, flag, win, stream = self.ef._unmold_args(detections, mrcnn_mask, window, layout, class_map, stream)
        kept = C.c_int32(0)
        self._seg_call(name, lead, C.c_void_p(detections.data_ptr() or None), C.c_void_p(mrcnn_mask.data_ptr() or None), _ptr(win),
                       None if class_map is None else C.c_void_p(class_map.data_ptr()), R, M, Cn, flag, int(frame), self._seg_flags(isflann, superpixels),
                       C.c_void_p(stream.cuda_stream or None), C.byref(kept))
        return int(kept.value)

    def process_segmentation_unmolded(self, detections, mrcnn_mask, window, frame, class_map=None, isflann=False, superpixels=False, layout="nhwc", stream=None):
        """ProcessSegmentation on the default detector's raw output on the handle's GPU (ifx_process_segmentation_unmolded): ElasticFusion.unmold_detections at the
        frame's size, then process_segmentation_device on the masks it keeps -- the reference's MaskRCNN.unmold_detections and bridge (build/mask_ori.py).
        Tensors and window as for unmold_detections (R <= 256), written on `stream` (default: the current one).  Returns kept."""
        return self._unmolded_call("ifx_process_segmentation_unmolded", (), detections, mrcnn_mask, window, frame, layout, class_map, isflann, superpixels, stream)

    def process_segmentation_deferred_unmolded(self, ticket, detections, mrcnn_mask, window, frame, class_map=None, isflann=False, superpixels=False, layout="nhwc",
                                               stream=None):
        """The deferred call on the default detector's raw output: tensors and stream exactly as for process_segmentation_unmolded; releases the ticket."""
        return self._unmolded_call("ifx_process_segmentation_deferred_unmolded", (int(ticket),), detections, mrcnn_mask, window, frame, layout, class_map, isflann,
                                   superpixels, stream)

    def molded_input_size(self, min_dim=800, max_dim=1024):
        """(nw, nh, S, S, top, left, top + nh, left + nw) of detector_input_molded for this handle's frame size (ifx_molded_input_size: host only)"""
        return molded_input_size(self.ef.w, self.ef.h, min_dim, max_dim)

    def detector_input_molded(self, ticket=None, min_dim=800, max_dim=1024, mean=MOLD_MEAN_PIXEL, channels_last=True, out=None, stream=None):
        """ifx_detector_input_molded: what MaskRCNN.mold_inputs (deps/mask_rcnn/model.py:2247-2283) makes of a frame on the CPU -- utils.resize_image's size rule
        and Pillow resize, the centred zero padding to max_dim x max_dim, the mean subtracted, channels last -- bit for bit, from the frame processed last
        (ticket=None) or the frame of a snapshot(superpixels=True) ticket, which is NOT released.  stream, out and the enqueue-only protocol as for detector_input.
        Returns (tensor [1,S,S,3] (channels_last) or [1,3,S,S] float32, window (y1, x1, y2, x2) for the unmold calls, scale)."""
        ef = self.ef
        size, mean3, layout, out, stream = _molded_args(ef, ef.w, ef.h, min_dim, max_dim, mean, channels_last, out, stream)
        ef._chk(self.L.ifx_detector_input_molded(ef.handle, -1 if ticket is None else int(ticket), int(min_dim), int(max_dim), mean3, layout, C.c_void_p(out.data_ptr()),
                                                 int(out.numel()), C.c_void_p(stream.cuda_stream or None)), "ifx_detector_input_molded")
        return _molded_result(size, out, ef.w, ef.h, int(min_dim), int(max_dim))

    def paste_roi_masks(self, roi_masks, boxes, class_ids, threshold=0.5, stream=None):
        """The ingestion of process_segmentation_rois alone (ifx_paste_roi_masks): (the pasted 0/255 masks [N,H,W] in the bridge's order, the same after the
        overlap clean, the order as input indices, the class ids in that order), as numpy arrays."""
        m, M, bx, cls, n, stream = self._device_rois(roi_masks, boxes, class_ids, stream)
        return self._stage_call("ifx_paste_roi_masks", n, stream, C.c_void_p(m.data_ptr() or None), M, C.c_void_p(bx.data_ptr() or None), float(threshold),
                                C.c_void_p(cls.data_ptr() or None))

    # -- the opposite direction: the detector's input tensor from the frame that is already on the device (include/ifx_c_api.h)
    def detector_input_size(self, min_size=800, max_size=None, size_divisible=0):
        """(ow, oh, W', H') of detector_input for this handle's frame size (ifx_detector_input_size: host only)"""
        return detector_input_size(self.ef.w, self.ef.h, min_size, max_size, size_divisible)

    def detector_input(self, ticket=None, min_size=800, max_size=None, size_divisible=0, mean=(102.9801, 115.9465, 122.7717), std=(1., 1., 1.), to_bgr255=True,
                       swap_rb=False, out=None, stream=None):
        """ifx_detector_input: what maskrcnn-benchmark's COCODemo.build_transform + to_image_list make of a frame on the CPU (Pillow's bilinear resize to min_size /
        max_size, ToTensor, x255 and / or channel flip, Normalize, zero padding to a multiple of size_divisible), bit for bit, from the frame processed last
        (ticket=None) or the frame of a snapshot(superpixels=True) ticket, which is NOT released.  Parameters: see detector_prep.
        stream: the CONSUMER's torch stream, the one the detector runs on (default: the current stream).  The call is enqueue-only: the kernel runs on the handle's
        main stream behind whatever `stream` holds so far (an earlier forward pass may still read `out`), and `stream` waits for it on the device; no host
        synchronisation.  out: a [1,3,H',W'] float32 tensor to reuse.  Returns (tensor [1,3,H',W'] float32 on the handle's device, (oh, ow))."""
        p = detector_prep(min_size, max_size, size_divisible, mean, std, to_bgr255, swap_rb)
        size = np.zeros(4, np.int32)
        if self.L.ifx_detector_input_size(self.ef.w, self.ef.h, C.byref(p), _ptr(size)) < 0:
            raise IfxError(f"ifx_detector_input_size: refused (min_size {min_size}, max_size {max_size}, size_divisible {size_divisible}, std {tuple(std)})")
        out, stream = _detector_out(self.ef, size, out, stream)
        self.ef._chk(self.L.ifx_detector_input(self.ef.handle, -1 if ticket is None else int(ticket), C.byref(p), C.c_void_p(out.data_ptr()), int(out.numel()),
                                               C.c_void_p(stream.cuda_stream or None)), "ifx_detector_input")
        return out, (int(size[1]), int(size[0]))

    def release_snapshot(self, ticket):
        self.ef._chk(self.L.ifx_segmentation_snapshot_release(self.ef.handle, int(ticket)), "ifx_segmentation_snapshot_release")

    def snapshot_stats(self, ticket):
        """ifx_segmentation_snapshot_stats: the tick pinned, its pixels with a surfel, of those lost at the last deferred call (-1: none yet), tickets in use"""
        out = np.zeros(4, np.int32)
        self.ef._chk(self.L.ifx_segmentation_snapshot_stats(self.ef.handle, int(ticket), _ptr(out)), "ifx_segmentation_snapshot_stats")
        return dict(tick=int(out[0]), pixels=int(out[1]), lost=int(out[2]), in_use=int(out[3]))

    def set_compare_map_type(self, t):
        """the reference's compareMapType (IF/Core/InstanceFusion.h:227): 1 box IoU (default), 2 mask IoU over dilated pixel sets (option compare_map)"""
        self.ef.set_option("compare_map", int(t))

    def segmentation_matches(self):
        """ifx_segmentation_matches: (best, target) of the last segmentation call -- per mask the compare map's match and the instance it voted for, -1 for none"""
        best, target = np.full(256, -1, np.int32), np.full(256, -1, np.int32)
        n = self.ef._chk(self.L.ifx_segmentation_matches(self.ef.handle, _ptr(best), _ptr(target), 256), "ifx_segmentation_matches")
        return best[:n].copy(), target[:n].copy()

    def labels(self):
        n = self.ef.getMapSurfelCount()
        out = np.zeros(max(n, 1), np.int32)
        m = self.ef._chk(self.L.ifx_labels(self.ef.handle, _ptr(out), n), "ifx_labels")
        return out[:m]

    def precision_recall(self):
        """computePrecisionAndRecall: surfels per instance, per ground-truth id, per (gt, instance)."""
        a, b, c = np.zeros(96, np.int32), np.zeros(256, np.int32), np.zeros((256, 96), np.int32)
        self.ef._chk(self.L.ifx_precision_recall(self.ef.handle, _ptr(a), _ptr(b), _ptr(c)), "ifx_precision_recall")
        return a, b, c

    def renderProjectMap(self):
        """InstanceFusion::renderProjectMap: instance colour under every pixel (H x W x 4 float32)."""
        out = np.zeros((self.ef.h, self.ef.w, 4), np.float32)
        self.ef._chk(self.L.ifx_render_project_map(self.ef.handle, _ptr(out), None), "ifx_render_project_map")
        return out

    def getInstanceTable(self):
        out = np.zeros(96, np.int32)
        self.ef._chk(self.L.ifx_instance_table(self.ef.handle, _ptr(out)), "ifx_instance_table")
        return out

    def getLoopClosureInstanceTable(self):
        out = np.zeros(96 * 5, np.int32)
        self.ef._chk(self.L.ifx_loop_closure_instance_table(self.ef.handle, _ptr(out)), "ifx_loop_closure_instance_table")
        return out.reshape(96, 5)

    # superpixel refinement stages (IF/Core/InstanceFusion_superpixel.cpp)
    def gSLICrInterface(self, rgb):
        rgb = np.ascontiguousarray(rgb, np.uint8)
        seg = np.zeros(rgb.shape[:2], np.int32)
        n = self.ef._chk(self.L.ifx_slic_segment(self.ef.handle, _ptr(rgb), _ptr(seg)), "ifx_slic_segment")
        return seg, n

    def mergeSuperPixel(self, depth, seg):
        depth = np.ascontiguousarray(depth, np.uint16)
        seg = np.ascontiguousarray(seg, np.int32).copy()
        fin = np.zeros_like(seg)
        info = np.zeros((seg.size // 256, 30), np.float32)
        self.ef._chk(self.L.ifx_merge_superpixels(self.ef.handle, _ptr(depth), _ptr(seg), _ptr(fin), _ptr(info)), "ifx_merge_superpixels")
        return seg, fin, info

    def maskSuperPixelFilter_OverSeg(self, fin, masks):
        fin = np.ascontiguousarray(fin, np.int32)
        masks = np.ascontiguousarray(masks, np.uint8).copy()
        self.ef._chk(self.L.ifx_mask_superpixel_filter(self.ef.handle, _ptr(fin), _ptr(masks), int(masks.shape[0])), "ifx_mask_superpixel_filter")
        return masks

    def maskGeometricFilter(self, model_depth, masks, ori, unavailable=None):
        depth = np.ascontiguousarray(model_depth, np.uint16)
        masks = np.ascontiguousarray(masks, np.uint8).copy()
        ori = np.ascontiguousarray(ori, np.uint8)
        un = np.zeros(masks.shape[0], np.uint8) if unavailable is None else np.ascontiguousarray(unavailable, np.uint8).copy()
        self.ef._chk(self.L.ifx_mask_geometric_filter(self.ef.handle, _ptr(depth), _ptr(masks), _ptr(ori), int(masks.shape[0]), _ptr(un)), "ifx_mask_geometric_filter")
        return masks, un

    def computeMapBoundingBox(self, bboxType=True, ratio=1000000.0):
        """InstanceFusion::computeMapBoundingBox: (boxes 96x6, ground normal, ground frame, instance frames, 648 ground votes)"""
        boxes, gn, gc, im, gv = np.zeros((96, 6), np.float32), np.zeros(3, np.float32), np.zeros((4, 4), np.float32), np.zeros((96, 4, 4), np.float32), np.zeros(648, np.int32)
        self.ef._chk(self.L.ifx_map_bounding_boxes(self.ef.handle, int(bool(bboxType)), float(ratio), _ptr(boxes), _ptr(gn), _ptr(gc), _ptr(im), _ptr(gv)), "ifx_map_bounding_boxes")
        return boxes, gn, gc, im, gv

    def getInstancePointCloud(self, inst=-1, bboxType=True, max_records=1 << 20):
        """InstanceFusion::getInstancePointCloud: (surfels per instance, records of `inst` {slot, xyz, normal, rgb})"""
        counts = np.zeros(96, np.int32)
        out = np.zeros((max_records if inst >= 0 else 1, 10), np.float32)
        n = self.ef._chk(self.L.ifx_instance_point_cloud(self.ef.handle, int(bool(bboxType)), _ptr(counts), int(inst), _ptr(out), max_records if inst >= 0 else 0), "ifx_instance_point_cloud")
        return counts, out[:n]

    def flannKnnVoteSurfelMap(self, with_neighbours=False):
        n = self.ef.slots
        nbr = np.full((max(n, 1), 10), -1, np.int32) if with_neighbours else None
        self.ef._chk(self.L.ifx_knn_vote_colour(self.ef.handle, _ptr(nbr) if with_neighbours else None, n if with_neighbours else 0), "ifx_knn_vote_colour")
        return nbr[:n] if with_neighbours else None

    def maskCleanOverlap(self, masks):
        masks = np.ascontiguousarray(masks, np.uint8).copy()
        self.ef._chk(self.L.ifx_mask_clean_overlap(self.ef.handle, _ptr(masks), int(masks.shape[0])), "ifx_mask_clean_overlap")
        return masks
