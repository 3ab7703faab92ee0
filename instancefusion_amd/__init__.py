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


class ViewParams(C.Structure):
    """ifx_view_params: the camera and the flags of ifx_render_view (include/ifx_c_api.h)"""
    _fields_ = [("mvp", C.c_float * 16), ("w", C.c_int32), ("h", C.c_int32), ("threshold", C.c_float), ("color_type", C.c_int32), ("unstable", C.c_int32),
                ("draw_window", C.c_int32), ("time", C.c_int32), ("time_delta", C.c_int32), ("clear_rgb", C.c_float * 3)]


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
    "ifx_owner_segmentation_snapshot": (C.c_int, [_P, C.c_int]),
    "ifx_owner_segmentation_begin_deferred": (C.c_int, [_P, C.c_int, _P, _P, C.c_int, C.c_int, C.c_int]),
    "ifx_owner_segmentation_begin_deferred_device": (C.c_int, [_P, C.c_int, C.c_int, C.c_int, _P, C.c_int, C.c_float, _P, C.c_int, C.c_int, C.c_int, _P]),
    "ifx_owner_process_segmentation_deferred": (C.c_int, [_P, C.c_int, _P, _P, C.c_int, C.c_int, C.c_int]),
    "ifx_owner_process_segmentation_deferred_device": (C.c_int, [_P, C.c_int, C.c_int, C.c_int, _P, C.c_int, C.c_float, _P, C.c_int, C.c_int, C.c_int, _P]),
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
    "ifx_tracker_meet_adopted": (C.c_int, [_P]),
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
    "ifx_combined_predict_ex": (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int]),
    "ifx_reloc_gate": (C.c_int, [_P, _P, C.c_float, _P, _P, _P]),
    "ifx_reloc_state": (C.c_int, [_P, _P]),
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
    "ifx_render_view": (C.c_int, [_P, C.POINTER(ViewParams), _P, _P, _P, _P]),
    "ifx_render_view_big_quads": (C.c_int, [_P]),
    "ifx_owner_render_view_begin": (C.c_int, [_P, C.POINTER(ViewParams), C.c_int, C.c_int]),
    "ifx_owner_render_view_resume": (C.c_int, [_P, _P, _P, _P, _P]),
    "ifx_owner_render_view": (C.c_int, [_P, C.POINTER(ViewParams), _P, _P, _P, _P]),
    "ifx_owner_render_view_big_quads": (C.c_int, [_P]),
    "ifx_set_instance_gt": (C.c_int, [_P, _P]),
    "ifx_precision_recall": (C.c_int, [_P, _P, _P, _P]),
    "ifx_instance_table": (C.c_int, [_P, _P]),
    "ifx_loop_closure_instance_table": (C.c_int, [_P, _P]),
    "ifx_merge_instances": (C.c_int, [_P, _P, C.c_int]),
    "ifx_instance_duplicates": (C.c_int, [_P, C.c_float, _P, C.c_int]),
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
    "ids_after": (np.int32, 1), "ids_tmp": (np.int32, 1), "snap_ids": (np.int32, 1), "index": (np.uint32, 1), "index_vc": (np.float32, 4),
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

# option "id_rule" (include/ifx_c_api.h): which rule draws the surfel-id images
ID_RULE_RAY_DISC = 0     # default: a ray through each pixel centre against the disc, f32 depth keys
ID_RULE_REFERENCE = 1    # the reference's surfel_ids.geom / .frag: screen-space quads, 24-bit depth



def view_params(mvp, size, color_type=None, threshold=None, unstable=False, draw_window=False, time=-1, time_delta=-1, clear_rgb=(1.0, 1.0, 1.0), draw_instances=False,
                draw_times=False, draw_colors=False, draw_normals=False):
    """the ifx_view_params of a render_view call (ElasticFusion.render_view documents the arguments)"""
    p = ViewParams()
    p.mvp[:] = [float(v) for v in np.ascontiguousarray(mvp, np.float32).reshape(16)]
    p.w, p.h = int(size[0]), int(size[1])
    p.threshold = float("nan") if threshold is None else float(threshold)
    p.color_type = int(view_color_type(draw_instances, draw_times, draw_colors, draw_normals) if color_type is None else color_type)
    p.unstable, p.draw_window, p.time, p.time_delta = int(bool(unstable)), int(bool(draw_window)), int(time), int(time_delta)
    p.clear_rgb[:] = [float(v) for v in clear_rgb]
    return p


def viewer_mvp(fx, fy, cx, cy, w, h, near, far, pose):
    """The reference viewer's camera as the 4x4 MVP of ifx_render_view: Pangolin's ProjectionMatrix(w, h, fu, fv, u0, v0, zNear, zFar) times the inverse of
    the (rigid) camera pose -- camera frame y down, z forward.  Computed in f64 and rounded to f32 once.  With the frame's intrinsics at the tracked pose
    the output of render_view has the orientation of pred_image."""
    T = [[float(v) for v in row] for row in np.asarray(pose, np.float64).reshape(4, 4)]
    Ti = [[0.0] * 4 for _ in range(4)]      # R^T, -(R^T t); every sum left to right, as ifx_host.hpp viewerMvp (the two agree bit for bit)
    for i in range(3):
        t = 0.0
        for j in range(3):
            Ti[i][j] = T[j][i]
            t += T[j][i] * T[j][3]
        Ti[i][3] = -t
    Ti[3][3] = 1.0
    fx, fy, cx, cy, w, h, near, far = (float(v) for v in (fx, fy, cx, cy, w, h, near, far))
    P = [[2.0 * fx / w, 0.0, 1.0 - 2.0 * cx / w, 0.0],
         [0.0, -(2.0 * fy / h), -(1.0 - 2.0 * cy / h), 0.0],
         [0.0, 0.0, (far + near) / (far - near), -(2.0 * far * near) / (far - near)],
         [0.0, 0.0, 1.0, 0.0]]
    out = np.zeros((4, 4), np.float64)
    for i in range(4):
        for j in range(4):
            s = 0.0
            for k in range(4):
                s += P[i][k] * Ti[k][j]
            out[i, j] = s
    return out.astype(np.float32)


def view_color_type(draw_instances=False, draw_times=False, draw_colors=False, draw_normals=False):
    """The GUI's flags as colorType, in the order GlobalModel::renderPointCloud resolves them (EF/GlobalModel.cpp:355): instances 4, normals 1, colours 2, times 3, else 0"""
    return 4 if draw_instances else 1 if draw_normals else 2 if draw_colors else 3 if draw_times else 0


# -- the detector side of the binding (detector.py): it needs the names above, and its names are this package's too
from .detector import (DET_SCALE_255, DET_SWAP_RB, MOLD_MEAN_PIXEL, MOLD_NCHW, MOLD_NHWC, UNMOLD_NCHW, UNMOLD_NHWC, _box_post_processor_class,  # noqa: E402,F401
                       _detector_out, _DetectorOperators, _DetectorOps, _device, _dp, _mask_post_processor_class, _molded_args, _molded_result, _ops_tensor, _pooler_class,
                       _rpn_post_processor_class, _sp, _stream_for, box_post_processor, detector_input_image, detector_input_molded_image, detector_input_size,
                       detector_ops, detector_prep, detector_resize_taps, fpn_level_thresholds, mask_post_processor, molded_input_size, pooler,
                       pyramid_level_thresholds, rpn_post_processor)


class ElasticFusion(_DetectorOperators):
    """Mirror of ``ElasticFusion`` / ``ElasticFusionInterface`` for the hot path.  ``id_rule``: ID_RULE_REFERENCE draws the id images with the reference's
    screen-space quad rule (option "id_rule"); None leaves the library's default.  ``reloc`` / ``frame_to_frame_rgb``: the constructor arguments of the same
    names (EF/ElasticFusion.h:47-62; options "reloc" / "frame_to_frame_rgb")."""

    def __init__(self, id_rule=None, reloc=False, frame_to_frame_rgb=False, **cfg):
        self.cfgd = default_config(**cfg)
        self.cfg = IfxConfig(**self.cfgd)
        self.L = lib()
        self.w, self.h = self.cfgd["width"], self.cfgd["height"]
        hp = _P()
        r = self.L.ifx_create(C.byref(self.cfg), C.byref(hp))
        if r != 0:
            raise IfxError(f"ifx_create failed ({r}): {self.L.ifx_global_error().decode()}")
        self.handle = hp
        self.last_frame_status = 0   # what the last processFrame returned: 0 ok, 1 lost (reloc)
        if id_rule is not None:
            self.set_option("id_rule", id_rule)
        if reloc:
            self.set_option("reloc", 1)
        if frame_to_frame_rgb:
            self.set_option("frame_to_frame_rgb", 1)

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
        self.last_frame_status = self._chk(self.L.ifx_process_frame_ex(self.handle, _ptr(rgb), _ptr(depth), int(timestamp), _ptr(tab), _ptr(ip), float(weightMultiplier),
                                                                       int(bool(bootstrap)), _ptr(out)), "ifx_process_frame_ex")
        return out.reshape(4, 4)

    def reloc_state(self):
        """ifx_reloc_state: the last tracking verdict of the relocalisation mode and whether the last frame ran its map passes"""
        o = np.zeros(12, np.float32)
        self._chk(self.L.ifx_reloc_state(self.handle, _ptr(o)), "ifx_reloc_state")
        return dict(ok=bool(o[0]), lost=bool(o[1]), last_frame_recovery=bool(o[2]), tracking_count=int(o[3]), icp_error=float(o[4]), cov_diag=o[5:11].copy(), fused=bool(o[11]))

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

    def tracker_meet_adopted(self):
        """shares of such blocks that the last arriver stepped in their place (option rgb_own; equal to tracker_meet_giveups() in that form, 0 in a healthy run)"""
        return self._chk(self.L.ifx_tracker_meet_adopted(self.handle), "ifx_tracker_meet_adopted")

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

    def render_view(self, mvp, size, color_type=None, threshold=None, unstable=False, draw_window=False, time=-1, time_delta=-1, clear_rgb=(1.0, 1.0, 1.0),
                    draw_instances=False, draw_times=False, draw_colors=False, draw_normals=False, device=False):
        """ifx_render_view: the map drawn from any camera, the reference viewer's surfel pass (GlobalModel::renderPointCloud + renderGlobalID).
        mvp: 4x4 (viewer_mvp builds the reference's); size: (w, h) of the viewport, unrelated to the frame's.  color_type 0..4, or the GUI's flags by
        name (view_color_type).  threshold None / time < 0 / time_delta < 0: the handle's own.  Returns (rgba [h, w, 4] f32, ids [h, w] int32: the slot
        under each pixel in the numbering of ids_after, -1 where nothing was drawn), top row first; device=True: two torch tensors on the GPU."""
        p = view_params(mvp, size, color_type, threshold, unstable, draw_window, time, draw_instances=draw_instances, draw_times=draw_times, draw_colors=draw_colors,
                        draw_normals=draw_normals, time_delta=time_delta, clear_rgb=clear_rgb)
        rgba, ids = self._view_outputs(size, device)
        if device:
            self._chk(self.L.ifx_render_view(self.handle, C.byref(p), None, None, C.c_void_p(rgba.data_ptr()), C.c_void_p(ids.data_ptr())), "ifx_render_view")
            self.sync()
            return rgba, ids
        self._chk(self.L.ifx_render_view(self.handle, C.byref(p), _ptr(rgba), _ptr(ids), None, None), "ifx_render_view")
        return rgba, ids

    def _view_outputs(self, size, device):
        """the two images of a render_view call: numpy arrays, or torch tensors on the handle's GPU whose memory is ours before the handle's stream writes it"""
        w, h = int(size[0]), int(size[1])
        if not (1 <= w <= 4096 and 1 <= h <= 4096):      # (the call refuses other sizes; the buffers only need to exist)
            w = h = 1
        if device:
            import torch
            dev = torch.device("cuda", self.cfgd["device"])
            rgba, ids = torch.empty((h, w, 4), dtype=torch.float32, device=dev), torch.empty((h, w), dtype=torch.int32, device=dev)
            torch.cuda.current_stream(dev).synchronize()
            return rgba, ids
        return np.zeros((h, w, 4), np.float32), np.zeros((h, w), np.int32)

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

    def combined_predict(self, pose, time, max_time, passthrough=0):
        """passthrough: the fill-in stage's mask (bit 0 fill_vertex + fill_normal, bit 1 fill_image take the frame at every pixel; EF/ElasticFusion.cpp:757-759)"""
        self._chk(self.L.ifx_combined_predict_ex(self.handle, _ptr(self._pose(pose)), int(time), int(max_time), int(passthrough)), "ifx_combined_predict_ex")

    def reloc_gate(self, lastA, icp_error, state):
        """The tracking gate of EF/ElasticFusion.cpp:371-423 on the device.  lastA: 6x6 f64; state: (lost, lastFrameRecovery, trackingCount).
        Returns (ok, (lost, lastFrameRecovery, trackingCount), the six diagonals of lastA^-1)."""
        a = np.ascontiguousarray(lastA, np.float64).reshape(36)
        st = np.array([int(bool(state[0])), int(bool(state[1])), int(state[2])], np.int32)
        ok = np.zeros(1, np.int32)
        cov = np.zeros(6, np.float64)
        self._chk(self.L.ifx_reloc_gate(self.handle, _ptr(a), float(icp_error), _ptr(st), _ptr(ok), _ptr(cov)), "ifx_reloc_gate")
        return bool(ok[0]), (bool(st[0]), bool(st[1]), int(st[2])), cov

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


def resolve_merge_pairs(pairs):
    """(from, to) pairs with their chains resolved to the roots (5 -> 3, 3 -> 1 becomes 5 -> 1, 3 -> 1), ascending in from, as [n, 2] int32.  ValueError for a from
    named twice with two targets, or a cycle; from == to and ids outside the table are left for ifx_merge_instances to refuse."""
    pairs = np.asarray(pairs, np.int32).reshape(-1, 2)
    to = {}
    for f, t in pairs.tolist():
        if to.setdefault(f, t) != t:
            raise ValueError(f"instance {f} is merged into two targets")
    out = []
    for f in sorted(to):
        t, steps = to[f], 0
        while t in to and t != f:
            t, steps = to[t], steps + 1
            if steps > len(to):
                break
        if f in to and (t == f and to[f] != f or steps > len(to)):
            raise ValueError(f"the merge pairs form a cycle through instance {f}")
        out.append((f, t))
    return np.asarray(out, np.int32).reshape(-1, 2)


def merge_instances(ef, pairs, resolve=True):
    """ifx_merge_instances on the handle of `ef` (every rank of a sharded map makes the same call); returns the pairs as passed to it"""
    pairs = resolve_merge_pairs(pairs) if resolve else np.ascontiguousarray(np.asarray(pairs, np.int32).reshape(-1, 2))
    ef._chk(ef.L.ifx_merge_instances(ef.handle, _ptr(pairs) if len(pairs) else None, int(len(pairs))), "ifx_merge_instances")
    return pairs


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
        self._seg_call(name, lead, _dp(m), fmt, float(threshold), _dp(cls), n, int(frame), self._seg_flags(isflann, superpixels), _sp(stream))
        # (the call returned after its work finished: m and cls may go; they were used on the handle's streams only behind `stream`)

    def _rois_call(self, name, lead, roi_masks, boxes, class_ids, frame, isflann, superpixels, threshold, stream):
        m, M, bx, cls, n, stream = self._device_rois(roi_masks, boxes, class_ids, stream)
        self._seg_call(name, lead, _dp(m), M, _dp(bx), float(threshold), _dp(cls), n, int(frame), self._seg_flags(isflann, superpixels), _sp(stream))

    def _stage_call(self, name, n, stream, *args):
        """the ingestion alone: (masks in the bridge's order, the same after the overlap clean, the order as input indices, the class ids in that order)"""
        ori = np.zeros((n, self.ef.h, self.ef.w), np.uint8)
        clean = np.zeros_like(ori)
        order, out_cls = np.zeros(n, np.int32), np.zeros(n, np.int32)
        self._seg_call(name, (), *args, n, _sp(stream), _ptr(ori), _ptr(clean), _ptr(order), _ptr(out_cls))
        return ori, clean, order, out_cls

    def _producer_stream(self, stream):
        """(the handle's torch device, the stream the caller's tensors were written on: the current one by default)"""
        return _device(self.ef), _stream_for(self.ef, stream)

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
        return self._stage_call("ifx_ingest_masks", n, stream, _dp(m), fmt, float(threshold), _dp(cls))

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
        self._seg_call(name, lead, _dp(mask_logits), _dp(boxes), _dp(scores), _dp(labels), _dp(count), _dp(class_map), R, Cn, M, C.byref(p), float(threshold),
                       int(frame), self._seg_flags(isflann, superpixels), _sp(stream), C.byref(kept))
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
        self._seg_call(name, lead, _dp(detections), _dp(mrcnn_mask), _ptr(win), _dp(class_map), R, M, Cn, flag, int(frame), self._seg_flags(isflann, superpixels),
                       _sp(stream), C.byref(kept))
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
        ef._chk(self.L.ifx_detector_input_molded(ef.handle, -1 if ticket is None else int(ticket), int(min_dim), int(max_dim), mean3, layout, _dp(out), int(out.numel()),
                                                 _sp(stream)), "ifx_detector_input_molded")
        return _molded_result(size, out, ef.w, ef.h, int(min_dim), int(max_dim))

    def paste_roi_masks(self, roi_masks, boxes, class_ids, threshold=0.5, stream=None):
        """The ingestion of process_segmentation_rois alone (ifx_paste_roi_masks): (the pasted 0/255 masks [N,H,W] in the bridge's order, the same after the
        overlap clean, the order as input indices, the class ids in that order), as numpy arrays."""
        m, M, bx, cls, n, stream = self._device_rois(roi_masks, boxes, class_ids, stream)
        return self._stage_call("ifx_paste_roi_masks", n, stream, _dp(m), M, _dp(bx), float(threshold), _dp(cls))

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
        self.ef._chk(self.L.ifx_detector_input(self.ef.handle, -1 if ticket is None else int(ticket), C.byref(p), _dp(out), int(out.numel()), _sp(stream)),
                     "ifx_detector_input")
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

    # -- duplicate instances after a loop closure (include/ifx_c_api.h: the reference's checkLoopClosure, IF/Core/InstanceTable.cpp:122-169)
    def merge_instances(self, pairs, resolve=True):
        """ifx_merge_instances: pairs of (from, to) -- the votes of `from` are added to `to` in every surfel, `from` leaves the table, labels and colours follow.
        resolve: chains (5 -> 3, 3 -> 1) are first resolved to their roots (5 -> 1, 3 -> 1), which the C entry refuses to guess; a cycle raises ValueError.
        Returns the pairs as merged, [n, 2] int32 ascending in from."""
        return merge_instances(self.ef, pairs, resolve)

    def duplicate_instances(self, iou=0.5):
        """ifx_instance_duplicates: (from, to) for the registered instances of one class whose projected boxes in the current view overlap with I / U > iou,
        resolved to their roots, ascending in from: what merge_instances takes."""
        out = np.zeros((95, 2), np.int32)
        n = self.ef._chk(self.L.ifx_instance_duplicates(self.ef.handle, float(iou), _ptr(out), 95), "ifx_instance_duplicates")
        return out[:n].copy()

    def check_loop_closure(self, table):
        """InstanceFusion::checkLoopClosure: `table` as getLoopClosureInstanceTable gives it ([96, 5] int32), its column 4 the instance every row matches.  Rows whose
        match is another instance are merged into it (chains resolved); the column is reset to the row index in place.  Returns the pairs merged."""
        table = np.asarray(table)
        t = table.reshape(96, 5)
        pairs = [(i, int(t[i, 4])) for i in range(96) if int(t[i, 4]) != i]
        done = self.merge_instances(pairs)
        t[:, 4] = np.arange(96)
        return done

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
