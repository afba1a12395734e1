"""ctypes binding of libbetapose_hip.so (include/betapose_hip.h).

The library is the product: if it is missing it is built in-tree with hipcc, and
if that is impossible the import of any engine class FAILS LOUDLY -- there is no
CPU or eager-PyTorch fallback on the product path.
"""
from __future__ import annotations

import ctypes as C
import os
import threading

_HERE = os.path.dirname(os.path.abspath(__file__))
# BP_LIB: an alternative build of the same library (tools only: `python -m betapose_amd.build --experimental` makes
# libbetapose_hip_exp.so with the measured-and-rejected kernels and the timing ablations compiled in)
LIB_PATH = os.environ.get("BP_LIB") or os.path.join(_HERE, "libbetapose_hip.so")
_lock = threading.Lock()
_lib = None

c_float_p = C.POINTER(C.c_float)
c_double_p = C.POINTER(C.c_double)
c_int_p = C.POINTER(C.c_int)
vp = C.c_void_p

# name -> (restype, argtypes); every symbol include/betapose_hip.h declares
PROTOTYPES = {
    "bp_last_error": (C.c_char_p, []),
    "bp_version": (C.c_int, []),
    "bp_device_count": (C.c_int, []),
    "bp_device_name": (C.c_int, [C.c_int, C.c_char_p, C.c_int]),
    "bp_yolo_create": (C.c_int, [C.c_char_p, C.c_char_p, C.c_int, C.c_int, C.c_int, C.POINTER(vp)]),
    "bp_yolo_create_from_memory": (C.c_int, [C.c_char_p, vp, C.c_size_t, C.c_int, C.c_int, C.c_int, C.POINTER(vp)]),
    "bp_yolo_clone": (C.c_int, [vp, C.POINTER(vp)]),
    "bp_kpd_clone": (C.c_int, [vp, C.POINTER(vp)]),
    "bp_yolo_destroy": (None, [vp]),
    "bp_yolo_rows": (C.c_int, [vp]),
    "bp_yolo_attrs": (C.c_int, [vp]),
    "bp_yolo_forward": (C.c_int, [vp, vp, C.c_int, vp, vp]),
    "bp_yolo_forward_select": (C.c_int, [vp, vp, C.c_int, C.c_float, C.c_int, vp, vp, vp]),
    "bp_yolo_forward_select_classes": (C.c_int, [vp, vp, C.c_int, C.c_float, C.c_int, vp, C.c_int, vp, vp, vp]),
    "bp_yolo_select": (C.c_int, [vp, C.c_int, C.c_int, C.c_int, C.c_float, C.c_int, vp, vp]),
    "bp_yolo_tap_count": (C.c_int, [vp]),
    "bp_yolo_tap_info": (C.c_int, [vp, C.c_int, C.c_char_p, C.c_int, c_int_p, c_int_p, c_int_p]),
    "bp_yolo_tap_copy": (C.c_int, [vp, C.c_int, C.c_int, vp, vp]),
    "bp_kpd_create": (C.c_int, [vp, C.c_size_t, C.c_int, C.c_int, C.c_int, C.POINTER(vp)]),
    "bp_kpd_destroy": (None, [vp]),
    "bp_kpd_forward": (C.c_int, [vp, vp, C.c_int, vp, vp]),
    "bp_kpd_forward_argmax": (C.c_int, [vp, vp, C.c_int, vp, vp, vp]),
    "bp_kpd_launch_count": (C.c_int, [vp, C.c_int]),
    "bp_kpd_tap_count": (C.c_int, [vp]),
    "bp_kpd_tap_info": (C.c_int, [vp, C.c_int, C.c_char_p, C.c_int, c_int_p, c_int_p, c_int_p]),
    "bp_kpd_tap_copy": (C.c_int, [vp, C.c_int, C.c_int, vp, vp]),
    "bp_yolo_set_policy": (C.c_int, [vp, C.c_int, C.c_int, C.c_int, C.c_int]),
    "bp_kpd_set_policy": (C.c_int, [vp, C.c_int, C.c_int, C.c_int, C.c_int]),
    "bp_yolo_set_precision": (C.c_int, [vp, C.c_int]),
    "bp_kpd_set_precision": (C.c_int, [vp, C.c_int]),
    "bp_calibrate_ticks": (C.c_int, [C.c_longlong, c_float_p, vp]),
    "bp_yolo_set_prefetch": (C.c_int, [vp, C.c_int]),
    "bp_kpd_set_prefetch": (C.c_int, [vp, C.c_int]),
    "bp_yolo_set_fusion": (C.c_int, [vp, C.c_int]),
    "bp_kpd_set_fusion": (C.c_int, [vp, C.c_int]),
    "bp_yolo_fused_launches": (C.c_int, [vp, C.c_int, C.POINTER(C.c_int)]),
    "bp_kpd_fused_launches": (C.c_int, [vp, C.c_int, C.POINTER(C.c_int)]),
    "bp_yolo_xcd_errors": (C.c_int, [vp, C.POINTER(C.c_int), vp]),
    "bp_kpd_xcd_errors": (C.c_int, [vp, C.POINTER(C.c_int), vp]),
    "bp_yolo_set_stamps": (C.c_int, [vp, vp, C.c_int]),
    "bp_kpd_set_stamps": (C.c_int, [vp, vp, C.c_int]),
    "bp_yolo_op_name": (C.c_int, [vp, C.c_int, C.c_char_p, C.c_int]),
    "bp_kpd_op_name": (C.c_int, [vp, C.c_int, C.c_char_p, C.c_int]),
    "bp_yolo_op_stats": (C.c_int, [vp, c_double_p, c_double_p, C.c_int]),
    "bp_kpd_op_stats": (C.c_int, [vp, c_double_p, c_double_p, C.c_int]),
    "bp_yolo_device_bytes": (C.c_size_t, [vp]),
    "bp_kpd_device_bytes": (C.c_size_t, [vp]),
    "bp_crop": (C.c_int, [vp, C.c_int, C.c_int, C.c_int, vp, C.c_int, vp, vp, vp, vp, C.c_int, C.c_int, vp]),
    "bp_resize_bicubic": (C.c_int, [vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, vp, vp, vp]),
    "bp_conv2d": (C.c_int, [vp, C.c_int, C.c_int, C.c_int, C.c_int, vp, vp, C.c_int, C.c_int, C.c_int, C.c_int,
                            C.c_int, C.c_int, vp, C.c_int, C.c_int, C.c_int, vp, C.c_int, c_float_p, vp]),
    "bp_conv2d_planes": (C.c_int, [vp, C.c_int, C.c_int, C.c_int, C.c_int, vp, vp, C.c_int, C.c_int, C.c_int, C.c_int,
                                   C.c_int, C.c_int, vp, C.c_int, C.c_int, C.c_int, vp, vp, C.c_int, c_float_p, vp]),
    "bp_conv2d_se": (C.c_int, [vp, C.c_int, C.c_int, C.c_int, C.c_int, vp, vp, C.c_int, C.c_int, C.c_int, C.c_int,
                               C.c_int, C.c_int, vp, C.c_int, C.c_int, C.c_int, vp, vp, vp, vp, C.c_int, c_float_p, vp]),
    "bp_avgpool": (C.c_int, [vp, C.c_int, C.c_int, C.c_int, C.c_int, vp, c_int_p, vp]),
    "bp_fc": (C.c_int, [vp, vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_float, vp, vp]),
    "bp_maxpool3s2p1": (C.c_int, [vp, C.c_int, C.c_int, C.c_int, C.c_int, vp, vp, C.c_int, vp]),
    "bp_pixel_shuffle2": (C.c_int, [vp, C.c_int, C.c_int, C.c_int, C.c_int, vp, vp, C.c_int, vp]),
    "bp_pipeline_create": (C.c_int, [vp, vp, C.c_int, C.c_int, C.c_int, C.c_float, C.c_int, vp, vp, vp, C.POINTER(vp)]),
    "bp_pipeline_kernel_count": (C.c_int, [vp]),
    "bp_yolo_profile": (C.c_int, [vp, C.c_int, C.c_int, c_float_p, c_int_p, C.c_int, vp]),
    "bp_kpd_profile": (C.c_int, [vp, C.c_int, C.c_int, c_float_p, c_int_p, C.c_int, vp]),
    "bp_pipeline_destroy": (None, [vp]),
    "bp_pipeline_frames": (vp, [vp]),
    "bp_pipeline_results": (vp, [vp]),
    "bp_pipeline_heatmaps": (vp, [vp]),
    "bp_pipeline_set_fixed_box": (C.c_int, [vp, vp]),
    "bp_pipeline_run": (C.c_int, [vp, C.c_int, vp]),
    "bp_pipeline_prepare": (C.c_int, [vp]),
    "bp_pipeline_latency_faults": (C.c_int, [vp]),
    "bp_scene_create": (C.c_int, [vp, vp, vp, C.c_int, C.c_int, C.c_int, C.c_float, C.c_int, vp, vp, C.POINTER(vp)]),
    "bp_scene_destroy": (None, [vp]),
    "bp_scene_results": (vp, [vp]),
    "bp_scene_poses": (vp, [vp]),
    "bp_scene_set_pose_solver": (C.c_int, [vp, C.c_int, vp, C.c_int, vp, C.c_int, vp]),
    "bp_scene_set_pose_ransac": (C.c_int, [vp, C.c_int, C.c_double, C.c_int, C.c_double]),
    "bp_scene_prepare": (C.c_int, [vp]),
    "bp_scene_run": (C.c_int, [vp, C.c_int, vp]),
    "bp_scene_kernel_count": (C.c_int, [vp]),
    "bp_yolo_select_nms": (C.c_int, [vp, C.c_int, C.c_int, C.c_int, C.c_float, C.c_int, C.c_int, C.c_float, C.c_int, vp, vp, vp]),
    "bp_yolo_forward_select_nms": (C.c_int, [vp, vp, C.c_int, C.c_float, C.c_int, C.c_int, C.c_float, C.c_int, vp, vp, vp, vp]),
    "bp_crop_candidates": (C.c_int, [vp, C.c_int, C.c_int, C.c_int, C.c_int, vp, C.c_int, vp, vp, vp, vp, C.c_int, C.c_int, vp]),
    "bp_cands_create": (C.c_int, [vp, vp, C.c_int, C.c_int, C.c_int, C.c_float, C.c_int, C.c_int, C.c_float, vp, vp, C.POINTER(vp)]),
    "bp_cands_destroy": (None, [vp]),
    "bp_cands_results": (vp, [vp]),
    "bp_cands_counts": (vp, [vp]),
    "bp_cands_prepare": (C.c_int, [vp]),
    "bp_cands_run": (C.c_int, [vp, C.c_int, vp]),
    "bp_cands_kernel_count": (C.c_int, [vp]),
    "bp_cands_set_pose_solver": (C.c_int, [vp, vp, C.c_int, vp, C.c_int, vp]),
    "bp_cands_pose": (vp, [vp]),
    "bp_cands_merged": (vp, [vp]),
    "bp_cands_info": (vp, [vp]),
    "bp_pose_from_candidate_records": (C.c_int, [vp, vp, C.c_int, C.c_int, vp, C.c_int, vp, C.c_int, vp, vp, vp, vp]),
    "bp_cands_set_instance_poses": (C.c_int, [vp, C.c_int, vp]),
    "bp_cands_instance_poses": (vp, [vp]),
    "bp_pose_instances_from_merged": (C.c_int, [vp, vp, vp, C.c_int, C.c_int, vp, C.c_int, vp, C.c_int, vp, vp]),
    "bp_heatmap_argmax": (C.c_int, [vp, C.c_int, C.c_int, C.c_int, C.c_int, vp, vp]),
    "bp_pose_errors": (C.c_int, [vp, C.c_int, vp, vp, C.c_int, vp, C.c_int, vp, vp]),
    "bp_pose_errors_sym": (C.c_int, [vp, C.c_int, vp, vp, C.c_int, vp, C.c_int, vp, C.c_int, vp, vp]),
    "bp_render_depth": (C.c_int, [vp, C.c_int, vp, C.c_int, vp, C.c_int, vp, C.c_int, C.c_int, C.c_double, C.c_double, vp, vp,
                                  vp]),
    "bp_render_depth_host": (C.c_int, [vp, C.c_int, vp, C.c_int, vp, C.c_int, vp, C.c_int, C.c_int, C.c_double, C.c_double, vp,
                                       vp]),
    "bp_render_color": (C.c_int, [vp, C.c_int, vp, C.c_int, vp, vp, C.c_int, vp, C.c_int, vp, C.c_int, C.c_int, C.c_double,
                                  C.c_double, C.c_double, vp, C.c_int, vp, vp, vp, vp]),
    "bp_render_color_host": (C.c_int, [vp, C.c_int, vp, C.c_int, vp, C.c_int, vp, vp, C.c_int, vp, C.c_int, C.c_int,
                                       C.c_double, C.c_double, C.c_double, vp, C.c_int, vp, vp, vp]),
    "bp_texture_mips_bytes": (C.c_size_t, [C.c_int, C.c_int, C.c_int]),
    "bp_texture_mips": (C.c_int, [vp, C.c_int, C.c_int, C.c_int, vp, vp]),
    "bp_texture_mips_host": (C.c_int, [vp, C.c_int, C.c_int, C.c_int, vp]),
    "bp_render_color_textured": (C.c_int, [vp, C.c_int, vp, C.c_int, vp, vp, vp, C.c_int, C.c_int, C.c_int, vp, C.c_int, vp,
                                           C.c_int, vp, C.c_int, C.c_int, C.c_double, C.c_double, C.c_double, vp, C.c_int, vp,
                                           vp, vp, vp]),
    "bp_render_color_textured_host": (C.c_int, [vp, C.c_int, vp, C.c_int, vp, C.c_int, vp, vp, vp, C.c_int, C.c_int, C.c_int,
                                                vp, C.c_int, vp, C.c_int, C.c_int, C.c_double, C.c_double, C.c_double, vp,
                                                C.c_int, vp, vp, vp]),
    "bp_draw_boxes": (C.c_int, [vp, C.c_int, vp, vp, vp, C.c_int, vp, C.c_int, C.c_int, C.c_double, C.c_double, vp, vp]),
    "bp_draw_boxes_host": (C.c_int, [vp, C.c_int, vp, vp, vp, C.c_int, vp, C.c_int, C.c_int, C.c_double, C.c_double, vp]),
    "bp_overlay": (C.c_int, [vp, vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, vp, vp]),
    "bp_overlay_host": (C.c_int, [vp, vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, vp]),
    "bp_vsd_errors": (C.c_int, [vp, C.c_int, vp, C.c_int, vp, vp, C.c_int, vp, vp, C.c_int, C.c_int, C.c_int, C.c_double, vp,
                                C.c_double, vp, C.c_int, C.c_double, C.c_double, C.c_double, C.c_int, vp, vp, vp]),
    "bp_image_gradients": (C.c_int, [vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, vp, vp, vp]),
    "bp_image_gradients_host": (C.c_int, [vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, vp, vp]),
    "bp_gradient_scores": (C.c_int, [vp, vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, vp, vp, vp, vp]),
    "bp_gradient_scores_host": (C.c_int, [vp, vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, vp, vp, vp]),
    "bp_annotate_keypoints": (C.c_int, [vp, C.c_int, vp, C.c_int, vp, C.c_int, C.c_int, C.c_double, C.c_double, vp, vp, C.c_int,
                                        vp, C.c_double, C.c_double, vp, vp, vp, vp]),
    "bp_annotate_keypoints_host": (C.c_int, [vp, C.c_int, vp, C.c_int, vp, C.c_int, C.c_int, C.c_double, C.c_double, vp, vp,
                                             C.c_int, vp, C.c_double, C.c_double, vp, vp, vp]),
    "bp_mask_boxes": (C.c_int, [vp, C.c_int, C.c_int, C.c_int, vp, C.c_double, vp, C.c_int, vp, C.c_double, vp, vp, vp]),
    "bp_mask_boxes_host": (C.c_int, [vp, C.c_int, C.c_int, C.c_int, vp, C.c_double, vp, C.c_int, vp, C.c_double, vp, vp]),
    "bp_vertex_boxes": (C.c_int, [vp, C.c_int, vp, C.c_int, vp, C.c_int, C.c_int, vp, vp]),
    "bp_vertex_boxes_host": (C.c_int, [vp, C.c_int, vp, C.c_int, vp, C.c_int, C.c_int, vp]),
    "bp_kpd_targets": (C.c_int, [vp, vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, vp, C.c_int, vp, vp, vp,
                                 vp]),
    "bp_kpd_targets_host": (C.c_int, [vp, vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, vp, C.c_int, vp, vp,
                                      vp]),
    "bp_kpd_inputs": (C.c_int, [vp, C.c_int, C.c_int, C.c_int, vp, vp, vp, vp, vp, C.c_int, C.c_int, C.c_int, vp, vp]),
    "bp_kpd_inputs_host": (C.c_int, [vp, C.c_int, C.c_int, C.c_int, vp, vp, vp, vp, vp, C.c_int, C.c_int, C.c_int, vp]),
    "bp_kpd_augment": (C.c_int, [vp, C.c_int, C.c_int, C.c_int, C.c_int, vp, vp, vp, vp, vp]),
    "bp_kpd_augment_host": (C.c_int, [vp, C.c_int, C.c_int, C.c_int, C.c_int, vp, vp, vp, vp]),
    "bp_heatmap_loss_acc": (C.c_int, [vp, vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, vp, vp, vp, vp, vp, vp, vp, vp]),
    "bp_heatmap_loss_acc_host": (C.c_int, [vp, vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, vp, vp, vp, vp, vp, vp, vp]),
    "bp_yolo_loss_partials": (C.c_size_t, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]),
    "bp_yolo_inputs": (C.c_int, [vp, C.c_int, C.c_int, C.c_int, vp, vp, vp, vp, C.c_int, C.c_int, C.c_int, vp, vp]),
    "bp_yolo_inputs_host": (C.c_int, [vp, C.c_int, C.c_int, C.c_int, vp, vp, vp, vp, C.c_int, C.c_int, C.c_int, vp]),
    "bp_yolo_truth": (C.c_int, [vp, C.c_int, vp, vp, vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, vp, vp, vp,
                                vp]),
    "bp_yolo_truth_host": (C.c_int, [vp, C.c_int, vp, vp, vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, vp, vp,
                                     vp]),
    "bp_yolo_loss": (C.c_int, [vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, vp, C.c_int, vp, vp,
                               C.c_int, C.c_float, C.c_float, C.c_int, vp, vp, vp, vp, vp, vp]),
    "bp_yolo_loss_host": (C.c_int, [vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, vp, C.c_int, vp,
                                    vp, C.c_int, C.c_float, C.c_float, C.c_int, vp, vp, vp, vp, vp]),
    "bp_yolo_map_max_dets": (C.c_int, []),
    "bp_yolo_detections_scratch": (C.c_size_t, [C.c_int, C.c_int, C.c_int]),
    "bp_detector_map_reduce_scratch": (C.c_size_t, [C.c_int, C.c_int]),
    "bp_yolo_detections": (C.c_int, [vp, C.c_int, C.c_int, C.c_int, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_float, C.c_float,
                                     C.c_int, vp, vp, vp, vp]),
    "bp_yolo_detections_host": (C.c_int, [vp, C.c_int, C.c_int, C.c_int, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_float,
                                          C.c_float, C.c_int, vp, vp]),
    "bp_detector_map_match": (C.c_int, [vp, vp, C.c_int, C.c_int, C.c_int, vp, C.c_int, vp, C.c_float, C.c_float, C.c_int, C.c_int,
                                        C.c_int, vp, vp, vp, vp, vp, vp]),
    "bp_detector_map_match_host": (C.c_int, [vp, vp, C.c_int, C.c_int, C.c_int, vp, C.c_int, vp, C.c_float, C.c_float, C.c_int,
                                             C.c_int, C.c_int, vp, vp, vp, vp]),
    "bp_detector_map_reduce": (C.c_int, [vp, C.c_int, vp, C.c_int, C.c_int, vp, C.c_int, vp, vp, vp, vp, vp]),
    "bp_detector_map_reduce_host": (C.c_int, [vp, C.c_int, vp, C.c_int, C.c_int, vp, C.c_int, vp, vp, vp]),
    "bp_train_conv_scratch": (C.c_size_t, [C.c_int] * 7),
    "bp_train_update_chunk": (C.c_int, []),
    "bp_train_conv": (C.c_int, [C.c_int, vp, vp, vp] + [C.c_int] * 7 + [vp, vp]),
    "bp_train_conv_host": (C.c_int, [C.c_int, vp, vp, vp] + [C.c_int] * 7 + [vp]),
    "bp_train_bn_forward": (C.c_int, [vp, C.c_int, C.c_int, C.c_int] + [vp] * 8 + [C.c_int] * 3 + [vp]),
    "bp_train_bn_forward_host": (C.c_int, [vp, C.c_int, C.c_int, C.c_int] + [vp] * 8 + [C.c_int] * 3),
    "bp_train_bn_backward": (C.c_int, [vp] * 7 + [C.c_int] * 3 + [vp] * 3 + [C.c_int] * 2 + [vp]),
    "bp_train_bn_backward_host": (C.c_int, [vp] * 7 + [C.c_int] * 3 + [vp] * 3 + [C.c_int] * 2),
    "bp_train_update": (C.c_int, [vp, C.c_int, C.c_int, C.c_float, C.c_float, C.c_float, vp]),
    "bp_train_update_host": (C.c_int, [vp, C.c_int, C.c_float, C.c_float, C.c_float]),
    "bp_kpd_train_conv_scratch": (C.c_size_t, [C.c_int] * 7),
    "bp_kpd_train_update_chunk": (C.c_int, []),
    "bp_kpd_train_conv": (C.c_int, [C.c_int, vp, vp, vp] + [C.c_int] * 7 + [vp, vp]),
    "bp_kpd_train_conv_host": (C.c_int, [C.c_int, vp, vp, vp] + [C.c_int] * 7 + [vp]),
    "bp_kpd_train_bn_forward": (C.c_int, [vp, C.c_int, C.c_int, C.c_int] + [vp] * 7 + [C.c_int] * 3 + [vp]),
    "bp_kpd_train_bn_forward_host": (C.c_int, [vp, C.c_int, C.c_int, C.c_int] + [vp] * 7 + [C.c_int] * 3),
    "bp_kpd_train_bn_backward": (C.c_int, [vp] * 6 + [C.c_int] * 3 + [vp] * 2 + [C.c_int] * 2 + [vp]),
    "bp_kpd_train_bn_backward_host": (C.c_int, [vp] * 6 + [C.c_int] * 3 + [vp] * 2 + [C.c_int] * 2),
    "bp_kpd_train_tail_forward": (C.c_int, [vp] * 4 + [C.c_int] * 3 + [vp]),
    "bp_kpd_train_tail_forward_host": (C.c_int, [vp] * 4 + [C.c_int] * 3),
    "bp_kpd_train_tail_backward": (C.c_int, [vp] * 7 + [C.c_int] * 3 + [vp]),
    "bp_kpd_train_tail_backward_host": (C.c_int, [vp] * 7 + [C.c_int] * 3),
    "bp_kpd_train_pool_forward": (C.c_int, [vp, C.c_int, C.c_int, vp, vp]),
    "bp_kpd_train_pool_forward_host": (C.c_int, [vp, C.c_int, C.c_int, vp]),
    "bp_kpd_train_pool_backward": (C.c_int, [vp, vp, C.c_int, C.c_int, vp]),
    "bp_kpd_train_pool_backward_host": (C.c_int, [vp, vp, C.c_int, C.c_int]),
    "bp_kpd_train_sigmoid_forward": (C.c_int, [vp, vp, C.c_longlong, vp]),
    "bp_kpd_train_sigmoid_forward_host": (C.c_int, [vp, vp, C.c_longlong]),
    "bp_kpd_train_sigmoid_backward": (C.c_int, [vp, vp, C.c_longlong, vp]),
    "bp_kpd_train_sigmoid_backward_host": (C.c_int, [vp, vp, C.c_longlong]),
    "bp_kpd_train_maxpool_forward": (C.c_int, [vp, C.c_int, C.c_int, C.c_int, vp, vp, vp]),
    "bp_kpd_train_maxpool_forward_host": (C.c_int, [vp, C.c_int, C.c_int, C.c_int, vp, vp]),
    "bp_kpd_train_maxpool_backward": (C.c_int, [vp, vp, C.c_int, C.c_int, C.c_int, vp, vp]),
    "bp_kpd_train_maxpool_backward_host": (C.c_int, [vp, vp, C.c_int, C.c_int, C.c_int, vp]),
    "bp_kpd_train_rmsprop": (C.c_int, [vp, C.c_int, C.c_int] + [C.c_double] * 5 + [vp]),
    "bp_kpd_train_rmsprop_host": (C.c_int, [vp, C.c_int] + [C.c_double] * 5),
    "bp_voxel_grid_host": (C.c_int, [vp, C.c_int, C.c_double, vp, c_int_p]),
    "bp_sift_octave": (C.c_int, [vp, C.c_int, C.c_int, vp, C.c_int, C.c_int, C.c_double, vp, vp, vp]),
    "bp_sift_octave_host": (C.c_int, [vp, C.c_int, C.c_int, vp, C.c_int, C.c_int, C.c_double, vp, vp]),
    "bp_farthest_points": (C.c_int, [vp, C.c_int, C.c_int, C.c_int, vp, vp, vp]),
    "bp_farthest_points_host": (C.c_int, [vp, C.c_int, C.c_int, C.c_int, vp, vp]),
    "bp_thin_points": (C.c_int, [vp, C.c_int, C.c_int, vp, vp, vp]),
    "bp_thin_points_host": (C.c_int, [vp, C.c_int, C.c_int, vp, vp]),
    "bp_icp_normal_equations": (C.c_int, [vp, C.c_int, vp, C.c_int, vp, C.c_int, vp, vp, C.c_int, C.c_int, C.c_int, C.c_double, vp,
                                          C.c_double, C.c_double, C.c_double, C.c_double, C.c_int, vp, vp]),
    "bp_icp_normal_equations_host": (C.c_int, [vp, C.c_int, vp, C.c_int, vp, C.c_int, vp, vp, C.c_int, C.c_int, C.c_int,
                                               C.c_double, vp, C.c_double, C.c_double, C.c_double, C.c_double, vp]),
    "bp_refine_depth": (C.c_int, [vp, C.c_int, vp, C.c_int, vp, C.c_int, vp, vp, C.c_int, C.c_int, C.c_int, C.c_double, vp,
                                  C.c_int, C.c_double, C.c_double, C.c_int, C.c_double, C.c_double, C.c_int, vp, vp, vp]),
    "bp_refine_depth_host": (C.c_int, [vp, C.c_int, vp, C.c_int, vp, C.c_int, vp, vp, C.c_int, C.c_int, C.c_int, C.c_double, vp,
                                       C.c_int, C.c_double, C.c_double, C.c_int, C.c_double, C.c_double, vp, vp]),
    "bp_pipeline_set_pose_solver": (C.c_int, [vp, vp, C.c_int, vp, C.c_int, vp]),
    "bp_pipeline_poses": (vp, [vp]),
    "bp_pose_from_records": (C.c_int, [vp, C.c_int, vp, C.c_int, vp, C.c_int, vp, vp]),
    "bp_solve_pnp_batch": (C.c_int, [vp, C.c_int, vp, C.c_int, C.c_int, vp, vp, vp, vp]),
    "bp_pnp_ransac_samples": (C.c_int, [C.c_int, C.c_int, vp]),
    "bp_pnp_ransac_trials_needed": (C.c_int, [C.c_int, C.c_double, vp]),
    "bp_pnp_ransac_workspace_bytes": (C.c_size_t, [C.c_int, C.c_int]),
    "bp_solve_pnp_ransac_batch": (C.c_int, [vp, C.c_int, vp, C.c_int, C.c_int, vp, C.c_double, C.c_int, C.c_double, vp, vp, vp,
                                            vp, C.c_size_t, vp]),
    "bp_pipeline_set_pose_ransac": (C.c_int, [vp, C.c_double, C.c_int, C.c_double]),
    "bp_pose_ransac_workspace_bytes": (C.c_size_t, [C.c_int, C.c_int]),
    "bp_pose_from_records_ransac": (C.c_int, [vp, C.c_int, vp, C.c_int, vp, C.c_int, C.c_double, C.c_int, C.c_double, vp, vp,
                                              C.c_size_t, vp]),
    "bp_solve_pnp": (C.c_int, [vp, vp, C.c_int, vp, vp, vp]),
    "bp_solve_pnp_status": (C.c_int, [vp, vp, C.c_int, vp, vp, vp, vp]),
    "bp_solve_pnp_refined": (C.c_int, [vp, vp, C.c_int, vp, vp, vp]),
    "bp_solve_pnp_ransac": (C.c_int, [vp, vp, C.c_int, vp, C.c_double, C.c_int, C.c_double, vp, vp, vp]),
    "bp_pose_nms": (C.c_int, [vp, vp, vp, vp, C.c_int, C.c_int, vp, vp, vp, vp]),
    "bp_darknet_last_error": (C.c_char_p, []),
    "bp_darknet_create": (C.c_int, [C.c_char_p, C.c_char_p, C.c_int, C.POINTER(vp)]),
    "bp_darknet_destroy": (None, [vp]),
    "bp_darknet_width": (C.c_int, [vp]),
    "bp_darknet_height": (C.c_int, [vp]),
    "bp_darknet_classes": (C.c_int, [vp]),
    "bp_darknet_detect_rgb": (C.c_int, [vp, vp, C.c_int, C.c_int, C.c_float, C.c_float, vp, C.c_int]),
    "bp_darknet_detect_png": (C.c_int, [vp, vp, C.c_size_t, C.c_float, C.c_float, vp, C.c_int]),
    "bp_darknet_detect_image": (C.c_int, [vp, vp, C.c_size_t, C.c_float, C.c_float, vp, C.c_int]),
    "bp_image_decode_rgb": (C.c_int, [vp, C.c_size_t, vp, C.c_size_t, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "bp_darknet_detect_file": (C.c_int, [vp, C.c_char_p, C.c_float, C.c_float, vp, C.c_int]),
    "bp_yolo_create_darknet": (C.c_int, [C.c_char_p, C.c_char_p, C.c_int, C.c_int, C.c_int, C.POINTER(vp)]),
    "bp_stream_create_masked": (C.c_int, [vp, C.c_int, C.POINTER(vp)]),
    "bp_stream_destroy": (C.c_int, [vp]),
    "bp_probe_placement": (C.c_int, [C.c_int, vp, vp, vp]),
    "bp_png_info": (C.c_int, [vp, C.c_size_t, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "bp_png_decode_bgr": (C.c_int, [vp, C.c_size_t, vp, C.c_size_t, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "bp_loader_create": (C.c_int, [C.POINTER(C.c_char_p), C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                   C.POINTER(vp)]),
    "bp_loader_destroy": (None, [vp]),
    "bp_loader_next": (C.c_int, [vp, C.POINTER(C.c_longlong), C.POINTER(vp)]),
    "bp_loader_release": (C.c_int, [vp, C.c_longlong]),
    "bp_upload": (C.c_int, [vp, vp, C.c_size_t, vp]),
    "bp_synth_background": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_uint, C.c_uint, vp, vp]),
    "bp_synth_background_host": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_uint, C.c_uint, vp]),
    "bp_synth_windows": (C.c_int, [vp, C.c_int, C.c_int, C.c_int, vp, C.c_int, C.c_int, C.c_int, vp, vp]),
    "bp_synth_windows_host": (C.c_int, [vp, C.c_int, C.c_int, C.c_int, vp, C.c_int, C.c_int, C.c_int, vp]),
    "bp_synth_compose": (C.c_int, [vp, vp, vp, C.c_int, C.c_int, C.c_int, vp, C.c_uint, C.c_uint, vp, vp]),
    "bp_synth_compose_host": (C.c_int, [vp, vp, vp, C.c_int, C.c_int, C.c_int, vp, C.c_uint, C.c_uint, vp]),
    "bp_synth_sensor_depth": (C.c_int, [vp, C.c_int, C.c_int, C.c_int, C.c_double, vp, C.c_uint, C.c_uint, vp, vp]),
    "bp_synth_sensor_depth_host": (C.c_int, [vp, C.c_int, C.c_int, C.c_int, C.c_double, vp, C.c_uint, C.c_uint, vp]),
    "bp_synth_instances": (C.c_int, [vp, C.c_int, C.c_int, C.c_int, C.c_int, vp, vp, vp, vp, vp]),
    "bp_synth_instances_host": (C.c_int, [vp, C.c_int, C.c_int, C.c_int, C.c_int, vp, vp, vp, vp]),
}

RESULT_FLOATS = 316
POSE_DOUBLES = 166          # include/betapose_hip.h BP_POSE_DOUBLES
PNP_MAX_POINTS = 64
MAX_SCENE_CLASSES = 16      # include/betapose_hip.h BP_MAX_SCENE_CLASSES
MAX_CANDIDATES = 8          # include/betapose_hip.h BP_MAX_CANDIDATES
MERGED_FLOATS = 152         # include/betapose_hip.h BP_MERGED_FLOATS


class BetaposeHipError(RuntimeError):
    pass


def lib():
    """Load (building first if needed) the HIP library.  Raises on failure."""
    global _lib
    with _lock:
        if _lib is not None:
            return _lib
        # torch ships its own libamdhip64; load it FIRST so this library binds to the same HIP runtime
        # (loading /opt/rocm's copy first leaves two runtimes in the process and ours then sees no device)
        import torch  # noqa: F401
        if not os.path.exists(LIB_PATH):
            from .build import build
            build(verbose=False)
        try:
            L = C.CDLL(LIB_PATH)
        except OSError as e:
            raise BetaposeHipError("cannot load %s: %s (run `python -m betapose_amd.build`)" % (LIB_PATH, e))
        for name, (res, args) in PROTOTYPES.items():
            fn = getattr(L, name)   # AttributeError if the .so is stale/incomplete
            fn.restype = res
            fn.argtypes = args
        _lib = L
        return L


def check(rc: int) -> None:
    if rc != 0:
        msg = lib().bp_last_error()
        raise BetaposeHipError(msg.decode() if msg else "libbetapose_hip error %d" % rc)


def require_gpu() -> None:
    """Product entry points call this: no GPU / no HIP extension => hard error."""
    import torch
    if not torch.cuda.is_available():
        raise BetaposeHipError("betapose_amd needs an AMD GPU (gfx950): torch.cuda.is_available() is False; "
                               "there is no CPU fallback on the product path")
    if lib().bp_device_count() <= 0:
        raise BetaposeHipError("libbetapose_hip.so sees no HIP device")


def ptr(t) -> int:
    """Device/host pointer of a contiguous torch tensor or numpy array."""
    if t is None:
        return None
    if hasattr(t, "data_ptr"):
        if not t.is_contiguous():
            raise ValueError("tensor must be contiguous")
        return t.data_ptr()
    return t.ctypes.data


def current_stream() -> int:
    import torch
    return torch.cuda.current_stream().cuda_stream
