/* betapose_hip.h -- C ABI of libbetapose_hip.so (MI355X / gfx950).
 *
 * Drop-in boundary for the per-frame inference hot path of sjtuytc/betapose
 * (SURVEY.md section 8b).  Plain C: opaque handles, raw device/host pointers and
 * sizes, int status codes (0 = ok, <0 = error; text via bp_last_error()).  Nothing
 * here throws, calls exit() or keeps hidden global engine state, so one engine per
 * rank/stream can coexist.  All "d_" pointers are device (HIP) pointers; `stream`
 * is a hipStream_t passed as void* (NULL = default stream).  Calls on one handle
 * must be serialised by the caller; different handles may be used from different
 * host threads.
 *
 * What each entry point replaces in the reference (paths under
 * /root/reference/3_6Dpose_estimator):
 *   bp_yolo_create*        Darknet(cfgfile, reso) + load_weights(path)      yolo/darknet.py:217-221,365-432
 *                          (C twin: init(cfg, weights, gpu)                 train_YOLO/src/yolo_v2_class.hpp:49)
 *   bp_yolo_forward        Darknet.forward -> [B, 10647, 5+C]               yolo/darknet.py:319-363,129-169
 *   bp_yolo_forward_select + dynamic_write_results (nms hard-wired off)     yolo/util.py:104-223
 *   bp_kpd_create          InferenNet_fast.__init__ / load_state_dict      KPD/src/main_fast_inference.py:26-40
 *   bp_kpd_forward         InferenNet_fast.forward -> [B,50,80,64]         main_fast_inference.py:42-46, models/FastPose.py:28-35
 *   bp_kpd_forward_argmax  + the arg-max half of getPrediction              KPD/src/utils/eval.py:113-131
 *   bp_crop                crop_from_dets + cropBox + box rescale          dataloader.py:354-364,794-835; KPD/src/utils/img.py:242-262
 *   bp_resize_bicubic      transforms.Resize((416,416), 3) + ToTensor      dataloader.py:94-99,162
 *   bp_pipeline_*          DetectionLoader.update -> DetectionProcessor.update -> main loop
 *                          (dataloader.py:330-401,438-457; betapose_evaluate.py:145-176) fused on device
 *   bp_yolo_forward_select_classes, bp_scene_*
 *                          the same chain for K objects of one frame behind ONE multi-class detector pass
 *                          (write_results' class filter generalised; the reference runs one process per object)
 *   bp_yolo_select_nms, bp_yolo_forward_select_nms, bp_crop_candidates, bp_cands_*, bp_pose_from_candidate_records,
 *   bp_pose_instances_from_merged
 *                          write_results with its NMS branch live (yolo/util.py:180-196, hard-coded off in the reference)
 *                          feeding pose_nms several candidates per frame (pPose_nms.py:24-122), PnP on result[0]
 *   bp_solve_pnp           pnp (cv2.solvePnP + cv2.Rodrigues)                 utils/utils.py:17-41
 *   bp_solve_pnp_ransac    the commented-out cv2.solvePnPRansac variant       utils/utils.py:32-36
 *   bp_pose_nms            pose_nms                                           pPose_nms.py:24-122
 *   bp_pipeline_set_pose_solver, bp_pipeline_poses, bp_pose_from_records
 *                          DataWriter.update's per-frame tail on device: key-point   dataloader.py:704-727
 *                          decode (getPrediction), pPose-NMS at n = 1, pruning to   KPD/src/utils/eval.py:113-147
 *                          --left_keypoints, pnp                                     pPose_nms.py:24-122, utils/utils.py:17-41
 *   bp_solve_pnp_batch     pnp over P independent problems on device            utils/utils.py:17-41
 *   bp_solve_pnp_ransac_batch, bp_pipeline_set_pose_ransac, bp_pose_from_records_ransac
 *                          the solvePnPRansac variant on device, hypotheses in parallel   utils/utils.py:32-36
 *   bp_pose_errors         add_err / projection_error_2d + the commented-out   utils/metrics.py:10-33,99-127
 *                          closest-point (ADD-S) loop, over every vertex
 *   bp_pose_errors_sym     no reference counterpart: the BOP errors MSSD and MSPD over an object's symmetry set
 *   bp_render_depth, bp_render_depth_host
 *                          Renderer.render's depth image (OpenGL through vispy)   utils/renderer.py
 *   bp_render_color, bp_render_color_textured, bp_texture_mips, bp_draw_boxes, bp_overlay (and their _host twins)
 *                          Renderer.draw_model / draw_boundingbox / finish and      utils/renderer.py:137-181
 *                          draw_detections_3D's paste over the frame                utils/utils.py:269-301
 *   bp_image_gradients, bp_gradient_scores (and their _host twins)
 *                          verify_6D_poses: compute_grads_and_mags and the score     utils/utils.py:558-610
 *                          sum |g_ren . g_scene| / (count(ren_mags > 0) + 1) of every rendered pose hypothesis
 *   bp_vsd_errors          no reference counterpart: the BOP error VSD over those renders and the test depth image
 *   bp_annotate_keypoints, bp_vertex_boxes (and their _host twins)
 *                          sinobj.apply_pose / project_all / project_kp     2_keypoint_annotator/annotate_keypoint.py:108-175
 *                          plus the visibility flags the annotator meant to write (kp_label's docstring, wrap_kp)
 *   bp_mask_boxes, bp_mask_boxes_host
 *                          get_bbox_from_mask over a render, and over its BOP-visible part    utils/utils.py:136-151
 *   bp_kpd_targets, bp_kpd_targets_host
 *                          generateSampleBox's label half: transformBox +    train_KPD/src/utils/pose.py:113-126
 *                          drawGaussian per part                               train_KPD/src/utils/img.py:61-110
 *   bp_kpd_inputs, bp_kpd_augment, bp_heatmap_loss_acc (and their _host twins)
 *                          generateSampleBox's image half and augmentation:     train_KPD/src/utils/pose.py:20-28,107-143
 *                          cropBox, flip, shuffleLR (torchsample's Rotate is    train_KPD/src/utils/img.py:131-200
 *                          restated from its published source, never compared); train()'s MSELoss(out * setMask, labels)
 *                          and heatmapAccuracy                                  train_KPD/src/utils/eval.py:49-108
 *   bp_yolo_inputs, bp_yolo_truth, bp_yolo_loss (and their _host twins)
 *                          load_data_detection (no OpenCV), fill_truth_detection,  train_YOLO/src/data.c:189-225,303-392,811-859
 *                          forward_yolo_layer with train = 1                       train_YOLO/src/yolo_layer.c:166-282
 *   bp_yolo_detections, bp_detector_map_match, bp_detector_map_reduce (and their _host twins)
 *                          get_network_boxes + do_nms_sort,                        train_YOLO/src/yolo_layer.c:365-392, box.c:331-363
 *                          validate_detector_map (`./darknet detector map`)       train_YOLO/src/detector.c:556-888
 *   bp_train_conv, bp_train_bn_forward, bp_train_bn_backward, bp_train_update (and their _host twins)
 *                          train_network_datum's CPU path: forward / backward /     train_YOLO/src/network.c:193-292,
 *                          update of convolutional layers with batch norm          convolutional_layer.c:674-925, batchnorm_layer.c:65-163
 *   bp_kpd_train_conv, bp_kpd_train_bn_forward / _backward, bp_kpd_train_tail_forward / _backward,
 *   bp_kpd_train_pool_*, bp_kpd_train_sigmoid_*, bp_kpd_train_maxpool_*, bp_kpd_train_rmsprop (and their _host twins)
 *                          train() / valid() for FastPose_SE under RMSprop            train_KPD/src/train.py:19-109,
 *                          (PyTorch's batch norm, bottleneck tail, SE gate)           models/layers/SE_Resnet.py, SE_module.py, DUC.py
 *   bp_sift_octave, bp_farthest_points, bp_thin_points (and their _host twins), bp_voxel_grid_host
 *                          pcl::SIFTKeypoint as extract_sift sets it up (restated     1_keypoint_designator/main.cpp:41-73
 *                          from its published description, never compared with PCL), a farthest-point alternative,
 *                          and Model3D.refine without its [n][n][3] arrays             utils/model.py:29-46
 *   bp_refine_depth, bp_refine_depth_host, bp_icp_normal_equations, bp_icp_normal_equations_host
 *                          no reference counterpart: projective point-to-plane ICP of a pose against the test depth image
 *   bp_synth_background, bp_synth_windows, bp_synth_compose, bp_synth_sensor_depth, bp_synth_instances (and their _host twins)
 *                          no reference counterpart: training frames and sensor depth synthesised from renders
 *   bp_png_*, bp_loader_*  cv2.imread on ImageLoader's thread (PNG frames)   dataloader.py:150-179
 *   bp_upload              the H2D of a frame (img.cuda())                    dataloader.py:339
 *   bp_darknet_*           Detector(cfg, weights, gpu) / Detector::detect    train_YOLO/src/yolo_v2_class.cpp:95-317
 *                          (+ init/detect_image/detect_mat/dispose: include/yolo_v2_class_compat.h)
 *   bp_*_set_precision, bp_*_set_policy, bp_stream_create_masked, bp_probe_placement, bp_conv2d*, bp_avgpool, bp_fc,
 *   bp_maxpool3s2p1, bp_pixel_shuffle2, bp_*_tap_*, bp_*_profile, bp_*_op_stats: no reference counterpart (tuning, measurement and test hooks)
 *
 * Weight streams.  "YOLO stream" = payload of a Darknet .weights file after its
 * header (train_YOLO/src/parser.c:1148-1174): per [convolutional] block in cfg order
 * {bn.bias, bn.scale, bn.mean, bn.var | conv.bias}, conv.weight[out,in,k,k], fp32.
 * "KPD stream" = the FastPose state_dict flattened the same way: convs in
 * module-definition order (preact.conv1; per bottleneck conv1, conv2, conv3,
 * [se.fc.0.weight, se.fc.0.bias, se.fc.2.weight, se.fc.2.bias, downsample.0];
 * duc1.conv, duc2.conv, conv_out) with {bn.bias, bn.weight, running_mean,
 * running_var} (or conv.bias for conv_out) before each conv.weight.  The Python host
 * unpickles the .pkl; C never parses pickle.
 */
#ifndef BETAPOSE_HIP_H
#define BETAPOSE_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct bp_yolo bp_yolo;
typedef struct bp_kpd bp_kpd;
typedef struct bp_pipeline bp_pipeline;
typedef struct bp_scene bp_scene;
typedef struct bp_cands bp_cands;

/* floats per frame in the pipeline result record:
 *   [0..7]   select: idx (int bits; -1 = no detection), x1,y1,x2,y2 (YOLO-input pixels), obj, cls_conf, cls_idx
 *   [8..15]  pt1.x, pt1.y, pt2.x, pt2.y (crop window, frame pixels), box x1,y1,x2,y2 (frame pixels)
 *   [16..]   50 x (argmax idx (int bits), max, left, right, up, down)                       */
#define BP_RESULT_FLOATS 316
#define BP_KP_FLOATS 6
#define BP_SEL_FLOATS 8
/* class ids one shared detector pass can select for (bp_yolo_forward_select_classes, bp_scene_create) */
#define BP_MAX_SCENE_CLASSES 16
/* candidate boxes one frame can yield (bp_yolo_select_nms, bp_cands_create) */
#define BP_MAX_CANDIDATES 8
/* floats per merged pose of the candidate pose tail: pick (int bits), proposal score, 50 x (x, y, score) */
#define BP_MERGED_FLOATS 152

/* doubles per frame in the pose record of the device pose tail (bp_pipeline_set_pose_solver, bp_pose_from_records):
 *   [0]        status: 0 ok, 1 no detection, 2 dropped by pPose-NMS, < 0 the solver's status as bp_solve_pnp reports it
 *              (-1 too few points, -2 degenerate or non-finite; with RANSAC on: -1 fewer than six points, -2 no
 *              six-point consensus, else the status of the refit on the inliers)
 *   [1]        key points handed to the PnP (after the left_number pruning)
 *   [2..10]    R row-major, [11..13] t -- NaN unless status 0
 *   [14]       proposal score
 *   [15]       0; with RANSAC on (bp_pipeline_set_pose_ransac, bp_pose_from_records_ransac) the inlier set: an
 *              integer-valued double whose bit j is the j-th point handed to the PnP (at most 50 bits, exact in f64);
 *              0 for status 1, 2, -1 and -2
 *   [16..165]  50 x (x, y, score) after pPose-NMS (the - 0.3 applied; f32 values held exactly), zero for status 1 and 2 */
#define BP_POSE_DOUBLES 166
#define BP_PNP_MAX_POINTS 64

const char* bp_last_error(void);
int bp_version(void);
int bp_device_count(void);                      /* yolo_v2_class.hpp:52 get_device_count */
int bp_device_name(int device, char* out, int cap);

/* ---- detector ---- */
int bp_yolo_create(const char* cfg_path, const char* weights_path, int reso, int max_batch, int device, bp_yolo** out);
int bp_yolo_create_from_memory(const char* cfg_text, const float* stream, size_t n_floats, int reso, int max_batch,
                               int device, bp_yolo** out);
/* second engine over the SAME device filters (own activations/workspace): one per concurrent stream */
int bp_yolo_clone(const bp_yolo* y, bp_yolo** out);
void bp_yolo_destroy(bp_yolo* y);
int bp_yolo_rows(const bp_yolo* y);             /* 10647 at reso 416 */
int bp_yolo_attrs(const bp_yolo* y);            /* 5 + classes */
int bp_yolo_forward(bp_yolo* y, const float* d_img_nchw, int batch, float* d_pred, void* stream);
/* d_pred may be NULL; d_sel: [batch][8] */
int bp_yolo_forward_select(bp_yolo* y, const float* d_img_nchw, int batch, float conf, int num_classes, float* d_pred,
                           float* d_sel, void* stream);
/* One pass of a MULTI-class detector, the best box of each of K <= BP_MAX_SCENE_CLASSES classes: a row with objectness > conf
 * whose arg-max class (first maximum, over min(num_classes, attrs - 5) scores) is class_ids[k] is a candidate of slot k, and
 * the candidate with the highest objectness wins (lower row on ties) -- write_results' rule (yolo/util.py:118-223, NMS off)
 * with `class 0` generalised.  class_ids: host, distinct, each below the class count.  d_sel [batch][K][8]: bp_yolo_forward_select's
 * record with [6] = the winning class's score and [7] = the class id; index -1 and zeros for a class without a row.  With
 * class_ids = {0} it is bp_yolo_forward_select's record bit for bit.  d_pred may be NULL (the records are then decoded
 * straight from the head tensors; same records). */
int bp_yolo_forward_select_classes(bp_yolo* y, const float* d_img_nchw, int batch, float conf, int num_classes,
                                   const int* class_ids, int K, float* d_pred, float* d_sel, void* stream);
/* dynamic_write_results on an existing prediction tensor (yolo/util.py:104-223, NMS hard-wired off):
 * d_pred [batch][rows][attrs] -> d_sel [batch][8] */
int bp_yolo_select(const float* d_pred, int batch, int rows, int attrs, float conf, int num_classes, float* d_sel,
                   void* stream);
/* Select with box NMS: write_results with its NMS branch live and the final arg-max removed (yolo/util.py:176-196).  A row is
 * live if objectness > conf and its first-max class is class_id; live rows are visited by descending objectness (lower row
 * on ties); each visited survivor is kept and removes every later row whose IoU with it is not < nms_conf (bbox_iou,
 * yolo/bbox.py:51-77, f32, + 1 on widths and heights, corner boxes in detector-input pixels; a NaN IoU removes); stop after
 * max_candidates <= BP_MAX_CANDIDATES survivors.  dynamic_write_results' second pass at nms_conf - 0.05 when more than 100
 * boxes survive is not reproduced: with at most 8 survivors kept it is moot.  d_sel [batch][max_candidates][8]: the select
 * record of each survivor in survivor order ([6] = the class's score, [7] = the class id), unused slots index -1 and zeros;
 * d_counts [batch]: survivors.  Candidate 0 is bp_yolo_select's / bp_yolo_forward_select's record bit for bit (class 0).
 * The forward form decodes straight from the head tensors when d_pred is NULL; both forms write identical records.
 * At most 12 288 rows per image. */
int bp_yolo_select_nms(const float* d_pred, int batch, int rows, int attrs, float conf, int num_classes, int class_id,
                       float nms_conf, int max_candidates, float* d_sel, int* d_counts, void* stream);
int bp_yolo_forward_select_nms(bp_yolo* y, const float* d_img_nchw, int batch, float conf, int num_classes, int class_id,
                               float nms_conf, int max_candidates, float* d_pred, float* d_sel, int* d_counts, void* stream);
/* test/inspection hooks: intermediate layer outputs (dense NCHW copies) */
int bp_yolo_tap_count(const bp_yolo* y);
int bp_yolo_tap_info(const bp_yolo* y, int i, char* name, int cap, int* C, int* H, int* W);
int bp_yolo_tap_copy(bp_yolo* y, int i, int batch, float* d_out_nchw, void* stream);

/* ---- key-point detector ---- */
int bp_kpd_create(const float* stream, size_t n_floats, int n_classes, int max_batch, int device, bp_kpd** out);
int bp_kpd_clone(const bp_kpd* k, bp_kpd** out);
void bp_kpd_destroy(bp_kpd* k);
int bp_kpd_forward(bp_kpd* k, const float* d_inps_nchw, int batch, float* d_hm, void* stream);
/* d_hm may be NULL; d_kp: [batch][50][6] */
int bp_kpd_forward_argmax(bp_kpd* k, const float* d_inps_nchw, int batch, float* d_hm, float* d_kp, void* stream);
/* launches one bp_kpd_forward_argmax pass makes at this batch under the current plan (recorded into a throw-away graph,
 * nothing executes); < 0 on error.  bp_cands_kernel_count = bp_pipeline_kernel_count at batch 1 - this at 1 + this at C. */
int bp_kpd_launch_count(bp_kpd* k, int batch);
int bp_kpd_tap_count(const bp_kpd* k);
int bp_kpd_tap_info(const bp_kpd* k, int i, char* name, int cap, int* C, int* H, int* W);
int bp_kpd_tap_copy(bp_kpd* k, int i, int batch, float* d_out_nchw, void* stream);

/* launch-policy knobs (tuning / tests): split-K target block count, minimum K-chunks (of 32) per slice, maximum
 * slices, forced tile (-1 auto) */
int bp_yolo_set_policy(bp_yolo* y, int sk_target_blocks, int sk_min_chunks, int sk_max_splits, int force_tile);
int bp_kpd_set_policy(bp_kpd* k, int sk_target_blocks, int sk_min_chunks, int sk_max_splits, int force_tile);
/* what the matrix cores multiply, for every conv with Cin % 32 == 0 (activations, accumulation and outputs are fp32 in
 * all modes; converted filter copies are made on first use and shared by clones; a pipeline re-captures its graph):
 *   0  fp32 MFMA (v_mfma_f32_32x32x2_f32);
 *   1  fp16 operands, one fp16 MFMA per product (BASELINE configs[2]; results carry fp16 rounding, ~1e-3);
 *   2  fp32-accurate on the bf16 pipe: operands split exactly into three bf16 terms, six partial products
 *      (dropped terms <= 2^-23 relative, below the fp32 accumulation rounding);
 *   3  mode 1 with fp16 SKIP CONNECTIONS: a residual (YOLO shortcut, ResNet bottleneck add) is read from the fp16 operand plane
 *      its producer wrote for the next convolution, and tensors that only convolutions and residual adds read are not stored as
 *      fp32 at all -- activations travel as fp16 between layers, accumulation stays fp32.  Same stated tolerances as mode 1
 *      (batched fp16 runs are bound by what the layers write: +8.5 % frames/s at 28 frames per launch). */
int bp_yolo_set_precision(bp_yolo* y, int precision);
int bp_kpd_set_precision(bp_kpd* k, int precision);
/* per-op static description: returns number of ops; fills up to cap entries of (flops, bytes) per image */
int bp_yolo_op_stats(const bp_yolo* y, double* flops, double* bytes, int cap);
int bp_kpd_op_stats(const bp_kpd* k, double* flops, double* bytes, int cap);
/* eager run with hipEvent pairs around every fused-conv kernel (not its split-K reduce) and every other op:
 * ms[i] = mean device time of op i over `iters` runs; info[i*4..] = (is_conv, tile id, vec path, splits).
 * Returns the number of ops (arrays may be NULL to query). */
int bp_yolo_profile(bp_yolo* y, int batch, int iters, float* ms, int* info, int cap, void* stream);
/* in-situ timing of the convolutions WHILE the pipeline runs (several frames in flight, graph replay): every conv launch
 * whose grid has at most `slots` blocks writes 8 u64 marks of the device-wide 100 MHz reference clock (s_memrealtime) per block (entry, index math done, -, K loop done,
 * stores done, slab parked, slices combined, -) at d_buf + (conv ordinal * slots + block) * 8.  NULL switches it off; a
 * captured pipeline graph is rebuilt on the next run.  op_name: the layer behind op i of bp_*_op_stats / bp_*_profile; returns 1 for a convolution, 0 for any other op, -1 on error. */
/* how long `ticks` marks of the clock those stamps read take (one thread spinning on s_memtime between two events) */
int bp_calibrate_ticks(long long ticks, float* ms, void* stream);
/* lone-frame latency mode (off by default): split-K launches keep all K slices of an output tile on ONE XCD and hand the
 * partial sums over inside that XCD's L2 (checked in every launch against the XCC_ID the hardware reports: a block that is
 * not where the round-robin dispatch puts it raises an error word instead of reading stale sums, bp_*_xcd_errors below), and every convolution launch
 * carries blocks that pull the NEXT convolution's filters into the L2 of the XCD that will read them.  +4.7 % frames/s
 * with one frame at a time (fp16 +4.8 %), a loss of 1-2 % with two or more frames in flight (no idle CUs to spare); results
 * are bit-identical either way.  A captured pipeline graph is rebuilt on the next run. */
int bp_yolo_set_prefetch(bp_yolo* y, int on);
int bp_kpd_set_prefetch(bp_kpd* k, int on);
/* conv -> conv fusion (round 5; default on, bf16x3 mode): a Darknet-53 residual block's 1x1 + 3x3 + shortcut (yolo/darknet.py:319-363)
 * and a bottleneck's conv1 + conv2 (+ conv3 + skip connection; KPD/src/models/layers/SE_Resnet.py:25-42) run as ONE launch on 8 x 8 output
 * patches where the block's maps are large and its channel counts small (208x208 / 104x104 detector blocks, 80x64 key-point blocks): the
 * intermediate tensors stay in LDS.  Same results as the unfused plan within fp32 rounding (a different summation order in the 3x3).
 * set_fusion(0) restores one launch per convolution; fused_launches reports how many groups the current plan fuses at `batch`.  A captured
 * pipeline graph is rebuilt on the next run. */
int bp_yolo_set_fusion(bp_yolo* y, int on);
int bp_kpd_set_fusion(bp_kpd* k, int on);
int bp_yolo_fused_launches(bp_yolo* y, int batch, int* launches);
int bp_kpd_fused_launches(bp_kpd* k, int batch, int* launches);
/* the latency mode's placement check: *count != 0 when, since the last call, a split-K launch found a K slice on another XCD
 * than its reducing block.  Such a launch raises an error word and does NOT store the affected tile (no trap: the context and the
 * other streams live on), so the frame's results are invalid: switch the mode off (bp_*_set_prefetch(., 0)) and run the frame
 * again.  Waits for `stream`, clears the word.  Always 0 outside the latency mode. */
int bp_yolo_xcd_errors(bp_yolo* y, int* count, void* stream);
int bp_kpd_xcd_errors(bp_kpd* k, int* count, void* stream);
int bp_yolo_set_stamps(bp_yolo* y, unsigned long long* d_buf, int slots);
int bp_kpd_set_stamps(bp_kpd* k, unsigned long long* d_buf, int slots);
int bp_yolo_op_name(const bp_yolo* y, int i, char* out, int cap);
int bp_kpd_op_name(const bp_kpd* k, int i, char* out, int cap);
int bp_kpd_profile(bp_kpd* k, int batch, int iters, float* ms, int* info, int cap, void* stream);
size_t bp_yolo_device_bytes(const bp_yolo* y);
size_t bp_kpd_device_bytes(const bp_kpd* k);

/* ---- stand-alone device stages ---- */
/* d_frames: [batch][H][W][3] u8 BGR.  Either d_sel ([batch][8], box in reso-pixel units, rescaled by W/reso, H/reso)
 * or d_boxes ([batch][4] frame-pixel x1,y1,x2,y2) gives the boxes.  Outputs: d_out_nchw [batch][3][oh][ow] and/or
 * d_out_nhwc [batch][oh][ow][3]; d_pts [batch][8]. */
int bp_crop(const uint8_t* d_frames, int batch, int H, int W, const float* d_sel, int reso, const float* d_boxes,
            float* d_out_nchw, float* d_out_nhwc, float* d_pts, int oh, int ow, void* stream);
/* bp_crop over C candidate boxes per frame: d_frames [frames][H][W][3], d_sel [frames * C][8] or d_boxes [frames * C][4];
 * crop n reads frame n / C with box n; outputs as bp_crop's at batch frames * C.  A slot without a box (index -1, zeros)
 * crops as a frame without a detection does. */
int bp_crop_candidates(const uint8_t* d_frames, int frames, int C, int H, int W, const float* d_sel, int reso,
                       const float* d_boxes, float* d_out_nchw, float* d_out_nhwc, float* d_pts, int oh, int ow, void* stream);
/* Pillow-exact antialiased bicubic: d_in [batch][H][W][3] u8 -> d_out_u8 [batch][oh][ow][3] (nullable) and/or
 * d_out_nhwc f32 /255 (nullable).  swap_rb: read BGR, write RGB. */
int bp_resize_bicubic(const uint8_t* d_in, int batch, int H, int W, int oh, int ow, int swap_rb, uint8_t* d_out_u8,
                      float* d_out_nhwc, void* stream);
/* the arg-max half of getPrediction on an existing heat-map tensor (KPD/src/utils/eval.py:113-131): d_hm [batch][C][H][W]
 * -> d_kp [batch][C][6] = (flat arg-max index as int bits -- first maximum wins --, max, left, right, up, down; the four
 * neighbours are 0 when the maximum lies on the border) */
int bp_heatmap_argmax(const float* d_hm, int batch, int C, int H, int W, float* d_kp, void* stream);
/* add_err / projection_error_2d (utils/metrics.py:10-22,99-127) and ADD-S (the closest-point form the reference
 * keeps commented out, :23-33), f64, for P pose pairs of one model.  d_model [n][3] object frame; d_gt, d_est
 * [P][12] row-major [R|t]; K host 3x3 (may be NULL when (want & 4) == 0); want: 1 ADD, 2 ADD-S, 4 2-D;
 * d_out [P][3] = (ADD, ADD-S, 2-D px), unrequested columns untouched.  Synchronises `stream`. */
int bp_pose_errors(const double* d_model, int n, const double* d_gt, const double* d_est, int P,
                   const double* K, int want, double* d_out, void* stream);
/* The BOP symmetry-aware errors, f64, for P pose pairs of one model: MSSD = min_S max_x |E x - G S x| (metres) and
 * MSPD = min_S max_x |proj(E x) - proj(G S x)| (pixels), E the estimate, G the ground truth, S over the symmetry set.
 * d_model [n][3] object frame; d_gt, d_est [P][12] and d_sym [S][12] row-major [R|t] (the set should hold the
 * identity); K host 3x3 (may be NULL when (want & 2) == 0); want: 1 MSSD, 2 MSPD; d_out [P][2] = (MSSD, MSPD),
 * unrequested columns untouched.  Bit-identical from run to run.  Synchronises `stream`. */
int bp_pose_errors_sym(const double* d_model, int n, const double* d_gt, const double* d_est, int P, const double* d_sym,
                       int S, const double* K, int want, double* d_out, void* stream);
/* Depth images of a triangle mesh at P poses.  d_model [n][3] f64 object frame, d_faces [F][3] int32, d_poses [P][12]
 * row-major [R|t] f64, K host 3x3; the centre of pixel (x, y) lies at image coordinates (x + pixel_center,
 * y + pixel_center) (0 BOP's convention, 0.5 the reference renderer's).  Coverage: vertices snapped to 1/256 px, int64
 * edge functions, top-left rule, both windings; depth: the pixel ray's f64 intersection with the triangle's camera-space
 * plane, clamped to the triangle's depth range, rounded to f32; z-buffer: minimum.  d_depth [P][H][W] f32, 0 where
 * nothing was drawn.  A triangle with a vertex at z < near_z (> 0) or projecting beyond +-2^14 px, or with a face index
 * outside [0, n), is skipped whole (no near-plane clipping) and counted in d_skipped [P].  H * W <= 2^24.
 * bp_render_depth_host is the same on host memory, without a GPU, bit-identical to the device image; it refuses a face
 * index outside [0, n).  bp_render_depth synchronises `stream`. */
int bp_render_depth(const double* d_model, int n, const int* d_faces, int F, const double* d_poses, int P, const double* K,
                    int H, int W, double pixel_center, double near_z, float* d_depth, int* d_skipped, void* stream);
int bp_render_depth_host(const double* poses, int P, const double* vertices, int n, const int* faces, int F, const double* K,
                         int H, int W, double pixel_center, double near_z, float* depth, int* skipped);
/* Colour images of a triangle mesh with per-vertex colours at P poses, several poses per image.  Geometry, coverage and
 * depth are bp_render_depth's, unchanged.  d_colors [n][3] uint8 (channel order is the caller's); image_index HOST [P]
 * int32, the image each pose is drawn into, non-decreasing with values in [0, I), or NULL for pose p -> image p (then
 * I == P).  Of the fragments of a pixel the one with the smallest 64-bit key (f32 depth bits << 32) | (p * F + f) wins:
 * nearest first, then the lowest pose slot, then the lowest face; P * F <= 2^32 - 2.  The winner's colour: with A, B, C
 * the face's camera-space vertices in the face's own order, X the point of the pixel's ray at the fragment's f64 depth
 * and n = (B - A) x (C - A), the weights ((B - X) x (C - X)) . n / n.n (and cyclic) are clamped to [0, 1] and normalised
 * (1/3 each for a degenerate face) and mix the vertex colours in f64; N = +-n / |n| facing the camera,
 * L = (light - X) / |light - X| (0 at the light), light_w = min(ambient + 0.5 max(L . N, 0), 1); a channel is
 * min(255, floor(light_w c + 0.5)).  light: host [3], camera space.  d_color [I][H][W][3] uint8 (0 where nothing is
 * drawn), d_depth [I][H][W] f32 (0 where nothing is drawn; equal to bp_render_depth's bit for bit when every image
 * holds one pose), d_skipped [P] as bp_render_depth.  accumulate != 0: d_color and d_depth hold an earlier call's
 * result (of any mesh) on entry; a pixel with depth > 0 takes part with the key (depth bits << 32) | 0xFFFFFFFF and
 * keeps its colour and depth unless a fragment with a smaller key arrives.  accumulate == 0: every byte of both is
 * written.  Images and poses are processed in chunks that keep the workspaces under 256 MB; the result does not depend
 * on it and is the same from run to run.  bp_render_color_host is the same on host memory, without a GPU, byte-identical;
 * it refuses a face index outside [0, n).  bp_render_color synchronises `stream`. */
int bp_render_color(const double* d_model, int n, const int* d_faces, int F, const unsigned char* d_colors,
                    const double* d_poses, int P, const int* image_index, int I, const double* K, int H, int W,
                    double pixel_center, double near_z, double ambient, const double* light, int accumulate,
                    unsigned char* d_color, float* d_depth, int* d_skipped, void* stream);
int bp_render_color_host(const double* poses, int P, const double* vertices, int n, const int* faces, int F,
                         const unsigned char* colors, const int* image_index, int I, const double* K, int H, int W,
                         double pixel_center, double near_z, double ambient, const double* light, int accumulate,
                         unsigned char* color, float* depth, int* skipped);
/* A texture in the place of the vertex colours.  The pyramid: level 0 is the image [Ht][Wt][3] uint8
 * (row 0 the top), level l + 1 has ceil(w / 2) x ceil(h / 2) texels, each (a + b + c + d + 2) >> 2 per channel of its
 * 2 x 2 block with the partner index clamped where a dimension is odd, down to 1 x 1: 1 + ceil(log2(max(Wt, Ht)))
 * levels, of which a call builds or reads the first `levels`.  A texel is one dword, channel k in byte k; the levels
 * follow each other.  Wt, Ht <= 8192.  bp_texture_mips_bytes: the bytes of the first `levels` levels, 0 for sizes or
 * levels out of range.  bp_texture_mips is enqueued on `stream` and does not synchronise it; bp_texture_mips_host is the
 * same on host memory, byte-identical. */
size_t bp_texture_mips_bytes(int Wt, int Ht, int levels);
int bp_texture_mips(const unsigned char* d_texture, int Wt, int Ht, int levels, uint32_t* d_mips, void* stream);
int bp_texture_mips_host(const unsigned char* texture, int Wt, int Ht, int levels, uint32_t* mips);
/* bp_render_color with a texture: every argument of bp_render_color means what it means there, and visibility, depth,
 * the weights wa, wb, wc and light_w of the winning fragment are its own.  d_uv [F][3][2] f64: (u, v) of every face
 * corner, v upwards (v = 1 is the image's top row); d_mips, Wt, Ht: a pyramid of bp_texture_mips, of which the first
 * `levels` levels are read (1: the image alone, no mip-mapping).  The fragment's (u, v) is the corner coordinates mixed
 * by wa, wb, wc.  Its level: with (u, v) taken by unclamped barycentrics where the rays of pixels (x, y), (x + 1, y) and
 * (x, y + 1) meet the face's plane, rx and ry are the squared lengths of the two differences of (u Wt, v Ht), and
 * level = the number of l < levels - 1 with rx > 4^l or ry > 4^l (a comparison with a NaN is false).  The sample: a
 * coordinate that is NaN becomes 0, its magnitude is limited to 2^30, it wraps as u - floor(u); s = u w - 0.5,
 * t = (1 - v) h - 0.5 in the level's size; floor(256 s), floor(256 t) give the texel and an 8-bit fraction per axis; the
 * four taps are wrapped modulo the level's size before they are loaded; a channel is ((c00 (256 - fx) + c10 fx)
 * (256 - fy) + (c01 (256 - fx) + c11 fx) fy + 32768) >> 16 and takes the place of the mixed vertex colour:
 * min(255, floor(light_w c + 0.5)).  d_uv == NULL: d_colors is used and the call is bp_render_color; otherwise d_colors
 * is not read and may be NULL.  Accumulation works across the two kinds of call in either order.  The _host twin is the
 * same on host memory, byte-identical.  bp_render_color_textured synchronises `stream`. */
int bp_render_color_textured(const double* d_model, int n, const int* d_faces, int F, const unsigned char* d_colors,
                             const double* d_uv, const uint32_t* d_mips, int Wt, int Ht, int levels, const double* d_poses,
                             int P, const int* image_index, int I, const double* K, int H, int W, double pixel_center,
                             double near_z, double ambient, const double* light, int accumulate, unsigned char* d_color,
                             float* d_depth, int* d_skipped, void* stream);
int bp_render_color_textured_host(const double* poses, int P, const double* vertices, int n, const int* faces, int F,
                                  const unsigned char* colors, const double* uv, const uint32_t* mips, int Wt, int Ht,
                                  int levels, const int* image_index, int I, const double* K, int H, int W,
                                  double pixel_center, double near_z, double ambient, const double* light, int accumulate,
                                  unsigned char* color, float* depth, int* skipped);
/* The 12 edges of a 3-D bounding box at P poses, drawn one pixel wide over d_color [I][H][W][3] uint8 without a depth
 * test (Renderer.draw_boundingbox, utils/renderer.py).  d_corners [8][3] f64 object frame in the order of
 * Model3D._compute_bbox (x outermost, then z, then y, min before max), d_corner_colors [8][3] uint8; image_index, I,
 * K, pixel_center as bp_render_color.  An edge is clipped against z = near_z (dropped when wholly behind, shortened
 * when it crosses), projected, clipped to +-2^20 px, snapped to 1/256 px and stepped along its major axis over the
 * pixel positions inside the image; a pixel's colour mixes the two corner colours linearly by its position along the
 * snapped edge, in integers.  Where edges overlap the highest (pose slot, edge) wins.  P <= 2^24.  bp_draw_boxes_host is
 * the same on host memory, byte-identical.  bp_draw_boxes synchronises `stream`. */
int bp_draw_boxes(const double* d_poses, int P, const double* d_corners, const unsigned char* d_corner_colors,
                  const int* image_index, int I, const double* K, int H, int W, double pixel_center, double near_z,
                  unsigned char* d_color, void* stream);
int bp_draw_boxes_host(const double* poses, int P, const double* corners, const unsigned char* corner_colors,
                       const int* image_index, int I, const double* K, int H, int W, double pixel_center, double near_z,
                       unsigned char* color);
/* A render over frames: where depth > 0, out = (alpha color + (256 - alpha) frame + 128) >> 8 per channel, elsewhere
 * out = frame; alpha in 0 .. 256 (256: the reference's out[mask] = col[mask], utils/utils.py:299-300).  frames, color,
 * out [I][H][W][3] uint8, depth [I][H][W] f32; out may be frames.  bp_overlay is enqueued on `stream` and does not
 * synchronise it. */
int bp_overlay(const unsigned char* d_frames, const unsigned char* d_color, const float* d_depth, int I, int H, int W,
               int alpha, unsigned char* d_out, void* stream);
int bp_overlay_host(const unsigned char* frames, const unsigned char* color, const float* depth, int I, int H, int W,
                    int alpha, unsigned char* out);
/* Pose verification by gradient agreement (the reference's verify_6D_poses).  All arithmetic up to the
 * unit vectors is integer, and the sum is integer, so host and device give the same bytes.
 *   gray   of a uint8 pixel: (4899 R + 9617 G + 1868 B + 8192) >> 14; byte red_channel (0 or 2) is R, byte 1 is G
 *   Sobel  ksize 5, separable, d = [-1, -2, 0, 2, 1], s = [1, 4, 6, 4, 1]: gx = s along y then d along x, gy = d along y
 *          then s along x (correlation); border reflect-101 (-1 -> 1, -2 -> 2, W -> W - 2, W + 1 -> W - 3), so H, W >= 3.
 *          |g| <= 12240 and m2 = gx^2 + gy^2 <= 299 635 200 fits an int32
 *   mask   a pixel is kept iff m2 >= min_sq.  The reference's `sqrt(m2) + 0.001 < 5` masks an 8-bit image's pixel iff
 *          m2 <= 24: min_sq = 25; applied to a render that is float in [0, 1] it masks iff m2 < (4.999 * 255)^2 =
 *          1 624 974.8 in 8-bit units: min_sq = 1 624 975
 *   unit   of a kept pixel: mag = sqrtf((float)m2) + 0.001f, nx = (float)gx / mag, ny = (float)gy / mag, square root and
 *          quotients correctly rounded to f32; a masked pixel has nx = ny = 0 and magnitude 0
 *   term   t = fabsf(rnx * snx + rny * sny) (two products, one sum, no contraction), q = (uint32) lrintf(t * 2^24), and 0
 *          where t is NaN or above 2 (a scene gradient that is no unit vector)
 * bp_image_gradients: d_images [I][H][W][3] uint8 -> d_grad [I][H][W][2] f32 = (nx, ny) and, unless NULL, d_mag [I][H][W]
 * f32.  I = 0 is a no-op.
 * bp_gradient_scores: P renders d_renders [P][H][W][3] uint8 against the gradients d_scene_grad [T][H][W][2] of the frames
 * (bp_image_gradients' output), render p against frame d_frame_index[p].  Per render, in one fused kernel whose render
 * gradients never reach memory: d_sum[p] (uint64) = the sum of q over the render's kept pixels, d_count[p] = the number
 * of kept render pixels, d_score[p] (f64) = sum / 2^24 / (count + 1).  The rows are zeroed by the call and accumulated
 * with integer atomics: no workspace, and the same bytes from run to run.  A pose whose frame index lies outside
 * [0, T) gets score NaN, sum 0 and count -1.  P = 0 is a no-op.
 * Both are enqueued on `stream` and do not synchronise it. */
int bp_image_gradients(const unsigned char* d_images, int I, int H, int W, int red_channel, int min_sq, float* d_grad,
                       float* d_mag, void* stream);
int bp_image_gradients_host(const unsigned char* images, int I, int H, int W, int red_channel, int min_sq, float* grad,
                            float* mag);
int bp_gradient_scores(const unsigned char* d_renders, const float* d_scene_grad, const int* d_frame_index, int P, int T, int H,
                       int W, int red_channel, int render_min_sq, uint64_t* d_sum, int* d_count, double* d_score, void* stream);
int bp_gradient_scores_host(const unsigned char* renders, const float* scene_grad, const int* frame_index, int P, int T, int H,
                            int W, int red_channel, int render_min_sq, uint64_t* sum, int* count, double* score);
/* BOP's Visible Surface Discrepancy (step cost, normalised by the diameter, visibility mode bop19) of P pose pairs of
 * one mesh: both poses of a pair are rendered as bp_render_depth does and compared with the test depth image
 * d_test_index[p] of d_depth_test [T][H][W] uint16 (depth = raw * depth_scale in pose units, 0 = missing).  taus: host,
 * n_tau <= 16.  d_err [P][n_tau] f64; d_counts [P][4] int32 = (rendered ground-truth pixels, visible ground-truth
 * pixels, intersection, union) -- counts[1] / counts[0] is BOP's visible fraction.  Pairs are processed `chunk` at a
 * time (0: as many as keep the workspaces under 256 MB); the results do not depend on it and are bit-identical from run
 * to run.  A pair whose test index lies outside [0, T) gets NaN errors and counts of -1.  Synchronises `stream`. */
int bp_vsd_errors(const double* d_model, int n, const int* d_faces, int F, const double* d_gt, const double* d_est, int P,
                  const double* K, const uint16_t* d_depth_test, int T, int H, int W, double depth_scale,
                  const int* d_test_index, double delta, const double* taus, int n_tau, double diameter, double pixel_center,
                  double near_z, int chunk, double* d_err, int* d_counts, void* stream);
/* Key-point annotation of P poses x Kp model points (stage 2 of the reference).  Per pair: X = R m + t,
 * u = (fx X + s Y) / Z + cx, v = fy Y / Z + cy (K = [fx s cx; 0 fy cy; 0 0 1]), and the pixel the projection falls in,
 * (floor(u - pixel_center + 0.5), floor(v - pixel_center + 0.5)).  d_xy [P][Kp][2] f64 = (u, v), d_z [P][Kp] f64 = Z,
 * d_flags [P][Kp] uint8, bits: 1 FRONT (Z >= near_z); 2 IN_IMAGE (that pixel exists); 4 SELF_VISIBLE (FRONT and IN_IMAGE,
 * and not: the pose's own render covers the pixel (D > 0) with D < Z - self_tol); 8 SCENE_VISIBLE (FRONT and IN_IMAGE,
 * and the scene depth S at the pixel is 0 = missing or Z - S <= delta); 16 SCENE_KNOWN (S > 0).  d_model_depth
 * [P][H][W] f32 is bp_render_depth's output for the same poses and pixel_center, or NULL; d_scene_depth [T][H][W] f32 in
 * pose units with d_scene_index [P], or both NULL.  A depth input that is not given leaves its visibility bit set for
 * every FRONT and IN_IMAGE point.  A point that is not FRONT gets xy = (-1, -1), z = Z and flags 0.  A scene index
 * outside [0, T) is an error (the device call reads the index back to check it, which synchronises `stream` once; its
 * kernel is then enqueued on `stream` without another synchronisation).  bp_annotate_keypoints_host is the same on host
 * memory, without a GPU, bit-identical. */
int bp_annotate_keypoints(const double* d_poses, int P, const double* d_kp, int Kp, const double* K, int H, int W,
                          double pixel_center, double near_z, const float* d_model_depth, const float* d_scene_depth, int T,
                          const int* d_scene_index, double self_tol, double delta, double* d_xy, double* d_z,
                          unsigned char* d_flags, void* stream);
int bp_annotate_keypoints_host(const double* poses, int P, const double* kp, int Kp, const double* K, int H, int W,
                               double pixel_center, double near_z, const float* model_depth, const float* scene_depth, int T,
                               const int* scene_index, double self_tol, double delta, double* xy, double* z,
                               unsigned char* flags);
/* Boxes of P depth images d_depth [P][H][W] f32 (0 = nothing): d_boxes [P][2][4] int32, box 0 around the covered pixels
 * (depth > 0), box 1 around those of them that are visible by bp_vsd_errors' rule for the ground truth (distances along
 * the pixel's ray; visible when not more than delta behind the scene surface, or the scene depth is 0 = missing), each
 * (xmin, xmax, ymin, ymax) inclusive and -1 x4 when empty; d_counts [P][2] int32 the two pixel counts.  The scene depth
 * is given as in bp_annotate_keypoints; without it box 1 equals box 0.  Integer reductions only: bit-identical from run
 * to run and to bp_mask_boxes_host.  Synchronises `stream`. */
int bp_mask_boxes(const float* d_depth, int P, int H, int W, const double* K, double pixel_center, const float* d_scene_depth,
                  int T, const int* d_scene_index, double delta, int* d_boxes, int* d_counts, void* stream);
int bp_mask_boxes_host(const float* depth, int P, int H, int W, const double* K, double pixel_center, const float* scene_depth,
                       int T, const int* scene_index, double delta, int* boxes, int* counts);
/* The reference's mask_bbox of P poses of n vertices: every vertex is projected as above and splatted into pixel
 * (int(u), int(v)), truncated toward zero; d_boxes [P][4] int32 = (xmin, xmax, ymin, ymax) over the vertices with
 * 0 < int(u) < W and 0 < int(v) < H (the reference's strict bounds), -1 x4 when there is none.  Synchronises `stream`. */
int bp_vertex_boxes(const double* d_poses, int P, const double* d_vertices, int n, const double* K, int H, int W, int* d_boxes,
                    void* stream);
int bp_vertex_boxes_host(const double* poses, int P, const double* vertices, int n, const double* K, int H, int W, int* boxes);
/* Heat-map targets of B samples x Kp parts (generateSampleBox, 'coco' branch): d_parts [B][Kp][2] f64 image
 * coordinates, windows d_ul, d_br [B][2] f32, d_g [size][size] f32 the Gaussian patch (size odd; drawGaussian's
 * 6 sigma + 1).  A part is drawn iff x > 0 and it lies strictly inside its window; its centre is transformBox's (float32
 * arithmetic, round half to even; only resH scales, as there); d_out [B][Kp][resH][resW] f32 holds d_g clipped to the
 * map about the centre and 0 elsewhere, d_centres [B][Kp][2] int32 the centre, (-1, -1) for a part that is not drawn;
 * d_set_mask (same shape as d_out, or NULL) is filled with ones.  Every element is written.  Enqueued on `stream`
 * without synchronising it. */
int bp_kpd_targets(const double* d_parts, const float* d_ul, const float* d_br, int B, int Kp, int inpH, int inpW, int resH,
                   int resW, const float* d_g, int size, float* d_out, int* d_centres, float* d_set_mask, void* stream);
int bp_kpd_targets_host(const double* parts, const float* ul, const float* br, int B, int Kp, int inpH, int inpW, int resH,
                        int resW, const float* g, int size, float* out, int* centres, float* set_mask);
/* KPD training samples (the rest of generateSampleBox, and train()'s criterion and metric).  Each device function is
 * bit-identical to its _host twin, which needs no GPU, and is enqueued on `stream` without synchronising it.
 *
 * bp_kpd_inputs: the network input of B samples.  d_frames [N][H][W][3] uint8 RGB, d_frame_index [B] int32 (an index
 * outside [0, N) gives a zero sample), windows d_ul, d_br [B][2] f32 as bp_kpd_targets takes them, d_gains [B][3] f32 or
 * NULL (no multiply), d_blank [B] uint8 or NULL (non-zero: the sample is all zeros, generateSampleBox's jointNum == 0).
 * A tap of the frame is clamp(u8 / 255 * gain, 0, 1) - mean, mean = (0.406, 0.457, 0.480) for R, G, B, in f32.  The
 * window's corners are truncated toward zero, (w, h) = br - ul; lenH = max(h, w * inpH / inpW), lenW = lenH * inpW /
 * inpH; the crop sits in a zero image of PH = max(int(lenH), h) by PW = max(int(lenW), w) at offset
 * (ceil((PH - h) / 2), ceil((PW - w) / 2)), and that image is resized to d_inp [B][3][inpH][inpW] f32 bilinearly with
 * align_corners = True (cropBox).  A window without area gives a zero sample.  Every element is written. */
int bp_kpd_inputs(const unsigned char* d_frames, int N, int H, int W, const int* d_frame_index, const float* d_ul,
                  const float* d_br, const float* d_gains, const unsigned char* d_blank, int B, int inpH, int inpW, float* d_inp,
                  void* stream);
int bp_kpd_inputs_host(const unsigned char* frames, int N, int H, int W, const int* frame_index, const float* ul, const float* br,
                       const float* gains, const unsigned char* blank, int B, int inpH, int inpW, float* inp);
/* bp_kpd_augment: d_y = the augmented d_x, both [B][C][H][W] f32 and distinct.  d_flip [B] uint8: column j takes column
 * W - 1 - j, and channel c reads channel d_perm[c] (d_perm [C] int32 or NULL = identity: shuffleLR as a table; an entry
 * outside [0, C) counts as c).  d_cs [B][2] f64 = (cos, sin) of the sample's rotation angle, formed by the caller;
 * exactly (1, 0) means no rotation.  Rotation: the source of pixel (row, col) is A (dst - centre) + centre, A = [[cos,
 * -sin], [sin, cos]], centre = (H / 2 - 0.5, W / 2 - 0.5), in f64; the coordinate is clamped to the map, and the four
 * taps about its floor are blended in f32.  The taps are read through the flip, so the result is the rotation of the
 * flipped map.  Every element is written. */
int bp_kpd_augment(const float* d_x, int B, int C, int H, int W, const unsigned char* d_flip, const double* d_cs,
                   const int* d_perm, float* d_y, void* stream);
int bp_kpd_augment_host(const float* x, int B, int C, int H, int W, const unsigned char* flip, const double* cs, const int* perm,
                        float* y);
/* bp_heatmap_loss_acc: d_out, d_labels, d_set_mask (or NULL = ones) and d_grad (or NULL), all [B][K][H][W] f32.
 * *d_loss (f64) = the mean of (out * mask - label)^2, the difference in f32, the squares summed in f64 in a fixed order
 * (no atomics: the same bits on every run, stream and grid).  d_grad = ((f32)(2 / (B K H W)) * (out * mask - label)) *
 * mask.  d_preds, d_gt [B][K][2] int32 = the (x, y) of the largest value of out * mask and of the label, the lowest
 * index among equals (getPreds); d_dists [K][B] f32 = their distance / (H / 10), or -1 unless gt.x > 0 and gt.y > 0
 * (calc_dists); d_acc [K + 1] f32: [1 + k] the share of channel k's counted samples with dist <= 0.5, -1 when none
 * counts, [0] the mean of the non-negative ones, 0 when there is none (heatmapAccuracy over every channel).
 * d_partial [B * K] f64 is scratch. */
int bp_heatmap_loss_acc(const float* d_out, const float* d_labels, const float* d_set_mask, int B, int K, int H, int W,
                        double* d_partial, double* d_loss, float* d_acc, int* d_preds, int* d_gt, float* d_dists, float* d_grad,
                        void* stream);
int bp_heatmap_loss_acc_host(const float* out, const float* labels, const float* set_mask, int B, int K, int H, int W,
                             double* partial, double* loss, float* acc, int* preds, int* gt, float* dists, float* grad);
/* Detector training: Darknet's detection data path and its [yolo] layer's training forward.  Each
 * device function is bit-identical to its _host twin, which needs no GPU.
 *
 * bp_yolo_inputs: d_out [B][3][net_h][net_w] f32 = one sample of load_data_detection per row of the batch, without its
 * random draws: frame d_frame_index[b] of d_frames [N][H][W][3] uint8 RGB as u8 / 255 (an index outside [0, N) gives a
 * zero sample), crop_image by d_crop [B][4] int32 = (pleft, ptop, swidth, sheight) with positions clamped into the frame,
 * resize_image's two-pass bilinear to (net_w, net_h), flip_image where d_flip [B] uint8 is set, distort_image by
 * d_hsv [B][3] f32 = (dhue, dsat, dexp) or NULL for no distortion.  swidth, sheight, net_w or net_h below 2 is an
 * error (the device call reads d_crop back to check it).  Every element is written. */
int bp_yolo_inputs(const unsigned char* d_frames, int N, int H, int W, const int* d_frame_index, const int* d_crop,
                   const unsigned char* d_flip, const float* d_hsv, int B, int net_h, int net_w, float* d_out, void* stream);
int bp_yolo_inputs_host(const unsigned char* frames, int N, int H, int W, const int* frame_index, const int* crop,
                        const unsigned char* flip, const float* hsv, int B, int net_h, int net_w, float* out);
/* bp_yolo_truth: fill_truth_detection with correct_boxes.  d_labels [M][5] f32 = (id, x, y, w, h) as parsed from the
 * label files, sample b owning rows d_first[b] .. d_first[b + 1] (d_first [B + 1] int32; the host call rejects a list
 * that decreases or leaves [0, M], the kernel clamps it); d_swap [M] int32 = the index randomize_boxes draws at each
 * step, within the sample's slice (one outside it swaps nothing); d_geom [B][4] f32 = (dx, dy, sx, sy) as
 * load_data_detection passes them; d_order [M] int32 is scratch.  d_truth [B][max_boxes][5] f32 = (x, y, w, h, id),
 * zero past the d_kept[b] rows kept.  The list is cut to max_boxes before the filter, as in the reference.
 * small_object changes no output there and none here. */
int bp_yolo_truth(const float* d_labels, int M, const int* d_first, const int* d_swap, const float* d_geom,
                  const unsigned char* d_flip, int B, int classes, int max_boxes, int net_w, int net_h, int small_object,
                  int* d_order, float* d_truth, int* d_kept, void* stream);
int bp_yolo_truth_host(const float* labels, int M, const int* first, const int* swap, const float* geom, const unsigned char* flip,
                       int B, int classes, int max_boxes, int net_w, int net_h, int small_object, int* order, float* truth,
                       int* kept);
/* bp_yolo_loss: forward_yolo_layer with train = 1 for one head.  d_x [B][channels][h][w] f32 is the raw head output,
 * channels = n * (5 + classes) (anything else is an error, as is focal_loss != 0); d_anchors [total][2] f32, d_mask [n]
 * int32 with values in [0, total) (read back and checked); d_truth [B][max_boxes][5] f32.  d_act (or NULL) = l.output,
 * d_delta = l.delta, both shaped as d_x and distinct from it; *d_cost (f64) = the sum of delta^2, in f64 in a fixed
 * order; d_stats [7] f64 = the sums of IoU, class, obj and any-obj, the recall .5 and .75 counts and the count that the
 * reference's log line divides.  exp, log and the logistic are computed in f64 without a math library.  A truth row
 * with a negative id, or whose cell lies outside the grid (x or y of exactly 1), is passed over; the reference indexes
 * outside its arrays there.  d_partial [bp_yolo_loss_partials(B, n, classes, h, w)] f64 is scratch.  No atomics: the
 * same bits on every run and stream. */
size_t bp_yolo_loss_partials(int B, int n, int classes, int h, int w);
int bp_yolo_loss(const float* d_x, int B, int channels, int n, int classes, int h, int w, int net_w, int net_h,
                 const float* d_anchors, int total, const int* d_mask, const float* d_truth, int max_boxes, float ignore_thresh,
                 float truth_thresh, int focal_loss, float* d_act, float* d_delta, double* d_cost, double* d_stats,
                 double* d_partial, void* stream);
int bp_yolo_loss_host(const float* x, int B, int channels, int n, int classes, int h, int w, int net_w, int net_h,
                      const float* anchors, int total, const int* mask, const float* truth, int max_boxes, float ignore_thresh,
                      float truth_thresh, int focal_loss, float* act, float* delta, double* cost, double* stats, double* partial);
/* Detector validation: Darknet's `detector map`.  Each device function is bit-identical to its _host
 * twin, which needs no GPU.  Integers inside float32 rows travel as their bits.
 *
 * bp_yolo_detections: get_network_boxes(net, 1, 1, thresh, 0, 0, 0, &n, 0) followed by do_nms_sort(dets, n, classes, nms)
 * for every image of d_pred [B][rows][attrs] f32, the decoded tensor bp_yolo_forward writes (attrs = 5 + classes, boxes in
 * detector-input pixels, rows ordered head, anchor, gy, gx).  heads [nheads][4] int32 = (first row, anchors, gh, gw) is a
 * HOST array in both calls; the heads follow each other from row 0 and cover every row.  A row with objectness > thresh
 * (thresh >= 0) is a candidate: box / (net_w, net_h), prob[k] = objectness * cls[k], 0 unless > thresh; its candidate
 * index counts head, cell, anchor as Darknet does.  For each class the candidates are sorted by prob[k] descending,
 * stably over the order the previous class left (initially the candidate index), and every entry with prob[k] != 0
 * zeroes prob[k] of every later entry whose box_iou with it is > nms.  nms <= 0 skips this.  d_dets [B][max_dets][6 +
 * classes] f32 = (x, y, w, h, objectness, candidate index, prob[classes]) in the order the last class's sort left, zero
 * past the count; d_count [B] int32 = the true number of candidates.  An image with d_count[b] > max_dets has a zero
 * block: it is reported, never cut.  max_dets <= bp_yolo_map_max_dets() (4096) on the device, any on the host.
 * d_scratch holds bp_yolo_detections_scratch(B, max_dets, classes) bytes. */
int bp_yolo_map_max_dets(void);
size_t bp_yolo_detections_scratch(int B, int max_dets, int classes);
int bp_yolo_detections(const float* d_pred, int B, int rows, int attrs, const int* heads, int nheads, int net_w, int net_h,
                       int classes, float thresh, float nms, int max_dets, float* d_dets, int* d_count, void* d_scratch,
                       void* stream);
int bp_yolo_detections_host(const float* pred, int B, int rows, int attrs, const int* heads, int nheads, int net_w, int net_h,
                            int classes, float thresh, float nms, int max_dets, float* dets, int* count);
/* bp_detector_map_match: detector.c:665-756 for a batch.  d_dets, d_count as above (an image whose count exceeds max_dets
 * gives no record); d_labels [M][5] f32 = (id, x, y, w, h) with d_first [B + 1] int32 as bp_yolo_truth takes them.  For
 * every detection and class with prob > 0, in that order, a record of 6 words: (p, image_base + b, class, truth, max_iou,
 * position within the image); truth = truth_base + the index in d_labels of the same-class label with the greatest
 * box_iou > iou_thresh (the first on ties), or -1.  d_rec [B][rec_stride][6] f32, zero past the count; d_rec_count [B] =
 * the true number (records past rec_stride are dropped, also from the statistics: size it from d_count).
 * d_truth_classes_count [classes] int32 is ADDED to, one per label whose id is a whole number in [0, classes) (any other
 * label is passed over).  d_img_stats [B][3] f64 = (tp, fp, iou_sum) over the records with p > thresh_calc as the
 * reference counts them: a true positive has a truth that no earlier record of the image claims, whatever that
 * record's prob or class; all else is a false positive.  d_claim [M + 1] int32 is scratch. */
int bp_detector_map_match(const float* d_dets, const int* d_count, int B, int max_dets, int classes, const float* d_labels, int M,
                          const int* d_first, float iou_thresh, float thresh_calc, int truth_base, int image_base, int rec_stride,
                          float* d_rec, int* d_rec_count, int* d_truth_classes_count, double* d_img_stats, int* d_claim,
                          void* stream);
int bp_detector_map_match_host(const float* dets, const int* count, int B, int max_dets, int classes, const float* labels, int M,
                               const int* first, float iou_thresh, float thresh_calc, int truth_base, int image_base,
                               int rec_stride, float* rec, int* rec_count, int* truth_classes_count, double* img_stats);
/* bp_detector_map_reduce: detector.c:774-876 over the run's D records, d_rec [D][6] in any order.  Ranks: p descending,
 * then image, position (and index) ascending.  A record is a true positive when it is the first in rank order to claim
 * its truth (< truths = unique_truth_count), a later claimant counts as neither, a record without a truth is a false
 * positive of its class.  d_ap [classes] f64 = the 11-point AP (recall >= point * 0.1 in double); d_stats [8] f64 = mAP,
 * then precision, recall and F1 in float32 as the reference forms them (NaN where it divides 0 by 0), average IoU, TP, FP
 * and FN at thresh_calc from d_img_stats [N][3] added in index order; d_pr (or NULL) [classes][D][2] f64 = (precision,
 * recall) of every rank.  d_scratch holds bp_detector_map_reduce_scratch(D, truths) bytes. */
size_t bp_detector_map_reduce_scratch(int D, int truths);
int bp_detector_map_reduce(const float* d_rec, int D, const int* d_truth_classes_count, int classes, int truths,
                           const double* d_img_stats, int N, double* d_ap, double* d_stats, double* d_pr, void* d_scratch,
                           void* stream);
int bp_detector_map_reduce_host(const float* rec, int D, const int* truth_classes_count, int classes, int truths,
                                const double* img_stats, int N, double* ap, double* stats, double* pr);
/* One Darknet training iteration: train_network_datum's CPU path for convolutional layers, in four
 * calls that betapose_amd/darknet_train.py strings together.  Tensors are f32 [N][C][H][W], filters [K][C][size][size];
 * size is 1 or 3, stride 1 or 2, padding size / 2.  Each device function is meant to be bit-identical to its _host twin,
 * which needs no GPU.  No floating-point atomics.
 *
 * bp_train_conv: one implicit GEMM on the fp32 matrix pipe in one of three roles.  role 0: y [N][K][OH][OW] = the raw
 * convolution of x [N][C][H][W] with w (every element written); role 1: w, here the filter UPDATES, += delta (y) x
 * im2col(x), summed over (n, oy, ox) ascending in slices of 2048 added in order, through d_scratch
 * [bp_train_conv_scratch()] floats; role 2: x, here the INPUT's delta, += w^T delta (y).  An element is one fmaf chain
 * over k = (ky, kx, channel) ascending.
 * bp_train_bn_forward: x [N][C][S] the raw convolution.  bn and train: mean, var [C] (f64 sums in a fixed order, the
 * variance over N * S - 1, so N * S = 1 is an error), rolling = .9 rolling + .1 batch, x_norm and out = leaky(x_norm *
 * scale + bias); bn and not train: the rolling pair normalises; not bn: out = act(x + bias), the other pointers may be
 * NULL.  leaky 0 is the linear activation.
 * bp_train_bn_backward: delta [N][C][S] (of out) becomes the delta of the raw convolution: the activation's gradient
 * keyed on out, bias_updates += sum, and with bn scale_updates += sum(delta x_norm), the scaling, mean_delta,
 * variance_delta and normalize_delta as Darknet forms them.  stat [2][C] is scratch.
 * bp_train_update: update_convolutional_layer for every tensor of a table of (parameter, update, count, kind) rows of
 * four 64-bit words, on the side that runs it; kind 1 (filters): u += decay_term * p first; then p += rate_over_batch *
 * u; u *= momentum, each a rounded f32 step.  blocks = the sum over the rows of ceil(count / bp_train_update_chunk()). */
size_t bp_train_conv_scratch(int N, int C, int H, int W, int K, int size, int stride);
int bp_train_update_chunk(void);
int bp_train_conv(int role, float* d_x, float* d_w, float* d_y, int N, int C, int H, int W, int K, int size, int stride,
                  float* d_scratch, void* stream);
int bp_train_conv_host(int role, float* x, float* w, float* y, int N, int C, int H, int W, int K, int size, int stride,
                       float* scratch);
int bp_train_bn_forward(const float* d_x, int N, int C, int S, const float* d_scales, const float* d_biases,
                        float* d_rolling_mean, float* d_rolling_var, float* d_mean, float* d_var, float* d_x_norm, float* d_out,
                        int bn, int leaky, int train, void* stream);
int bp_train_bn_forward_host(const float* x, int N, int C, int S, const float* scales, const float* biases, float* rolling_mean,
                             float* rolling_var, float* mean, float* var, float* x_norm, float* out, int bn, int leaky,
                             int train);
int bp_train_bn_backward(const float* d_out, float* d_delta, const float* d_x, const float* d_x_norm, const float* d_mean,
                         const float* d_var, const float* d_scales, int N, int C, int S, float* d_bias_updates,
                         float* d_scale_updates, float* d_stat, int bn, int leaky, void* stream);
int bp_train_bn_backward_host(const float* out, float* delta, const float* x, const float* x_norm, const float* mean,
                              const float* var, const float* scales, int N, int C, int S, float* bias_updates,
                              float* scale_updates, float* stat, int bn, int leaky);
int bp_train_update(const void* d_table, int tensors, int blocks, float rate_over_batch, float decay_term, float momentum,
                    void* stream);
int bp_train_update_host(const void* table, int tensors, float rate_over_batch, float decay_term, float momentum);
/* One training iteration of the key-point detector (train_KPD/src/train.py train() / valid() for FastPose_SE), DESIGN.md
 * 3.14.  float32 [N][C][S] activations and gradients (the loss's gradient, torch's sign).  Each device function is meant
 * to be bit-identical to its _host twin, which needs no GPU.  No floating-point atomics.  On the device a tensor whose S
 * is a multiple of 4 must be 16-byte aligned.
 *
 * bp_kpd_train_conv: bp_train_conv's core, unchanged, admitting size 7 too (padding size / 2: the 7 x 7 / 2 stem); a
 * Linear is size 1 on a 1 x 1 map with N the batch.  Gradients are added to their buffers.
 * bp_kpd_train_bn_forward: torch's BatchNorm2d.  bn and train: mean [C] and invstd [C] = 1 / sqrt(var + 1e-5) from f64
 * sums in a fixed order (biased variance; N * S = 1 is an error), running = .9 running + .1 batch (the variance
 * unbiased), out = relu?(((x - mean) * invstd) * w + b); bn and not train: the running pair normalises; not bn: out =
 * relu?(x + b), the other pointers may be NULL.
 * bp_kpd_train_bn_backward: d (of out) becomes the gradient of x in place: m = relu ? d * (out > 0) : d, grad_b += sum(m),
 * grad_w += sum(m * (x - mean)) * invstd, d = (m - sum / n - (x - mean) * dotp * invstd^2 / n) * invstd * w; not bn: d = m.
 * bp_kpd_train_tail_forward: out = relu(y * s[n][c] + res), s NULL in a block without SE.  _backward: m = dout * (out > 0),
 * dres += m, dy = m * s, ds [N][C] = sum_S m * y.
 * bp_kpd_train_pool_forward: pool [rows] = the f64 sum of each row of S values, times 1 / S.  _backward: dy += dpool / S.
 * bp_kpd_train_sigmoid_forward: s = 1 / (1 + exp(-x)) with the library's own exp.  _backward: g = g * (1 - s) * s in place.
 * bp_kpd_train_maxpool_forward: 3 x 3, stride 2, padding 1 (-inf) over [planes][H][W]; arg [planes][OH][OW] int32 holds
 * iy * W + ix of the window's first maximum in scan order.  _backward: dx (written) gathers the outputs that chose it.
 * bp_kpd_train_rmsprop: torch.optim.RMSprop (not centred) for every tensor of a table of (parameter, gradient, square_avg,
 * momentum buffer, count) rows of five 64-bit words, on the side that runs it, in torch's single-tensor order with the
 * roundings of torch's CPU kernels (g + wd p, v + ((1 - alpha) g) g and p - lr b are fused multiply-adds).  blocks = the sum over the rows of ceil(count / bp_kpd_train_update_chunk()). */
size_t bp_kpd_train_conv_scratch(int N, int C, int H, int W, int K, int size, int stride);
int bp_kpd_train_update_chunk(void);
int bp_kpd_train_conv(int role, float* d_x, float* d_w, float* d_y, int N, int C, int H, int W, int K, int size, int stride,
                      float* d_scratch, void* stream);
int bp_kpd_train_conv_host(int role, float* x, float* w, float* y, int N, int C, int H, int W, int K, int size, int stride,
                           float* scratch);
int bp_kpd_train_bn_forward(const float* d_x, int N, int C, int S, const float* d_w, const float* d_b, float* d_running_mean,
                            float* d_running_var, float* d_mean, float* d_invstd, float* d_out, int bn, int relu, int train,
                            void* stream);
int bp_kpd_train_bn_forward_host(const float* x, int N, int C, int S, const float* w, const float* b, float* running_mean,
                                 float* running_var, float* mean, float* invstd, float* out, int bn, int relu, int train);
int bp_kpd_train_bn_backward(const float* d_out, float* d_d, const float* d_x, const float* d_mean, const float* d_invstd,
                             const float* d_w, int N, int C, int S, float* d_grad_w, float* d_grad_b, int bn, int relu,
                             void* stream);
int bp_kpd_train_bn_backward_host(const float* out, float* d, const float* x, const float* mean, const float* invstd, const float* w,
                                  int N, int C, int S, float* grad_w, float* grad_b, int bn, int relu);
int bp_kpd_train_tail_forward(const float* d_y, const float* d_s, const float* d_res, float* d_out, int N, int C, int S,
                              void* stream);
int bp_kpd_train_tail_forward_host(const float* y, const float* s, const float* res, float* out, int N, int C, int S);
int bp_kpd_train_tail_backward(const float* d_out, const float* d_dout, const float* d_y, const float* d_s, float* d_dres,
                               float* d_dy, float* d_ds, int N, int C, int S, void* stream);
int bp_kpd_train_tail_backward_host(const float* out, const float* dout, const float* y, const float* s, float* dres, float* dy,
                                    float* ds, int N, int C, int S);
int bp_kpd_train_pool_forward(const float* d_y, int rows, int S, float* d_pool, void* stream);
int bp_kpd_train_pool_forward_host(const float* y, int rows, int S, float* pool);
int bp_kpd_train_pool_backward(const float* d_dpool, float* d_dy, int rows, int S, void* stream);
int bp_kpd_train_pool_backward_host(const float* dpool, float* dy, int rows, int S);
int bp_kpd_train_sigmoid_forward(const float* d_x, float* d_s, long long n, void* stream);
int bp_kpd_train_sigmoid_forward_host(const float* x, float* s, long long n);
int bp_kpd_train_sigmoid_backward(const float* d_s, float* d_g, long long n, void* stream);
int bp_kpd_train_sigmoid_backward_host(const float* s, float* g, long long n);
int bp_kpd_train_maxpool_forward(const float* d_x, int planes, int H, int W, float* d_out, int* d_arg, void* stream);
int bp_kpd_train_maxpool_forward_host(const float* x, int planes, int H, int W, float* out, int* arg);
int bp_kpd_train_maxpool_backward(const float* d_dout, const int* d_arg, int planes, int H, int W, float* d_dx, void* stream);
int bp_kpd_train_maxpool_backward_host(const float* dout, const int* arg, int planes, int H, int W, float* dx);
int bp_kpd_train_rmsprop(const void* d_table, int tensors, int blocks, double lr, double alpha, double eps, double weight_decay,
                         double momentum, void* stream);
int bp_kpd_train_rmsprop_host(const void* table, int tensors, double lr, double alpha, double eps, double weight_decay,
                              double momentum);
/* Key-point designation (stage 1 of the reference).  All geometry is float64, points are [n][3], every sum runs in
 * ascending index order and every choice among equals goes to the lower index; each device function is bit-identical to
 * its _host twin, which needs no GPU.
 *
 * bp_voxel_grid_host: the centroid of every occupied cell of a grid of size `leaf` (cell floor(p / leaf) per axis), the
 * cells in ascending key x + y * dx + z * dx * dy; out [n][3] receives *n_out rows.  When the grid has more than
 * INT32_MAX cells the cloud is copied through unchanged (PCL's "leaf size is too small").  Host only.
 *
 * bp_sift_octave: one octave of the 3-D SIFT detector on the scalar field `field` (0, 1, 2: the x, y or z coordinate).
 * scales [ns] (host, positive, ascending, 4 <= ns <= 12) are the Gaussian sigmas.  G_i(p) is the mean of the field over
 * the points q with d2 = |p - q|^2 <= 9 sigma_i^2 under the weights exp(-d2 / (2 sigma_i^2)) (an exponential of the
 * library's own, within 1e-14 of libm's); d_dog [n][ns-1] = G_{j+1} - G_j.  d_flags [n][ns-3] int8: entry j-1 is -1 / +1
 * where DoG[p][j] is at least min_contrast in magnitude, strictly below / above DoG[p][j-1] and DoG[p][j+1], and not
 * above / below any of DoG[q][j-1 .. j+1] over the min(k, n) nearest points q (p among them, 1 <= k <= 64); 0
 * elsewhere.  All pairs are visited: n <= 131072.  Enqueued on `stream` without synchronising it.
 *
 * bp_farthest_points: K <= n <= 2^20 indices d_idx [K], the first `start` (negative: the point farthest from the
 * centroid), each next one the point with the largest squared distance to those chosen so far; d_d2 [K] is that
 * distance (for the first: its squared distance from the centroid).  Synchronises `stream`.
 *
 * bp_thin_points: Model3D.refine's rounds, n - keep of them (n <= 16384): delete the first point, in row-major pair
 * order, of the pair with the smallest distance sqrt(d2).  The rounds stop early at the first one whose smallest
 * distance is not below 100.0, from where the reference deletes a carried position over and over (the caller does
 * that).  d_alive [n] uint8: 1 for a survivor; d_state [2] int32: the rounds done and the position, among the survivors
 * before it was deleted, of the last deleted point (0 when none was).  Synchronises `stream`. */
int bp_voxel_grid_host(const double* points, int n, double leaf, double* out, int* n_out);
int bp_sift_octave(const double* d_points, int n, int field, const double* scales, int ns, int k, double min_contrast,
                   double* d_dog, signed char* d_flags, void* stream);
int bp_sift_octave_host(const double* points, int n, int field, const double* scales, int ns, int k, double min_contrast,
                        double* dog, signed char* flags);
int bp_farthest_points(const double* d_points, int n, int K, int start, int* d_idx, double* d_d2, void* stream);
int bp_farthest_points_host(const double* points, int n, int K, int start, int* idx, double* d2);
int bp_thin_points(const double* d_points, int n, int keep, unsigned char* d_alive, int* d_state, void* stream);
int bp_thin_points_host(const double* points, int n, int keep, unsigned char* alive, int* state);
/* Depth refinement of P estimated poses of one mesh: projective point-to-plane ICP of the mesh's render (as
 * bp_render_depth draws it) against the test depth image d_test_index[p] of d_depth_test [T][H][W] uint16 (depth =
 * raw * depth_scale in pose units, 0 = missing).  Up to `iterations` times: render at the current pose; every pixel
 * whose render and whose four neighbours' renders are drawn and whose test depth is present gives the model point
 * q = z_r d on its ray d, the normal n of the rendered surface from the neighbours' points (turned towards the camera),
 * the residual r = (z_t - z_r)(n.d) and the row J = [(q - t) x n, n]; pixels with -(n.d)/|d| < min_cos or
 * |z_t - z_r| > max_dist are left out.  A xi = b with A = sum J^T J, b = sum J^T r, xi = (omega, v), then
 * R <- exp(omega) R, t <- t + v.  One more accumulation follows the last step.  A pose stops early with status
 * 1 TOO_FEW (fewer than min_pixels pixels), 2 SINGULAR (no pivot), 3 DIVERGED (|omega| > 0.5 rad or |v| > 4 max_dist;
 * the pose before that step is kept); 0 OK took every step.  A pose that ends with a larger rms residual than it began
 * with is returned as it came, bit for bit, with status 4 REJECTED; a test index outside [0, T) gives 5 NO_IMAGE and the
 * pose unchanged.  d_poses_out [P][12] (must not be d_poses); d_stats [P][6] f64 = (N_first, rms_first, N_last, rms_last,
 * iterations_done, status), N the number of pixels that took part, the *_last pair describing the returned pose.
 * Poses are processed `chunk` at a time (0: as many as keep the workspaces under 256 MB); the results do not depend on
 * it and are bit-identical from run to run (no floating-point atomics).  The loop over the iterations runs on `stream`
 * without a host round trip; the call synchronises `stream` at its end.
 * bp_icp_normal_equations is ONE accumulation at the given poses: d_out [P][29] f64 = A's upper triangle row by row
 * (21), b (6), N, E = sum r^2; zeros for a test index outside [0, T).
 * The *_host calls are the same on host memory, without a GPU: every pixel's decision and term has the device's bits,
 * the sums differ by the rounding of their order.  They refuse a face index outside [0, n). */
int bp_refine_depth(const double* d_model, int n, const int* d_faces, int F, const double* d_poses, int P, const double* K,
                    const uint16_t* d_depth_test, int T, int H, int W, double depth_scale, const int* d_test_index,
                    int iterations, double max_dist, double min_cos, int min_pixels, double pixel_center, double near_z,
                    int chunk, double* d_poses_out, double* d_stats, void* stream);
int bp_refine_depth_host(const double* poses, int P, const double* vertices, int n, const int* faces, int F, const double* K,
                         const uint16_t* depth_test, int T, int H, int W, double depth_scale, const int* test_index,
                         int iterations, double max_dist, double min_cos, int min_pixels, double pixel_center, double near_z,
                         double* poses_out, double* stats);
int bp_icp_normal_equations(const double* d_model, int n, const int* d_faces, int F, const double* d_poses, int P,
                            const double* K, const uint16_t* d_depth_test, int T, int H, int W, double depth_scale,
                            const int* d_test_index, double max_dist, double min_cos, double pixel_center, double near_z,
                            int chunk, double* d_out, void* stream);
int bp_icp_normal_equations_host(const double* poses, int P, const double* vertices, int n, const int* faces, int F,
                                 const double* K, const uint16_t* depth_test, int T, int H, int W, double depth_scale,
                                 const int* test_index, double max_dist, double min_cos, double pixel_center, double near_z,
                                 double* out);
/* one fused convolution on device tensors (unit tests / kernel benchmarks).  h_w: host OIHW filter, h_bias host or NULL.
 * d_in NHWC [N,H,W,Cin]; d_out per store_mode (0 NHWC, 1 nearest-x2 NHWC, 2 PixelShuffle(2) NHWC, 3 NCHW);
 * act 0 linear / 1 leaky(0.1) / 2 relu; d_res NHWC residual or NULL; splits 0 auto; tile -1 auto, else a kernel id
 * (csrc/bp_common.h ConvTile) plus the operand mode: 0 = 64x64 block, 1 = 128x64 (fp32 MFMA); 13..16 = conv_pl.hip (both
 * operands by LDS-DMA from 16-bit planes: 64x64, 128x128, 128x64, 256x128 blocks); + 256 fp16 operands, + 512 bf16x3.
 * bp_conv2d_planes additionally returns the operand planes the epilogue emits for the next layer
 * (d_out_planes [np][output elements] u16: one fp16 plane or three bf16 planes that sum to the fp32 output exactly). */
int bp_conv2d(const float* d_in, int N, int H, int W, int Cin, const float* h_w, const float* h_bias, int Cout, int k,
              int stride, int pad, int act, int store_mode, const float* d_res, int res_after_act, int tile, int splits,
              float* d_out, int iters, float* ms_per_iter, void* stream);
int bp_conv2d_planes(const float* d_in, int N, int H, int W, int Cin, const float* h_w, const float* h_bias, int Cout, int k,
                     int stride, int pad, int act, int store_mode, const float* d_res, int res_after_act, int tile, int splits,
                     float* d_out, unsigned short* d_out_planes, int iters, float* ms_per_iter, void* stream);
/* ... and the wider form both forward to, with the launch forms of the SE blocks:
 * d_res_scale  device [N][Cout] f32 or NULL: the skip connection multiplied by a gate per image and channel (needs d_res);
 * d_pool_out   device [ceil(M / 64)][Cout] f32 or NULL, M = N OH OW: the launch's epilogue also writes the column sums of
 *              conv + bias over every 64-row slab (the global average pool as slice sums).  Only under the engine's own
 *              precondition -- a 64x64 tile, NHWC store, no residual, linear activation, Cout % 4 == 0, and N == 1 or
 *              OH OW % 64 == 0 -- otherwise the call fails and nothing is launched. */
int bp_conv2d_se(const float* d_in, int N, int H, int W, int Cin, const float* h_w, const float* h_bias, int Cout, int k,
                 int stride, int pad, int act, int store_mode, const float* d_res, int res_after_act, int tile, int splits,
                 float* d_out, unsigned short* d_out_planes, const float* d_res_scale, float* d_pool_out, int iters,
                 float* ms_per_iter, void* stream);
/* The auxiliary kernels of the SE blocks and the DUC layers, one launch each (unit tests); every call waits for its launch.
 * bp_avgpool: d_in NHWC view [N][HW][C] with row stride in_ld >= C -> d_out [N][*parts][C], the SUMS of *parts pixel slices
 *   of ceil(HW / *parts) pixels each (empty slices 0); d_out NULL: only *parts is returned.
 * bp_fc: d_out[b][o] = act(h_bias[o] + sum_i h_w[o][i] x[b][i]), act 0 linear / 2 relu / 3 sigmoid, x = d_in [N][Cin]
 *   (in_parts == 1) or in_scale * sum_p d_in[b][p][i] (d_in [N][in_parts][Cin]); Cin % 4 == 0; h_w host [Cout][Cin].
 * bp_maxpool3s2p1: NHWC [N][H][W][C] -> [N][(H-1)/2+1][(W-1)/2+1][C], 3x3 / stride 2 / pad 1, C % 4 == 0.
 * bp_pixel_shuffle2: NHWC [N][H][W][C] -> [N][2H][2W][C/4], out[c, 2h+i, 2w+j] = in[4c + 2i + j, h, w].
 *   d_out_planes: NULL (np 0), or [np][output elements] u16 operand planes of the output (np 1 fp16 / 3 bf16x3). */
int bp_avgpool(const float* d_in, int in_ld, int N, int HW, int C, float* d_out, int* parts, void* stream);
int bp_fc(const float* d_in, const float* h_w, const float* h_bias, int N, int Cin, int Cout, int act, int in_parts, float in_scale,
          float* d_out, void* stream);
int bp_maxpool3s2p1(const float* d_in, int N, int H, int W, int C, float* d_out, unsigned short* d_out_planes, int np, void* stream);
int bp_pixel_shuffle2(const float* d_in, int N, int H, int W, int C, float* d_out, unsigned short* d_out_planes, int np, void* stream);

/* ---- whole frame on device: resize -> detector -> select -> crop -> KPD -> arg-max, optionally as one hipGraph ---- */
/* d_frames [batch][H][W][3] u8 BGR, d_results [batch][BP_RESULT_FLOATS], d_hm [batch][50][80][64]: caller-owned
 * device buffers (NULL -> allocated and owned by the pipeline). */
int bp_pipeline_create(bp_yolo* y, bp_kpd* k, int frame_h, int frame_w, int batch, float conf, int num_classes,
                       uint8_t* d_frames, float* d_results, float* d_hm, bp_pipeline** out);
void bp_pipeline_destroy(bp_pipeline* p);
uint8_t* bp_pipeline_frames(bp_pipeline* p);    /* device [batch][H][W][3] u8 BGR, caller fills */
int bp_pipeline_kernel_count(bp_pipeline* p);   /* kernel launches per run (after the first graph capture) */
float* bp_pipeline_results(bp_pipeline* p);     /* device [batch][BP_RESULT_FLOATS] */
float* bp_pipeline_heatmaps(bp_pipeline* p);    /* device [batch][50][80][64] */
int bp_pipeline_set_fixed_box(bp_pipeline* p, const float* box_xyxy_or_null);
int bp_pipeline_run(bp_pipeline* p, int use_graph, void* stream);
/* While either engine is in the lone-frame latency mode (bp_*_set_prefetch) bp_pipeline_run waits for the frame, reads the engines'
 * placement error words and, on a fault, clears them, switches the mode off for both engines and runs the same frame again on the
 * ordinary hand-off: every caller gets a valid record.  bp_pipeline_latency_faults = frames re-run that way so far (-1: null). */
int bp_pipeline_latency_faults(const bp_pipeline* p);
/* Set-up step: capture and instantiate the frame's hipGraph now (records the launches, executes nothing), so that the first
 * bp_pipeline_run(use_graph = 1) is a plain graph launch.  Called again after a precision / policy change it rebuilds the graph.
 * (It creates the pipeline's capture stream: call it AFTER the caller's own streams have launched something -- HIP binds streams to
 * its four hardware queues as they are first used, and two pipelines prepared first were seen to share one queue.) */
int bp_pipeline_prepare(bp_pipeline* p);

/* ---- device pose tail (opt-in): what pipeline.finish_record does on the host, per frame on the GPU ----
 * Key-point decode and pPose-NMS in f32 and the pruning bit-identical to the host tail; the PnP is bp_solve_pnp's algorithm
 * in f64 in the host's operation order (agrees with it to rounding).  kp3d [50][3] f64 = the 3-D key points, K [9] host,
 * left_number >= 0 = key points kept (--left_keypoints).
 * bp_pipeline_set_pose_solver: kp3d host; NULL switches the tail off.  Either way the captured graph is dropped (as
 * bp_pipeline_set_fixed_box does); while it is on, every run ends with one more launch that writes the pose records into
 * d_poses [batch][BP_POSE_DOUBLES] (device; NULL: the pipeline's own buffer, as bp_pipeline_create's d_results). */
int bp_pipeline_set_pose_solver(bp_pipeline* p, const double* kp3d, int n_kp, const double* K, int left_number,
                                double* d_poses);
double* bp_pipeline_poses(bp_pipeline* p);      /* device [batch][BP_POSE_DOUBLES]; NULL while no solver was ever set */
/* the tail alone, on records made any way: d_records [batch][BP_RESULT_FLOATS], d_kp3d device, d_poses [batch][166] */
int bp_pose_from_records(const float* d_records, int batch, const double* d_kp3d, int n_kp, const double* K, int left_number,
                         double* d_poses, void* stream);
/* bp_solve_pnp over P independent problems of n <= BP_PNP_MAX_POINTS points, one wave each: d_pts3d [n][3] shared by all
 * (shared_3d = 1) or [P][n][3], d_pts2d [P][n][2], K [9] host -> d_Rt [P][12] ([R | t] row-major, NaN unless the status is
 * 0), d_status [P] (bp_solve_pnp's codes: 0, -1 too few points, -2 degenerate).  Asynchronous on `stream`. */
int bp_solve_pnp_batch(const double* d_pts3d, int shared_3d, const double* d_pts2d, int n, int P, const double* K,
                       double* d_Rt, int* d_status, void* stream);

/* ---- RANSAC PnP on device (the solvePnPRansac variant, utils/utils.py:32-36) ----
 * The device result is the result of bp_solve_pnp_ransac's sequential loop: same samples, same inlier test, same early
 * stop, the refit by bp_solve_pnp_batch's solver on the same inlier set -- R, t agree with the host to the rounding that
 * solver's contract leaves, masks and statuses are equal unless a point's reprojection error sits within that rounding
 * of the threshold.  All max_trials hypotheses run in parallel (one wave each), then one wave per problem replays the
 * host's loop over their inlier counts and refits.
 *
 * bp_pnp_ransac_samples: the sampler's draws, idx [max_trials][6] -- six distinct indices below n per trial; depends on
 * (n, max_trials) only.  bp_pnp_ransac_trials_needed: need [n + 1], the trial limit after a hypothesis with cnt inliers
 * (INT_MAX: no limit), applied as `if (need[cnt] < trials) trials = max(it + 1, need[cnt])`.  Host only, no device work. */
int bp_pnp_ransac_samples(int n, int max_trials, int* idx);
int bp_pnp_ransac_trials_needed(int n, double confidence, int* need);
size_t bp_pnp_ransac_workspace_bytes(int P, int max_trials);
/* P problems of n <= BP_PNP_MAX_POINTS points (layout as bp_solve_pnp_batch).  d_Rt [P][12], NaN unless the status is 0;
 * d_status [P]: 0, -1 (n < 6), -2 (no six-point consensus) or the refit's status; d_inliers [P][n] u8 or NULL, all zero
 * for status -1 / -2.  d_workspace: bp_pnp_ransac_workspace_bytes(P, max_trials) bytes, 8-byte aligned, the caller's,
 * in use until the stream has passed the call.  Asynchronous on `stream`, no allocation, capturable. */
int bp_solve_pnp_ransac_batch(const double* d_pts3d, int shared_3d, const double* d_pts2d, int n, int P, const double* K,
                              double reproj_err, int max_trials, double confidence, double* d_Rt, int* d_status,
                              unsigned char* d_inliers, void* d_workspace, size_t workspace_bytes, void* stream);
/* The device pose tail with RANSAC in place of the plain PnP: needs a pose solver set (bp_pipeline_set_pose_solver keeps
 * the setting); max_trials = 0 switches back to the iterative tail.  Drops the captured graph.  While on, the tail is
 * three launches (prepare: decode / NMS / pruning; hypotheses; select-and-refit) instead of one and slot [15] of the
 * pose record carries the inlier set.  The workspace is the pipeline's. */
int bp_pipeline_set_pose_ransac(bp_pipeline* p, double reproj_err, int max_trials, double confidence);
size_t bp_pose_ransac_workspace_bytes(int batch, int max_trials);
/* bp_pose_from_records with the RANSAC solver; d_workspace: bp_pose_ransac_workspace_bytes(batch, max_trials) bytes */
int bp_pose_from_records_ransac(const float* d_records, int batch, const double* d_kp3d, int n_kp, const double* K,
                                int left_number, double reproj_err, int max_trials, double confidence, double* d_poses,
                                void* d_workspace, size_t workspace_bytes, void* stream);

/* ---- scene: ONE multi-class detector pass per frame feeding K objects' pose chains (opt-in; bp_pipeline_* is unchanged) ----
 * Multi-object scenes run one detector per object with bp_pipeline: K resizes and K detector passes per frame.  A scene
 * resizes the frame once, runs the shared detector `y` once with the per-class select (class_ids[k] = object k's class),
 * then per object k: crop from row k's box -> kpds[k] -> arg-max -> (opt-in) that object's pose tail.  One stream, one
 * hipGraph, the launches in that order; one frame per scene (frames in flight = scenes on separate streams over engine
 * clones).  d_frames [H][W][3] u8 BGR and d_results [K][BP_RESULT_FLOATS] are the caller's (NULL: the scene's own);
 * row k is the record bp_pipeline writes for that object, select slots [6], [7] = class score, class id.  A class
 * without a detection leaves its row as bp_pipeline leaves a frame without a box (index -1).  kpds: K distinct engines. */
int bp_scene_create(bp_yolo* y, bp_kpd* const* kpds, const int* class_ids, int K, int frame_h, int frame_w, float conf,
                    int num_classes, uint8_t* d_frames, float* d_results, bp_scene** out);
void bp_scene_destroy(bp_scene* s);
float* bp_scene_results(bp_scene* s);           /* device [K][BP_RESULT_FLOATS] */
/* slot k's device pose tail, as bp_pipeline_set_pose_solver / bp_pipeline_set_pose_ransac: d_poses_row = that object's
 * [BP_POSE_DOUBLES] row (NULL: row k of the scene's own [K][BP_POSE_DOUBLES] buffer, bp_scene_poses).  Drops the graph. */
int bp_scene_set_pose_solver(bp_scene* s, int k, const double* kp3d, int n_kp, const double* K, int left_number,
                             double* d_poses_row);
int bp_scene_set_pose_ransac(bp_scene* s, int k, double reproj_err, int max_trials, double confidence);
double* bp_scene_poses(bp_scene* s);            /* NULL until a solver was set without a buffer */
int bp_scene_prepare(bp_scene* s);              /* capture + instantiate now; re-captures after a plan change of any engine */
int bp_scene_run(bp_scene* s, int use_graph, void* stream);
int bp_scene_kernel_count(bp_scene* s);         /* graph nodes per run (after the first capture), -1 before */

/* ---- candidates: several NMS survivors per frame, merged by pPose-NMS (opt-in; bp_pipeline_* and bp_scene_* are unchanged) ----
 * One frame per object, one stream, one hipGraph: resize -> detector -> select with box NMS -> one crop launch over the C
 * boxes -> key-point net at batch C -> arg-max -> (opt-in) the candidate pose tail.  k's max_batch must be >= C.  d_frame
 * [H][W][3] u8 BGR and d_results [C][BP_RESULT_FLOATS] are the caller's (NULL: the object's own); row c is the record
 * bp_pipeline writes for candidate c; bp_cands_counts: device int [1], the survivors.  The graph always runs at batch C:
 * unused slots are carried (index -1) and ignored by the tail.  With C = 1 the row is bp_pipeline's, bit for bit. */
int bp_cands_create(bp_yolo* y, bp_kpd* k, int max_candidates, int frame_h, int frame_w, float conf, int num_classes,
                    int class_id, float nms_conf, uint8_t* d_frame, float* d_results, bp_cands** out);
void bp_cands_destroy(bp_cands* s);
float* bp_cands_results(bp_cands* s);           /* device [C][BP_RESULT_FLOATS] */
int* bp_cands_counts(bp_cands* s);              /* device [1] */
int bp_cands_prepare(bp_cands* s);
int bp_cands_run(bp_cands* s, int use_graph, void* stream);
int bp_cands_kernel_count(bp_cands* s);         /* graph nodes per run (after the first capture), -1 before */
/* The candidate pose tail, one wave64 workgroup per frame: decode of the n = count valid candidates (f32, bit-identical to
 * the host), the full pPose-NMS over them as bp_pose_nms (pick, merged x / y / score and proposal score bit-identical; only
 * tanhf / expf may round differently from the host's libm, and they feed the comparison simi > gamma alone), result[0] = the
 * first merged pose that survives the filters, the left_number pruning, the iterative PnP.
 *   d_pose [BP_POSE_DOUBLES]: the frame's row for result[0], today's layout; status 2 = every merged pose was filtered
 *     out, 1 = no candidate
 *   merged [C][BP_MERGED_FLOATS] f32: for each merged pose j < m the pick (int bits), the proposal score, 50 x (x, y, score)
 *   info [4] int: n, m, index of result[0] among the merged poses (-1: none), bit mask of the candidates merged into it
 * bp_cands_set_pose_solver: kp3d host [50][3]; NULL switches the tail off; drops the graph; d_pose NULL: the object's own
 * row (bp_cands_pose).  bp_cands_merged / bp_cands_info: device, NULL until a solver was set.  A RANSAC variant does not
 * exist yet. */
int bp_cands_set_pose_solver(bp_cands* s, const double* kp3d, int n_kp, const double* K, int left_number, double* d_pose);
double* bp_cands_pose(bp_cands* s);
float* bp_cands_merged(bp_cands* s);
int* bp_cands_info(bp_cands* s);
/* the tail alone: d_records [frames][C][BP_RESULT_FLOATS], d_counts [frames], d_kp3d device [50][3] -> d_poses [frames][166],
 * d_merged [frames][C][152], d_info [frames][4] */
int bp_pose_from_candidate_records(const float* d_records, const int* d_counts, int frames, int C, const double* d_kp3d,
                                   int n_kp, const double* K, int left_number, double* d_poses, float* d_merged, int* d_info,
                                   void* stream);
/* A pose for EVERY merged candidate (opt-in; the tail above solves result[0] alone), one wave64 workgroup per (frame, slot):
 *   inst_poses [C][BP_POSE_DOUBLES] f64, row j in the pose row's layout: status, points used, R [9], t [3], proposal
 *     score, slot 15 = 0, 50 x (x, y, score)
 *   j = 0            the frame's existing pose row (d_pose), all 166 doubles, whatever its status (0, 1 = no candidate,
 *                    2 = everything filtered, < 0 = PnP failed); the PnP of result[0] is not repeated
 *   0 < j < m        merged pose j through the same left_number pruning and iterative PnP: status = the solver's code,
 *                    R and t NaN when it is non-zero, proposal score = merged[j][1], the 50 unpruned key points
 *   j >= max(m, 1)   status 1, NaN in R and t, zeros elsewhere (the "no candidate" row)
 * bp_cands_set_instance_poses: needs a pose solver (error otherwise; switching the solver off switches this off); drops
 * the graph; on: the frame graph ends in one more launch (bp_cands_kernel_count + 1); d_inst_poses NULL: the object's own
 * buffer.  bp_cands_instance_poses: device, NULL until switched on. */
int bp_cands_set_instance_poses(bp_cands* s, int on, double* d_inst_poses);
double* bp_cands_instance_poses(bp_cands* s);
/* the instance launch alone, on the outputs of bp_pose_from_candidate_records: d_merged [frames][C][152], d_info [frames][4],
 * d_poses [frames][166], d_kp3d device [50][3] -> d_inst_poses [frames][C][166]; frames <= 65535 */
int bp_pose_instances_from_merged(const float* d_merged, const int* d_info, const double* d_poses, int frames, int C,
                                  const double* d_kp3d, int n_kp, const double* K, int left_number, double* d_inst_poses,
                                  void* stream);

/* ---- host post-processing (no device work) ---- */
/* pnp (utils/utils.py:17-41): a restatement of cv2.solvePnP's default SOLVEPNP_ITERATIVE (planar / DLT initialisation,
 * CvLevMarq on (Rodrigues vector, t): <= 20 steps, FLT_EPSILON) followed by cv2.Rodrigues; f64.
 * pts3d [n][3], pts2d [n][2], K [9] row-major; outputs R [9] row-major, t [3].  n >= 6 (>= 4 for a planar model). */
int bp_solve_pnp(const double* pts3d, const double* pts2d, int n, const double* K, double* R, double* t);
/* ... a failed solve reported, not raised: *status = the solver's code (0 solved, -1 too few points, -2 degenerate; R and
 * t are then not to be read), the codes bp_solve_pnp_batch and the pose rows carry */
int bp_solve_pnp_status(const double* pts3d, const double* pts2d, int n, const double* K, double* R, double* t, int* status);
/* opt-in, NOT what the reference calls: Hartley-conditioned DLT + the same reprojection objective minimised to
 * convergence -- for callers who want the optimum where the raw-DLT start of SOLVEPNP_ITERATIVE lands in a wrong basin
 * (small distant objects).  n >= 6, non-planar. */
int bp_solve_pnp_refined(const double* pts3d, const double* pts2d, int n, const double* K, double* R, double* t);
/* the variant utils/utils.py:32-36 keeps commented out (cv2.solvePnPRansac, reprojectionError = 12): 6-point
 * hypotheses through the solver above, reproducible sampler; inliers [n] (nullable) receives the consensus mask. */
int bp_solve_pnp_ransac(const double* pts3d, const double* pts2d, int n, const double* K, double reproj_err,
                        int max_trials, double confidence, double* R, double* t, unsigned char* inliers);
/* pose_nms (pPose_nms.py:24-122), f32: bboxes [n][4], bbox_scores [n], preds [n][K][2], scores [n][K] -> returns m <= n
 * merged poses (or a negative status): pick [m] (candidate kept), pose [m][K][2] (the - 0.3 applied), score [m][K],
 * proposal score [m].  Output arrays sized for n. */
int bp_pose_nms(const float* bboxes, const float* bbox_scores, const float* preds, const float* scores, int n, int K,
                int* out_pick, float* out_pose, float* out_score, float* out_prop);

/* ---- Darknet-API-compatible detector (replaces the reference's CPU/CUDA Detector, train_YOLO/src/yolo_v2_class.cpp) ----
 * cfg WITH a [net] block (width == height); BatchNorm folded the Darknet-C way; detections as Detector::detect makes
 * them: candidates with objectness > thresh, prob = objectness * class probability, per-class NMS, boxes in image
 * pixels.  The six yolo_v2_class symbols themselves are declared in include/yolo_v2_class_compat.h. */
typedef struct bp_darknet bp_darknet;
typedef struct bp_bbox {
    unsigned int x, y, w, h;
    float prob;
    unsigned int obj_id, track_id, frames_counter;
} bp_bbox;
const char* bp_darknet_last_error(void);
int bp_darknet_create(const char* cfg_path, const char* weights_path, int device, bp_darknet** out);
void bp_darknet_destroy(bp_darknet* d);
int bp_darknet_width(const bp_darknet* d);
int bp_darknet_height(const bp_darknet* d);
int bp_darknet_classes(const bp_darknet* d);
/* planar_rgb: host [3][h][w] floats 0..1 (Darknet's `image`).  Returns the number of detections (the first `cap` are
 * written to out), < 0 on error. */
int bp_darknet_detect_rgb(bp_darknet* d, const float* planar_rgb, int w, int h, float thresh, float nms, bp_bbox* out,
                          int cap);
/* encoded image in memory: PNG, baseline JPEG or uncompressed BMP (what load_image / stb_image hands the reference's
 * Detector, image.c:1820-1875); bp_darknet_detect_png is the older name of the same entry point */
int bp_darknet_detect_image(bp_darknet* d, const unsigned char* data, size_t n, float thresh, float nms, bp_bbox* out,
                            int cap);
int bp_image_decode_rgb(const unsigned char* data, size_t n, unsigned char* out_rgb, size_t cap, int* h, int* w);
int bp_darknet_detect_png(bp_darknet* d, const unsigned char* png, size_t n, float thresh, float nms, bp_bbox* out,
                          int cap);
int bp_darknet_detect_file(bp_darknet* d, const char* png_path, float thresh, float nms, bp_bbox* out, int cap);
/* detector engine from a Darknet cfg/.weights pair with Darknet-C BatchNorm folding (used by bp_darknet_create) */
int bp_yolo_create_darknet(const char* cfg_path, const char* weights_path, int reso, int max_batch, int device,
                           bp_yolo** out);

/* ---- HIP streams confined to a subset of the CUs (one frame pipeline per XCD) ---- */
/* cu_mask: `words` x 32 bits, bit i = CU i of the device in the driver's numbering (on MI355X bit i lies on XCD i % 8,
 * checked by bp_probe_placement).  The stream is a plain hipStream_t (void*) usable with every call above. */
int bp_stream_create_masked(const uint32_t* cu_mask, int words, void** out_stream);
int bp_stream_destroy(void* stream);
/* launches `blocks` workgroups on `stream` and reports where each ran: h_xcc[b] = XCD id (0..7), h_hw_id[b] = raw
 * HW_ID register (may be NULL) */
int bp_probe_placement(int blocks, int* h_xcc, int* h_hw_id, void* stream);

/* ---- frame input (host; replaces cv2.imread on ImageLoader's thread, dataloader.py:150-179) ---- */
/* PNG -> cv2.imread(IMREAD_COLOR) convention: [h][w][3] u8 in B,G,R order; alpha dropped, grey replicated, palette
 * expanded, 16-bit samples reduced to the high byte.  Adam7-interlaced files are rejected. */
int bp_png_info(const unsigned char* data, size_t n, int* h, int* w, int* channels);
int bp_png_decode_bgr(const unsigned char* data, size_t n, unsigned char* out_bgr, size_t cap, int* h, int* w);
/* read-ahead loader: `threads` workers decode the PNG files `paths[0..n)` (each H x W) in list order into a ring of
 * `depth` host slots (pinned with hipHostMalloc when `pinned` and a GPU is present).
 * bp_loader_next: 0 = *bgr points at frame *index until bp_loader_release(*index); 1 = list exhausted;
 * <0 = that frame failed (bp_last_error(); it must still be released).  One consumer thread. */
typedef struct bp_loader bp_loader;
int bp_loader_create(const char* const* paths, int n, int H, int W, int threads, int depth, int pinned, bp_loader** out);
void bp_loader_destroy(bp_loader* l);
int bp_loader_next(bp_loader* l, long long* index, const unsigned char** bgr);
int bp_loader_release(bp_loader* l, long long index);
/* asynchronous host -> device copy on `stream` (h_src should be a loader slot or other pinned memory) */
int bp_upload(void* d_dst, const void* h_src, size_t bytes, void* stream);

/* ---- training-scene synthesiser (no reference counterpart) ----
 * Images are [I][H][W][3] uint8, H, W <= 32768 and H W <= 2^24.  Image i of a call is scene `first_image` + i of the
 * random source, a 32-bit mix keyed by (seed, stream, scene, pixel, channel): a scene's bytes do not depend on how the
 * scenes are split over calls.  All per-pixel arithmetic is integer or fixed point; every _host twin works on host
 * memory and gives the same bytes.  The per-image tables (`windows`, `params`) are HOST memory in both forms.  The
 * device forms are enqueued on `stream` and do not synchronise it. */
/* Procedural backgrounds: four octaves of lattice value noise (cells of 64, 32, 16, 8 px, bilinear in Q8) weighted,
 * scaled and added to a base colour, all drawn per scene. */
int bp_synth_background(int I, int H, int W, unsigned seed, unsigned first_image, unsigned char* d_out, void* stream);
int bp_synth_background_host(int I, int H, int W, unsigned seed, unsigned first_image, unsigned char* out);
/* Windows of a photograph bank d_bank [Nb][Hb][Wb][3] resampled to H x W, bilinear in fixed point, pixel centres
 * aligned; windows [I][6] int32 = (bank image, x0, y0, w, h, flip), each window inside its image. */
int bp_synth_windows(const unsigned char* d_bank, int Nb, int Hb, int Wb, const int* windows, int I, int H, int W,
                     unsigned char* d_out, void* stream);
int bp_synth_windows_host(const unsigned char* bank, int Nb, int Hb, int Wb, const int* windows, int I, int H, int W,
                          unsigned char* out);
/* The composite of a render (d_color, d_depth of bp_render_color) over a background through a camera model, per pixel
 * and channel: paste with an inside feather ((a F + (9 - a) B + 4) / 9, a = pixels with depth > 0 in the 3 x 3
 * neighbourhood clamped to the image; B where the centre has none), separable binomial blur of radius r (rows, then
 * columns, clamped edges, each pass rounded half up), gain (Q8) and offset, noise (Irwin-Hall of 12 bytes, times a Q8
 * sigma), clamp.  params [I][9] int32 = (feather 0/1, r 0..2, gain[3] 0..4096, offset[3] -255..255, sigma 0..16384).
 * The output must not be an input. */
int bp_synth_compose(const unsigned char* d_background, const unsigned char* d_color, const float* d_depth, int I, int H, int W,
                     const int* params, unsigned seed, unsigned first_image, unsigned char* d_out, void* stream);
int bp_synth_compose_host(const unsigned char* background, const unsigned char* color, const float* depth, int I, int H, int W,
                          const int* params, unsigned seed, unsigned first_image, unsigned char* out);
/* A depth sensor's image of a scene depth [I][H][W] f32 in metres: uint16 counts = depth / depth_scale rounded half up
 * (0 stays 0, at most 65 535), plus noise of sigma noise_k count^2 / 2^28 counts, and set to 0 with probability
 * hole_p / 256 where the counts of the 3 x 3 neighbourhood (clamped) span more than edge_counts.
 * params [I][3] int32 = (noise_k 0..65535, edge_counts >= 0, hole_p 0..256). */
int bp_synth_sensor_depth(const float* d_depth, int I, int H, int W, double depth_scale, const int* params, unsigned seed,
                          unsigned first_image, uint16_t* d_out, void* stream);
int bp_synth_sensor_depth_host(const float* depth, int I, int H, int W, double depth_scale, const int* params, unsigned seed,
                               unsigned first_image, uint16_t* out);
/* Instance ownership of scenes of J objects.  alone [J][I][H][W] f32: alone[j][i] is object j's depth
 * image rendered alone in scene i (bp_render_depth's, 0 where nothing was drawn).  Per pixel, among the objects with
 * present[i][j] != 0 and a depth > 0 the smallest depth wins, and among depths of exactly the same float32 bits the
 * HIGHEST j: bp_render_color's accumulation rule when the objects are drawn in ascending j.  ids [I][H][W] uint8 =
 * 1 + the winner (0: nothing drawn), depth [I][H][W] f32 = its depth (0).  stats [I][J][10] int32 = (px_all, px_visib,
 * full xmin, xmax, ymin, ymax, visible xmin, xmax, ymin, ymax): px_all counts the pixels with alone[j][i] > 0, px_visib
 * those with ids == j + 1; the boxes are inclusive and -1 four times when their count is 0.  An object that is not
 * present keeps its full count and box; its visible count is 0.  1 <= J <= 32, H W <= 2^24, I J < 2^28.  Integer
 * arithmetic after one float comparison per (pixel, object): host and device give the same bytes.  The device form
 * accumulates in d_stats itself (no workspace), is enqueued on `stream` and does not synchronise it; every byte of the
 * three outputs is written; d_depth must not be d_alone. */
int bp_synth_instances(const float* d_alone, int J, int I, int H, int W, const unsigned char* d_present, unsigned char* d_ids,
                       float* d_depth, int* d_stats, void* stream);
int bp_synth_instances_host(const float* alone, int J, int I, int H, int W, const unsigned char* present, unsigned char* ids,
                            float* depth, int* stats);

#ifdef __cplusplus
}
#endif
#endif /* BETAPOSE_HIP_H */
