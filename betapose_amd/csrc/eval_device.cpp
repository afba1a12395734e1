// The device drivers of the evaluation tools: what one call of the pose metrics, the rasterisers, VSD, the annotator and
// the depth refinement enqueues on device pointers -- the chunk-size rule, the workspaces, the launch sequence and the
// closing synchronize (a driver's workspaces live in a local arena).  Arguments have been checked by the caller
// (c_api_eval.cpp); the kernels are launched through the launchers of pose_tail.h, raster.h, annotate.h and icp.h.
#include <algorithm>

#include "annotate.h"
#include "kpd_sample.h"
#include "designate.h"
#include "engine.h"
#include "icp.h"
#include "pose_tail.h"
#include "raster.h"
#include "yolo_map.h"
#include "yolo_train.h"

namespace bp {

constexpr size_t RASTER_WS_BYTES = (size_t)256 << 20;      // what the chunked calls keep their workspaces under

namespace {
// The chunk-size rule: items per pass of `count` items whose workspace takes bytes_per_item each -- as many as keep it
// under RASTER_WS_BYTES (or `asked`, a caller's own chunk, where that is not 0), at least 1, at most count
size_t chunk_items(size_t bytes_per_item, size_t count, size_t asked = 0) {
    return std::max<size_t>(1, std::min(asked ? asked : RASTER_WS_BYTES / bytes_per_item, count));
}

// the call's image_index [P] on the device, NULL for NULL (pose p -> image p)
int* upload_image_index(Arena& a, const int* image_index, int P, hipStream_t s) {
    if (!image_index) return nullptr;
    int* d_index = (int*)a.alloc_bytes((size_t)P * sizeof(int));
    BP_HIP(hipMemcpyAsync(d_index, image_index, (size_t)P * sizeof(int), hipMemcpyHostToDevice, s));
    return d_index;
}

// The renders of one chunk of poses: `slots` z-buffers, posed meshes and skipped counters (zeroed here; nobody reads them)
struct RasterChunk {
    size_t HW;
    uint32_t* zbuf;
    void* ws;
    int* skipped;
    RasterChunk(Arena& a, int n, size_t slots, size_t HW, hipStream_t s)
        : HW(HW), zbuf((uint32_t*)a.alloc_bytes(slots * HW * sizeof(uint32_t))), ws(a.alloc_bytes(raster_vertex_bytes(n, (int)slots))),
          skipped((int*)a.alloc_bytes(slots * sizeof(int))) {
        BP_HIP(hipMemsetAsync(skipped, 0, slots * sizeof(int), s));
    }
    // zbuf [(na + nb)][H][W] <- +inf, then poses_a[0 .. na) and poses_b[0 .. nb) drawn into it (launch_raster)
    void draw(const double* model, int n, const int* faces, int F, const double* poses_a, int na, const double* poses_b, int nb,
              const RsCam& cam, int H, int W, hipStream_t s) {
        BP_HIP(hipMemsetD32Async((hipDeviceptr_t)zbuf, 0x7f800000, (size_t)(na + nb) * HW, s));   // +inf
        launch_raster(model, n, faces, F, poses_a, na, poses_b, nb, cam, H, W, ws, zbuf, skipped, s);
    }
};
}  // namespace

// ------------------------------------------------------------------ pose metrics
void pose_errors(const double* d_model, int n, const double* d_gt, const double* d_est, int P, const double* K, int want,
                 double* d_out, hipStream_t s) {
    Arena a;
    double* partial = (double*)a.alloc_bytes((size_t)P * pose_error_blocks(n) * 3 * sizeof(double));
    launch_pose_errors(d_model, n, d_gt, d_est, P, K, want, partial, d_out, s);
    BP_HIP(hipGetLastError());
    BP_HIP(hipStreamSynchronize(s));   // partials live in a local arena
}

void pose_errors_sym(const double* d_model, int n, const double* d_gt, const double* d_est, int P, const double* d_sym, int S,
                     const double* K, int want, double* d_out, hipStream_t s) {
    Arena a;
    double* scratch = (double*)a.alloc_bytes(pose_errors_sym_scratch_bytes(n, P, S));
    launch_pose_errors_sym(d_model, n, d_gt, d_est, P, d_sym, S, K, want, scratch, d_out, s);
    BP_HIP(hipGetLastError());
    BP_HIP(hipStreamSynchronize(s));   // the per-symmetry maxima live in a local arena
}

// ------------------------------------------------------------------ depth and colour rasterisers
void render_depth(const double* d_poses, int P, const double* d_model, int n, const int* d_faces, int F, const double* K, int H,
                  int W, double pixel_center, double near_z, float* d_depth, int* d_skipped, hipStream_t s) {
    const size_t HW = (size_t)H * W;
    const size_t chunk = chunk_items(raster_vertex_bytes(n, 1), (size_t)P);
    const RsCam cam = raster_cam(K, pixel_center, near_z);
    Arena a;
    void* ws = a.alloc_bytes(raster_vertex_bytes(n, (int)chunk));
    BP_HIP(hipMemsetD32Async((hipDeviceptr_t)d_depth, 0x7f800000, (size_t)P * HW, s));   // +inf
    BP_HIP(hipMemsetAsync(d_skipped, 0, (size_t)P * sizeof(int), s));
    for (size_t p0 = 0; p0 < (size_t)P; p0 += chunk) {
        const int c = (int)std::min(chunk, (size_t)P - p0);
        launch_raster(d_model, n, d_faces, F, d_poses + p0 * 12, c, nullptr, 0, cam, H, W, ws, (uint32_t*)d_depth + p0 * HW,
                      d_skipped + p0, s);
    }
    launch_raster_finish((uint32_t*)d_depth, (size_t)P * HW, s);
    BP_HIP(hipGetLastError());
    BP_HIP(hipStreamSynchronize(s));   // the vertex workspace lives in a local arena
}

// poses [*p0, return) of the call go to images [i0, i1); *p0 on entry: the first pose not yet consumed
static int raster_pose_range(const int* image_index, int P, int i1, int p0) {
    if (!image_index) return std::min(P, i1);
    int p = p0;
    while (p < P && image_index[p] < i1) ++p;
    return p;
}

void render_color(const double* d_poses, int P, const double* d_model, int n, const int* d_faces, int F,
                  const unsigned char* d_colors, const int* image_index, int I, const double* K, int H, int W,
                  double pixel_center, double near_z, double ambient, const double* light, int accumulate,
                  unsigned char* d_color, float* d_depth, int* d_skipped, hipStream_t s, const ColorTexture* tex) {
    const size_t HW = (size_t)H * W;
    // images in flight: 8 bytes of key per pixel; poses in flight: their vertex workspace; each under RASTER_WS_BYTES
    const size_t ichunk = chunk_items(HW * 8, (size_t)I), pchunk = chunk_items(raster_vertex_bytes(n, 1), (size_t)P);
    const RsCam cam = raster_cam(K, pixel_center, near_z);
    Arena a;
    unsigned long long* keys = (unsigned long long*)a.alloc_bytes(ichunk * HW * 8);
    void* ws = a.alloc_bytes(raster_vertex_bytes(n, (int)pchunk));
    int* d_index = upload_image_index(a, image_index, P, s);
    BP_HIP(hipMemsetAsync(d_skipped, 0, (size_t)P * sizeof(int), s));
    const ColorLight lt{ambient, light[0], light[1], light[2]};
    int p0 = 0;
    for (size_t i0 = 0; i0 < (size_t)I; i0 += ichunk) {
        const int m = (int)std::min(ichunk, (size_t)I - i0);
        const int p1 = raster_pose_range(image_index, P, (int)i0 + m, p0);
        launch_color_clear(keys, d_depth + i0 * HW, accumulate, (size_t)m * HW, s);
        for (int q0 = p0; q0 < p1; q0 += (int)pchunk) {
            const int c = std::min((int)pchunk, p1 - q0);
            launch_raster_transform(d_model, n, d_poses + (size_t)q0 * 12, c, nullptr, 0, cam, ws, s);
            launch_color_visibility(d_faces, F, n, ws, q0, c, d_index, (int)i0, cam, H, W, keys, d_skipped, s);
        }
        if (tex)
            launch_color_resolve_tex(keys, m, d_model, d_faces, F, *tex, d_poses, cam, H, W, lt, d_color + i0 * HW * 3,
                                     d_depth + i0 * HW, s);
        else
            launch_color_resolve(keys, m, d_model, d_faces, F, d_colors, d_poses, cam, H, W, lt, d_color + i0 * HW * 3,
                                 d_depth + i0 * HW, s);
        p0 = p1;
    }
    BP_HIP(hipGetLastError());
    BP_HIP(hipStreamSynchronize(s));   // the keys and the vertex workspace live in a local arena
}

void draw_boxes(const double* d_poses, int P, const double* d_corners, const unsigned char* d_corner_colors,
                const int* image_index, int I, const double* K, int H, int W, double pixel_center, double near_z,
                unsigned char* d_color, hipStream_t s) {
    const size_t HW = (size_t)H * W;
    const size_t ichunk = chunk_items(HW * 4, (size_t)I);
    const RsCam cam = raster_cam(K, pixel_center, near_z);
    Arena a;
    uint32_t* ids = (uint32_t*)a.alloc_bytes(ichunk * HW * 4);
    int* d_index = upload_image_index(a, image_index, P, s);
    int p0 = 0;
    for (size_t i0 = 0; i0 < (size_t)I; i0 += ichunk) {
        const int m = (int)std::min(ichunk, (size_t)I - i0);
        const int p1 = raster_pose_range(image_index, P, (int)i0 + m, p0);
        if (p1 > p0)
            launch_draw_boxes(d_poses, p0, p1 - p0, d_corners, d_corner_colors, d_index, (int)i0, m, cam, H, W, ids,
                              d_color + i0 * HW * 3, s);
        p0 = p1;
    }
    BP_HIP(hipGetLastError());
    BP_HIP(hipStreamSynchronize(s));   // the id planes live in a local arena
}

void overlay(const unsigned char* d_frames, const unsigned char* d_color, const float* d_depth, int I, int H, int W, int alpha,
             unsigned char* d_out, hipStream_t s) {
    launch_overlay(d_frames, d_color, d_depth, (size_t)I * H * W, alpha, d_out, s);
    BP_HIP(hipGetLastError());
}

// ------------------------------------------------------------------ VSD
void vsd_errors(const double* d_model, int n, const int* d_faces, int F, const double* d_gt, const double* d_est, int P,
                const double* K, const uint16_t* d_depth_test, int T, int H, int W, double depth_scale, const int* d_test_index,
                double delta, const double* taus, int n_tau, double diameter, double pixel_center, double near_z, int chunk,
                double* d_err, int* d_counts, hipStream_t s) {
    const size_t HW = (size_t)H * W;
    // without a chunk of the caller's, both workspaces (2 c z-buffers, 2 c posed meshes) stay under RASTER_WS_BYTES:
    // the larger of the two per-pair sizes decides (the smaller of the two quotients, taken before the clamp)
    const size_t c = chunk_items(std::max(2 * HW * sizeof(float), raster_vertex_bytes(n, 2)), (size_t)P, (size_t)chunk);
    const RsCam cam = raster_cam(K, pixel_center, near_z);
    VsdTaus tv{};
    for (int k = 0; k < n_tau; ++k) tv.tau[k] = taus[k];
    Arena a;
    RasterChunk r(a, n, 2 * c, HW, s);
    int* acc = (int*)a.alloc_bytes((size_t)P * VSD_ACC * sizeof(int));
    BP_HIP(hipMemsetAsync(acc, 0, (size_t)P * VSD_ACC * sizeof(int), s));
    for (size_t p0 = 0; p0 < (size_t)P; p0 += c) {
        const int m = (int)std::min(c, (size_t)P - p0);
        r.draw(d_model, n, d_faces, F, d_gt + p0 * 12, m, d_est + p0 * 12, m, cam, H, W, s);
        launch_vsd_reduce(r.zbuf, m, d_depth_test, T, d_test_index + p0, H, W, K, pixel_center, depth_scale, delta, tv, n_tau,
                          diameter, acc + p0 * VSD_ACC, s);
    }
    launch_vsd_finish(acc, d_test_index, T, P, n_tau, d_err, d_counts, s);
    BP_HIP(hipGetLastError());
    BP_HIP(hipStreamSynchronize(s));   // the renders live in a local arena
}

// ------------------------------------------------------------------ the key-point annotator
void annotate_keypoints(const double* d_poses, int P, const double* d_kp, int Kp, const double* K, int H, int W,
                        double pixel_center, double near_z, const float* d_model_depth, const float* d_scene_depth,
                        const int* d_scene_index, double self_tol, double delta, double* d_xy, double* d_z,
                        unsigned char* d_flags, hipStream_t s) {
    launch_annotate_keypoints(d_poses, P, d_kp, Kp, K, H, W, pixel_center, near_z, d_model_depth, d_scene_depth,
                              d_scene_index, self_tol, delta, d_xy, d_z, d_flags, s);
    BP_HIP(hipGetLastError());
}

void mask_boxes(const float* d_depth, int P, int H, int W, const double* K, double pixel_center, const float* d_scene_depth,
                const int* d_scene_index, double delta, int* d_boxes, int* d_counts, hipStream_t s) {
    Arena a;
    int* acc = (int*)a.alloc_bytes((size_t)P * 2 * ANNOT_BOX_INTS * sizeof(int));
    launch_mask_boxes(d_depth, P, H, W, K, pixel_center, d_scene_depth, d_scene_index, delta, acc, d_boxes, d_counts, s);
    BP_HIP(hipGetLastError());
    BP_HIP(hipStreamSynchronize(s));   // the accumulators live in a local arena
}

void vertex_boxes(const double* d_poses, int P, const double* d_vertices, int n, const double* K, int H, int W, int* d_boxes,
                  hipStream_t s) {
    Arena a;
    int* acc = (int*)a.alloc_bytes((size_t)P * ANNOT_BOX_INTS * sizeof(int));
    launch_vertex_boxes(d_poses, P, d_vertices, n, K, H, W, acc, d_boxes, s);
    BP_HIP(hipGetLastError());
    BP_HIP(hipStreamSynchronize(s));   // the accumulators live in a local arena
}

void kpd_targets(const double* d_parts, const float* d_ul, const float* d_br, int B, int Kp, int inpH, int inpW, int resH,
                 int resW, const float* d_g, int size, float* d_out, int* d_centres, float* d_set_mask, hipStream_t s) {
    launch_kpd_targets(d_parts, d_ul, d_br, B, Kp, inpH, inpW, resH, resW, d_g, size, d_out, d_centres, d_set_mask, s);
    BP_HIP(hipGetLastError());
}

// ------------------------------------------------------------------ KPD training samples
void kpd_inputs(const unsigned char* d_frames, int N, int H, int W, const int* d_frame_index, const float* d_ul, const float* d_br,
                const float* d_gains, const unsigned char* d_blank, int B, int inpH, int inpW, float* d_inp, hipStream_t s) {
    launch_kpd_inputs(d_frames, N, H, W, d_frame_index, d_ul, d_br, d_gains, d_blank, B, inpH, inpW, d_inp, s);
    BP_HIP(hipGetLastError());
}

void kpd_augment(const float* d_x, int B, int C, int H, int W, const unsigned char* d_flip, const double* d_cs, const int* d_perm,
                 float* d_y, hipStream_t s) {
    launch_kpd_augment(d_x, B, C, H, W, d_flip, d_cs, d_perm, d_y, s);
    BP_HIP(hipGetLastError());
}

void heatmap_loss_acc(const float* d_out, const float* d_labels, const float* d_set_mask, int B, int K, int H, int W,
                      double* d_partial, double* d_loss, float* d_acc, int* d_preds, int* d_gt, float* d_dists, float* d_grad,
                      hipStream_t s) {
    launch_heatmap_loss_acc(d_out, d_labels, d_set_mask, B, K, H, W, d_partial, d_loss, d_acc, d_preds, d_gt, d_dists, d_grad, s);
    BP_HIP(hipGetLastError());
}

// ------------------------------------------------------------------ detector training
void yolo_inputs(const unsigned char* d_frames, int N, int H, int W, const int* d_frame_index, const int* d_crop,
                 const unsigned char* d_flip, const float* d_hsv, int B, int net_h, int net_w, float* d_out, hipStream_t s) {
    launch_yolo_inputs(d_frames, N, H, W, d_frame_index, d_crop, d_flip, d_hsv, B, net_h, net_w, d_out, s);
    BP_HIP(hipGetLastError());
}

void yolo_truth(const float* d_labels, int M, const int* d_first, const int* d_swap, const float* d_geom,
                const unsigned char* d_flip, int B, int classes, int max_boxes, int net_w, int net_h, int small_object,
                int* d_order, float* d_truth, int* d_kept, hipStream_t s) {
    launch_yolo_truth(d_labels, M, d_first, d_swap, d_geom, d_flip, B, classes, max_boxes, net_w, net_h, small_object, d_order,
                      d_truth, d_kept, s);
    BP_HIP(hipGetLastError());
}

void yolo_loss(const float* d_x, int B, int n, int classes, int h, int w, int net_w, int net_h, const float* d_anchors, int total,
               const int* d_mask, const float* d_truth, int max_boxes, float ignore_thresh, float truth_thresh, float* d_act,
               float* d_delta, double* d_cost, double* d_stats, double* d_partial, hipStream_t s) {
    launch_yolo_loss(d_x, B, n, classes, h, w, net_w, net_h, d_anchors, total, d_mask, d_truth, max_boxes, ignore_thresh,
                     truth_thresh, d_act, d_delta, d_cost, d_stats, d_partial, s);
    BP_HIP(hipGetLastError());
}

// ------------------------------------------------------------------ detector validation
void yolo_detections(const float* d_pred, int B, int rows, const int* heads, int nheads, int net_w, int net_h, int classes,
                     float thresh, float nms, int max_dets, float* d_dets, int* d_count, void* d_scratch, hipStream_t s) {
    launch_yolo_detections(d_pred, B, rows, heads, nheads, net_w, net_h, classes, thresh, nms, max_dets, d_dets, d_count, d_scratch, s);
    BP_HIP(hipGetLastError());
}

void map_match(const float* d_dets, const int* d_count, int B, int max_dets, int classes, const float* d_labels, int M,
               const int* d_first, float iou_thresh, float thresh_calc, int truth_base, int image_base, int rec_stride, float* d_rec,
               int* d_rec_count, int* d_truth_classes_count, double* d_img_stats, int* d_claim, hipStream_t s) {
    launch_map_match(d_dets, d_count, B, max_dets, classes, d_labels, M, d_first, iou_thresh, thresh_calc, truth_base, image_base,
                     rec_stride, d_rec, d_rec_count, d_truth_classes_count, d_img_stats, d_claim, s);
    BP_HIP(hipGetLastError());
}

void map_reduce(const float* d_rec, int D, const int* d_truth_classes_count, int classes, int truths, const double* d_img_stats,
                int N, double* d_ap, double* d_stats, double* d_pr, void* d_scratch, hipStream_t s) {
    launch_map_reduce(d_rec, D, d_truth_classes_count, classes, truths, d_img_stats, N, d_ap, d_stats, d_pr, d_scratch, s);
    BP_HIP(hipGetLastError());
}

// ------------------------------------------------------------------ the key-point designator
void sift_octave(const double* d_points, int n, int field, const double* scales, int ns, int k, double min_contrast,
                 double* d_dog, signed char* d_flags, hipStream_t s) {
    launch_sift_octave(d_points, n, field, scales, ns, k, min_contrast, d_dog, d_flags, s);
    BP_HIP(hipGetLastError());
}

void farthest_points(const double* d_points, int n, int K, int start, int* d_idx, double* d_d2, hipStream_t s) {
    Arena a;
    double* mind = (double*)a.alloc_bytes((size_t)n * sizeof(double));
    launch_farthest_points(d_points, n, K, start, mind, d_idx, d_d2, s);
    BP_HIP(hipGetLastError());
    BP_HIP(hipStreamSynchronize(s));   // the minimum distances live in a local arena
}

void thin_points(const double* d_points, int n, int keep, unsigned char* d_alive, int* d_state, hipStream_t s) {
    Arena a;
    double* nn_d = (double*)a.alloc_bytes((size_t)n * sizeof(double));
    int* nn_j = (int*)a.alloc_bytes((size_t)n * sizeof(int));
    int* list = (int*)a.alloc_bytes((size_t)n * sizeof(int));
    launch_thin_points(d_points, n, keep, nn_d, nn_j, list, d_alive, d_state, s);
    BP_HIP(hipGetLastError());
    BP_HIP(hipStreamSynchronize(s));   // the neighbour table lives in a local arena
}

// ------------------------------------------------------------------ depth refinement (ICP)
// poses per chunk of the device calls: without a chunk of the caller's, the z-buffers and the posed meshes of a chunk
// each stay under RASTER_WS_BYTES (the larger of the two per-pose sizes decides)
static size_t icp_chunk(int chunk, int n, int P, size_t HW) {
    return chunk_items(std::max(HW * sizeof(float), raster_vertex_bytes(n, 1)), (size_t)P, (size_t)chunk);
}

void icp_normal_equations(const double* d_poses, int P, const double* d_model, int n, const int* d_faces, int F, const double* K,
                          const uint16_t* d_depth_test, int T, const int* d_test_index, int H, int W, const IcpParams& prm,
                          double near_z, int chunk, double* d_out, hipStream_t s) {
    const size_t HW = (size_t)H * W, c = icp_chunk(chunk, n, P, HW);
    const int slices = icp_slices(H, W);
    const RsCam cam = raster_cam(K, prm.c, near_z);
    Arena a;
    RasterChunk r(a, n, c, HW, s);
    double* partial = (double*)a.alloc_bytes(c * slices * ICP_ACC * sizeof(double));
    for (size_t p0 = 0; p0 < (size_t)P; p0 += c) {
        const int m = (int)std::min(c, (size_t)P - p0);
        r.draw(d_model, n, d_faces, F, d_poses + p0 * 12, m, nullptr, 0, cam, H, W, s);
        launch_icp_accumulate(r.zbuf, d_poses + p0 * 12, m, d_depth_test, T, d_test_index + p0, H, W, prm, nullptr, partial, s);
        launch_icp_sum(partial, d_test_index + p0, T, m, slices, d_out + p0 * ICP_ACC, s);
    }
    BP_HIP(hipGetLastError());
    BP_HIP(hipStreamSynchronize(s));   // the renders and partial sums live in a local arena
}

void refine_depth(const double* d_poses, int P, const double* d_model, int n, const int* d_faces, int F, const double* K,
                  const uint16_t* d_depth_test, int T, const int* d_test_index, int H, int W, const IcpParams& prm, double near_z,
                  int chunk, double* d_poses_out, double* d_stats, hipStream_t s) {
    const size_t HW = (size_t)H * W, c = icp_chunk(chunk, n, P, HW);
    const int slices = icp_slices(H, W);
    const RsCam cam = raster_cam(K, prm.c, near_z);
    Arena a;
    RasterChunk r(a, n, c, HW, s);
    double* partial = (double*)a.alloc_bytes(c * slices * ICP_ACC * sizeof(double));
    launch_icp_init(d_poses, d_test_index, T, P, d_poses_out, d_stats, s);
    for (size_t p0 = 0; p0 < (size_t)P; p0 += c) {
        const int m = (int)std::min(c, (size_t)P - p0);
        double* pose = d_poses_out + p0 * 12;
        double* stats = d_stats + p0 * ICP_STATS;
        // the whole loop is enqueued: no host round trip between the iterations
        for (int k = 0; k <= prm.iterations; ++k) {
            r.draw(d_model, n, d_faces, F, pose, m, nullptr, 0, cam, H, W, s);
            launch_icp_accumulate(r.zbuf, pose, m, d_depth_test, T, d_test_index + p0, H, W, prm, stats, partial, s);
            launch_icp_step(partial, m, slices, k, prm, d_poses + p0 * 12, pose, stats, s);
        }
    }
    BP_HIP(hipGetLastError());
    BP_HIP(hipStreamSynchronize(s));   // the renders and partial sums live in a local arena
}

}  // namespace bp
