// extern "C" boundary, the evaluation tools: pose metrics, depth and colour rasterisers, boxes, overlay, VSD, the key-point
// annotator and the depth refinement, host and device -- see include/betapose_hip.h.  Every function checks its
// arguments and makes one bp:: call: the host twin (*_host.cpp) or the device driver (eval_device.cpp).  What a host /
// device pair checks alike is stated once, in the check functions.
#include <vector>

#include "annotate.h"
#include "c_api_util.h"
#include "designate.h"
#include "icp.h"
#include "kpd_sample.h"
#include "pose_tail.h"
#include "raster.h"
#include "verify.h"
#include "yolo_map.h"
#include "yolo_train.h"

static void check_pixels(int H, int W) { BP_CHECK((long long)H * W <= (1ll << 24), "H * W must not exceed 2^24"); }

// what the rasteriser calls check alike
static void raster_check_sizes(int n, int F, int P, int H, int W, double near_z) {
    BP_CHECK(n > 0 && F > 0 && P > 0 && H > 0 && W > 0, "n, F, P, H and W must be positive");
    check_pixels(H, W);
    BP_CHECK(near_z > 0.0, "near must be positive");
}

// what the colour renderer's calls check of image_index (host, may be NULL): pose p -> image p needs I == P, otherwise
// non-decreasing values in [0, I), which lets a call split its work into pose ranges without splitting an image
static void raster_check_image_index(const int* image_index, int P, int I) {
    BP_CHECK(I > 0, "I must be positive");
    if (!image_index) {
        BP_CHECK(I == P, "without image_index the call needs I == P");
        return;
    }
    for (int p = 0; p < P; ++p) {
        BP_CHECK(image_index[p] >= 0 && image_index[p] < I, "image_index must lie in [0, I)");
        BP_CHECK(p == 0 || image_index[p] >= image_index[p - 1], "image_index must be non-decreasing");
    }
}

static void raster_check_color(int n, int F, int P, int H, int W, double near_z, const int* image_index, int I) {
    raster_check_sizes(n, F, P, H, W, near_z);
    raster_check_image_index(image_index, P, I);
    BP_CHECK((unsigned long long)P * (unsigned long long)F <= bp::COLOR_MAX_IDS, "P * F must not exceed 2^32 - 2");
}

// what the texture calls check alike: the size limit, and `levels` against the size
static void raster_check_texture(int Wt, int Ht, int levels) {
    BP_CHECK(Wt > 0 && Ht > 0, "Wt and Ht must be positive");
    BP_CHECK(Wt <= bp::texture_max_size() && Ht <= bp::texture_max_size(), "a texture must not exceed 8192 x 8192");
    BP_CHECK(levels >= 1 && levels <= bp::texture_full_levels(Wt, Ht), "levels must lie in 1 .. 1 + ceil(log2(max(Wt, Ht)))");
}

static void raster_check_boxes(int P, int I, int H, int W, double near_z) {
    BP_CHECK(P > 0 && I > 0 && H > 0 && W > 0, "P, I, H and W must be positive");
    check_pixels(H, W);
    BP_CHECK(P <= (1 << 24), "P must not exceed 2^24");
    BP_CHECK(near_z > 0.0, "near must be positive");
}

static void raster_check_overlay(int I, int H, int W, int alpha) {
    BP_CHECK(I > 0 && H > 0 && W > 0, "I, H and W must be positive");
    check_pixels(H, W);
    BP_CHECK(alpha >= 0 && alpha <= 256, "alpha must lie in 0 .. 256");
}

// ---- the key-point annotator (annotate.hip / annotate_host.cpp)
static void annot_check_image(int P, int H, int W) {
    BP_CHECK(P > 0 && H > 0 && W > 0, "P, H and W must be positive");
    check_pixels(H, W);
}
static void annot_check_keypoints(int P, int H, int W, int Kp, double near_z) {
    annot_check_image(P, H, W);
    BP_CHECK(Kp > 0 && (long long)P * Kp < (1ll << 31), "Kp must be positive and P * Kp below 2^31");
    BP_CHECK(near_z > 0.0, "near must be positive");
}
// scene depth and scene index come together; every index (host copy) must name one of the T images
static void annot_check_scene(const void* scene_depth, const void* scene_index, const int* host_index, int P, int T) {
    BP_CHECK((scene_depth != nullptr) == (scene_index != nullptr), "scene_depth and scene_index are given together");
    if (!scene_depth) return;
    BP_CHECK(T > 0, "T must be positive");
    for (int p = 0; p < P; ++p) BP_CHECK(host_index[p] >= 0 && host_index[p] < T, "a scene index lies outside [0, T)");
}
// the device calls read the index back to check it before any kernel uses it
static void annot_check_scene_device(const float* d_scene_depth, const int* d_scene_index, int P, int T, hipStream_t s) {
    std::vector<int> idx;
    if (d_scene_depth && d_scene_index) {
        idx.resize(P);
        BP_HIP(hipMemcpyAsync(idx.data(), d_scene_index, (size_t)P * sizeof(int), hipMemcpyDeviceToHost, s));
        BP_HIP(hipStreamSynchronize(s));
    }
    annot_check_scene(d_scene_depth, d_scene_index, idx.data(), P, T);
}

static void annot_check_targets(int B, int Kp, int inpH, int inpW, int resH, int resW, int size) {
    BP_CHECK(B > 0 && Kp > 0 && inpH > 0 && inpW > 0 && resH > 0 && resW > 0, "B, Kp and the resolutions must be positive");
    BP_CHECK(size >= 1 && size % 2 == 1 && size <= 1025, "the Gaussian table needs an odd size of at most 1025");
    // (the kernel indexes rows in groups of four floats: the width counts rounded up to a multiple of 4)
    BP_CHECK((long long)B * Kp * resH * ((resW + 3) / 4 * 4) < (1ll << 31), "the target tensor must hold fewer than 2^31 values");
}

// ---- KPD training samples (kpd_sample.hip / kpd_sample_host.cpp).  The kernels index rows in groups of four floats: a
// width counts rounded up to a multiple of 4.
static void sample_check_inputs(int N, int H, int W, int B, int inpH, int inpW) {
    BP_CHECK(N > 0 && H > 0 && W > 0 && B > 0 && inpH > 0 && inpW > 0, "N, H, W, B and the input resolution must be positive");
    check_pixels(H, W);
    BP_CHECK((long long)B * 3 * inpH * ((inpW + 3) / 4 * 4) < (1ll << 31), "the input tensor must hold fewer than 2^31 values");
}
static void sample_check_maps(int B, int C, int H, int W) {
    BP_CHECK(B > 0 && C > 0 && H > 0 && W > 0, "B, C, H and W must be positive");
    check_pixels(H, W);
    BP_CHECK((long long)B * C * H * ((W + 3) / 4 * 4) < (1ll << 31), "the map tensor must hold fewer than 2^31 values");
}

// ---- detector training (yolo_train.hip / yolo_train_host.cpp)
static void yolo_check_inputs(int N, int H, int W, int B, int net_h, int net_w) {
    BP_CHECK(N > 0 && H > 0 && W > 0 && B > 0, "N, H, W and B must be positive");
    BP_CHECK(net_h >= 2 && net_w >= 2, "net_h and net_w must be at least 2");
    check_pixels(H, W);
    BP_CHECK((long long)B * 3 * net_h * ((net_w + 3) / 4 * 4) < (1ll << 31), "the input tensor must hold fewer than 2^31 values");
}
// crop [B][4] (host copy): the resize needs two source columns and rows; the bounds keep every index an int
static void yolo_check_crop(const int* crop, int B) {
    for (int b = 0; b < B; ++b) {
        const int* c = crop + (size_t)b * 4;
        BP_CHECK(c[2] >= 2 && c[3] >= 2, "swidth and sheight must be at least 2");
        BP_CHECK(c[0] > -(1 << 24) && c[0] < (1 << 24) && c[1] > -(1 << 24) && c[1] < (1 << 24) && c[2] < (1 << 24) &&
                     c[3] < (1 << 24), "pleft, ptop, swidth and sheight must lie below 2^24 in magnitude");
    }
}
static void yolo_check_truth(int M, int B, int classes, int max_boxes, int net_w, int net_h) {
    BP_CHECK(M >= 0 && B > 0 && classes > 0 && max_boxes > 0 && net_w > 0 && net_h > 0,
             "B, classes, max_boxes, net_w and net_h must be positive, M not negative");
    BP_CHECK((long long)B * max_boxes * 5 < (1ll << 31), "the truth tensor must hold fewer than 2^31 values");
}
static void yolo_check_loss(int B, int n, int classes, int h, int w, int net_w, int net_h, int total, int max_boxes, int channels,
                            int focal_loss) {
    BP_CHECK(focal_loss == 0, "focal_loss is not supported");
    BP_CHECK(B > 0 && n > 0 && classes > 0 && h > 0 && w > 0 && net_w > 0 && net_h > 0 && total > 0 && max_boxes > 0,
             "B, n, classes, h, w, net_w, net_h, total and max_boxes must be positive");
    BP_CHECK(n <= total && classes <= (1 << 16), "n must not exceed total, classes not 65536");
    BP_CHECK(channels == n * (5 + classes), "the head's channel count must be n * (5 + classes)");
    check_pixels(h, w);
    BP_CHECK((long long)B * n * (5 + classes) * h * w < (1ll << 31), "the head's output must hold fewer than 2^31 values");
}
static void yolo_check_mask(const int* mask, int n, int total) {
    for (int i = 0; i < n; ++i) BP_CHECK(mask[i] >= 0 && mask[i] < total, "a mask entry lies outside [0, total)");
}

// ---- detector validation (yolo_map.hip / yolo_map_host.cpp)
static void map_check_detections(int B, int rows, int attrs, const int* heads, int nheads, int net_w, int net_h, int classes,
                                 float thresh, int max_dets, bool device) {
    BP_CHECK(B > 0 && rows > 0 && net_w > 0 && net_h > 0 && classes > 0 && max_dets > 0,
             "B, rows, net_w, net_h, classes and max_dets must be positive");
    BP_CHECK(classes <= (1 << 12) && attrs == 5 + classes, "attrs must be 5 + classes, classes at most 4096");
    BP_CHECK(thresh >= 0.0f, "thresh must not be negative");
    BP_CHECK(!device || max_dets <= bp::yolo_map_max_dets(), "max_dets exceeds the device's cap");
    BP_CHECK(nheads > 0 && nheads <= bp::yolo_map_max_heads(), "between 1 and 8 heads");
    long long at = 0;
    for (int h = 0; h < nheads; ++h) {
        const int* q = heads + h * 4;
        BP_CHECK(q[1] > 0 && q[2] > 0 && q[3] > 0 && q[2] <= (1 << 12) && q[3] <= (1 << 12) && q[1] <= (1 << 6),
                 "a head needs positive anchors, gh and gw");
        BP_CHECK(q[0] == at, "the heads must follow each other from row 0");
        at += (long long)q[1] * q[2] * q[3];
        BP_CHECK(at <= rows, "the heads hold more rows than pred");
    }
    BP_CHECK(at == rows, "the heads must cover every row of pred");
    BP_CHECK((long long)B * rows * attrs < (1ll << 31), "pred must hold fewer than 2^31 values");
    BP_CHECK((long long)B * max_dets * (6 + classes) < (1ll << 31), "the detection rows must hold fewer than 2^31 values");
}
static void map_check_match(int B, int max_dets, int classes, int M, int rec_stride, int truth_base, int image_base) {
    BP_CHECK(B > 0 && max_dets > 0 && classes > 0 && classes <= (1 << 12) && M >= 0 && rec_stride > 0,
             "B, max_dets, classes and rec_stride must be positive, M not negative");
    BP_CHECK((long long)max_dets * classes * 6 < (1ll << 31) && (long long)B * max_dets * (6 + classes) < (1ll << 31) &&
                 (long long)B * rec_stride * 6 < (1ll << 31), "the detection rows and records must hold fewer than 2^31 values");
    BP_CHECK(truth_base >= 0 && image_base >= 0 && (long long)truth_base + M < (1ll << 31) && (long long)image_base + B < (1ll << 31),
             "truth_base and image_base must stay below 2^31");
}
static void map_check_reduce(int D, int classes, int truths, int N) {
    BP_CHECK(D >= 0 && D <= (1 << 26) && classes > 0 && classes <= (1 << 12) && truths >= 0 && N >= 0,
             "D within [0, 2^26], classes positive, truths and N not negative");
    BP_CHECK((long long)classes * (D > 0 ? D : 1) * 2 < (1ll << 40), "the PR arrays are too large");
}

// what the four refinement calls check alike, and the parameter block they hand on
static bp::IcpParams icp_params(const double* K, int T, double depth_scale, int iterations, double max_dist, double min_cos,
                                int min_pixels, double pixel_center) {
    BP_CHECK(T > 0, "T must be positive");
    BP_CHECK(depth_scale > 0.0 && max_dist > 0.0, "depth_scale and max_dist must be positive");
    BP_CHECK(min_cos >= 0.0 && min_cos <= 1.0, "min_cos must lie in [0, 1]");
    BP_CHECK(iterations >= 0 && iterations <= 1000 && min_pixels >= 0, "iterations must lie in 0 .. 1000, min_pixels >= 0");
    return bp::IcpParams{K[0], K[4], K[2], K[5], pixel_center, depth_scale, max_dist, min_cos, min_pixels, iterations};
}

// ---- the key-point designator (designate.hip / designate_host.cpp)
static void designate_check_octave(int n, int field, const double* scales, int ns, int k, double min_contrast) {
    BP_CHECK(n >= 1 && n <= bp::DESIGNATE_MAX_OCTAVE, "n must lie in [1, 131072]");
    BP_CHECK(field >= 0 && field <= 2, "field must be 0, 1 or 2 (x, y or z)");
    BP_CHECK(ns >= 4 && ns <= DESIGNATE_MAX_SCALES, "ns must lie in [4, 12]");
    BP_CHECK(k >= 1 && k <= bp::DESIGNATE_MAX_K, "k must lie in [1, 64]");
    BP_CHECK(min_contrast >= 0.0, "min_contrast must not be negative");
    for (int i = 0; i < ns; ++i)
        BP_CHECK(scales[i] > 0.0 && scales[i] <= 1e150 && (i == 0 || scales[i] >= scales[i - 1]),
                 "the scales must be positive, finite and ascending");
}
static void designate_check_fps(int n, int K, int start) {
    BP_CHECK(n >= 1 && n <= bp::DESIGNATE_MAX_FPS, "n must lie in [1, 2^20]");
    BP_CHECK(K >= 1 && K <= n, "K must lie in [1, n]");
    BP_CHECK(start < n, "start must be below n (negative: the point farthest from the centroid)");
}
static void designate_check_thin(int n, int keep) {
    BP_CHECK(n >= 1 && n <= bp::DESIGNATE_MAX_THIN, "n must lie in [1, 16384]");
    BP_CHECK(keep >= 1, "keep must be positive");
}

// ---- pose verification (verify.hip / verify_host.cpp)
static void verify_check_image(int H, int W, int red_channel) {
    BP_CHECK(H >= 3 && W >= 3, "H and W must be at least 3 (the reflect-101 border of a 5-tap stencil)");
    check_pixels(H, W);
    BP_CHECK(red_channel == 0 || red_channel == 2, "red_channel must be 0 or 2");
}
static void verify_check_scores(int P, int T, int H, int W, int red_channel) {
    BP_CHECK(P >= 0 && T > 0, "P must not be negative, T must be positive");
    verify_check_image(H, W, red_channel);
}

extern "C" {

int bp_pose_errors(const double* d_model, int n, const double* d_gt, const double* d_est, int P, const double* K, int want,
                   double* d_out, void* stream) {
    BP_TRY
    BP_CHECK(d_model && d_gt && d_est && d_out, "null argument");
    BP_CHECK(n > 0 && P > 0, "n and P must be positive");
    BP_CHECK(want >= 1 && want <= 7, "want must be a non-empty mask of 1 (ADD), 2 (ADD-S), 4 (2-D)");
    BP_CHECK(K || !(want & 4), "K is required for the 2-D projection error");
    bp::pose_errors(d_model, n, d_gt, d_est, P, K, want, d_out, (hipStream_t)stream);
    return 0;
    BP_CATCH
}

int bp_pose_errors_sym(const double* d_model, int n, const double* d_gt, const double* d_est, int P, const double* d_sym,
                       int S, const double* K, int want, double* d_out, void* stream) {
    BP_TRY
    BP_CHECK(d_model && d_gt && d_est && d_sym && d_out, "null argument");
    BP_CHECK(n > 0 && P > 0 && S > 0, "n, P and S must be positive");
    BP_CHECK(want >= 1 && want <= 3, "want must be a non-empty mask of 1 (MSSD), 2 (MSPD)");
    BP_CHECK(K || !(want & 2), "K is required for the projection distance (MSPD)");
    bp::pose_errors_sym(d_model, n, d_gt, d_est, P, d_sym, S, K, want, d_out, (hipStream_t)stream);
    return 0;
    BP_CATCH
}

int bp_render_depth_host(const double* poses, int P, const double* vertices, int n, const int* faces, int F, const double* K,
                         int H, int W, double pixel_center, double near_z, float* depth, int* skipped) {
    BP_TRY
    BP_CHECK(poses && vertices && faces && K && depth && skipped, "null argument");
    raster_check_sizes(n, F, P, H, W, near_z);
    BP_CHECK(bp::render_depth_host(poses, P, vertices, n, faces, F, K, H, W, pixel_center, near_z, depth, skipped) == 0,
             "a face index lies outside [0, n)");
    return 0;
    BP_CATCH
}

int bp_render_depth(const double* d_model, int n, const int* d_faces, int F, const double* d_poses, int P, const double* K,
                    int H, int W, double pixel_center, double near_z, float* d_depth, int* d_skipped, void* stream) {
    BP_TRY
    BP_CHECK(d_model && d_faces && d_poses && K && d_depth && d_skipped, "null argument");
    raster_check_sizes(n, F, P, H, W, near_z);
    bp::render_depth(d_poses, P, d_model, n, d_faces, F, K, H, W, pixel_center, near_z, d_depth, d_skipped, (hipStream_t)stream);
    return 0;
    BP_CATCH
}

int bp_render_color_host(const double* poses, int P, const double* vertices, int n, const int* faces, int F,
                         const unsigned char* colors, const int* image_index, int I, const double* K, int H, int W,
                         double pixel_center, double near_z, double ambient, const double* light, int accumulate,
                         unsigned char* color, float* depth, int* skipped) {
    BP_TRY
    BP_CHECK(poses && vertices && faces && colors && K && light && color && depth && skipped, "null argument");
    raster_check_color(n, F, P, H, W, near_z, image_index, I);
    BP_CHECK(bp::render_color_host(poses, P, vertices, n, faces, F, colors, image_index, I, K, H, W, pixel_center, near_z, ambient,
                                   light, accumulate, color, depth, skipped) == 0,
             "a face index lies outside [0, n)");   // (its scan comes before it touches anything)
    return 0;
    BP_CATCH
}

int bp_render_color(const double* d_model, int n, const int* d_faces, int F, const unsigned char* d_colors,
                    const double* d_poses, int P, const int* image_index, int I, const double* K, int H, int W,
                    double pixel_center, double near_z, double ambient, const double* light, int accumulate,
                    unsigned char* d_color, float* d_depth, int* d_skipped, void* stream) {
    BP_TRY
    BP_CHECK(d_model && d_faces && d_colors && d_poses && K && light && d_color && d_depth && d_skipped, "null argument");
    raster_check_color(n, F, P, H, W, near_z, image_index, I);
    bp::render_color(d_poses, P, d_model, n, d_faces, F, d_colors, image_index, I, K, H, W, pixel_center, near_z, ambient, light,
                     accumulate, d_color, d_depth, d_skipped, (hipStream_t)stream);
    return 0;
    BP_CATCH
}

size_t bp_texture_mips_bytes(int Wt, int Ht, int levels) {
    if (Wt <= 0 || Ht <= 0 || Wt > bp::texture_max_size() || Ht > bp::texture_max_size() || levels < 1 ||
        levels > bp::texture_full_levels(Wt, Ht))
        return 0;
    return bp::texture_mips_texels(Wt, Ht, levels) * sizeof(uint32_t);
}

int bp_texture_mips_host(const unsigned char* texture, int Wt, int Ht, int levels, uint32_t* mips) {
    BP_TRY
    BP_CHECK(texture && mips, "null argument");
    raster_check_texture(Wt, Ht, levels);
    bp::texture_mips_host(texture, Wt, Ht, levels, mips);
    return 0;
    BP_CATCH
}

int bp_texture_mips(const unsigned char* d_texture, int Wt, int Ht, int levels, uint32_t* d_mips, void* stream) {
    BP_TRY
    BP_CHECK(d_texture && d_mips, "null argument");
    raster_check_texture(Wt, Ht, levels);
    bp::launch_texture_mips(d_texture, Wt, Ht, levels, d_mips, (hipStream_t)stream);
    BP_HIP(hipGetLastError());
    return 0;
    BP_CATCH
}

int bp_render_color_textured_host(const double* poses, int P, const double* vertices, int n, const int* faces, int F,
                                  const unsigned char* colors, const double* uv, const uint32_t* mips, int Wt, int Ht,
                                  int levels, const int* image_index, int I, const double* K, int H, int W,
                                  double pixel_center, double near_z, double ambient, const double* light, int accumulate,
                                  unsigned char* color, float* depth, int* skipped) {
    BP_TRY
    BP_CHECK(poses && vertices && faces && K && light && color && depth && skipped, "null argument");
    BP_CHECK(uv ? mips != nullptr : colors != nullptr, "null argument: uv needs the pyramid, no uv needs colors");
    raster_check_color(n, F, P, H, W, near_z, image_index, I);
    if (uv) raster_check_texture(Wt, Ht, levels);
    const bp::ColorTexture tex{uv, mips, Wt, Ht, levels};
    const int rc = uv ? bp::render_color_textured_host(poses, P, vertices, n, faces, F, tex, image_index, I, K, H, W, pixel_center,
                                                       near_z, ambient, light, accumulate, color, depth, skipped)
                      : bp::render_color_host(poses, P, vertices, n, faces, F, colors, image_index, I, K, H, W, pixel_center,
                                              near_z, ambient, light, accumulate, color, depth, skipped);
    BP_CHECK(rc == 0, "a face index lies outside [0, n)");   // (the scan comes before anything is touched)
    return 0;
    BP_CATCH
}

int bp_render_color_textured(const double* d_model, int n, const int* d_faces, int F, const unsigned char* d_colors,
                             const double* d_uv, const uint32_t* d_mips, int Wt, int Ht, int levels, const double* d_poses,
                             int P, const int* image_index, int I, const double* K, int H, int W, double pixel_center,
                             double near_z, double ambient, const double* light, int accumulate, unsigned char* d_color,
                             float* d_depth, int* d_skipped, void* stream) {
    BP_TRY
    BP_CHECK(d_model && d_faces && d_poses && K && light && d_color && d_depth && d_skipped, "null argument");
    BP_CHECK(d_uv ? d_mips != nullptr : d_colors != nullptr, "null argument: uv needs the pyramid, no uv needs colors");
    raster_check_color(n, F, P, H, W, near_z, image_index, I);
    if (d_uv) raster_check_texture(Wt, Ht, levels);
    const bp::ColorTexture tex{d_uv, d_mips, Wt, Ht, levels};
    bp::render_color(d_poses, P, d_model, n, d_faces, F, d_colors, image_index, I, K, H, W, pixel_center, near_z, ambient, light,
                     accumulate, d_color, d_depth, d_skipped, (hipStream_t)stream, d_uv ? &tex : nullptr);
    return 0;
    BP_CATCH
}

int bp_draw_boxes_host(const double* poses, int P, const double* corners, const unsigned char* corner_colors,
                       const int* image_index, int I, const double* K, int H, int W, double pixel_center, double near_z,
                       unsigned char* color) {
    BP_TRY
    BP_CHECK(poses && corners && corner_colors && K && color, "null argument");
    raster_check_boxes(P, I, H, W, near_z);
    raster_check_image_index(image_index, P, I);
    bp::draw_boxes_host(poses, P, corners, corner_colors, image_index, I, K, H, W, pixel_center, near_z, color);
    return 0;
    BP_CATCH
}

int bp_draw_boxes(const double* d_poses, int P, const double* d_corners, const unsigned char* d_corner_colors,
                  const int* image_index, int I, const double* K, int H, int W, double pixel_center, double near_z,
                  unsigned char* d_color, void* stream) {
    BP_TRY
    BP_CHECK(d_poses && d_corners && d_corner_colors && K && d_color, "null argument");
    raster_check_boxes(P, I, H, W, near_z);
    raster_check_image_index(image_index, P, I);
    bp::draw_boxes(d_poses, P, d_corners, d_corner_colors, image_index, I, K, H, W, pixel_center, near_z, d_color,
                   (hipStream_t)stream);
    return 0;
    BP_CATCH
}

int bp_overlay_host(const unsigned char* frames, const unsigned char* color, const float* depth, int I, int H, int W, int alpha,
                    unsigned char* out) {
    BP_TRY
    BP_CHECK(frames && color && depth && out, "null argument");
    raster_check_overlay(I, H, W, alpha);
    bp::overlay_host(frames, color, depth, I, H, W, alpha, out);
    return 0;
    BP_CATCH
}

int bp_overlay(const unsigned char* d_frames, const unsigned char* d_color, const float* d_depth, int I, int H, int W, int alpha,
               unsigned char* d_out, void* stream) {
    BP_TRY
    BP_CHECK(d_frames && d_color && d_depth && d_out, "null argument");
    raster_check_overlay(I, H, W, alpha);
    bp::overlay(d_frames, d_color, d_depth, I, H, W, alpha, d_out, (hipStream_t)stream);
    return 0;
    BP_CATCH
}

int bp_image_gradients_host(const unsigned char* images, int I, int H, int W, int red_channel, int min_sq, float* grad,
                            float* mag) {
    BP_TRY
    BP_CHECK(I >= 0, "I must not be negative");
    verify_check_image(H, W, red_channel);
    if (I == 0) return 0;
    BP_CHECK(images && grad, "null argument");
    bp::image_gradients_host(images, I, H, W, red_channel, min_sq, grad, mag);
    return 0;
    BP_CATCH
}

int bp_image_gradients(const unsigned char* d_images, int I, int H, int W, int red_channel, int min_sq, float* d_grad,
                       float* d_mag, void* stream) {
    BP_TRY
    BP_CHECK(I >= 0, "I must not be negative");
    verify_check_image(H, W, red_channel);
    if (I == 0) return 0;
    BP_CHECK(d_images && d_grad, "null argument");
    bp::launch_image_gradients(d_images, I, H, W, red_channel, min_sq, d_grad, d_mag, (hipStream_t)stream);
    return 0;
    BP_CATCH
}

int bp_gradient_scores_host(const unsigned char* renders, const float* scene_grad, const int* frame_index, int P, int T, int H,
                            int W, int red_channel, int render_min_sq, uint64_t* sum, int* count, double* score) {
    BP_TRY
    verify_check_scores(P, T, H, W, red_channel);
    if (P == 0) return 0;
    BP_CHECK(renders && scene_grad && frame_index && sum && count && score, "null argument");
    bp::gradient_scores_host(renders, scene_grad, frame_index, P, T, H, W, red_channel, render_min_sq, sum, count, score);
    return 0;
    BP_CATCH
}

int bp_gradient_scores(const unsigned char* d_renders, const float* d_scene_grad, const int* d_frame_index, int P, int T, int H,
                       int W, int red_channel, int render_min_sq, uint64_t* d_sum, int* d_count, double* d_score, void* stream) {
    BP_TRY
    verify_check_scores(P, T, H, W, red_channel);
    if (P == 0) return 0;
    BP_CHECK(d_renders && d_scene_grad && d_frame_index && d_sum && d_count && d_score, "null argument");
    bp::launch_gradient_scores(d_renders, d_scene_grad, d_frame_index, P, T, H, W, red_channel, render_min_sq,
                               (unsigned long long*)d_sum, d_count, d_score, (hipStream_t)stream);
    return 0;
    BP_CATCH
}

int bp_vsd_errors(const double* d_model, int n, const int* d_faces, int F, const double* d_gt, const double* d_est, int P,
                  const double* K, const uint16_t* d_depth_test, int T, int H, int W, double depth_scale,
                  const int* d_test_index, double delta, const double* taus, int n_tau, double diameter, double pixel_center,
                  double near_z, int chunk, double* d_err, int* d_counts, void* stream) {
    BP_TRY
    BP_CHECK(d_model && d_faces && d_gt && d_est && K && d_depth_test && d_test_index && taus && d_err && d_counts,
             "null argument");
    raster_check_sizes(n, F, P, H, W, near_z);
    BP_CHECK(T > 0, "T must be positive");
    BP_CHECK(n_tau >= 1 && n_tau <= bp::VSD_MAX_TAUS, "n_tau must lie in 1 .. 16");
    BP_CHECK(diameter > 0.0 && depth_scale > 0.0 && chunk >= 0, "diameter and depth_scale must be positive, chunk >= 0");
    bp::vsd_errors(d_model, n, d_faces, F, d_gt, d_est, P, K, d_depth_test, T, H, W, depth_scale, d_test_index, delta, taus, n_tau,
                   diameter, pixel_center, near_z, chunk, d_err, d_counts, (hipStream_t)stream);
    return 0;
    BP_CATCH
}

int bp_annotate_keypoints_host(const double* poses, int P, const double* kp, int Kp, const double* K, int H, int W,
                               double pixel_center, double near_z, const float* model_depth, const float* scene_depth, int T,
                               const int* scene_index, double self_tol, double delta, double* xy, double* z,
                               unsigned char* flags) {
    BP_TRY
    BP_CHECK(poses && kp && K && xy && z && flags, "null argument");
    annot_check_keypoints(P, H, W, Kp, near_z);
    annot_check_scene(scene_depth, scene_index, scene_index, P, T);
    bp::annotate_keypoints_host(poses, P, kp, Kp, K, H, W, pixel_center, near_z, model_depth, scene_depth, scene_index, self_tol,
                                delta, xy, z, flags);
    return 0;
    BP_CATCH
}

int bp_annotate_keypoints(const double* d_poses, int P, const double* d_kp, int Kp, const double* K, int H, int W,
                          double pixel_center, double near_z, const float* d_model_depth, const float* d_scene_depth, int T,
                          const int* d_scene_index, double self_tol, double delta, double* d_xy, double* d_z,
                          unsigned char* d_flags, void* stream) {
    BP_TRY
    BP_CHECK(d_poses && d_kp && K && d_xy && d_z && d_flags, "null argument");
    annot_check_keypoints(P, H, W, Kp, near_z);
    annot_check_scene_device(d_scene_depth, d_scene_index, P, T, (hipStream_t)stream);
    bp::annotate_keypoints(d_poses, P, d_kp, Kp, K, H, W, pixel_center, near_z, d_model_depth, d_scene_depth, d_scene_index,
                           self_tol, delta, d_xy, d_z, d_flags, (hipStream_t)stream);
    return 0;
    BP_CATCH
}

int bp_mask_boxes_host(const float* depth, int P, int H, int W, const double* K, double pixel_center, const float* scene_depth,
                       int T, const int* scene_index, double delta, int* boxes, int* counts) {
    BP_TRY
    BP_CHECK(depth && K && boxes && counts, "null argument");
    annot_check_image(P, H, W);
    annot_check_scene(scene_depth, scene_index, scene_index, P, T);
    bp::mask_boxes_host(depth, P, H, W, K, pixel_center, scene_depth, scene_index, delta, boxes, counts);
    return 0;
    BP_CATCH
}

int bp_mask_boxes(const float* d_depth, int P, int H, int W, const double* K, double pixel_center, const float* d_scene_depth,
                  int T, const int* d_scene_index, double delta, int* d_boxes, int* d_counts, void* stream) {
    BP_TRY
    BP_CHECK(d_depth && K && d_boxes && d_counts, "null argument");
    annot_check_image(P, H, W);
    BP_CHECK(P < (1 << 28), "P must be below 2^28");
    annot_check_scene_device(d_scene_depth, d_scene_index, P, T, (hipStream_t)stream);
    bp::mask_boxes(d_depth, P, H, W, K, pixel_center, d_scene_depth, d_scene_index, delta, d_boxes, d_counts, (hipStream_t)stream);
    return 0;
    BP_CATCH
}

int bp_vertex_boxes_host(const double* poses, int P, const double* vertices, int n, const double* K, int H, int W, int* boxes) {
    BP_TRY
    BP_CHECK(poses && vertices && K && boxes, "null argument");
    annot_check_image(P, H, W);
    BP_CHECK(n > 0, "n must be positive");
    bp::vertex_boxes_host(poses, P, vertices, n, K, H, W, boxes);
    return 0;
    BP_CATCH
}

int bp_vertex_boxes(const double* d_poses, int P, const double* d_vertices, int n, const double* K, int H, int W, int* d_boxes,
                    void* stream) {
    BP_TRY
    BP_CHECK(d_poses && d_vertices && K && d_boxes, "null argument");
    annot_check_image(P, H, W);
    BP_CHECK(n > 0 && P < (1 << 28), "n must be positive and P below 2^28");
    bp::vertex_boxes(d_poses, P, d_vertices, n, K, H, W, d_boxes, (hipStream_t)stream);
    return 0;
    BP_CATCH
}

int bp_kpd_targets_host(const double* parts, const float* ul, const float* br, int B, int Kp, int inpH, int inpW, int resH,
                        int resW, const float* g, int size, float* out, int* centres, float* set_mask) {
    BP_TRY
    BP_CHECK(parts && ul && br && g && out && centres, "null argument");
    annot_check_targets(B, Kp, inpH, inpW, resH, resW, size);
    bp::kpd_targets_host(parts, ul, br, B, Kp, inpH, inpW, resH, resW, g, size, out, centres, set_mask);
    return 0;
    BP_CATCH
}

int bp_kpd_targets(const double* d_parts, const float* d_ul, const float* d_br, int B, int Kp, int inpH, int inpW, int resH,
                   int resW, const float* d_g, int size, float* d_out, int* d_centres, float* d_set_mask, void* stream) {
    BP_TRY
    BP_CHECK(d_parts && d_ul && d_br && d_g && d_out && d_centres, "null argument");
    annot_check_targets(B, Kp, inpH, inpW, resH, resW, size);
    bp::kpd_targets(d_parts, d_ul, d_br, B, Kp, inpH, inpW, resH, resW, d_g, size, d_out, d_centres, d_set_mask,
                    (hipStream_t)stream);
    return 0;
    BP_CATCH
}

int bp_kpd_inputs_host(const unsigned char* frames, int N, int H, int W, const int* frame_index, const float* ul, const float* br,
                       const float* gains, const unsigned char* blank, int B, int inpH, int inpW, float* inp) {
    BP_TRY
    BP_CHECK(frames && frame_index && ul && br && inp, "null argument");
    sample_check_inputs(N, H, W, B, inpH, inpW);
    bp::kpd_inputs_host(frames, N, H, W, frame_index, ul, br, gains, blank, B, inpH, inpW, inp);
    return 0;
    BP_CATCH
}

int bp_kpd_inputs(const unsigned char* d_frames, int N, int H, int W, const int* d_frame_index, const float* d_ul,
                  const float* d_br, const float* d_gains, const unsigned char* d_blank, int B, int inpH, int inpW, float* d_inp,
                  void* stream) {
    BP_TRY
    BP_CHECK(d_frames && d_frame_index && d_ul && d_br && d_inp, "null argument");
    sample_check_inputs(N, H, W, B, inpH, inpW);
    bp::kpd_inputs(d_frames, N, H, W, d_frame_index, d_ul, d_br, d_gains, d_blank, B, inpH, inpW, d_inp, (hipStream_t)stream);
    return 0;
    BP_CATCH
}

int bp_kpd_augment_host(const float* x, int B, int C, int H, int W, const unsigned char* flip, const double* cs, const int* perm,
                        float* y) {
    BP_TRY
    BP_CHECK(x && flip && cs && y && x != y, "null argument, or x and y are the same tensor");
    sample_check_maps(B, C, H, W);
    bp::kpd_augment_host(x, B, C, H, W, flip, cs, perm, y);
    return 0;
    BP_CATCH
}

int bp_kpd_augment(const float* d_x, int B, int C, int H, int W, const unsigned char* d_flip, const double* d_cs,
                   const int* d_perm, float* d_y, void* stream) {
    BP_TRY
    BP_CHECK(d_x && d_flip && d_cs && d_y && d_x != d_y, "null argument, or x and y are the same tensor");
    sample_check_maps(B, C, H, W);
    bp::kpd_augment(d_x, B, C, H, W, d_flip, d_cs, d_perm, d_y, (hipStream_t)stream);
    return 0;
    BP_CATCH
}

int bp_heatmap_loss_acc_host(const float* out, const float* labels, const float* set_mask, int B, int K, int H, int W,
                             double* partial, double* loss, float* acc, int* preds, int* gt, float* dists, float* grad) {
    BP_TRY
    BP_CHECK(out && labels && partial && loss && acc && preds && gt && dists, "null argument");
    sample_check_maps(B, K, H, W);
    bp::heatmap_loss_acc_host(out, labels, set_mask, B, K, H, W, partial, loss, acc, preds, gt, dists, grad);
    return 0;
    BP_CATCH
}

int bp_heatmap_loss_acc(const float* d_out, const float* d_labels, const float* d_set_mask, int B, int K, int H, int W,
                        double* d_partial, double* d_loss, float* d_acc, int* d_preds, int* d_gt, float* d_dists, float* d_grad,
                        void* stream) {
    BP_TRY
    BP_CHECK(d_out && d_labels && d_partial && d_loss && d_acc && d_preds && d_gt && d_dists, "null argument");
    sample_check_maps(B, K, H, W);
    bp::heatmap_loss_acc(d_out, d_labels, d_set_mask, B, K, H, W, d_partial, d_loss, d_acc, d_preds, d_gt, d_dists, d_grad,
                         (hipStream_t)stream);
    return 0;
    BP_CATCH
}

size_t bp_yolo_loss_partials(int B, int n, int classes, int h, int w) {
    if (B <= 0 || n <= 0 || classes <= 0 || h <= 0 || w <= 0) return 0;
    return bp::yolo_loss_partials(B, n, classes, h, w);
}

int bp_yolo_inputs_host(const unsigned char* frames, int N, int H, int W, const int* frame_index, const int* crop,
                        const unsigned char* flip, const float* hsv, int B, int net_h, int net_w, float* out) {
    BP_TRY
    BP_CHECK(frames && frame_index && crop && flip && out, "null argument");
    yolo_check_inputs(N, H, W, B, net_h, net_w);
    yolo_check_crop(crop, B);
    bp::yolo_inputs_host(frames, N, H, W, frame_index, crop, flip, hsv, B, net_h, net_w, out);
    return 0;
    BP_CATCH
}

int bp_yolo_inputs(const unsigned char* d_frames, int N, int H, int W, const int* d_frame_index, const int* d_crop,
                   const unsigned char* d_flip, const float* d_hsv, int B, int net_h, int net_w, float* d_out, void* stream) {
    BP_TRY
    BP_CHECK(d_frames && d_frame_index && d_crop && d_flip && d_out, "null argument");
    yolo_check_inputs(N, H, W, B, net_h, net_w);
    // the crop is read back to be checked before any kernel uses it
    std::vector<int> crop((size_t)B * 4);
    BP_HIP(hipMemcpyAsync(crop.data(), d_crop, crop.size() * sizeof(int), hipMemcpyDeviceToHost, (hipStream_t)stream));
    BP_HIP(hipStreamSynchronize((hipStream_t)stream));
    yolo_check_crop(crop.data(), B);
    bp::yolo_inputs(d_frames, N, H, W, d_frame_index, d_crop, d_flip, d_hsv, B, net_h, net_w, d_out, (hipStream_t)stream);
    return 0;
    BP_CATCH
}

int bp_yolo_truth_host(const float* labels, int M, const int* first, const int* swap, const float* geom, const unsigned char* flip,
                       int B, int classes, int max_boxes, int net_w, int net_h, int small_object, int* order, float* truth,
                       int* kept) {
    BP_TRY
    BP_CHECK(first && geom && flip && truth && kept && (M == 0 || (labels && swap && order)), "null argument");
    yolo_check_truth(M, B, classes, max_boxes, net_w, net_h);
    BP_CHECK(first[0] >= 0 && first[B] <= M, "first must lie within [0, M]");
    for (int b = 0; b < B; ++b) BP_CHECK(first[b] <= first[b + 1], "first must be non-decreasing");
    bp::yolo_truth_host(labels, M, first, swap, geom, flip, B, classes, max_boxes, net_w, net_h, small_object, order, truth, kept);
    return 0;
    BP_CATCH
}

int bp_yolo_truth(const float* d_labels, int M, const int* d_first, const int* d_swap, const float* d_geom,
                  const unsigned char* d_flip, int B, int classes, int max_boxes, int net_w, int net_h, int small_object,
                  int* d_order, float* d_truth, int* d_kept, void* stream) {
    BP_TRY
    BP_CHECK(d_first && d_geom && d_flip && d_truth && d_kept && (M == 0 || (d_labels && d_swap && d_order)), "null argument");
    yolo_check_truth(M, B, classes, max_boxes, net_w, net_h);
    bp::yolo_truth(d_labels, M, d_first, d_swap, d_geom, d_flip, B, classes, max_boxes, net_w, net_h, small_object, d_order,
                   d_truth, d_kept, (hipStream_t)stream);
    return 0;
    BP_CATCH
}

int bp_yolo_loss_host(const float* x, int B, int channels, int n, int classes, int h, int w, int net_w, int net_h,
                      const float* anchors, int total, const int* mask, const float* truth, int max_boxes, float ignore_thresh,
                      float truth_thresh, int focal_loss, float* act, float* delta, double* cost, double* stats, double* partial) {
    BP_TRY
    BP_CHECK(x && anchors && mask && truth && delta && cost && stats && partial && x != delta, "null argument, or x and delta are the same tensor");
    yolo_check_loss(B, n, classes, h, w, net_w, net_h, total, max_boxes, channels, focal_loss);
    yolo_check_mask(mask, n, total);
    bp::yolo_loss_host(x, B, n, classes, h, w, net_w, net_h, anchors, total, mask, truth, max_boxes, ignore_thresh, truth_thresh,
                       act, delta, cost, stats, partial);
    return 0;
    BP_CATCH
}

int bp_yolo_loss(const float* d_x, int B, int channels, int n, int classes, int h, int w, int net_w, int net_h,
                 const float* d_anchors, int total, const int* d_mask, const float* d_truth, int max_boxes, float ignore_thresh,
                 float truth_thresh, int focal_loss, float* d_act, float* d_delta, double* d_cost, double* d_stats,
                 double* d_partial, void* stream) {
    BP_TRY
    BP_CHECK(d_x && d_anchors && d_mask && d_truth && d_delta && d_cost && d_stats && d_partial && d_x != d_delta,
             "null argument, or x and delta are the same tensor");
    yolo_check_loss(B, n, classes, h, w, net_w, net_h, total, max_boxes, channels, focal_loss);
    // the mask indexes the anchors: it is read back to be checked before any kernel uses it
    std::vector<int> mask(n);
    BP_HIP(hipMemcpyAsync(mask.data(), d_mask, (size_t)n * sizeof(int), hipMemcpyDeviceToHost, (hipStream_t)stream));
    BP_HIP(hipStreamSynchronize((hipStream_t)stream));
    yolo_check_mask(mask.data(), n, total);
    bp::yolo_loss(d_x, B, n, classes, h, w, net_w, net_h, d_anchors, total, d_mask, d_truth, max_boxes, ignore_thresh,
                  truth_thresh, d_act, d_delta, d_cost, d_stats, d_partial, (hipStream_t)stream);
    return 0;
    BP_CATCH
}

int bp_yolo_map_max_dets(void) { return bp::yolo_map_max_dets(); }

size_t bp_yolo_detections_scratch(int B, int max_dets, int classes) {
    if (B <= 0 || max_dets <= 0 || classes <= 0) return 0;
    return bp::yolo_detections_scratch(B, max_dets, classes);
}

size_t bp_detector_map_reduce_scratch(int D, int truths) {
    if (D < 0 || D > (1 << 26) || truths < 0) return 0;
    return bp::map_reduce_scratch(D, truths);
}

int bp_yolo_detections_host(const float* pred, int B, int rows, int attrs, const int* heads, int nheads, int net_w, int net_h,
                            int classes, float thresh, float nms, int max_dets, float* dets, int* count) {
    BP_TRY
    BP_CHECK(pred && heads && dets && count, "null argument");
    map_check_detections(B, rows, attrs, heads, nheads, net_w, net_h, classes, thresh, max_dets, false);
    bp::yolo_detections_host(pred, B, rows, heads, nheads, net_w, net_h, classes, thresh, nms, max_dets, dets, count);
    return 0;
    BP_CATCH
}

int bp_yolo_detections(const float* d_pred, int B, int rows, int attrs, const int* heads, int nheads, int net_w, int net_h,
                       int classes, float thresh, float nms, int max_dets, float* d_dets, int* d_count, void* d_scratch,
                       void* stream) {
    BP_TRY
    BP_CHECK(d_pred && heads && d_dets && d_count && d_scratch, "null argument");
    map_check_detections(B, rows, attrs, heads, nheads, net_w, net_h, classes, thresh, max_dets, true);
    bp::yolo_detections(d_pred, B, rows, heads, nheads, net_w, net_h, classes, thresh, nms, max_dets, d_dets, d_count, d_scratch,
                        (hipStream_t)stream);
    return 0;
    BP_CATCH
}

int bp_detector_map_match_host(const float* dets, const int* count, int B, int max_dets, int classes, const float* labels, int M,
                               const int* first, float iou_thresh, float thresh_calc, int truth_base, int image_base,
                               int rec_stride, float* rec, int* rec_count, int* truth_classes_count, double* img_stats) {
    BP_TRY
    BP_CHECK(dets && count && first && rec && rec_count && truth_classes_count && img_stats && (M == 0 || labels), "null argument");
    map_check_match(B, max_dets, classes, M, rec_stride, truth_base, image_base);
    BP_CHECK(first[0] >= 0 && first[B] <= M, "first must lie within [0, M]");
    for (int b = 0; b < B; ++b) BP_CHECK(first[b] <= first[b + 1], "first must be non-decreasing");
    bp::map_match_host(dets, count, B, max_dets, classes, labels, M, first, iou_thresh, thresh_calc, truth_base, image_base,
                       rec_stride, rec, rec_count, truth_classes_count, img_stats);
    return 0;
    BP_CATCH
}

int bp_detector_map_match(const float* d_dets, const int* d_count, int B, int max_dets, int classes, const float* d_labels, int M,
                          const int* d_first, float iou_thresh, float thresh_calc, int truth_base, int image_base, int rec_stride,
                          float* d_rec, int* d_rec_count, int* d_truth_classes_count, double* d_img_stats, int* d_claim,
                          void* stream) {
    BP_TRY
    BP_CHECK(d_dets && d_count && d_first && d_rec && d_rec_count && d_truth_classes_count && d_img_stats && d_claim &&
                 (M == 0 || d_labels), "null argument");
    map_check_match(B, max_dets, classes, M, rec_stride, truth_base, image_base);
    bp::map_match(d_dets, d_count, B, max_dets, classes, d_labels, M, d_first, iou_thresh, thresh_calc, truth_base, image_base,
                  rec_stride, d_rec, d_rec_count, d_truth_classes_count, d_img_stats, d_claim, (hipStream_t)stream);
    return 0;
    BP_CATCH
}

int bp_detector_map_reduce_host(const float* rec, int D, const int* truth_classes_count, int classes, int truths,
                                const double* img_stats, int N, double* ap, double* stats, double* pr) {
    BP_TRY
    BP_CHECK(truth_classes_count && ap && stats && (D == 0 || rec) && (N == 0 || img_stats), "null argument");
    map_check_reduce(D, classes, truths, N);
    bp::map_reduce_host(rec, D, truth_classes_count, classes, truths, img_stats, N, ap, stats, pr);
    return 0;
    BP_CATCH
}

int bp_detector_map_reduce(const float* d_rec, int D, const int* d_truth_classes_count, int classes, int truths,
                           const double* d_img_stats, int N, double* d_ap, double* d_stats, double* d_pr, void* d_scratch,
                           void* stream) {
    BP_TRY
    BP_CHECK(d_truth_classes_count && d_ap && d_stats && d_scratch && (D == 0 || d_rec) && (N == 0 || d_img_stats), "null argument");
    map_check_reduce(D, classes, truths, N);
    bp::map_reduce(d_rec, D, d_truth_classes_count, classes, truths, d_img_stats, N, d_ap, d_stats, d_pr, d_scratch,
                   (hipStream_t)stream);
    return 0;
    BP_CATCH
}

int bp_icp_normal_equations_host(const double* poses, int P, const double* vertices, int n, const int* faces, int F,
                                 const double* K, const uint16_t* depth_test, int T, int H, int W, double depth_scale,
                                 const int* test_index, double max_dist, double min_cos, double pixel_center, double near_z,
                                 double* out) {
    BP_TRY
    BP_CHECK(poses && vertices && faces && K && depth_test && test_index && out, "null argument");
    raster_check_sizes(n, F, P, H, W, near_z);
    const bp::IcpParams prm = icp_params(K, T, depth_scale, 0, max_dist, min_cos, 0, pixel_center);
    BP_CHECK(bp::icp_normal_equations_host(poses, P, vertices, n, faces, F, K, depth_test, T, test_index, H, W, prm, near_z,
                                           out) == 0,
             "a face index lies outside [0, n)");
    return 0;
    BP_CATCH
}

int bp_refine_depth_host(const double* poses, int P, const double* vertices, int n, const int* faces, int F, const double* K,
                         const uint16_t* depth_test, int T, int H, int W, double depth_scale, const int* test_index,
                         int iterations, double max_dist, double min_cos, int min_pixels, double pixel_center, double near_z,
                         double* poses_out, double* stats) {
    BP_TRY
    BP_CHECK(poses && vertices && faces && K && depth_test && test_index && poses_out && stats, "null argument");
    raster_check_sizes(n, F, P, H, W, near_z);
    const bp::IcpParams prm = icp_params(K, T, depth_scale, iterations, max_dist, min_cos, min_pixels, pixel_center);
    BP_CHECK(bp::refine_depth_host(poses, P, vertices, n, faces, F, K, depth_test, T, test_index, H, W, prm, near_z, poses_out,
                                   stats) == 0,
             "a face index lies outside [0, n)");
    return 0;
    BP_CATCH
}

int bp_icp_normal_equations(const double* d_model, int n, const int* d_faces, int F, const double* d_poses, int P,
                            const double* K, const uint16_t* d_depth_test, int T, int H, int W, double depth_scale,
                            const int* d_test_index, double max_dist, double min_cos, double pixel_center, double near_z,
                            int chunk, double* d_out, void* stream) {
    BP_TRY
    BP_CHECK(d_model && d_faces && d_poses && K && d_depth_test && d_test_index && d_out, "null argument");
    raster_check_sizes(n, F, P, H, W, near_z);
    BP_CHECK(chunk >= 0, "chunk must not be negative");
    const bp::IcpParams prm = icp_params(K, T, depth_scale, 0, max_dist, min_cos, 0, pixel_center);
    bp::icp_normal_equations(d_poses, P, d_model, n, d_faces, F, K, d_depth_test, T, d_test_index, H, W, prm, near_z, chunk, d_out,
                             (hipStream_t)stream);
    return 0;
    BP_CATCH
}

int bp_refine_depth(const double* d_model, int n, const int* d_faces, int F, const double* d_poses, int P, const double* K,
                    const uint16_t* d_depth_test, int T, int H, int W, double depth_scale, const int* d_test_index,
                    int iterations, double max_dist, double min_cos, int min_pixels, double pixel_center, double near_z,
                    int chunk, double* d_poses_out, double* d_stats, void* stream) {
    BP_TRY
    BP_CHECK(d_model && d_faces && d_poses && K && d_depth_test && d_test_index && d_poses_out && d_stats, "null argument");
    BP_CHECK(d_poses_out != d_poses, "d_poses_out must not be d_poses: a rejected pose gets its input back");
    raster_check_sizes(n, F, P, H, W, near_z);
    BP_CHECK(chunk >= 0, "chunk must not be negative");
    const bp::IcpParams prm = icp_params(K, T, depth_scale, iterations, max_dist, min_cos, min_pixels, pixel_center);
    bp::refine_depth(d_poses, P, d_model, n, d_faces, F, K, d_depth_test, T, d_test_index, H, W, prm, near_z, chunk, d_poses_out,
                     d_stats, (hipStream_t)stream);
    return 0;
    BP_CATCH
}

int bp_voxel_grid_host(const double* points, int n, double leaf, double* out, int* n_out) {
    BP_TRY
    BP_CHECK(points && out && n_out, "null argument");
    BP_CHECK(n >= 1, "n must be positive");
    BP_CHECK(leaf > 0.0 && leaf <= 1e300, "leaf must be positive and finite");
    bp::voxel_grid_host(points, n, leaf, out, n_out);
    return 0;
    BP_CATCH
}

int bp_sift_octave_host(const double* points, int n, int field, const double* scales, int ns, int k, double min_contrast,
                        double* dog, signed char* flags) {
    BP_TRY
    BP_CHECK(points && scales && dog && flags, "null argument");
    designate_check_octave(n, field, scales, ns, k, min_contrast);
    bp::sift_octave_host(points, n, field, scales, ns, k, min_contrast, dog, flags);
    return 0;
    BP_CATCH
}

int bp_sift_octave(const double* d_points, int n, int field, const double* scales, int ns, int k, double min_contrast,
                   double* d_dog, signed char* d_flags, void* stream) {
    BP_TRY
    BP_CHECK(d_points && scales && d_dog && d_flags, "null argument");
    designate_check_octave(n, field, scales, ns, k, min_contrast);
    bp::sift_octave(d_points, n, field, scales, ns, k, min_contrast, d_dog, d_flags, (hipStream_t)stream);
    return 0;
    BP_CATCH
}

int bp_farthest_points_host(const double* points, int n, int K, int start, int* idx, double* d2) {
    BP_TRY
    BP_CHECK(points && idx && d2, "null argument");
    designate_check_fps(n, K, start);
    bp::farthest_points_host(points, n, K, start, idx, d2);
    return 0;
    BP_CATCH
}

int bp_farthest_points(const double* d_points, int n, int K, int start, int* d_idx, double* d_d2, void* stream) {
    BP_TRY
    BP_CHECK(d_points && d_idx && d_d2, "null argument");
    designate_check_fps(n, K, start);
    bp::farthest_points(d_points, n, K, start, d_idx, d_d2, (hipStream_t)stream);
    return 0;
    BP_CATCH
}

int bp_thin_points_host(const double* points, int n, int keep, unsigned char* alive, int* state) {
    BP_TRY
    BP_CHECK(points && alive && state, "null argument");
    designate_check_thin(n, keep);
    bp::thin_points_host(points, n, keep, alive, state);
    return 0;
    BP_CATCH
}

int bp_thin_points(const double* d_points, int n, int keep, unsigned char* d_alive, int* d_state, void* stream) {
    BP_TRY
    BP_CHECK(d_points && d_alive && d_state, "null argument");
    designate_check_thin(n, keep);
    bp::thin_points(d_points, n, keep, d_alive, d_state, (hipStream_t)stream);
    return 0;
    BP_CATCH
}

}  // extern "C"
