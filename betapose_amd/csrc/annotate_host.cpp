// Host twins of the key-point annotator (include/betapose_hip.h bp_annotate_keypoints_host, bp_mask_boxes_host,
// bp_vertex_boxes_host, bp_kpd_targets_host): plain loops around the arithmetic of annotate_math.inc, the text
// annotate.hip compiles too.  Every reduction here is an integer minimum, maximum or sum, none of which depends on the
// order of its operands, so these results and the kernels' are equal bit for bit.
#include <cmath>
#include <cstdint>

#include "annotate.h"

#pragma clang fp contract(off)

namespace bp {

namespace {
#include "annotate_math.inc"

struct Box {
    int xmin = AN_BOX_EMPTY_MIN, xmax = AN_BOX_EMPTY_MAX, ymin = AN_BOX_EMPTY_MIN, ymax = AN_BOX_EMPTY_MAX, count = 0;
    void add(int x, int y) {
        if (x < xmin) xmin = x;
        if (x > xmax) xmax = x;
        if (y < ymin) ymin = y;
        if (y > ymax) ymax = y;
        ++count;
    }
    void write(int* out) const {
        out[0] = count ? xmin : -1;
        out[1] = count ? xmax : -1;
        out[2] = count ? ymin : -1;
        out[3] = count ? ymax : -1;
    }
};
}  // namespace

void annotate_keypoints_host(const double* poses, int P, const double* kp, int Kp, const double* K, int H, int W,
                             double pixel_center, double near, const float* model_depth, const float* scene_depth,
                             const int* scene_index, double self_tol, double delta, double* xy, double* z,
                             unsigned char* flags) {
    const AnCam cam = an_cam(K, pixel_center, near);
    const size_t HW = (size_t)H * W;
    for (int p = 0; p < P; ++p) {
        const float* md = model_depth ? model_depth + (size_t)p * HW : nullptr;
        const float* sc = scene_depth ? scene_depth + (size_t)scene_index[p] * HW : nullptr;
        for (int k = 0; k < Kp; ++k) {
            const size_t i = (size_t)p * Kp + k;
            flags[i] = (unsigned char)an_keypoint(cam, poses + (size_t)p * 12, kp + (size_t)k * 3, H, W, md, sc, self_tol,
                                                  delta, xy + i * 2, z + i);
        }
    }
}

void mask_boxes_host(const float* depth, int P, int H, int W, const double* K, double pixel_center, const float* scene_depth,
                     const int* scene_index, double delta, int* boxes, int* counts) {
    const AnCam cam = an_cam(K, pixel_center, 0.0);
    const size_t HW = (size_t)H * W;
    for (int p = 0; p < P; ++p) {
        const float* d = depth + (size_t)p * HW;
        const float* sc = scene_depth ? scene_depth + (size_t)scene_index[p] * HW : nullptr;
        Box full, vis;
        for (int y = 0; y < H; ++y)
            for (int x = 0; x < W; ++x) {
                const float D = d[(size_t)y * W + x];
                if (!(D > 0.0f)) continue;
                full.add(x, y);
                if (!sc || an_pixel_visible(cam, x, y, D, sc[(size_t)y * W + x], delta)) vis.add(x, y);
            }
        full.write(boxes + (size_t)p * 8);
        vis.write(boxes + (size_t)p * 8 + 4);
        counts[(size_t)p * 2] = full.count;
        counts[(size_t)p * 2 + 1] = vis.count;
    }
}

void vertex_boxes_host(const double* poses, int P, const double* vertices, int n, const double* K, int H, int W, int* boxes) {
    const AnCam cam = an_cam(K, 0.0, 0.0);
    for (int p = 0; p < P; ++p) {
        Box b;
        for (int i = 0; i < n; ++i) {
            int ix, iy;
            if (an_splat(cam, poses + (size_t)p * 12, vertices + (size_t)i * 3, H, W, &ix, &iy)) b.add(ix, iy);
        }
        b.write(boxes + (size_t)p * 4);
    }
}

void kpd_targets_host(const double* parts, const float* ul, const float* br, int B, int Kp, int inpH, int inpW, int resH,
                      int resW, const float* g, int size, float* out, int* centres, float* set_mask) {
    for (int b = 0; b < B; ++b)
        for (int k = 0; k < Kp; ++k) {
            const size_t i = (size_t)b * Kp + k;
            int cx, cy;
            an_target_centre(parts[i * 2], parts[i * 2 + 1], ul[b * 2], ul[b * 2 + 1], br[b * 2], br[b * 2 + 1], inpH, inpW, resH,
                             &cx, &cy);
            centres[i * 2] = cx;
            centres[i * 2 + 1] = cy;
            float* o = out + i * resH * resW;
            for (int y = 0; y < resH; ++y)
                for (int x = 0; x < resW; ++x) o[(size_t)y * resW + x] = an_target_value(g, size, cx, cy, x, y);
            if (set_mask)
                for (size_t j = 0; j < (size_t)resH * resW; ++j) set_mask[i * resH * resW + j] = 1.0f;
        }
}

}  // namespace bp
