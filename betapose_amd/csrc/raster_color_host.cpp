// Host twin of the colour renderer (include/betapose_hip.h bp_render_color_host, bp_draw_boxes_host, bp_overlay_host):
// plain loops over poses, edges and pixels around the arithmetic of raster_math.inc and raster_color_math.inc, the text
// raster_color.hip compiles too; the loop over a pose's triangles and their pixels is rs_walk_host (raster_walk.inc, the
// depth rasteriser's too) with the key buffer as its sink.  Visibility is a minimum over 64-bit keys and the box
// overlap rule a maximum over 32-bit ids, neither of which depends on the order of its operands, so these images and the
// kernels' are equal byte for byte.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

#include "raster.h"

#pragma clang fp contract(off)

namespace bp {

namespace {
#include "raster_math.inc"
#include "raster_walk.inc"
#include "raster_color_math.inc"
}  // namespace

void color_visibility_host(const double* poses, int P, const double* vertices, int n, const int* faces, int F,
                           const int* image_index, int I, const RsCam& cam, int H, int W, int accumulate, const float* depth,
                           unsigned long long* keys, int* skipped) {
    const size_t HW = (size_t)H * W;
    std::vector<double> X((size_t)n * 3);
    std::vector<int> S((size_t)n * 2);
    std::fill(keys, keys + (size_t)I * HW, RC_EMPTY_KEY);
    if (accumulate)
        for (size_t i = 0; i < (size_t)I * HW; ++i) {
            uint32_t bits;
            std::memcpy(&bits, &depth[i], 4);
            if (depth[i] > 0.0f) keys[i] = rc_key(bits, RC_KEEP);
        }
    for (int q = 0; q < P; ++q) {
        unsigned long long* kb = keys + (size_t)(image_index ? image_index[q] : q) * HW;
        skipped[q] = rs_walk_host(cam, poses + (size_t)q * 12, vertices, n, faces, F, H, W, X.data(), S.data(),
                                  [&](size_t at, uint32_t bits, int f) {    // smaller key wins
                                      const unsigned long long key = rc_key(bits, (uint32_t)((unsigned long long)q * F + f));
                                      if (key < kb[at]) kb[at] = key;
                                  });
    }
}

int render_color_host(const double* poses, int P, const double* vertices, int n, const int* faces, int F,
                      const unsigned char* colors, const int* image_index, int I, const double* K, int H, int W,
                      double pixel_center, double near, double ambient, const double* light, int accumulate,
                      unsigned char* color, float* depth, int* skipped) {
    for (int i = 0; i < F * 3; ++i)
        if (faces[i] < 0 || faces[i] >= n) return -1;
    const RsCam cam = raster_cam(K, pixel_center, near);
    const ColorLight lt{ambient, light[0], light[1], light[2]};
    const size_t HW = (size_t)H * W;
    std::vector<unsigned long long> keys((size_t)I * HW);
    color_visibility_host(poses, P, vertices, n, faces, F, image_index, I, cam, H, W, accumulate, depth, keys.data(), skipped);
    // resolve: shade the winner of every pixel from the model, the faces and the pose alone
    for (int i = 0; i < I; ++i)
        for (int y = 0; y < H; ++y)
            for (int x = 0; x < W; ++x) {
                const size_t at = (size_t)i * HW + (size_t)y * W + x;
                const unsigned long long key = keys[at];
                const uint32_t id = (uint32_t)key;
                if (key == RC_EMPTY_KEY) {
                    color[at * 3 + 0] = color[at * 3 + 1] = color[at * 3 + 2] = 0;
                    depth[at] = 0.0f;
                    continue;
                }
                if (id == RC_KEEP) continue;
                const int q = (int)(id / (uint32_t)F), f = (int)(id % (uint32_t)F);
                const double* pose = poses + (size_t)q * 12;
                const int* fv = faces + (size_t)f * 3;
                double A[3], B[3], C[3];
                rs_transform(pose, vertices[fv[0] * 3 + 0], vertices[fv[0] * 3 + 1], vertices[fv[0] * 3 + 2], A);
                rs_transform(pose, vertices[fv[1] * 3 + 0], vertices[fv[1] * 3 + 1], vertices[fv[1] * 3 + 2], B);
                rs_transform(pose, vertices[fv[2] * 3 + 0], vertices[fv[2] * 3 + 1], vertices[fv[2] * 3 + 2], C);
                rc_shade(cam, A, B, C, colors + (size_t)fv[0] * 3, colors + (size_t)fv[1] * 3, colors + (size_t)fv[2] * 3, x, y,
                         lt, color + at * 3);
                const uint32_t bits = (uint32_t)(key >> 32);
                std::memcpy(&depth[at], &bits, 4);
            }
    return 0;
}

void draw_boxes_host(const double* poses, int P, const double* corners, const unsigned char* corner_colors,
                     const int* image_index, int I, const double* K, int H, int W, double pixel_center, double near,
                     unsigned char* color) {
    const RsCam cam = raster_cam(K, pixel_center, near);
    const size_t HW = (size_t)H * W;
    std::vector<uint32_t> ids((size_t)I * HW, 0u);
    for (int q = 0; q < P; ++q) {
        uint32_t* plane = ids.data() + (size_t)(image_index ? image_index[q] : q) * HW;
        for (int e = 0; e < RC_BOX_EDGES; ++e) {
            RcEdge g;
            if (!rc_edge_setup(cam, poses + (size_t)q * 12, corners, e, H, W, &g)) continue;
            const uint32_t id = (uint32_t)q * RC_BOX_EDGES + e + 1;
            const long long minor_size = g.major_x ? H : W;
            for (int p = g.p0; p <= g.p1; ++p) {
                const long long j = rc_edge_minor(g, p);
                if (j < 0 || j >= minor_size) continue;
                uint32_t& dst = plane[g.major_x ? (size_t)j * W + p : (size_t)p * W + j];
                if (id > dst) dst = id;
            }
        }
    }
    for (int i = 0; i < I; ++i)
        for (int y = 0; y < H; ++y)
            for (int x = 0; x < W; ++x) {
                const size_t at = (size_t)i * HW + (size_t)y * W + x;
                if (!ids[at]) continue;
                const int q = (int)((ids[at] - 1) / RC_BOX_EDGES), e = (int)((ids[at] - 1) % RC_BOX_EDGES);
                RcEdge g;
                rc_edge_setup(cam, poses + (size_t)q * 12, corners, e, H, W, &g);
                rc_edge_color(g, g.major_x ? x : y, corner_colors, color + at * 3);
            }
}

void overlay_host(const unsigned char* frames, const unsigned char* color, const float* depth, int I, int H, int W, int alpha,
                  unsigned char* out) {
    const size_t count = (size_t)I * H * W;
    for (size_t i = 0; i < count; ++i) {
        const bool drawn = depth[i] > 0.0f;
        for (int k = 0; k < 3; ++k)
            out[i * 3 + k] = drawn ? rc_blend(alpha, color[i * 3 + k], frames[i * 3 + k]) : frames[i * 3 + k];
    }
}

}  // namespace bp
