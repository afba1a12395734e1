// Host twins of the textured colour renderer (include/betapose_hip.h bp_texture_mips_host,
// bp_render_color_textured_host) and the pyramid's sizes, which the C entries and the device driver ask for: plain loops
// over texels and pixels around the arithmetic of raster_math.inc, raster_color_math.inc and raster_texture_math.inc, the
// text raster_texture.hip compiles too.  Visibility is raster_color_host.cpp's (color_visibility_host), unchanged: only
// the resolve differs.  Integers and f64 in a fixed order: these images and the kernels' are equal byte for byte.
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

#include "raster.h"

#pragma clang fp contract(off)

namespace bp {

namespace {
#include "raster_math.inc"
#include "raster_color_math.inc"
#include "raster_texture_math.inc"
}  // namespace

int texture_max_size() { return TX_MAX_SIZE; }

int texture_full_levels(int Wt, int Ht) { return tx_full_levels(Wt, Ht); }

size_t texture_mips_texels(int Wt, int Ht, int levels) {
    int lw, lh;
    return tx_level_offset(Wt, Ht, levels, &lw, &lh);
}

void texture_mips_host(const unsigned char* image, int Wt, int Ht, int levels, uint32_t* mips) {
    const size_t texels = (size_t)Wt * Ht;
    for (size_t i = 0; i < texels; ++i) mips[i] = tx_pack(image[i * 3 + 0], image[i * 3 + 1], image[i * 3 + 2]);
    int sw = Wt, sh = Ht;
    uint32_t* src = mips;
    for (int l = 1; l < levels; ++l) {
        const int dw = tx_half(sw), dh = tx_half(sh);
        uint32_t* dst = src + (size_t)sw * sh;
        for (int y = 0; y < dh; ++y)
            for (int x = 0; x < dw; ++x) dst[(size_t)y * dw + x] = tx_box(src, sw, sh, x, y);
        src = dst;
        sw = dw;
        sh = dh;
    }
}

int render_color_textured_host(const double* poses, int P, const double* vertices, int n, const int* faces, int F,
                               const ColorTexture& tex, const int* image_index, int I, const double* K, int H, int W,
                               double pixel_center, double near, double ambient, const double* light, int accumulate,
                               unsigned char* color, float* depth, int* skipped) {
    for (int i = 0; i < F * 3; ++i)
        if (faces[i] < 0 || faces[i] >= n) return -1;
    const RsCam cam = raster_cam(K, pixel_center, near);
    const ColorLight lt{ambient, light[0], light[1], light[2]};
    const size_t HW = (size_t)H * W;
    std::vector<unsigned long long> keys((size_t)I * HW);
    color_visibility_host(poses, P, vertices, n, faces, F, image_index, I, cam, H, W, accumulate, depth, keys.data(), skipped);
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
                tx_shade(cam, A, B, C, tex.uv + (size_t)f * 6, tex.mips, tex.Wt, tex.Ht, tex.levels, x, y, lt, color + at * 3);
                const uint32_t bits = (uint32_t)(key >> 32);
                std::memcpy(&depth[at], &bits, 4);
            }
    return 0;
}

}  // namespace bp
