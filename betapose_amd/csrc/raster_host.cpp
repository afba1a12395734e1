// Host twin of the depth rasteriser (include/betapose_hip.h bp_render_depth_host): plain loops over poses, triangles and
// the pixels of each clamped bounding box around the arithmetic of raster_math.inc, the text raster.hip compiles too.  The
// z-buffer is a minimum over f32 bit patterns, which does not depend on the order the triangles are drawn in, so this
// image and the kernel's are equal bit for bit.
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
}  // namespace

int render_depth_host(const double* poses, int P, const double* vertices, int n, const int* faces, int F, const double* K,
                      int H, int W, double pixel_center, double near, float* depth, int* skipped) {
    for (int i = 0; i < F * 3; ++i)
        if (faces[i] < 0 || faces[i] >= n) return -1;
    const RsCam cam{K[0], K[4], K[2], K[5], pixel_center, near};
    const size_t HW = (size_t)H * W;
    std::vector<double> X((size_t)n * 3);
    std::vector<int> S((size_t)n * 2);
    std::vector<uint32_t> zbuf(HW);
    for (int p = 0; p < P; ++p) {
        const double* pose = poses + (size_t)p * 12;
        for (int i = 0; i < n; ++i) {
            rs_transform(pose, vertices[i * 3 + 0], vertices[i * 3 + 1], vertices[i * 3 + 2], &X[(size_t)i * 3]);
            rs_project(cam, &X[(size_t)i * 3], &S[(size_t)i * 2], &S[(size_t)i * 2 + 1]);
        }
        std::fill(zbuf.begin(), zbuf.end(), RS_EMPTY);
        int skip = 0;
        for (int f = 0; f < F; ++f) {
            const int a = faces[f * 3 + 0], b = faces[f * 3 + 1], c = faces[f * 3 + 2];
            if (S[a * 2] == RS_INVALID || S[b * 2] == RS_INVALID || S[c * 2] == RS_INVALID) {
                ++skip;
                continue;
            }
            RsTri t;
            if (!rs_setup(&X[(size_t)a * 3], &X[(size_t)b * 3], &X[(size_t)c * 3], S[a * 2], S[a * 2 + 1], S[b * 2],
                          S[b * 2 + 1], S[c * 2], S[c * 2 + 1], H, W, &t))
                continue;
            for (int y = t.by0; y <= t.by1; ++y)
                for (int x = t.bx0; x <= t.bx1; ++x) {
                    if (!rs_covers(t, x, y)) continue;
                    const uint32_t bits = rs_depth_bits(cam, t, x, y);
                    uint32_t& dst = zbuf[(size_t)y * W + x];
                    if (bits < dst) dst = bits;
                }
        }
        skipped[p] = skip;
        float* out = depth + (size_t)p * HW;
        for (size_t i = 0; i < HW; ++i) {
            const uint32_t bits = zbuf[i] == RS_EMPTY ? 0u : zbuf[i];
            std::memcpy(&out[i], &bits, 4);
        }
    }
    return 0;
}

}  // namespace bp
