// Host twin of the depth rasteriser (include/betapose_hip.h bp_render_depth_host): a loop over poses round rs_walk_host
// (raster_walk.inc, the walk raster.hip and the colour renderer compile too) with the z-buffer as its sink.  The z-buffer
// is a minimum over f32 bit patterns, which does not depend on the order the triangles are drawn in, so this image and
// the kernel's are equal bit for bit.
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
}  // namespace

int render_depth_host(const double* poses, int P, const double* vertices, int n, const int* faces, int F, const double* K,
                      int H, int W, double pixel_center, double near, float* depth, int* skipped) {
    for (int i = 0; i < F * 3; ++i)
        if (faces[i] < 0 || faces[i] >= n) return -1;
    const RsCam cam = raster_cam(K, pixel_center, near);
    const size_t HW = (size_t)H * W;
    std::vector<double> X((size_t)n * 3);
    std::vector<int> S((size_t)n * 2);
    std::vector<uint32_t> zbuf(HW);
    for (int p = 0; p < P; ++p) {
        std::fill(zbuf.begin(), zbuf.end(), RS_EMPTY);
        skipped[p] = rs_walk_host(cam, poses + (size_t)p * 12, vertices, n, faces, F, H, W, X.data(), S.data(),
                                  [&](size_t at, uint32_t bits, int) {      // smaller bits win
                                      if (bits < zbuf[at]) zbuf[at] = bits;
                                  });
        float* out = depth + (size_t)p * HW;
        for (size_t i = 0; i < HW; ++i) {
            const uint32_t bits = zbuf[i] == RS_EMPTY ? 0u : zbuf[i];
            std::memcpy(&out[i], &bits, 4);
        }
    }
    return 0;
}

}  // namespace bp
