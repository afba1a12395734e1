// Host twin of the depth refinement (include/betapose_hip.h bp_refine_depth_host, bp_icp_normal_equations_host): plain
// loops over poses, iterations and pixels around the arithmetic of icp_math.inc, the text icp.hip compiles too, over the
// host renderer (raster_host.cpp).  Every pixel's decision and term has the device's bits; the terms are summed here in
// row-major pixel order, on the device lane by lane, so the sums agree to the rounding of an f64 sum.
#include <cmath>
#include <cstdint>
#include <vector>

#include "icp.h"
#include "pose_tail.h"
#include "raster.h"

#pragma clang fp contract(off)

namespace bp {

namespace {
#include "pnp_math.inc"
#include "icp_math.inc"

// acc[ICP_ACC] = the normal equations of one render [H][W] (0 = nothing drawn) against one test image
void accumulate(const float* depth, const uint16_t* test, int H, int W, const IcpParams& prm, const double* pose, double* acc) {
    for (int k = 0; k < ICP_ACC; ++k) acc[k] = 0.0;
    const double t[3] = {pose[3], pose[7], pose[11]};
    for (int y = 1; y < H - 1; ++y)
        for (int x = 1; x < W - 1; ++x) {
            const size_t i = (size_t)y * W + x;
            double J[6], r;
            if (icp_pixel(prm, x, y, (double)depth[i], (double)depth[i - 1], (double)depth[i + 1], (double)depth[i - W],
                          (double)depth[i + W], (double)test[i] * prm.depth_scale, t, J, &r))
                icp_add(acc, J, r);
        }
}

}  // namespace

int icp_normal_equations_host(const double* poses, int P, const double* vertices, int n, const int* faces, int F,
                              const double* K, const uint16_t* depth_test, int T, const int* test_index, int H, int W,
                              const IcpParams& prm, double near, double* out) {
    const size_t HW = (size_t)H * W;
    std::vector<float> depth(HW);
    int skipped;
    for (int p = 0; p < P; ++p) {
        double* acc = out + (size_t)p * ICP_ACC;
        for (int k = 0; k < ICP_ACC; ++k) acc[k] = 0.0;
        if (render_depth_host(poses + (size_t)p * 12, 1, vertices, n, faces, F, K, H, W, prm.c, near, depth.data(), &skipped))
            return -1;
        const int ti = test_index[p];
        if (ti < 0 || ti >= T) continue;
        accumulate(depth.data(), depth_test + (size_t)ti * HW, H, W, prm, poses + (size_t)p * 12, acc);
    }
    return 0;
}

int refine_depth_host(const double* poses, int P, const double* vertices, int n, const int* faces, int F, const double* K,
                      const uint16_t* depth_test, int T, const int* test_index, int H, int W, const IcpParams& prm, double near,
                      double* poses_out, double* stats) {
    for (int i = 0; i < F * 3; ++i)
        if (faces[i] < 0 || faces[i] >= n) return -1;
    const size_t HW = (size_t)H * W;
    std::vector<float> depth(HW);
    int skipped;
    double acc[ICP_ACC];
    for (int p = 0; p < P; ++p) {
        const double* in = poses + (size_t)p * 12;
        double* pose = poses_out + (size_t)p * 12;
        double* st = stats + (size_t)p * ICP_STATS;
        const int ti = test_index[p];
        icp_init(in, ti >= 0 && ti < T, pose, st);
        for (int k = 0; k <= prm.iterations && st[5] == ICP_RUNNING; ++k) {
            render_depth_host(pose, 1, vertices, n, faces, F, K, H, W, prm.c, near, depth.data(), &skipped);
            accumulate(depth.data(), depth_test + (size_t)ti * HW, H, W, prm, pose, acc);
            icp_step(acc, k, prm, in, pose, st);
        }
    }
    return 0;
}

}  // namespace bp
