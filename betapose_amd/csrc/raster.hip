// Depth images of a triangle mesh at many poses (include/betapose_hip.h bp_render_depth; the renders of bp_vsd_errors).
// The arithmetic of one vertex, one triangle and one pixel is raster_math.inc and the walk over a pose's triangles and
// their pixels is raster_walk.inc, texts the host twin (raster_host.cpp) and the colour renderer compile too; here is what
// is launched:
//   1. raster_transform_kernel, one lane per (pose, vertex): camera-space xyz (f64) and the projection snapped to
//      1/256 px, into a per-call workspace.  A vertex shared by six triangles is transformed and divided once.
//   2. raster_tri_kernel, one lane per (pose, triangle): rs_walk with the z-buffer as its sink.
// The z-buffer is a minimum over f32 bit patterns (positive floats order as unsigned integers) by atomicMin on global
// memory.  A minimum does not depend on the order of its operands, so the image is the same whatever the scheduling, and
// equal to the host twin's bit for bit.  A face index outside [0, n) or a vertex that failed the near / range test skips
// the triangle and counts it in skipped[pose].
#include "bp_common.h"
#include "raster.h"

#pragma clang fp contract(off)

namespace bp {

namespace {

#include "raster_math.inc"
#define RS_WALK_DEVICE      // the kernels' walk too, not only the host's
#include "raster_walk.inc"

constexpr int RS_THREADS = 256;

__device__ __forceinline__ const double* rs_pose(const double* a, int na, const double* b, int q) {
    return q < na ? a + (size_t)q * 12 : b + (size_t)(q - na) * 12;
}

__global__ __launch_bounds__(RS_THREADS) void raster_transform_kernel(const double* __restrict__ model, int n,
                                                                      const double* __restrict__ poses_a, int na,
                                                                      const double* __restrict__ poses_b, int poses, RsCam cam,
                                                                      double* __restrict__ xyz, int* __restrict__ uv) {
    const int i = blockIdx.x * RS_THREADS + threadIdx.x;
    if (i >= n) return;
    const double x = model[(size_t)i * 3 + 0], y = model[(size_t)i * 3 + 1], z = model[(size_t)i * 3 + 2];
    for (int q = blockIdx.y; q < poses; q += gridDim.y) {
        const double* pose = rs_pose(poses_a, na, poses_b, q);
        double X[3];
        int sx, sy;
        rs_transform(pose, x, y, z, X);
        rs_project(cam, X, &sx, &sy);
        double* o = xyz + ((size_t)q * n + i) * 3;
        o[0] = X[0];
        o[1] = X[1];
        o[2] = X[2];
        int* s = uv + ((size_t)q * n + i) * 2;
        s[0] = sx;
        s[1] = sy;
    }
}

struct DepthSink {      // smaller bits win
    uint32_t* __restrict__ zb;
    __device__ __forceinline__ void operator()(size_t at, uint32_t bits, int) const { atomicMin(&zb[at], bits); }
};

__global__ __launch_bounds__(RS_THREADS) void raster_tri_kernel(const int* __restrict__ faces, int F, int n,
                                                                const double* __restrict__ xyz, const int* __restrict__ uv,
                                                                int poses, RsCam cam, int H, int W, uint32_t* __restrict__ zbuf,
                                                                int* __restrict__ skipped) {
    const RsFace face = rs_face(faces, F, blockIdx.x * RS_THREADS + threadIdx.x);
    for (int q = blockIdx.y; q < poses; q += gridDim.y)     // (uniform over the block: the walk's ballots see whole waves)
        rs_walk(cam, face, F, n, xyz + (size_t)q * n * 3, uv + (size_t)q * n * 2, H, W, skipped + q,
                DepthSink{zbuf + (size_t)q * H * W});
}

__global__ __launch_bounds__(RS_THREADS) void raster_finish_kernel(uint32_t* __restrict__ zbuf, size_t count) {
    for (size_t i = (size_t)blockIdx.x * RS_THREADS + threadIdx.x; i < count; i += (size_t)gridDim.x * RS_THREADS)
        if (zbuf[i] == RS_EMPTY) zbuf[i] = 0u;
}

}  // namespace

size_t raster_vertex_bytes(int n, int poses) { return (size_t)poses * n * (3 * sizeof(double) + 2 * sizeof(int)); }

void launch_raster_transform(const double* model, int n, const double* poses_a, int na, const double* poses_b, int nb,
                             const RsCam& cam, void* vertex_ws, hipStream_t s) {
    const int poses = na + nb;
    double* xyz = (double*)vertex_ws;
    int* uv = (int*)(xyz + (size_t)poses * n * 3);
    const int gy = poses < 65535 ? poses : 65535;
    hipLaunchKernelGGL(raster_transform_kernel, dim3((n + RS_THREADS - 1) / RS_THREADS, gy), dim3(RS_THREADS), 0, s, model, n,
                       poses_a, na, poses_b, poses, cam, xyz, uv);
}

void launch_raster(const double* model, int n, const int* faces, int F, const double* poses_a, int na, const double* poses_b,
                   int nb, const RsCam& cam, int H, int W, void* vertex_ws, uint32_t* zbuf, int* skipped, hipStream_t s) {
    launch_raster_transform(model, n, poses_a, na, poses_b, nb, cam, vertex_ws, s);
    const int poses = na + nb;
    const double* xyz = (const double*)vertex_ws;
    const int gy = poses < 65535 ? poses : 65535;
    hipLaunchKernelGGL(raster_tri_kernel, dim3((F + RS_THREADS - 1) / RS_THREADS, gy), dim3(RS_THREADS), 0, s, faces, F, n, xyz,
                       (const int*)(xyz + (size_t)poses * n * 3), poses, cam, H, W, zbuf, skipped);
}

void launch_raster_finish(uint32_t* zbuf, size_t count, hipStream_t s) {
    size_t blocks = (count + RS_THREADS - 1) / RS_THREADS;
    if (blocks > 65535) blocks = 65535;
    hipLaunchKernelGGL(raster_finish_kernel, dim3((unsigned)blocks), dim3(RS_THREADS), 0, s, zbuf, count);
}

}  // namespace bp
