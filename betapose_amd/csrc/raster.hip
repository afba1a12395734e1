// Depth images of a triangle mesh at many poses (include/betapose_hip.h bp_render_depth; the renders of bp_vsd_errors).
// The arithmetic of one vertex, one triangle and one pixel is raster_math.inc, the text the host twin (raster_host.cpp)
// compiles too; here is who loops over what:
//   1. raster_transform_kernel, one lane per (pose, vertex): camera-space xyz (f64) and the projection snapped to
//      1/256 px, into a per-call workspace.  A vertex shared by six triangles is transformed and divided once.
//   2. raster_tri_kernel, one lane per (pose, triangle).  A LineMod-sized mesh gives tens of thousands of triangles of
//      1-4 px per pose: the lane walks its clamped bounding box alone.  A triangle whose box holds more than RS_COOP_AREA
//      pixels (a close-up box: 12 triangles over the whole frame) is left for the wave: the big lanes are collected with
//      __ballot, each one's set-up is broadcast with __shfl and the box's pixels are strided over the 64 lanes.  No
//      worklist, no second launch.
// The z-buffer is a minimum over f32 bit patterns (positive floats order as unsigned integers) by atomicMin on global
// memory.  A minimum does not depend on the order of its operands, so the image is the same whatever the scheduling, and
// equal to the host twin's bit for bit.  Every pixel loop runs over a box that rs_setup has clamped to the image, so
// every store index is in range by construction; a face index outside [0, n) or a vertex that failed the near / range
// test skips the triangle and counts it in skipped[pose].
#include "bp_common.h"
#include "raster.h"

#pragma clang fp contract(off)

namespace bp {

namespace {

#include "raster_math.inc"

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

__device__ __forceinline__ void rs_draw(const RsCam& cam, const RsTri& t, int x, int y, int W, uint32_t* __restrict__ zb) {
    if (rs_covers(t, x, y)) atomicMin(&zb[(size_t)y * W + x], rs_depth_bits(cam, t, x, y));
}

__global__ __launch_bounds__(RS_THREADS) void raster_tri_kernel(const int* __restrict__ faces, int F, int n,
                                                                const double* __restrict__ xyz, const int* __restrict__ uv,
                                                                int poses, RsCam cam, int H, int W, uint32_t* __restrict__ zbuf,
                                                                int* __restrict__ skipped) {
    const int f = blockIdx.x * RS_THREADS + threadIdx.x;
    const int lane = threadIdx.x & 63;
    int ia = -1, ib = -1, ic = -1;
    if (f < F) {
        ia = faces[(size_t)f * 3 + 0];
        ib = faces[(size_t)f * 3 + 1];
        ic = faces[(size_t)f * 3 + 2];
    }
    const bool in_range = (unsigned)ia < (unsigned)n && (unsigned)ib < (unsigned)n && (unsigned)ic < (unsigned)n;
    for (int q = blockIdx.y; q < poses; q += gridDim.y) {   // (uniform over the block: the ballots below see whole waves)
        const double* X = xyz + (size_t)q * n * 3;
        const int* S = uv + (size_t)q * n * 2;
        uint32_t* zb = zbuf + (size_t)q * H * W;
        RsTri t = {};
        int have = 0, skip = 0;
        if (f < F) {
            if (!in_range) {
                skip = 1;
            } else {
                const int ax = S[(size_t)ia * 2], ay = S[(size_t)ia * 2 + 1];
                const int bx = S[(size_t)ib * 2], by = S[(size_t)ib * 2 + 1];
                const int cx = S[(size_t)ic * 2], cy = S[(size_t)ic * 2 + 1];
                if (ax == RS_INVALID || bx == RS_INVALID || cx == RS_INVALID) {
                    skip = 1;
                } else {
                    double A[3], B[3], C[3];
#pragma unroll
                    for (int k = 0; k < 3; ++k) {
                        A[k] = X[(size_t)ia * 3 + k];
                        B[k] = X[(size_t)ib * 3 + k];
                        C[k] = X[(size_t)ic * 3 + k];
                    }
                    have = rs_setup(A, B, C, ax, ay, bx, by, cx, cy, H, W, &t);
                }
            }
        }
        const unsigned long long sk = __ballot(skip);
        if (lane == 0 && sk) atomicAdd(&skipped[q], (int)__popcll(sk));

        int big = 0;
        if (have) {
            const int w = t.bx1 - t.bx0 + 1, h = t.by1 - t.by0 + 1;   // w * h <= H * W <= 2^24
            if (w * h > RS_COOP_AREA) {
                big = 1;
            } else {
                for (int y = t.by0; y <= t.by1; ++y)
                    for (int x = t.bx0; x <= t.bx1; ++x) rs_draw(cam, t, x, y, W, zb);
            }
        }
        // the wave takes its big triangles one after the other, 64 pixels of the box at a time
        unsigned long long todo = __ballot(big);
        while (todo) {
            const int src = __ffsll((long long)todo) - 1;
            todo &= todo - 1;
            RsTri u;
            u.x0 = __shfl(t.x0, src, 64); u.y0 = __shfl(t.y0, src, 64);
            u.x1 = __shfl(t.x1, src, 64); u.y1 = __shfl(t.y1, src, 64);
            u.x2 = __shfl(t.x2, src, 64); u.y2 = __shfl(t.y2, src, 64);
            u.bx0 = __shfl(t.bx0, src, 64); u.by0 = __shfl(t.by0, src, 64);
            u.bx1 = __shfl(t.bx1, src, 64); u.by1 = __shfl(t.by1, src, 64);
            u.nx = __shfl(t.nx, src, 64); u.ny = __shfl(t.ny, src, 64);
            u.nz = __shfl(t.nz, src, 64); u.nd = __shfl(t.nd, src, 64);
            u.zmin = __shfl(t.zmin, src, 64); u.zmax = __shfl(t.zmax, src, 64);
            const int w = u.bx1 - u.bx0 + 1, cnt = w * (u.by1 - u.by0 + 1);
            for (int k = lane; k < cnt; k += 64) rs_draw(cam, u, u.bx0 + k % w, u.by0 + k / w, W, zb);
        }
    }
}

__global__ __launch_bounds__(RS_THREADS) void raster_finish_kernel(uint32_t* __restrict__ zbuf, size_t count) {
    for (size_t i = (size_t)blockIdx.x * RS_THREADS + threadIdx.x; i < count; i += (size_t)gridDim.x * RS_THREADS)
        if (zbuf[i] == RS_EMPTY) zbuf[i] = 0u;
}

}  // namespace

size_t raster_vertex_bytes(int n, int poses) { return (size_t)poses * n * (3 * sizeof(double) + 2 * sizeof(int)); }

void launch_raster(const double* model, int n, const int* faces, int F, const double* poses_a, int na, const double* poses_b,
                   int nb, const double* K, int H, int W, double pixel_center, double near, void* vertex_ws, uint32_t* zbuf,
                   int* skipped, hipStream_t s) {
    const RsCam cam{K[0], K[4], K[2], K[5], pixel_center, near};
    const int poses = na + nb;
    double* xyz = (double*)vertex_ws;
    int* uv = (int*)(xyz + (size_t)poses * n * 3);
    const int gy = poses < 65535 ? poses : 65535;
    hipLaunchKernelGGL(raster_transform_kernel, dim3((n + RS_THREADS - 1) / RS_THREADS, gy), dim3(RS_THREADS), 0, s, model, n,
                       poses_a, na, poses_b, poses, cam, xyz, uv);
    hipLaunchKernelGGL(raster_tri_kernel, dim3((F + RS_THREADS - 1) / RS_THREADS, gy), dim3(RS_THREADS), 0, s, faces, F, n, xyz,
                       uv, poses, cam, H, W, zbuf, skipped);
}

void launch_raster_transform(const double* model, int n, const double* poses, int count, const double* K, double pixel_center,
                             double near, void* vertex_ws, hipStream_t s) {
    const RsCam cam{K[0], K[4], K[2], K[5], pixel_center, near};
    double* xyz = (double*)vertex_ws;
    int* uv = (int*)(xyz + (size_t)count * n * 3);
    const int gy = count < 65535 ? count : 65535;
    hipLaunchKernelGGL(raster_transform_kernel, dim3((n + RS_THREADS - 1) / RS_THREADS, gy), dim3(RS_THREADS), 0, s, model, n,
                       poses, count, (const double*)nullptr, count, cam, xyz, uv);
}

void launch_raster_finish(uint32_t* zbuf, size_t count, hipStream_t s) {
    size_t blocks = (count + RS_THREADS - 1) / RS_THREADS;
    if (blocks > 65535) blocks = 65535;
    hipLaunchKernelGGL(raster_finish_kernel, dim3((unsigned)blocks), dim3(RS_THREADS), 0, s, zbuf, count);
}

}  // namespace bp
