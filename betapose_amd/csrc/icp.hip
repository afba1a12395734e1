// Depth refinement of estimated poses on the GPU (include/betapose_hip.h bp_refine_depth, bp_icp_normal_equations):
// projective point-to-plane ICP of the mesh's render (raster.hip) against the test depth image.  The arithmetic of one
// pixel and of one step is icp_math.inc, the text the host twin (icp_host.cpp) compiles too; here is who loops over what:
//   1. icp_accumulate_kernel, one block per (pose, slice of ICP_PIX pixels).  A lane walks its pixels of the slice in
//      index order and keeps the 29 f64 sums of the normal equations (A's upper triangle, b, N, E) in registers; the
//      sums are reduced over the wave by a shuffle tree, over the block's waves in LDS in wave order, and ONE partial per
//      block is stored to the workspace [pose][slice][29].  No floating-point atomic anywhere: which lane sums which
//      pixel, the tree and the order of the waves are fixed by the image size alone, so two calls, two streams and two
//      chunk sizes give the same bits.
//   2. icp_step_kernel, one wave per pose: lanes 0 .. 28 sum their entry over the slices in index order, lane 0 applies
//      the guards, solve6 and rodrigues_exp and updates the pose row and the stats in device memory.
//   A pose whose status is final is skipped by both; the loop over the iterations is enqueued by the caller (c_api.cpp)
//   without a host round trip.
// Every load index is in range by construction: a pixel reads its four neighbours only when 1 <= x <= W - 2 and
// 1 <= y <= H - 2, a test image only for an index in [0, T).
#include "bp_common.h"
#include "icp.h"
#include "pose_tail.h"

#pragma clang fp contract(off)

namespace bp {

namespace {

#include "pnp_math.inc"
#include "icp_math.inc"

constexpr int ICP_THREADS = 256;
constexpr int ICP_PIX = ICP_THREADS * 8;        // pixels per block
constexpr uint32_t ICP_EMPTY = 0x7f800000u;     // the z-buffer's cleared value (raster_math.inc RS_EMPTY)

__device__ __forceinline__ double icp_z(uint32_t bits) { return bits == ICP_EMPTY ? 0.0 : (double)__uint_as_float(bits); }

__global__ __launch_bounds__(ICP_THREADS) void icp_accumulate_kernel(const uint32_t* __restrict__ zbuf,
                                                                     const double* __restrict__ poses, int P,
                                                                     const uint16_t* __restrict__ depth_test, int T,
                                                                     const int* __restrict__ test_index, int H, int W,
                                                                     IcpParams prm, const double* __restrict__ stats,
                                                                     double* __restrict__ partial) {
    __shared__ double part[ICP_THREADS / 64][ICP_ACC];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int HW = H * W;                        // <= 2^24
    const int i0 = blockIdx.x * ICP_PIX, i1 = min(HW, i0 + ICP_PIX);
    for (int p = blockIdx.y; p < P; p += gridDim.y) {       // (uniform over the block)
        const int ti = test_index[p];
        if ((unsigned)ti >= (unsigned)T) continue;
        if (stats && stats[(size_t)p * ICP_STATS + 5] != ICP_RUNNING) continue;
        const uint32_t* zb = zbuf + (size_t)p * HW;
        const uint16_t* zt = depth_test + (size_t)ti * HW;
        const double t[3] = {poses[(size_t)p * 12 + 3], poses[(size_t)p * 12 + 7], poses[(size_t)p * 12 + 11]};
        double acc[ICP_ACC];
#pragma unroll
        for (int k = 0; k < ICP_ACC; ++k) acc[k] = 0.0;
        for (int i = i0 + tid; i < i1; i += ICP_THREADS) {
            const int y = i / W, x = i - y * W;
            if (x < 1 || x > W - 2 || y < 1 || y > H - 2) continue;
            const uint32_t bc = zb[i];
            if (bc == ICP_EMPTY) continue;                  // (what icp_pixel decides for it, without the other loads)
            double J[6], r;
            if (icp_pixel(prm, x, y, icp_z(bc), icp_z(zb[i - 1]), icp_z(zb[i + 1]), icp_z(zb[i - W]), icp_z(zb[i + W]),
                          (double)zt[i] * prm.depth_scale, t, J, &r))
                icp_add(acc, J, r);
        }
#pragma unroll
        for (int k = 0; k < ICP_ACC; ++k) {
            double v = acc[k];
            for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
            if (lane == 0) part[wave][k] = v;
        }
        __syncthreads();
        if (tid < ICP_ACC) {
            double v = part[0][tid];
            for (int w = 1; w < ICP_THREADS / 64; ++w) v += part[w][tid];
            partial[((size_t)p * gridDim.x + blockIdx.x) * ICP_ACC + tid] = v;
        }
        __syncthreads();   // part is rewritten for the next pose
    }
}

// the slices of pose p summed in index order into sh[ICP_ACC]
__device__ __forceinline__ void icp_sum_slices(const double* __restrict__ partial, int p, int slices, double* sh) {
    const int tid = threadIdx.x;
    if (tid < ICP_ACC) {
        const double* src = partial + (size_t)p * slices * ICP_ACC + tid;
        double v = src[0];
        for (int s = 1; s < slices; ++s) v += src[(size_t)s * ICP_ACC];
        sh[tid] = v;
    }
    __syncthreads();
}

__global__ __launch_bounds__(64) void icp_init_kernel(const double* __restrict__ poses_in, const int* __restrict__ test_index,
                                                      int T, int P, double* __restrict__ poses, double* __restrict__ stats) {
    const int p = blockIdx.x * 64 + threadIdx.x;
    if (p >= P) return;
    icp_init(poses_in + (size_t)p * 12, (unsigned)test_index[p] < (unsigned)T, poses + (size_t)p * 12,
             stats + (size_t)p * ICP_STATS);
}

__global__ __launch_bounds__(64) void icp_sum_kernel(const double* __restrict__ partial, const int* __restrict__ test_index,
                                                     int T, int slices, double* __restrict__ out) {
    __shared__ double sh[ICP_ACC];
    const int p = blockIdx.x;
    if ((unsigned)test_index[p] >= (unsigned)T) {           // (uniform over the block)
        if (threadIdx.x < ICP_ACC) out[(size_t)p * ICP_ACC + threadIdx.x] = 0.0;
        return;
    }
    icp_sum_slices(partial, p, slices, sh);
    if (threadIdx.x < ICP_ACC) out[(size_t)p * ICP_ACC + threadIdx.x] = sh[threadIdx.x];
}

__global__ __launch_bounds__(64) void icp_step_kernel(const double* __restrict__ partial, int slices, int k, IcpParams prm,
                                                      const double* __restrict__ poses_in, double* __restrict__ poses,
                                                      double* __restrict__ stats) {
    __shared__ double sh[ICP_ACC];
    const int p = blockIdx.x;
    if (stats[(size_t)p * ICP_STATS + 5] != ICP_RUNNING) return;   // (uniform over the block)
    icp_sum_slices(partial, p, slices, sh);
    if (threadIdx.x != 0) return;
    double acc[ICP_ACC], pose[12], st[ICP_STATS];
#pragma unroll
    for (int i = 0; i < ICP_ACC; ++i) acc[i] = sh[i];
#pragma unroll
    for (int i = 0; i < 12; ++i) pose[i] = poses[(size_t)p * 12 + i];
#pragma unroll
    for (int i = 0; i < ICP_STATS; ++i) st[i] = stats[(size_t)p * ICP_STATS + i];
    icp_step(acc, k, prm, poses_in + (size_t)p * 12, pose, st);
#pragma unroll
    for (int i = 0; i < 12; ++i) poses[(size_t)p * 12 + i] = pose[i];
#pragma unroll
    for (int i = 0; i < ICP_STATS; ++i) stats[(size_t)p * ICP_STATS + i] = st[i];
}

}  // namespace

int icp_slices(int H, int W) { return (H * W + ICP_PIX - 1) / ICP_PIX; }

void launch_icp_init(const double* poses_in, const int* test_index, int T, int P, double* poses_out, double* stats,
                     hipStream_t s) {
    hipLaunchKernelGGL(icp_init_kernel, dim3((P + 63) / 64), dim3(64), 0, s, poses_in, test_index, T, P, poses_out, stats);
}

void launch_icp_accumulate(const uint32_t* zbuf, const double* poses, int P, const uint16_t* depth_test, int T,
                           const int* test_index, int H, int W, const IcpParams& prm, const double* stats, double* partial,
                           hipStream_t s) {
    hipLaunchKernelGGL(icp_accumulate_kernel, dim3(icp_slices(H, W), P < 65535 ? P : 65535), dim3(ICP_THREADS), 0, s, zbuf,
                       poses, P, depth_test, T, test_index, H, W, prm, stats, partial);
}

void launch_icp_sum(const double* partial, const int* test_index, int T, int P, int slices, double* out, hipStream_t s) {
    hipLaunchKernelGGL(icp_sum_kernel, dim3(P), dim3(64), 0, s, partial, test_index, T, slices, out);
}

void launch_icp_step(const double* partial, int P, int slices, int k, const IcpParams& prm, const double* poses_in,
                     double* poses, double* stats, hipStream_t s) {
    hipLaunchKernelGGL(icp_step_kernel, dim3(P), dim3(64), 0, s, partial, slices, k, prm, poses_in, poses, stats);
}

}  // namespace bp
