// BOP's Visible Surface Discrepancy of P (ground-truth, estimated) pose pairs (include/betapose_hip.h bp_vsd_errors): the
// reduction over the two renders of a pair (raster.hip) and its test depth image.  It restates metrics.vsd_err, the numpy
// host definition, per pixel in f64 with the same operations in the same order:
//     dist    = z * sqrt(((x + c - cx) / fx)^2 + ((y + c - cy) / fy)^2 + 1)          (0 stays 0)
//     vis_gt  = dist_gt > 0 and (dist_gt - dist_test <= delta or dist_test == 0)
//     vis_est = the same for the estimate, or (vis_gt and dist_est > 0)
//     e(tau)  = (#{inter : |dist_gt - dist_est| / diameter >= tau} + union - inter) / union,   1 when union == 0
// Only INTEGER counts are accumulated -- rendered_gt, vis_gt, inter, union and one count per tau: per lane, by a wave
// shuffle tree, over the waves of a block in LDS, and over the pixel slices of a pair by integer atomicAdd.  Integer sums
// do not depend on their order, and the one division per (pair, tau) happens at the end (vsd_finish_kernel), so the
// results are bit-identical between calls, streams and chunk sizes.
#include "bp_common.h"
#include "raster.h"

#pragma clang fp contract(off)

namespace bp {

namespace {

constexpr int VSD_THREADS = 256;
constexpr int VSD_PIX = VSD_THREADS * 16;       // pixels per block
constexpr uint32_t VSD_EMPTY = 0x7f800000u;     // the z-buffer's cleared value (raster_math.inc RS_EMPTY)

struct VsdCam {
    double fx, fy, cx, cy, c;
};

__global__ __launch_bounds__(VSD_THREADS) void vsd_reduce_kernel(const uint32_t* __restrict__ zbuf, int pairs,
                                                                 const uint16_t* __restrict__ depth_test, int T,
                                                                 const int* __restrict__ test_index, int H, int W, VsdCam cam,
                                                                 double depth_scale, double delta, VsdTaus taus, int n_tau,
                                                                 double diameter, int* __restrict__ acc) {
    __shared__ int part[VSD_THREADS / 64][VSD_ACC];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int HW = H * W;                        // <= 2^24
    const int i0 = blockIdx.x * VSD_PIX, i1 = min(HW, i0 + VSD_PIX);
    for (int p = blockIdx.y; p < pairs; p += gridDim.y) {   // (uniform over the block)
        const int ti = test_index[p];
        if ((unsigned)ti >= (unsigned)T) continue;          // vsd_finish_kernel reports it
        const uint32_t* zg = zbuf + (size_t)p * HW;
        const uint32_t* ze = zbuf + ((size_t)pairs + p) * HW;
        const uint16_t* zt = depth_test + (size_t)ti * HW;
        int c[VSD_ACC];
#pragma unroll
        for (int k = 0; k < VSD_ACC; ++k) c[k] = 0;
        for (int i = i0 + tid; i < i1; i += VSD_THREADS) {
            const int y = i / W, x = i - y * W;
            const uint32_t bg = zg[i], be = ze[i];
            const double z_gt = bg == VSD_EMPTY ? 0.0 : (double)__uint_as_float(bg);
            const double z_est = be == VSD_EMPTY ? 0.0 : (double)__uint_as_float(be);
            const double z_test = (double)zt[i] * depth_scale;
            const double a = (((double)x + cam.c) - cam.cx) / cam.fx;
            const double b = (((double)y + cam.c) - cam.cy) / cam.fy;
            const double r = sqrt((a * a + b * b) + 1.0);
            const double d_gt = z_gt * r, d_est = z_est * r, d_test = z_test * r;
            const bool vis_gt = d_gt > 0.0 && ((d_gt - d_test <= delta) || d_test == 0.0);
            const bool vis_est = (d_est > 0.0 && ((d_est - d_test <= delta) || d_test == 0.0)) || (vis_gt && d_est > 0.0);
            const bool inter = vis_gt && vis_est;
            c[0] += d_gt > 0.0;
            c[1] += vis_gt;
            c[2] += inter;
            c[3] += vis_gt || vis_est;
            const double rel = fabs(d_gt - d_est) / diameter;
#pragma unroll
            for (int k = 0; k < VSD_MAX_TAUS; ++k) c[4 + k] += (k < n_tau && inter && rel >= taus.tau[k]);
        }
#pragma unroll
        for (int k = 0; k < VSD_ACC; ++k) {
            int v = c[k];
            for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
            if (lane == 0) part[wave][k] = v;
        }
        __syncthreads();
        if (tid < VSD_ACC) {
            int v = 0;
            for (int w = 0; w < VSD_THREADS / 64; ++w) v += part[w][tid];
            if (v) atomicAdd(&acc[(size_t)p * VSD_ACC + tid], v);
        }
        __syncthreads();   // part is rewritten for the next pair
    }
}

__global__ __launch_bounds__(64) void vsd_finish_kernel(const int* __restrict__ acc, const int* __restrict__ test_index, int T,
                                                        int P, int n_tau, double* __restrict__ err, int* __restrict__ counts) {
    const int p = blockIdx.x * 64 + threadIdx.x;
    if (p >= P) return;
    const int* a = acc + (size_t)p * VSD_ACC;
    const bool ok = (unsigned)test_index[p] < (unsigned)T;
    for (int k = 0; k < 4; ++k) counts[(size_t)p * 4 + k] = ok ? a[k] : -1;
    const int inter = a[2], uni = a[3];
    for (int k = 0; k < n_tau; ++k) {
        double e = 1.0;
        if (uni > 0) e = (double)(a[4 + k] + (uni - inter)) / (double)uni;
        err[(size_t)p * n_tau + k] = ok ? e : __builtin_nan("");
    }
}

}  // namespace

void launch_vsd_reduce(const uint32_t* zbuf, int pairs, const uint16_t* depth_test, int T, const int* test_index, int H, int W,
                       const double* K, double pixel_center, double depth_scale, double delta, const VsdTaus& taus, int n_tau,
                       double diameter, int* acc, hipStream_t s) {
    const VsdCam cam{K[0], K[4], K[2], K[5], pixel_center};
    const int slices = (H * W + VSD_PIX - 1) / VSD_PIX;
    hipLaunchKernelGGL(vsd_reduce_kernel, dim3(slices, pairs < 65535 ? pairs : 65535), dim3(VSD_THREADS), 0, s, zbuf, pairs,
                       depth_test, T, test_index, H, W, cam, depth_scale, delta, taus, n_tau, diameter, acc);
}

void launch_vsd_finish(const int* acc, const int* test_index, int T, int P, int n_tau, double* err, int* counts, hipStream_t s) {
    hipLaunchKernelGGL(vsd_finish_kernel, dim3((P + 63) / 64), dim3(64), 0, s, acc, test_index, T, P, n_tau, err, counts);
}

}  // namespace bp
