// Pose errors of P (ground-truth, estimated) pose pairs of one model, f64 (include/betapose_hip.h bp_pose_errors):
// ADD (utils/metrics.py:10-22), ADD-S -- the closest-point form the reference keeps commented out (:23-33), here over
// every vertex -- and the 2-D projection error (:99-127).
//
// Work happens in the ground-truth object frame: with R = R_g^T R_e, t = R_g^T (t_e - t_g) the ADD-S of a query vertex
// x_i is min_j |x_i - (R x_j + t)|, the same distance as in the camera frame, but the coordinates stay object-sized
// (~0.1 m), so the squared differences lose less.  A block owns PE_THREADS * PE_Q query vertices of one pose (grid.y,
// looped beyond its limit); the candidates stream through LDS in SoA tiles of PE_TILE points, double-buffered, each
// transformed once on its way in.  Every lane reads the same candidate (LDS broadcast), so a (query, candidate) pair
// costs three subtractions, one multiply, two FMAs and a min on the squared distance; the square root is taken once per
// query.  ADD and 2-D ride along (O(n) per pose).  Sums are deterministic: per thread in query order, wave tree, waves
// in order, one partial per (pose, block); pose_errors_finish adds a pose's partials in block order.  No atomics.
#include "bp_common.h"
#include "pose_tail.h"

namespace bp {

namespace {

constexpr int PE_THREADS = 256;
constexpr int PE_Q = 4;                 // query vertices per thread, in registers
constexpr int PE_TILE = 1024;           // candidates per LDS tile (3 x 8 KB, x2 buffers = 48 KB)
constexpr int PE_UNROLL = 8;            // candidates per step of the inner loop; PE_TILE is a multiple
constexpr double PE_FAR = 1e150;        // coordinate of the pad candidates past n: squared distance ~3e300, finite

struct PeCam {
    double k[9];
};

__device__ __forceinline__ double pe_wave_sum(double v) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    return v;   // lane 0 holds the sum
}

__global__ __launch_bounds__(PE_THREADS) void pose_errors_kernel(const double* __restrict__ model, int n,
                                                                 const double* __restrict__ gt,
                                                                 const double* __restrict__ est, int P, PeCam cam,
                                                                 int want, double* __restrict__ partial) {
    __shared__ __align__(16) double sx[2][PE_TILE];
    __shared__ __align__(16) double sy[2][PE_TILE];
    __shared__ __align__(16) double sz[2][PE_TILE];
    __shared__ double red[PE_THREADS / 64][3];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int ntile = (n + PE_TILE - 1) / PE_TILE;

    for (int p = blockIdx.y; p < P; p += gridDim.y) {
        const double* g = gt + (size_t)p * 12;
        const double* e = est + (size_t)p * 12;
        // relative pose in the ground-truth object frame ([R|t] row-major: element (r, c) at r * 4 + c)
        double R[9], t[3];
#pragma unroll
        for (int a = 0; a < 3; ++a) {
#pragma unroll
            for (int b = 0; b < 3; ++b) R[a * 3 + b] = g[a] * e[b] + g[4 + a] * e[4 + b] + g[8 + a] * e[8 + b];
            t[a] = g[a] * (e[3] - g[3]) + g[4 + a] * (e[7] - g[7]) + g[8 + a] * (e[11] - g[11]);
        }

        double qx[PE_Q], qy[PE_Q], qz[PE_Q], best[PE_Q];
        double s_add = 0.0, s_2d = 0.0;
        const int base = blockIdx.x * PE_THREADS * PE_Q + tid;
#pragma unroll
        for (int q = 0; q < PE_Q; ++q) {
            const int i = base + q * PE_THREADS;
            const bool ok = i < n;
            qx[q] = ok ? model[(size_t)i * 3 + 0] : 0.0;
            qy[q] = ok ? model[(size_t)i * 3 + 1] : 0.0;
            qz[q] = ok ? model[(size_t)i * 3 + 2] : 0.0;
            best[q] = __builtin_inf();
            if (!ok) continue;
            if (want & 1) {
                const double dx = qx[q] - (R[0] * qx[q] + R[1] * qy[q] + R[2] * qz[q] + t[0]);
                const double dy = qy[q] - (R[3] * qx[q] + R[4] * qy[q] + R[5] * qz[q] + t[1]);
                const double dz = qz[q] - (R[6] * qx[q] + R[7] * qy[q] + R[8] * qz[q] + t[2]);
                s_add += sqrt(dx * dx + dy * dy + dz * dz);
            }
            if (want & 4) {
                // as the host: (K [R|t]) [x; 1] in the camera, then divided by its third row
                double ug[3], ue[3];
#pragma unroll
                for (int r = 0; r < 3; ++r) {
                    const double* kr = cam.k + r * 3;
                    double mg[4], me[4];
#pragma unroll
                    for (int c = 0; c < 4; ++c) {
                        mg[c] = kr[0] * g[c] + kr[1] * g[4 + c] + kr[2] * g[8 + c];
                        me[c] = kr[0] * e[c] + kr[1] * e[4 + c] + kr[2] * e[8 + c];
                    }
                    ug[r] = mg[0] * qx[q] + mg[1] * qy[q] + mg[2] * qz[q] + mg[3];
                    ue[r] = me[0] * qx[q] + me[1] * qy[q] + me[2] * qz[q] + me[3];
                }
                const double du = ug[0] / ug[2] - ue[0] / ue[2], dv = ug[1] / ug[2] - ue[1] / ue[2];
                s_2d += sqrt(du * du + dv * dv);
            }
        }

        if (want & 2) {
            // candidate tile `tile` -> LDS buffer `buf`, transformed into the ground-truth frame; pads past n are far away
            auto stage = [&](int tile, int buf) {
                for (int k = tid; k < PE_TILE; k += PE_THREADS) {
                    const int j = tile * PE_TILE + k;
                    double X = PE_FAR, Y = PE_FAR, Z = PE_FAR;
                    if (j < n) {
                        const double x = model[(size_t)j * 3 + 0], y = model[(size_t)j * 3 + 1], z = model[(size_t)j * 3 + 2];
                        X = R[0] * x + R[1] * y + R[2] * z + t[0];
                        Y = R[3] * x + R[4] * y + R[5] * z + t[1];
                        Z = R[6] * x + R[7] * y + R[8] * z + t[2];
                    }
                    sx[buf][k] = X;
                    sy[buf][k] = Y;
                    sz[buf][k] = Z;
                }
            };
            stage(0, 0);
            __syncthreads();
            for (int tl = 0; tl < ntile; ++tl) {
                const int buf = tl & 1;
                // the other buffer was last read in iteration tl - 1, which ended at a barrier
                if (tl + 1 < ntile) stage(tl + 1, buf ^ 1);
                const int cnt = min(PE_TILE, n - tl * PE_TILE);
                const int steps = (cnt + PE_UNROLL - 1) / PE_UNROLL;   // the rounded-up tail reads pads
                const double2* X2 = reinterpret_cast<const double2*>(sx[buf]);
                const double2* Y2 = reinterpret_cast<const double2*>(sy[buf]);
                const double2* Z2 = reinterpret_cast<const double2*>(sz[buf]);
                for (int s = 0; s < steps; ++s) {
#pragma unroll
                    for (int u = 0; u < PE_UNROLL / 2; ++u) {
                        const int k2 = s * (PE_UNROLL / 2) + u;
                        const double2 cx = X2[k2], cy = Y2[k2], cz = Z2[k2];
#pragma unroll
                        for (int q = 0; q < PE_Q; ++q) {
                            double dx = qx[q] - cx.x, dy = qy[q] - cy.x, dz = qz[q] - cz.x;
                            double d = dx * dx;
                            d = fma(dy, dy, d);
                            d = fma(dz, dz, d);
                            best[q] = fmin(best[q], d);
                            dx = qx[q] - cx.y;
                            dy = qy[q] - cy.y;
                            dz = qz[q] - cz.y;
                            d = dx * dx;
                            d = fma(dy, dy, d);
                            d = fma(dz, dz, d);
                            best[q] = fmin(best[q], d);
                        }
                    }
                }
                __syncthreads();
            }
        }

        double s_adds = 0.0;
#pragma unroll
        for (int q = 0; q < PE_Q; ++q)
            if ((want & 2) && base + q * PE_THREADS < n) s_adds += sqrt(best[q]);

        s_add = pe_wave_sum(s_add);
        s_adds = pe_wave_sum(s_adds);
        s_2d = pe_wave_sum(s_2d);
        if (lane == 0) {
            red[wave][0] = s_add;
            red[wave][1] = s_adds;
            red[wave][2] = s_2d;
        }
        __syncthreads();
        if (tid < 3) {
            double v = 0.0;
            for (int w = 0; w < PE_THREADS / 64; ++w) v += red[w][tid];
            partial[((size_t)p * gridDim.x + blockIdx.x) * 3 + tid] = v;
        }
        __syncthreads();   // `red` and the tiles are reused by the next pose
    }
}

__global__ void pose_errors_finish(const double* __restrict__ partial, int nblk, int P, int n, int want,
                                   double* __restrict__ out) {
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= P) return;
    double s[3] = {0.0, 0.0, 0.0};
    for (int b = 0; b < nblk; ++b)
#pragma unroll
        for (int c = 0; c < 3; ++c) s[c] += partial[((size_t)p * nblk + b) * 3 + c];
#pragma unroll
    for (int c = 0; c < 3; ++c)
        if (want & (1 << c)) out[(size_t)p * 3 + c] = s[c] / (double)n;
}

}  // namespace

int pose_error_blocks(int n) { return (n + PE_THREADS * PE_Q - 1) / (PE_THREADS * PE_Q); }

// partial: [P][pose_error_blocks(n)][3] doubles of device scratch
void launch_pose_errors(const double* model, int n, const double* gt, const double* est, int P, const double* K,
                        int want, double* partial, double* out, hipStream_t s) {
    PeCam cam{};
    if (K)
        for (int i = 0; i < 9; ++i) cam.k[i] = K[i];
    const int nblk = pose_error_blocks(n);
    const dim3 grid(nblk, P < 65535 ? P : 65535);
    hipLaunchKernelGGL(pose_errors_kernel, grid, dim3(PE_THREADS), 0, s, model, n, gt, est, P, cam, want, partial);
    hipLaunchKernelGGL(pose_errors_finish, dim3((P + 255) / 256), dim3(256), 0, s, partial, nblk, P, n, want, out);
}

}  // namespace bp
