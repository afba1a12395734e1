// BOP symmetry-aware pose errors of P (ground-truth, estimated) pose pairs of one model, f64 (include/betapose_hip.h
// bp_pose_errors_sym):
//     MSSD = min_S max_x |E x - G S x|              (metres)
//     MSPD = min_S max_x |proj(E x) - proj(G S x)|  (pixels)
// with E the estimate, G the ground truth, S one of the object's symmetry transforms, x a model vertex.
//
// Lanes own symmetries, one each: a block of PS_THREADS lanes takes PS_THREADS consecutive symmetries of one pose
// (grid.x symmetry blocks, grid.y poses, looped beyond its limit) and one slice of the vertices (grid.z, so that few
// poses with few symmetries still fill the machine).  Per pose a lane folds its symmetry into two 3x4 matrices:
//   * MSSD works in the ground-truth object frame, as the ADD-S kernel of pose_metrics.hip does: with R = G_R^T E_R,
//     t = G_R^T (E_t - G_t) the distance is |(R x + t) - (S_R x + S_t)| = |D [x; 1]|, D = [R - S_R | t - S_t]: nine
//     FMAs, then a multiply and two FMAs for the squared length.  Coordinates stay object-sized.
//   * MSPD uses A = K G S, so a vertex costs nine FMAs, one division (the reciprocal of the depth) and the two
//     differences to the estimate's projected vertex, which is computed ONCE per vertex, on its way into LDS.
// Vertices stream through LDS in SoA tiles of PS_TILE points (x, y, z and the estimate's projection), double-buffered;
// every lane reads the same vertex (LDS broadcast).  A lane keeps the running MAXIMUM of the squared distances of its
// symmetry; sqrt(max d^2) == max sqrt(d^2) exactly, so the root is taken once per pose.  The kernel writes one maximum
// per (pose, vertex slice, symmetry); pose_errors_sym_finish takes the maximum over the slices, the minimum over the
// symmetries (lane-strided, then a wave shuffle) and the root.  Maximum and minimum do not depend on the order, and
// nothing here is an atomic: results are bit-identical from run to run and across grid shapes.
//
// Pads: tile slots past n hold vertex 0 (a real vertex cannot change the maximum it is already part of); lanes past S
// compute symmetry 0 and write nothing; a wave whose 64 symmetries all lie past S only helps staging the tiles.
#include "bp_common.h"
#include "pose_tail.h"

namespace bp {

namespace {

constexpr int PS_THREADS = 256;         // symmetries per block, one per lane
constexpr int PS_TILE = 512;            // vertices per LDS tile (5 arrays x 4 KB, x2 buffers = 40 KB)
constexpr int PS_UNROLL = 4;            // vertices per step of the inner loop; PS_TILE is a multiple
constexpr int PS_TARGET_WAVES = 4096;   // computing waves wanted in flight before the vertices are no longer split

struct PsCam {
    double k[9];
};

// vertex tiles per slice, and the number of slices that leaves none empty
__host__ __device__ inline int ps_tiles_per_slice(int ntile, int Z) { return (ntile + Z - 1) / Z; }

template <bool MSSD, bool MSPD>
__global__ __launch_bounds__(PS_THREADS) void pose_errors_sym_kernel(const double* __restrict__ model, int n,
                                                                     const double* __restrict__ gt,
                                                                     const double* __restrict__ est, int P,
                                                                     const double* __restrict__ sym, int S, PsCam cam,
                                                                     int tiles_per_slice, double* __restrict__ partial) {
    __shared__ __align__(16) double sx[2][PS_TILE];
    __shared__ __align__(16) double sy[2][PS_TILE];
    __shared__ __align__(16) double sz[2][PS_TILE];
    __shared__ __align__(16) double su[2][MSPD ? PS_TILE : 2];   // the estimate's projected vertex
    __shared__ __align__(16) double sv[2][MSPD ? PS_TILE : 2];
    const int tid = threadIdx.x;
    const int s_lane = blockIdx.x * PS_THREADS + tid;
    const bool writes = s_lane < S;
    // the whole wave's symmetries lie past S: it stages tiles and waits at the barriers, nothing else (wave-uniform)
    const bool computes = blockIdx.x * PS_THREADS + (tid & ~63) < S;
    const int ntile = (n + PS_TILE - 1) / PS_TILE;
    const int tile0 = blockIdx.z * tiles_per_slice;
    const int tile1 = min(ntile, tile0 + tiles_per_slice);
    const int Z = gridDim.z;
    const int Spad = gridDim.x * PS_THREADS;

    // this lane's symmetry, [R|t] row-major (pad lanes: symmetry 0)
    double sm[12];
    {
        const double* sp = sym + (size_t)(writes ? s_lane : 0) * 12;
#pragma unroll
        for (int i = 0; i < 12; ++i) sm[i] = sp[i];
    }

    for (int p = blockIdx.y; p < P; p += gridDim.y) {
        const double* g = gt + (size_t)p * 12;
        const double* e = est + (size_t)p * 12;

        // D = [R - S_R | t - S_t], R = G_R^T E_R, t = G_R^T (E_t - G_t)  ([R|t] row-major: element (r, c) at r * 4 + c)
        double D[12];
        if (MSSD) {
#pragma unroll
            for (int a = 0; a < 3; ++a) {
#pragma unroll
                for (int b = 0; b < 3; ++b)
                    D[a * 4 + b] = (g[a] * e[b] + g[4 + a] * e[4 + b] + g[8 + a] * e[8 + b]) - sm[a * 4 + b];
                D[a * 4 + 3] = (g[a] * (e[3] - g[3]) + g[4 + a] * (e[7] - g[7]) + g[8 + a] * (e[11] - g[11])) - sm[a * 4 + 3];
            }
        }
        // A = K (G o S) for this lane, Ke = K E for the staging
        double A[12], Ke[12];
        if (MSPD) {
            double GS[12];
#pragma unroll
            for (int r = 0; r < 3; ++r) {
#pragma unroll
                for (int c = 0; c < 4; ++c)
                    GS[r * 4 + c] = g[r * 4 + 0] * sm[c] + g[r * 4 + 1] * sm[4 + c] + g[r * 4 + 2] * sm[8 + c];
                GS[r * 4 + 3] += g[r * 4 + 3];
            }
#pragma unroll
            for (int r = 0; r < 3; ++r) {
                const double* kr = cam.k + r * 3;
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    A[r * 4 + c] = kr[0] * GS[c] + kr[1] * GS[4 + c] + kr[2] * GS[8 + c];
                    Ke[r * 4 + c] = kr[0] * e[c] + kr[1] * e[4 + c] + kr[2] * e[8 + c];
                }
            }
        }

        // vertex tile `tile` -> LDS buffer `buf`; slots past n repeat vertex 0
        auto stage = [&](int tile, int buf) {
            for (int k = tid; k < PS_TILE; k += PS_THREADS) {
                int j = tile * PS_TILE + k;
                if (j >= n) j = 0;
                const double x = model[(size_t)j * 3 + 0], y = model[(size_t)j * 3 + 1], z = model[(size_t)j * 3 + 2];
                sx[buf][k] = x;
                sy[buf][k] = y;
                sz[buf][k] = z;
                if (MSPD) {
                    const double u0 = Ke[0] * x + Ke[1] * y + Ke[2] * z + Ke[3];
                    const double u1 = Ke[4] * x + Ke[5] * y + Ke[6] * z + Ke[7];
                    const double u2 = Ke[8] * x + Ke[9] * y + Ke[10] * z + Ke[11];
                    su[buf][k] = u0 / u2;
                    sv[buf][k] = u1 / u2;
                }
            }
        };

        double far3 = -__builtin_inf(), far2 = -__builtin_inf();   // running maxima of the squared distances
        stage(tile0, 0);
        __syncthreads();
        for (int tl = tile0; tl < tile1; ++tl) {
            const int buf = (tl - tile0) & 1;
            // the other buffer was last read in the previous iteration, which ended at a barrier
            if (tl + 1 < tile1) stage(tl + 1, buf ^ 1);
            if (computes) {
                const int cnt = min(PS_TILE, n - tl * PS_TILE);
                const int steps = (cnt + PS_UNROLL - 1) / PS_UNROLL;   // the rounded-up tail reads pads (vertex 0)
                const double2* X2 = reinterpret_cast<const double2*>(sx[buf]);
                const double2* Y2 = reinterpret_cast<const double2*>(sy[buf]);
                const double2* Z2 = reinterpret_cast<const double2*>(sz[buf]);
                const double2* U2 = reinterpret_cast<const double2*>(su[buf]);
                const double2* V2 = reinterpret_cast<const double2*>(sv[buf]);
                for (int s = 0; s < steps; ++s) {
#pragma unroll
                    for (int u = 0; u < PS_UNROLL / 2; ++u) {
                        const int k2 = s * (PS_UNROLL / 2) + u;
                        const double2 cx = X2[k2], cy = Y2[k2], cz = Z2[k2];
                        if (MSSD) {
#pragma unroll
                            for (int h = 0; h < 2; ++h) {
                                const double x = h ? cx.y : cx.x, y = h ? cy.y : cy.x, z = h ? cz.y : cz.x;
                                const double dx = fma(D[0], x, fma(D[1], y, fma(D[2], z, D[3])));
                                const double dy = fma(D[4], x, fma(D[5], y, fma(D[6], z, D[7])));
                                const double dz = fma(D[8], x, fma(D[9], y, fma(D[10], z, D[11])));
                                far3 = fmax(far3, fma(dz, dz, fma(dy, dy, dx * dx)));
                            }
                        }
                        if (MSPD) {
                            const double2 cu = U2[k2], cv = V2[k2];
#pragma unroll
                            for (int h = 0; h < 2; ++h) {
                                const double x = h ? cx.y : cx.x, y = h ? cy.y : cy.x, z = h ? cz.y : cz.x;
                                const double w0 = fma(A[0], x, fma(A[1], y, fma(A[2], z, A[3])));
                                const double w1 = fma(A[4], x, fma(A[5], y, fma(A[6], z, A[7])));
                                const double w2 = fma(A[8], x, fma(A[9], y, fma(A[10], z, A[11])));
                                const double inv = 1.0 / w2;
                                const double du = fma(w0, inv, -(h ? cu.y : cu.x));
                                const double dv = fma(w1, inv, -(h ? cv.y : cv.x));
                                far2 = fmax(far2, fma(dv, dv, du * du));
                            }
                        }
                    }
                }
            }
            __syncthreads();
        }

        if (writes) {
            double* o = partial + (((size_t)p * Z + blockIdx.z) * Spad + s_lane) * 2;
            if (MSSD) o[0] = far3;
            if (MSPD) o[1] = far2;
        }
    }
}

// one wave per pose: max over the vertex slices, min over the symmetries, root
__global__ __launch_bounds__(64) void pose_errors_sym_finish(const double* __restrict__ partial, int P, int S, int Spad,
                                                             int Z, int want, double* __restrict__ out) {
    const int p = blockIdx.x, lane = threadIdx.x;
    if (p >= P) return;
    for (int c = 0; c < 2; ++c) {
        if (!(want & (1 << c))) continue;
        double best = __builtin_inf();
        for (int s = lane; s < S; s += 64) {
            double far = -__builtin_inf();
            for (int z = 0; z < Z; ++z) far = fmax(far, partial[(((size_t)p * Z + z) * Spad + s) * 2 + c]);
            best = fmin(best, far);
        }
        for (int o = 32; o > 0; o >>= 1) best = fmin(best, __shfl_down(best, o, 64));
        if (lane == 0) out[(size_t)p * 2 + c] = sqrt(best);
    }
}

struct PsShape {
    int sblk, Z, tiles_per_slice;
};

PsShape ps_shape(int n, int P, int S) {
    PsShape sh;
    sh.sblk = (S + PS_THREADS - 1) / PS_THREADS;
    const int ntile = (n + PS_TILE - 1) / PS_TILE;
    const long long waves = (long long)P * ((S + 63) / 64);
    long long Z = (PS_TARGET_WAVES + waves - 1) / waves;
    if (Z > ntile) Z = ntile;
    if (Z < 1) Z = 1;
    sh.tiles_per_slice = ps_tiles_per_slice(ntile, (int)Z);
    sh.Z = (ntile + sh.tiles_per_slice - 1) / sh.tiles_per_slice;   // no empty slice
    return sh;
}

}  // namespace

// bytes of device scratch launch_pose_errors_sym needs: [P][Z][sblk * PS_THREADS][2] doubles
size_t pose_errors_sym_scratch_bytes(int n, int P, int S) {
    const PsShape sh = ps_shape(n, P, S);
    return (size_t)P * sh.Z * sh.sblk * PS_THREADS * 2 * sizeof(double);
}

// sym: [S][12] row-major [R|t] on the device; out: [P][2] = (MSSD, MSPD); want bit 1 MSSD, bit 2 MSPD (K, host 3x3,
// is read only with bit 2); unrequested columns are left untouched
void launch_pose_errors_sym(const double* model, int n, const double* gt, const double* est, int P, const double* sym,
                            int S, const double* K, int want, double* scratch, double* out, hipStream_t s) {
    PsCam cam{};
    if (K)
        for (int i = 0; i < 9; ++i) cam.k[i] = K[i];
    const PsShape sh = ps_shape(n, P, S);
    const dim3 grid(sh.sblk, P < 65535 ? P : 65535, sh.Z);
    const dim3 block(PS_THREADS);
    if ((want & 3) == 3)
        hipLaunchKernelGGL((pose_errors_sym_kernel<true, true>), grid, block, 0, s, model, n, gt, est, P, sym, S, cam,
                           sh.tiles_per_slice, scratch);
    else if (want & 1)
        hipLaunchKernelGGL((pose_errors_sym_kernel<true, false>), grid, block, 0, s, model, n, gt, est, P, sym, S, cam,
                           sh.tiles_per_slice, scratch);
    else
        hipLaunchKernelGGL((pose_errors_sym_kernel<false, true>), grid, block, 0, s, model, n, gt, est, P, sym, S, cam,
                           sh.tiles_per_slice, scratch);
    hipLaunchKernelGGL(pose_errors_sym_finish, dim3(P), dim3(64), 0, s, scratch, P, S, sh.sblk * PS_THREADS, sh.Z, want,
                       out);
}

}  // namespace bp
