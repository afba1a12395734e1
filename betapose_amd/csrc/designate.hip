// Key-point designator on the device (include/betapose_hip.h bp_sift_octave, bp_farthest_points, bp_thin_points).  The
// arithmetic of one pair, one weight and one extremum test is designate_math.inc, the text the host twins
// (designate_host.cpp) compile too; here is who loops over what:
//   ds_scale_space_kernel   one lane owns one point p; blocks of 64 lanes, so 20 000 points give 313 blocks.  The points
//                           q come in tiles of DS_TILE through LDS (every lane reads the same q: a broadcast), in
//                           ascending q, and the lane adds them to its 2 * ns accumulators in registers, the scales
//                           tested from the widest down.  The work is split over p, never over q, which is what keeps
//                           every sum in the host's order.
//   ds_extrema_kernel       all pairs again: every lane keeps its min(k, n) nearest (d2, index), sorted, in LDS
//                           (lane-minor, so a wave's accesses at one rank fall on 64 banks), then tests its DoG values
//                           against its neighbours'.  Launched after the scale space on the same stream.
//   ds_fps_kernel           ONE block runs all K rounds: the minimum distances live in a scratch array that every lane
//                           reads and writes at its own indices only, the block's arg-max by (value, lower index) is a
//                           wave shuffle tree and one LDS exchange.  The centroid is summed by lane 0 in index order from
//                           chunks that the whole block stages into LDS.
//   ds_thin_init_kernel     one lane per point: its nearest neighbour (distance, j) over tiles of the cloud.
//   ds_thin_loop_kernel     ONE block runs the rounds: arg-min by (distance, lower i), the deletion, and the block
//                           together recomputes the neighbour of every point that pointed at the deleted one.
// No loop waits for another block; every loop is bounded by n, K or n - keep; there are no floating-point atomics (the
// one atomic is an integer LDS counter whose order does not reach the results).  Every index into points, dog, flags and
// the scratch arrays is below n (times the row length); every LDS index is below the array's extent.
#include "bp_common.h"
#include "designate.h"

#pragma clang fp contract(off)

namespace bp {

namespace {

#include "designate_math.inc"

constexpr int DS_LANES = 64;        // block of the two octave kernels
constexpr int DS_TILE = 256;        // points of q staged per step
constexpr int DS_FPS_THREADS = 1024;
constexpr int DS_THIN_THREADS = 256;
constexpr int DS_NONE = INT32_MAX;  // the index of "no point": loses every tie

struct DsPick {
    double d;
    int i;
};

// the block's best pick, in every lane.  MAX: by ds_more, else by ds_less.  slots [NT / 64 + 1] in LDS.  Two barriers; a
// following call may reuse the slots (the partials are read before the second barrier, the result after it and before
// the next call's first).
template <int NT, bool MAX>
__device__ __forceinline__ DsPick ds_block_pick(DsPick a, DsPick* slots) {
    constexpr int NW = NT / 64;
    for (int o = 32; o > 0; o >>= 1) {
        const double e = __shfl_down(a.d, o, 64);
        const int j = __shfl_down(a.i, o, 64);
        if (MAX ? ds_more(e, j, a.d, a.i) : ds_less(e, j, a.d, a.i)) a = DsPick{e, j};
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) slots[wave] = a;
    __syncthreads();
    if (wave == 0) {
        DsPick b = lane < NW ? slots[lane] : DsPick{MAX ? -1.0 : __builtin_inf(), DS_NONE};
        for (int o = 32; o > 0; o >>= 1) {
            const double e = __shfl_down(b.d, o, 64);
            const int j = __shfl_down(b.i, o, 64);
            if (MAX ? ds_more(e, j, b.d, b.i) : ds_less(e, j, b.d, b.i)) b = DsPick{e, j};
        }
        if (lane == 0) slots[NW] = b;
    }
    __syncthreads();
    return slots[NW];
}

// the tile [t0, t0 + DS_TILE) of the cloud into LDS (f only when tf is given); a barrier before and after
__device__ __forceinline__ void ds_stage_tile(const double* __restrict__ points, int n, int t0, int field, int threads,
                                              double* tx, double* ty, double* tz, double* tf) {
    __syncthreads();
    for (int i = threadIdx.x; i < DS_TILE; i += threads) {
        const int q = t0 + i;
        if (q < n) {
            const double* Q = points + (size_t)q * 3;
            tx[i] = Q[0];
            ty[i] = Q[1];
            tz[i] = Q[2];
            if (tf) tf[i] = Q[field];
        }
    }
    __syncthreads();
}

__global__ __launch_bounds__(DS_LANES) void ds_scale_space_kernel(const double* __restrict__ points, int n, int field,
                                                                  DsScales sc, double* __restrict__ dog) {
    __shared__ double tx[DS_TILE], ty[DS_TILE], tz[DS_TILE], tf[DS_TILE];
    const int p = blockIdx.x * DS_LANES + threadIdx.x;
    const bool live = p < n;
    const double* P = points + (size_t)(live ? p : n - 1) * 3;
    const double px = P[0], py = P[1], pz = P[2];
    double num[DS_MAX_SCALES], den[DS_MAX_SCALES];
#pragma unroll
    for (int s = 0; s < DS_MAX_SCALES; ++s) num[s] = den[s] = 0.0;
    for (int t0 = 0; t0 < n; t0 += DS_TILE) {
        ds_stage_tile(points, n, t0, field, DS_LANES, tx, ty, tz, tf);
        const int m = min(DS_TILE, n - t0);
        for (int i = 0; i < m; ++i) {
            const double d2 = ds_d2(px, py, pz, tx[i], ty[i], tz[i]);
            const double f = tf[i];
#pragma unroll
            for (int s = DS_MAX_SCALES - 1; s >= 0; --s) {
                if (s < sc.ns) {
                    if (!(d2 <= sc.r9[s])) break;
                    const double w = ds_weight(d2, sc.s2[s]);
                    num[s] += f * w;
                    den[s] += w;
                }
            }
        }
    }
    if (!live) return;
    const int nd = sc.ns - 1;
    double g_prev = num[0] / den[0];
#pragma unroll
    for (int j = 0; j < DS_MAX_SCALES - 1; ++j) {
        if (j < nd) {
            const double g = num[j + 1] / den[j + 1];
            dog[(size_t)p * nd + j] = g - g_prev;
            g_prev = g;
        }
    }
}

// dynamic LDS: ld [kk][64] f64, tx, ty, tz [DS_TILE] f64, li [kk][64] i32
__global__ __launch_bounds__(DS_LANES) void ds_extrema_kernel(const double* __restrict__ points, int n, int ns, int kk,
                                                              double min_contrast, const double* __restrict__ dog,
                                                              signed char* __restrict__ flags) {
    extern __shared__ double ds_smem[];
    double* ld = ds_smem;
    double* tx = ld + (size_t)kk * DS_LANES;
    double* ty = tx + DS_TILE;
    double* tz = ty + DS_TILE;
    int* li = reinterpret_cast<int*>(tz + DS_TILE);
    const int lane = threadIdx.x;
    const int p = blockIdx.x * DS_LANES + lane;
    const bool live = p < n;
    const double* P = points + (size_t)(live ? p : n - 1) * 3;
    const double px = P[0], py = P[1], pz = P[2];
    int cnt = 0;
    for (int t0 = 0; t0 < n; t0 += DS_TILE) {
        ds_stage_tile(points, n, t0, 0, DS_LANES, tx, ty, tz, nullptr);
        const int m = live ? min(DS_TILE, n - t0) : 0;
        for (int i = 0; i < m; ++i) {
            const double d2 = ds_d2(px, py, pz, tx[i], ty[i], tz[i]);
            if (cnt < kk || d2 < ld[(kk - 1) * DS_LANES + lane]) {      // (an equal d2 at a higher index orders after)
                int at = cnt < kk ? cnt++ : kk - 1;
                for (; at > 0 && ld[(at - 1) * DS_LANES + lane] > d2; --at) {
                    ld[at * DS_LANES + lane] = ld[(at - 1) * DS_LANES + lane];
                    li[at * DS_LANES + lane] = li[(at - 1) * DS_LANES + lane];
                }
                ld[at * DS_LANES + lane] = d2;
                li[at * DS_LANES + lane] = t0 + i;
            }
        }
    }
    if (!live) return;
    const int nd = ns - 1, nf = ns - 3;
    const double* row = dog + (size_t)p * nd;
    for (int j = 1; j <= ns - 3; ++j) {
        const double v = row[j];
        int sign = ds_own_sign(v, row[j - 1], row[j + 1], min_contrast);
        for (int t = 0; t < kk && sign; ++t) {
            const double* r = dog + (size_t)li[t * DS_LANES + lane] * nd + (j - 1);
            if (!ds_nbr_ok(sign, v, r[0], r[1], r[2])) sign = 0;
        }
        flags[(size_t)p * nf + (j - 1)] = (signed char)sign;
    }
}

__global__ __launch_bounds__(DS_FPS_THREADS) void ds_fps_kernel(const double* __restrict__ points, int n, int K, int start,
                                                                double* __restrict__ mind, int* __restrict__ idx,
                                                                double* __restrict__ d2out) {
    __shared__ double stage[DS_FPS_THREADS * 3];
    __shared__ double centre[3];
    __shared__ DsPick slots[DS_FPS_THREADS / 64 + 1];
    const int tid = threadIdx.x;
    double sx = 0.0, sy = 0.0, sz = 0.0;        // (lane 0's)
    for (int c0 = 0; c0 < n; c0 += DS_FPS_THREADS) {
        __syncthreads();
        if (c0 + tid < n) {
            const double* Q = points + (size_t)(c0 + tid) * 3;
            stage[tid * 3] = Q[0];
            stage[tid * 3 + 1] = Q[1];
            stage[tid * 3 + 2] = Q[2];
        }
        __syncthreads();
        if (tid == 0) {
            const int m = min(DS_FPS_THREADS, n - c0);
            for (int j = 0; j < m; ++j) {
                sx += stage[j * 3];
                sy += stage[j * 3 + 1];
                sz += stage[j * 3 + 2];
            }
        }
    }
    if (tid == 0) {
        centre[0] = sx / (double)n;
        centre[1] = sy / (double)n;
        centre[2] = sz / (double)n;
    }
    __syncthreads();
    const double cx = centre[0], cy = centre[1], cz = centre[2];
    const double inf = __builtin_inf();
    if (start < 0) {        // (uniform over the block)
        DsPick best{-1.0, DS_NONE};
        for (int i = tid; i < n; i += DS_FPS_THREADS) {
            const double* Q = points + (size_t)i * 3;
            const double d = ds_d2(Q[0], Q[1], Q[2], cx, cy, cz);
            if (ds_more(d, i, best.d, best.i)) best = DsPick{d, i};
        }
        start = ds_block_pick<DS_FPS_THREADS, true>(best, slots).i;
    }
    for (int i = tid; i < n; i += DS_FPS_THREADS) mind[i] = inf;
    if (tid == 0) {
        const double* Q = points + (size_t)start * 3;
        idx[0] = start;
        d2out[0] = ds_d2(Q[0], Q[1], Q[2], cx, cy, cz);
    }
    int last = start;
    for (int r = 1; r < K; ++r) {
        const double* L = points + (size_t)last * 3;
        const double lx = L[0], ly = L[1], lz = L[2];
        DsPick best{-1.0, DS_NONE};
        for (int i = tid; i < n; i += DS_FPS_THREADS) {
            const double* Q = points + (size_t)i * 3;
            const double d = ds_d2(Q[0], Q[1], Q[2], lx, ly, lz);
            double m = mind[i];
            if (d < m) {
                m = d;
                mind[i] = d;
            }
            if (ds_more(m, i, best.d, best.i)) best = DsPick{m, i};
        }
        best = ds_block_pick<DS_FPS_THREADS, true>(best, slots);
        if (tid == 0) {
            idx[r] = best.i;
            d2out[r] = best.d;
        }
        last = best.i;
    }
}

// the nearest living neighbour (distance, j) of point i over the j this lane visits: j = j0, j0 + step, ...
__device__ __forceinline__ DsPick ds_nearest_strided(const double* __restrict__ points, int n, int i,
                                                     const unsigned char* alive, int j0, int step) {
    const double* P = points + (size_t)i * 3;
    DsPick best{__builtin_inf(), DS_NONE};
    for (int j = j0; j < n; j += step) {
        if (j == i || !alive[j]) continue;
        const double d = ds_dist(P, points + (size_t)j * 3);
        if (ds_less(d, j, best.d, best.i)) best = DsPick{d, j};
    }
    return best;
}

__global__ __launch_bounds__(DS_THIN_THREADS) void ds_thin_init_kernel(const double* __restrict__ points, int n,
                                                                       double* __restrict__ nn_d, int* __restrict__ nn_j,
                                                                       unsigned char* __restrict__ alive) {
    __shared__ double tx[DS_TILE], ty[DS_TILE], tz[DS_TILE];
    const int i = blockIdx.x * DS_THIN_THREADS + threadIdx.x;
    const bool live = i < n;
    const double* Pp = points + (size_t)(live ? i : n - 1) * 3;
    const double P[3] = {Pp[0], Pp[1], Pp[2]};
    DsPick best{__builtin_inf(), DS_NONE};
    for (int t0 = 0; t0 < n; t0 += DS_TILE) {
        ds_stage_tile(points, n, t0, 0, DS_THIN_THREADS, tx, ty, tz, nullptr);
        const int m = min(DS_TILE, n - t0);
        for (int t = 0; t < m; ++t) {
            const int j = t0 + t;
            if (j == i) continue;
            const double Q[3] = {tx[t], ty[t], tz[t]};
            const double d = ds_dist(P, Q);
            if (ds_less(d, j, best.d, best.i)) best = DsPick{d, j};
        }
    }
    if (!live) return;
    nn_d[i] = best.d;
    nn_j[i] = best.i;
    alive[i] = 1;
}

__global__ __launch_bounds__(DS_THIN_THREADS) void ds_thin_loop_kernel(const double* __restrict__ points, int n, int keep,
                                                                       double* nn_d, int* nn_j, int* list,
                                                                       unsigned char* alive, int* __restrict__ state) {
    __shared__ DsPick slots[DS_THIN_THREADS / 64 + 1];
    __shared__ int s_cnt;
    const int tid = threadIdx.x;
    const int rounds = n > keep ? n - keep : 0;
    int done = 0, last = -1;
    for (; done < rounds; ++done) {
        DsPick best{__builtin_inf(), DS_NONE};
        for (int i = tid; i < n; i += DS_THIN_THREADS)
            if (alive[i] && ds_less(nn_d[i], i, best.d, best.i)) best = DsPick{nn_d[i], i};
        best = ds_block_pick<DS_THIN_THREADS, false>(best, slots);
        if (!(best.d < DS_THIN_CAP)) break;     // (uniform) the reference deletes the carried position from here on
        last = best.i;
        if (tid == 0) {
            alive[last] = 0;
            s_cnt = 0;
        }
        __syncthreads();
        for (int i = tid; i < n; i += DS_THIN_THREADS)
            if (alive[i] && nn_j[i] == last) list[atomicAdd(&s_cnt, 1)] = i;    // at most n entries; their order is free
        __syncthreads();
        const int cnt = s_cnt;
        for (int a = 0; a < cnt; ++a) {
            const int i = list[a];
            const DsPick nb = ds_block_pick<DS_THIN_THREADS, false>(
                ds_nearest_strided(points, n, i, alive, tid, DS_THIN_THREADS), slots);
            if (tid == 0) {
                nn_d[i] = nb.d;
                nn_j[i] = nb.i;
            }
        }
        __syncthreads();
    }
    if (tid == 0) s_cnt = 0;
    __syncthreads();
    int mine = 0;
    for (int i = tid; i < last; i += DS_THIN_THREADS) mine += alive[i];
    if (mine) atomicAdd(&s_cnt, mine);
    __syncthreads();
    if (tid == 0) {
        state[0] = done;
        state[1] = s_cnt;
    }
}

}  // namespace

void launch_sift_octave(const double* points, int n, int field, const double* scales, int ns, int k, double min_contrast,
                        double* dog, signed char* flags, hipStream_t s) {
    const DsScales sc = ds_scales(scales, ns);
    const int kk = k < n ? k : n;
    const int blocks = (n + DS_LANES - 1) / DS_LANES;
    hipLaunchKernelGGL(ds_scale_space_kernel, dim3(blocks), dim3(DS_LANES), 0, s, points, n, field, sc, dog);
    const size_t lds = (size_t)kk * DS_LANES * (sizeof(double) + sizeof(int)) + 3 * DS_TILE * sizeof(double);   // <= 54 KiB
    hipLaunchKernelGGL(ds_extrema_kernel, dim3(blocks), dim3(DS_LANES), lds, s, points, n, ns, kk, min_contrast,
                       (const double*)dog, flags);
}

void launch_farthest_points(const double* points, int n, int K, int start, double* mind, int* idx, double* d2,
                            hipStream_t s) {
    hipLaunchKernelGGL(ds_fps_kernel, dim3(1), dim3(DS_FPS_THREADS), 0, s, points, n, K, start, mind, idx, d2);
}

void launch_thin_points(const double* points, int n, int keep, double* nn_d, int* nn_j, int* list, unsigned char* alive,
                        int* state, hipStream_t s) {
    hipLaunchKernelGGL(ds_thin_init_kernel, dim3((n + DS_THIN_THREADS - 1) / DS_THIN_THREADS), dim3(DS_THIN_THREADS), 0, s,
                       points, n, nn_d, nn_j, alive);
    hipLaunchKernelGGL(ds_thin_loop_kernel, dim3(1), dim3(DS_THIN_THREADS), 0, s, points, n, keep, nn_d, nn_j, list, alive,
                       state);
}

}  // namespace bp
