// One Darknet training iteration on the device (include/betapose_hip.h bp_train_conv, bp_train_bn_forward,
// bp_train_bn_backward, bp_train_update).  The arithmetic is darknet_train_math.inc, the text the host twins
// (darknet_train_host.cpp) compile too; here is who loops over what:
//   dt_gemm_kernel         ONE implicit-GEMM core for the three roles of a convolution (forward, filter gradient, input
//                          gradient) on the fp32 matrix pipe: a block of 4 waves owns a 64 x 64 tile of D, each wave one
//                          32 x 32 tile in the 16 accumulator registers of v_mfma_f32_32x32x2_f32.  Per step the block
//                          gathers 16 k values of A (16 x 64) and B (16 x 64) from the fp32 tensors into LDS -- dt_a /
//                          dt_b say which element that is in each role, zero outside the image and past M, Ncol or the
//                          slice's end -- and issues 8 MFMAs, k ascending.  blockIdx.z is the reduction slice (filter
//                          gradient only): a chain from zero over a k range fixed by the shape, stored to its own plane.
//   dt_slices_kernel       one lane per filter element: adds its slices in order, then the sum to the update buffer.
//   dt_bn_forward_kernel   one block per channel over the [N][C][S] view: mean, then variance, as f64 sums (lane t takes
//                          elements t, t + 256, ... ascending; shuffle tree per wave; waves in order), the rolling pair,
//                          then normalise + scale + bias + leaky in one pass that keeps x_norm.
//   dt_bn_backward_kernel  one block per channel: the four sums of the backward pass in one read, then
//                          normalize_delta fused with the leaky gradient and the delta's scaling.
//   dt_update_kernel       one launch for every parameter tensor of the net from a table on the device: a block finds
//                          its tensor and chunk in the table, each element's three steps are done in registers.
// No floating-point atomics: every sum has the same bits from run to run, on any stream.  Bounds: every load goes
// through dt_a / dt_b, which test m, j, k and the tap against the shape; every store tests m < M and j < Ncol; the
// reductions and element-wise passes index e < N * S of channel f < C; the update tests its index against the count.
#include "bp_common.h"
#include "darknet_train.h"

#pragma clang fp contract(off)

namespace bp {

namespace {

#include "darknet_train_math.inc"

typedef float dt_f32x16 __attribute__((ext_vector_type(16)));

__global__ __launch_bounds__(DT_THREADS) void dt_gemm_kernel(DtG g, const float* __restrict__ a, const float* __restrict__ b,
                                                             float* d) {
    __shared__ float As[DT_BK][DT_BM];
    __shared__ float Bs[DT_BK][DT_BN];
    const int tid = threadIdx.x, lane = tid & (DT_WAVE - 1), wave = tid / DT_WAVE, wm = wave >> 1, wn = wave & 1;
    const int m0 = blockIdx.y * DT_BM, j0 = blockIdx.x * DT_BN, s = blockIdx.z;
    const int k0 = dt_slice_begin(g, s), k1 = dt_slice_end(g, s);
    const int col = tid & 63, row = tid >> 6;       // this lane's column of both tiles; its rows are row, row + 4, ...
    dt_f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.0f;
    for (int kb = k0; kb < k1; kb += DT_BK) {
#pragma unroll
        for (int i = 0; i < DT_BK / 4; ++i) {
            const int kk = row + 4 * i, k = kb + kk;
            As[kk][col] = k < k1 ? dt_a(g, a, m0 + col, k) : 0.0f;
            Bs[kk][col] = k < k1 ? dt_b(g, b, k, j0 + col) : 0.0f;
        }
        __syncthreads();
#pragma unroll
        for (int kk = 0; kk < DT_BK; kk += 2)      // lane l holds A[i = l & 31][k = l >> 5] and B[k = l >> 5][j = l & 31]
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(As[kk + (lane >> 5)][wm * 32 + (lane & 31)],
                                                       Bs[kk + (lane >> 5)][wn * 32 + (lane & 31)], acc, 0, 0, 0);
        __syncthreads();
    }
    const int j = j0 + wn * 32 + (lane & 31);
    if (j >= g.Ncol) return;
#pragma unroll
    for (int r = 0; r < 16; ++r) {                  // D: column on the lane, row = (r & 3) + 8 (r >> 2) + 4 (l >> 5)
        const int m = m0 + wm * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
        if (m < g.M) {
            const size_t i = dt_d_index(g, m, j, s);
            d[i] = g.role == DT_INPUT_GRAD ? d[i] + acc[r] : acc[r];
        }
    }
}

__global__ __launch_bounds__(DT_THREADS) void dt_slices_kernel(DtG g, const float* __restrict__ partial, float* __restrict__ wu) {
    const int e = blockIdx.x * DT_THREADS + threadIdx.x;
    if (e >= g.M * g.Ncol) return;
    const int m = e / g.Ncol, j = e - m * g.Ncol;
    float t = partial[dt_d_index(g, m, j, 0)];
    for (int s = 1; s < g.slices; ++s) t = t + partial[dt_d_index(g, m, j, s)];
    const size_t i = dt_filter_index(g, m, j);
    wu[i] = wu[i] + t;
}

// the sum of one value per lane of the block, in the order darknet_train_host.cpp dt_block_sum fixes; valid on every
// lane.  Every lane of the block must arrive.  w_sum is free again after the next barrier.
__device__ __forceinline__ double dt_block_sum(double v, double* w_sum) {
    for (int o = DT_WAVE / 2; o > 0; o >>= 1) v = v + __shfl_down(v, o, DT_WAVE);
    if ((threadIdx.x & (DT_WAVE - 1)) == 0) w_sum[threadIdx.x / DT_WAVE] = v;
    __syncthreads();
    double t = w_sum[0];
    for (int w = 1; w < DT_THREADS / DT_WAVE; ++w) t = t + w_sum[w];
    return t;
}

__device__ __forceinline__ size_t dt_at(int e, int f, int C, int S) { return ((size_t)(e / S) * C + f) * S + e % S; }

__global__ __launch_bounds__(DT_THREADS) void dt_bn_forward_kernel(const float* __restrict__ x, int N, int C, int S,
                                                                   const float* __restrict__ scales, const float* __restrict__ biases,
                                                                   float* rolling_mean, float* rolling_var, float* __restrict__ mean,
                                                                   float* __restrict__ var, float* __restrict__ x_norm,
                                                                   float* __restrict__ out, int bn, int leaky, int train) {
    __shared__ double w_sum[2][DT_THREADS / DT_WAVE];
    const int f = blockIdx.x, tid = threadIdx.x, count = N * S;
    float mu = 0.0f, v = 0.0f;
    if (bn && train) {          // (uniform over the block)
        double s = 0.0;
        for (int e = tid; e < count; e += DT_THREADS) s = s + (double)x[dt_at(e, f, C, S)];
        mu = dt_mean(dt_block_sum(s, w_sum[0]), count);
        s = 0.0;
        for (int e = tid; e < count; e += DT_THREADS) s = s + dt_sq(x[dt_at(e, f, C, S)], mu);
        v = dt_variance(dt_block_sum(s, w_sum[1]), count);
        if (tid == 0) {
            mean[f] = mu, var[f] = v;
            rolling_mean[f] = dt_roll(rolling_mean[f], mu), rolling_var[f] = dt_roll(rolling_var[f], v);
        }
    } else if (bn) {
        mu = rolling_mean[f], v = rolling_var[f];
    }
    const double den = bn ? dt_norm_den(v) : 1.0;
    const float sc = bn ? scales[f] : 1.0f, bi = biases[f];
    for (int e = tid; e < count; e += DT_THREADS) {
        const size_t i = dt_at(e, f, C, S);
        float val;
        if (bn) {
            const float xn = dt_norm(x[i], mu, den);
            if (train) x_norm[i] = xn;
            val = dt_scale_bias(xn, sc, bi);
        } else {
            val = x[i] + bi;
        }
        out[i] = dt_activate(val, leaky);
    }
}

__global__ __launch_bounds__(DT_THREADS) void dt_bn_backward_kernel(const float* __restrict__ out, float* delta,
                                                                    const float* __restrict__ x, const float* __restrict__ x_norm,
                                                                    const float* __restrict__ mean, const float* __restrict__ var,
                                                                    const float* __restrict__ scales, int N, int C, int S,
                                                                    float* bias_updates, float* scale_updates,
                                                                    float* __restrict__ stat, int bn, int leaky) {
    __shared__ double w_sum[4][DT_THREADS / DT_WAVE];
    const int f = blockIdx.x, tid = threadIdx.x, count = N * S;
    const float sc = bn ? scales[f] : 1.0f, mu = bn ? mean[f] : 0.0f, v = bn ? var[f] : 0.0f;
    double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
    for (int e = tid; e < count; e += DT_THREADS) {
        const size_t i = dt_at(e, f, C, S);
        const float d1 = delta[i] * dt_gradient(out[i], leaky);
        s0 = s0 + (double)d1;
        if (bn) {
            const float d2 = d1 * sc;
            s1 = s1 + (double)d1 * (double)x_norm[i];
            s2 = s2 + (double)d2;
            s3 = s3 + (double)d2 * (double)(x[i] - mu);
        }
    }
    const double t0 = dt_block_sum(s0, w_sum[0]);
    float md = 0.0f, vd = 0.0f;
    if (bn) {                   // (uniform over the block)
        const double t1 = dt_block_sum(s1, w_sum[1]);
        md = dt_mean_delta(dt_block_sum(s2, w_sum[2]), v);
        vd = dt_variance_delta(dt_block_sum(s3, w_sum[3]), v);
        if (tid == 0) scale_updates[f] = scale_updates[f] + (float)t1, stat[f] = md, stat[C + f] = vd;
    }
    if (tid == 0) bias_updates[f] = bias_updates[f] + (float)t0;
    for (int e = tid; e < count; e += DT_THREADS) {     // each lane rewrites the elements it alone read above
        const size_t i = dt_at(e, f, C, S);
        const float d1 = delta[i] * dt_gradient(out[i], leaky);
        delta[i] = bn ? dt_normalize_delta(d1 * sc, x[i], mu, v, md, vd, count) : d1;
    }
}

__global__ __launch_bounds__(DT_THREADS) void dt_update_kernel(const TrainTensor* __restrict__ table, int tensors,
                                                               float rate_over_batch, float decay_term, float momentum) {
    __shared__ int sh_t;
    __shared__ long long sh_first;
    if (threadIdx.x == 0) {
        long long blk = blockIdx.x;
        int t = 0;
        for (; t < tensors; ++t) {
            const long long nb = (table[t].count + DT_UPD_CHUNK - 1) / DT_UPD_CHUNK;
            if (blk < nb) break;
            blk -= nb;
        }
        sh_t = t, sh_first = blk * DT_UPD_CHUNK;
    }
    __syncthreads();
    if (sh_t >= tensors) return;
    const TrainTensor T = table[sh_t];
    const long long end = sh_first + DT_UPD_CHUNK < T.count ? sh_first + DT_UPD_CHUNK : T.count;
    for (long long i = sh_first + threadIdx.x; i < end; i += DT_THREADS) {
        float p = T.p[i], u = T.u[i];
        dt_update(p, u, (int)T.kind, rate_over_batch, decay_term, momentum);
        T.p[i] = p, T.u[i] = u;
    }
}

}  // namespace

void launch_train_conv(int role, float* x, float* w, float* y, int N, int C, int H, int W, int K, int size, int stride,
                       float* scratch, hipStream_t s) {
    const DtG g = dt_geom(role, N, C, H, W, K, size, stride);
    const float* a = role == DT_FILTER_GRAD ? y : w;
    const float* b = role == DT_INPUT_GRAD ? y : x;
    float* d = role == DT_FORWARD ? y : (role == DT_FILTER_GRAD ? scratch : x);
    const dim3 grid((g.Ncol + DT_BN - 1) / DT_BN, (g.M + DT_BM - 1) / DT_BM, g.slices);
    hipLaunchKernelGGL(dt_gemm_kernel, grid, dim3(DT_THREADS), 0, s, g, a, b, d);
    BP_HIP(hipGetLastError());
    if (role == DT_FILTER_GRAD) {
        hipLaunchKernelGGL(dt_slices_kernel, dim3((g.M * g.Ncol + DT_THREADS - 1) / DT_THREADS), dim3(DT_THREADS), 0, s, g,
                           (const float*)scratch, w);
        BP_HIP(hipGetLastError());
    }
}

void launch_train_bn_forward(const float* x, int N, int C, int S, const float* scales, const float* biases, float* rolling_mean,
                             float* rolling_var, float* mean, float* var, float* x_norm, float* out, int bn, int leaky, int train,
                             hipStream_t s) {
    hipLaunchKernelGGL(dt_bn_forward_kernel, dim3(C), dim3(DT_THREADS), 0, s, x, N, C, S, scales, biases, rolling_mean, rolling_var,
                       mean, var, x_norm, out, bn, leaky, train);
    BP_HIP(hipGetLastError());
}

void launch_train_bn_backward(const float* out, float* delta, const float* x, const float* x_norm, const float* mean,
                              const float* var, const float* scales, int N, int C, int S, float* bias_updates,
                              float* scale_updates, float* stat, int bn, int leaky, hipStream_t s) {
    hipLaunchKernelGGL(dt_bn_backward_kernel, dim3(C), dim3(DT_THREADS), 0, s, out, delta, x, x_norm, mean, var, scales, N, C, S,
                       bias_updates, scale_updates, stat, bn, leaky);
    BP_HIP(hipGetLastError());
}

void launch_train_update(const TrainTensor* table, int tensors, int blocks, float rate_over_batch, float decay_term,
                         float momentum, hipStream_t s) {
    hipLaunchKernelGGL(dt_update_kernel, dim3(blocks), dim3(DT_THREADS), 0, s, table, tensors, rate_over_batch, decay_term,
                       momentum);
    BP_HIP(hipGetLastError());
}

}  // namespace bp
