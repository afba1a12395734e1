// One key-point-detector training iteration on the device, outside its convolutions (include/betapose_hip.h
// bp_kpd_train_*; the convolutions and Linears are darknet_train.hip's dt_gemm_kernel, unchanged).  The arithmetic and
// every lane's loop are kpd_train_math.inc, the text the host twins (kpd_train_host.cpp) compile too; here is who runs
// which lane:
//   kt_bn_forward_kernel    one block per channel over the [N][C][S] view: the f64 sum, then the f64 sum of squared
//                           distances (lane t takes units t, t + 256, ... ascending; shuffle tree per wave; waves in
//                           order), lane 0 stores mean, invstd and the running pair, then the affine step with the
//                           optional ReLU in one pass.  Without batch norm it is the bias add (conv_out, the SE Linears).
//   kt_bn_backward_kernel   one block per channel: the ReLU mask keyed on the stored output, the two f64 sums in one
//                           read, grad_bias and grad_weight, then dx over the same elements, in place.  x_hat is
//                           recomputed from the raw convolution, not stored.
//   kt_rows_kernel          one block per row of S values: the SE pool (mode 0) or the gate's gradient sum(m * y).
//   kt_tail_forward_kernel, kt_tail_backward_kernel, kt_pool_backward_kernel, kt_sigmoid_*_kernel
//                           element-wise, one lane per unit.
//   kt_maxpool_forward_kernel   one lane per output: the window's first maximum and its int32 position.
//   kt_maxpool_backward_kernel  one lane per INPUT position: a gather over the (at most four) windows that hold it.
//   kt_rmsprop_kernel       one launch for every parameter tensor from a table on the device, as dt_update_kernel.
// A unit is four consecutive values read and written as one 16-byte access where S is a multiple of 4 (the C entry
// points then require 16-byte aligned tensors), else one scalar value; the RMSprop launch moves the whole quads of an
// aligned row as 16-byte accesses and the row's last elements as scalars; max-pool and sigmoid are scalar.
// No floating-point atomics: every sum has the same bits from run to run, on any stream.
// Bounds: a channel pass indexes unit u < N * S / V of channel f < C (gridDim.x = C); a row pass unit u < S / V of row
// blockIdx.x < rows; an element-wise pass tests its unit against total / V; s, ds, pool and dpool are indexed by
// element / S < N * C; max-pool tests every tap against H and W and its lane against planes * OH * OW (forward) or
// planes * H * W (backward), arg-max values lie in [0, H * W) by construction and are only compared; the update tests
// its index against the row's count and its block against the table's chunks.
#include "bp_common.h"
#include "kpd_train.h"

#pragma clang fp contract(off)

namespace bp {

namespace {

#include "darknet_train_math.inc"
#include "yolo_train_math.inc"

__host__ __device__ __forceinline__ void kt_ld4(const float* p, float* r) {
    const float4 v = *reinterpret_cast<const float4*>(p);
    r[0] = v.x, r[1] = v.y, r[2] = v.z, r[3] = v.w;
}
__host__ __device__ __forceinline__ void kt_st4(float* p, const float* r) {
    *reinterpret_cast<float4*>(p) = make_float4(r[0], r[1], r[2], r[3]);
}

#include "kpd_train_math.inc"

// the sum of one value per lane of the block, in the order kpd_train_host.cpp kt_block_sum fixes; valid on every lane.
// Every lane of the block must arrive.  w_sum is free again after the next barrier.
__device__ __forceinline__ double kt_block_sum(double v, double* w_sum) {
    for (int o = DT_WAVE / 2; o > 0; o >>= 1) v = v + __shfl_down(v, o, DT_WAVE);
    if ((threadIdx.x & (DT_WAVE - 1)) == 0) w_sum[threadIdx.x / DT_WAVE] = v;
    __syncthreads();
    double t = w_sum[0];
    for (int w = 1; w < DT_THREADS / DT_WAVE; ++w) t = t + w_sum[w];
    return t;
}

template <int V>
__global__ __launch_bounds__(DT_THREADS) void kt_bn_forward_kernel(const float* __restrict__ x, int N, int C, int S,
                                                                   const float* __restrict__ w, const float* __restrict__ b,
                                                                   float* running_mean, float* running_var, float* __restrict__ mean,
                                                                   float* __restrict__ invstd, float* __restrict__ out, int bn,
                                                                   int relu, int train) {
    __shared__ double w_sum[2][DT_THREADS / DT_WAVE];
    const int f = blockIdx.x, t = threadIdx.x, count = N * S;
    float mu = 0.0f, is = 1.0f;
    if (bn && train) {          // (uniform over the block)
        const double m = kt_block_sum(kt_bnf_sum<V>(x, f, C, S, count, t, 0, 0.0), w_sum[0]) / (double)count;
        const double ss = kt_block_sum(kt_bnf_sum<V>(x, f, C, S, count, t, 1, m), w_sum[1]), var = ss / (double)count;
        mu = (float)m, is = kt_invstd(var);
        if (t == 0) {
            mean[f] = mu, invstd[f] = is;
            running_mean[f] = kt_running(running_mean[f], m), running_var[f] = kt_running(running_var[f], ss / (double)(count - 1));
        }
    } else if (bn) {
        mu = running_mean[f], is = kt_invstd((double)running_var[f]);
    }
    kt_bnf_apply<V>(x, out, f, C, S, count, t, mu, is, bn ? w[f] : 1.0f, b[f], bn, relu);
}

template <int V>
__global__ __launch_bounds__(DT_THREADS) void kt_bn_backward_kernel(const float* __restrict__ out, float* d, const float* __restrict__ x,
                                                                    const float* __restrict__ mean, const float* __restrict__ invstd,
                                                                    const float* __restrict__ w, int N, int C, int S, float* grad_w,
                                                                    float* grad_b, int bn, int relu) {
    __shared__ double w_sum[2][DT_THREADS / DT_WAVE];
    const int f = blockIdx.x, t = threadIdx.x, count = N * S;
    const float mu = bn ? mean[f] : 0.0f, is = bn ? invstd[f] : 1.0f, wf = bn ? w[f] : 1.0f;
    double s0, s1;
    kt_bnb_sum<V>(out, d, x, f, C, S, count, t, mu, bn, relu, &s0, &s1);
    const double sum = kt_block_sum(s0, w_sum[0]);
    if (t == 0) grad_b[f] = grad_b[f] + (float)sum;
    double k = 0.0;
    if (bn) {                   // (uniform over the block)
        const double dotp = kt_block_sum(s1, w_sum[1]);
        if (t == 0) grad_w[f] = grad_w[f] + (float)(dotp * (double)is);
        k = kt_bn_k(dotp, is, count);
    }
    // each lane rewrites the elements it alone read above
    kt_bnb_apply<V>(out, d, x, f, C, S, count, t, mu, sum / (double)count, k, is, wf, bn, relu);
}

template <int V>
__global__ __launch_bounds__(DT_THREADS) void kt_rows_kernel(const float* __restrict__ y, const float* __restrict__ out,
                                                             const float* __restrict__ dout, int S, int mode, float* __restrict__ dst) {
    __shared__ double w_sum[DT_THREADS / DT_WAVE];
    const size_t at = (size_t)blockIdx.x * S;
    const double sum = kt_block_sum(kt_row_sum<V>(y + at, mode ? out + at : nullptr, mode ? dout + at : nullptr, S, threadIdx.x, mode), w_sum);
    if (threadIdx.x == 0) dst[blockIdx.x] = mode ? (float)sum : kt_pool(sum, S);
}

template <int V>
__global__ __launch_bounds__(DT_THREADS) void kt_tail_forward_kernel(const float* __restrict__ y, const float* __restrict__ sc,
                                                                     const float* __restrict__ res, float* __restrict__ out, int S,
                                                                     size_t units) {
    const size_t u = (size_t)blockIdx.x * DT_THREADS + threadIdx.x;
    if (u < units) kt_tail_fwd_unit<V>(y, sc, res, out, S, u);
}

template <int V>
__global__ __launch_bounds__(DT_THREADS) void kt_tail_backward_kernel(const float* __restrict__ out, const float* __restrict__ dout,
                                                                      const float* __restrict__ sc, float* dres, float* dy, int S,
                                                                      size_t units) {
    const size_t u = (size_t)blockIdx.x * DT_THREADS + threadIdx.x;
    if (u < units) kt_tail_bwd_unit<V>(out, dout, sc, dres, dy, S, u);
}

template <int V>
__global__ __launch_bounds__(DT_THREADS) void kt_pool_backward_kernel(const float* __restrict__ dpool, float* dy, int S, size_t units) {
    const size_t u = (size_t)blockIdx.x * DT_THREADS + threadIdx.x;
    if (u < units) kt_pool_bwd_unit<V>(dpool, dy, S, u);
}

__global__ __launch_bounds__(DT_THREADS) void kt_sigmoid_forward_kernel(const float* __restrict__ x, float* __restrict__ sg, long long n) {
    const long long i = (long long)blockIdx.x * DT_THREADS + threadIdx.x;
    if (i < n) sg[i] = kt_sigmoid(x[i]);
}

__global__ __launch_bounds__(DT_THREADS) void kt_sigmoid_backward_kernel(const float* __restrict__ sg, float* g, long long n) {
    const long long i = (long long)blockIdx.x * DT_THREADS + threadIdx.x;
    if (i < n) g[i] = kt_sigmoid_back(g[i], sg[i]);
}

__global__ __launch_bounds__(DT_THREADS) void kt_maxpool_forward_kernel(const float* __restrict__ x, int planes, int H, int W, int OH,
                                                                        int OW, float* __restrict__ out, int* __restrict__ arg) {
    const size_t o = (size_t)blockIdx.x * DT_THREADS + threadIdx.x;
    if (o >= (size_t)planes * OH * OW) return;
    const int ox = (int)(o % OW), oy = (int)(o / OW % OH);
    const size_t p = o / OW / OH;
    float best;
    arg[o] = kt_window(x + p * H * W, H, W, oy, ox, &best);
    out[o] = best;
}

__global__ __launch_bounds__(DT_THREADS) void kt_maxpool_backward_kernel(const float* __restrict__ dout, const int* __restrict__ arg,
                                                                         int planes, int H, int W, int OH, int OW, float* __restrict__ dx) {
    const size_t e = (size_t)blockIdx.x * DT_THREADS + threadIdx.x;
    if (e >= (size_t)planes * H * W) return;
    const int ix = (int)(e % W), iy = (int)(e / W % H);
    const size_t p = e / W / H;
    dx[e] = kt_pool_gather(dout + p * OH * OW, arg + p * OH * OW, H, W, OH, OW, iy, ix);
}

__global__ __launch_bounds__(DT_THREADS) void kt_rmsprop_kernel(const KpdTrainTensor* __restrict__ table, int tensors, KtOpt o) {
    __shared__ int sh_t;
    __shared__ long long sh_first;
    if (threadIdx.x == 0) {
        long long blk = blockIdx.x;
        int t = 0;
        for (; t < tensors; ++t) {
            const long long nb = (table[t].count + KT_UPD_CHUNK - 1) / KT_UPD_CHUNK;
            if (blk < nb) break;
            blk -= nb;
        }
        sh_t = t, sh_first = blk * KT_UPD_CHUNK;
    }
    __syncthreads();
    if (sh_t >= tensors) return;
    const KpdTrainTensor T = table[sh_t];
    const long long end = sh_first + KT_UPD_CHUNK < T.count ? sh_first + KT_UPD_CHUNK : T.count;
    // 16-byte accesses over the chunk's whole quads where the row's tensors are 16-byte aligned (a chunk starts at a
    // multiple of KT_UPD_CHUNK elements), scalar accesses for the row's last one to three elements or an unaligned row
    const bool mom = o.momentum > 0.0f;
    const bool vec = (((uintptr_t)T.p | (uintptr_t)T.g | (uintptr_t)T.v | (mom ? (uintptr_t)T.b : (uintptr_t)0)) & 15) == 0;
    const long long quads_end = vec ? sh_first + ((end - sh_first) & ~3ll) : sh_first;
    for (long long i = sh_first + 4 * (long long)threadIdx.x; i < quads_end; i += 4 * DT_THREADS) {
        float p[4], g[4], v[4], b[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        kt_ld4(T.p + i, p), kt_ld4(T.g + i, g), kt_ld4(T.v + i, v);
        if (mom) kt_ld4(T.b + i, b);
#pragma unroll
        for (int j = 0; j < 4; ++j) kt_rmsprop(p[j], g[j], v[j], b[j], o);
        kt_st4(T.p + i, p), kt_st4(T.v + i, v);
        if (mom) kt_st4(T.b + i, b);
    }
    for (long long i = quads_end + threadIdx.x; i < end; i += DT_THREADS) {
        float p = T.p[i], v = T.v[i], b = mom ? T.b[i] : 0.0f;
        kt_rmsprop(p, T.g[i], v, b, o);
        T.p[i] = p, T.v[i] = v;
        if (mom) T.b[i] = b;
    }
}

inline dim3 kt_grid(size_t n) { return dim3((unsigned)((n + DT_THREADS - 1) / DT_THREADS)); }

}  // namespace

#define KT_LAUNCH(kernel, grid, ...)                                                              \
    do {                                                                                          \
        hipLaunchKernelGGL(kernel, grid, dim3(DT_THREADS), 0, s, __VA_ARGS__);                    \
        BP_HIP(hipGetLastError());                                                                \
    } while (0)

void launch_kpd_train_bn_forward(const float* x, int N, int C, int S, const float* w, const float* b, float* running_mean,
                                 float* running_var, float* mean, float* invstd, float* out, int bn, int relu, int train,
                                 hipStream_t s) {
    if (kt_vec(S) == 4) KT_LAUNCH(kt_bn_forward_kernel<4>, dim3(C), x, N, C, S, w, b, running_mean, running_var, mean, invstd, out, bn, relu, train);
    else KT_LAUNCH(kt_bn_forward_kernel<1>, dim3(C), x, N, C, S, w, b, running_mean, running_var, mean, invstd, out, bn, relu, train);
}

void launch_kpd_train_bn_backward(const float* out, float* d, const float* x, const float* mean, const float* invstd, const float* w,
                                  int N, int C, int S, float* grad_w, float* grad_b, int bn, int relu, hipStream_t s) {
    if (kt_vec(S) == 4) KT_LAUNCH(kt_bn_backward_kernel<4>, dim3(C), out, d, x, mean, invstd, w, N, C, S, grad_w, grad_b, bn, relu);
    else KT_LAUNCH(kt_bn_backward_kernel<1>, dim3(C), out, d, x, mean, invstd, w, N, C, S, grad_w, grad_b, bn, relu);
}

void launch_kpd_train_tail_forward(const float* y, const float* sc, const float* res, float* out, int N, int C, int S, hipStream_t s) {
    const size_t total = (size_t)N * C * S;
    if (kt_vec(S) == 4) KT_LAUNCH(kt_tail_forward_kernel<4>, kt_grid(total / 4), y, sc, res, out, S, total / 4);
    else KT_LAUNCH(kt_tail_forward_kernel<1>, kt_grid(total), y, sc, res, out, S, total);
}

void launch_kpd_train_tail_backward(const float* out, const float* dout, const float* y, const float* sc, float* dres, float* dy,
                                    float* ds, int N, int C, int S, hipStream_t s) {
    const size_t total = (size_t)N * C * S;
    if (sc) {
        if (kt_vec(S) == 4) KT_LAUNCH(kt_rows_kernel<4>, dim3(N * C), y, out, dout, S, 1, ds);
        else KT_LAUNCH(kt_rows_kernel<1>, dim3(N * C), y, out, dout, S, 1, ds);
    }
    if (kt_vec(S) == 4) KT_LAUNCH(kt_tail_backward_kernel<4>, kt_grid(total / 4), out, dout, sc, dres, dy, S, total / 4);
    else KT_LAUNCH(kt_tail_backward_kernel<1>, kt_grid(total), out, dout, sc, dres, dy, S, total);
}

void launch_kpd_train_pool_forward(const float* y, int rows, int S, float* pool, hipStream_t s) {
    if (kt_vec(S) == 4) KT_LAUNCH(kt_rows_kernel<4>, dim3(rows), y, (const float*)nullptr, (const float*)nullptr, S, 0, pool);
    else KT_LAUNCH(kt_rows_kernel<1>, dim3(rows), y, (const float*)nullptr, (const float*)nullptr, S, 0, pool);
}

void launch_kpd_train_pool_backward(const float* dpool, float* dy, int rows, int S, hipStream_t s) {
    const size_t total = (size_t)rows * S;
    if (kt_vec(S) == 4) KT_LAUNCH(kt_pool_backward_kernel<4>, kt_grid(total / 4), dpool, dy, S, total / 4);
    else KT_LAUNCH(kt_pool_backward_kernel<1>, kt_grid(total), dpool, dy, S, total);
}

void launch_kpd_train_sigmoid_forward(const float* x, float* sg, long long n, hipStream_t s) {
    KT_LAUNCH(kt_sigmoid_forward_kernel, kt_grid((size_t)n), x, sg, n);
}

void launch_kpd_train_sigmoid_backward(const float* sg, float* g, long long n, hipStream_t s) {
    KT_LAUNCH(kt_sigmoid_backward_kernel, kt_grid((size_t)n), sg, g, n);
}

void launch_kpd_train_maxpool_forward(const float* x, int planes, int H, int W, float* out, int* arg, hipStream_t s) {
    const int OH = kt_pool_out(H), OW = kt_pool_out(W);
    KT_LAUNCH(kt_maxpool_forward_kernel, kt_grid((size_t)planes * OH * OW), x, planes, H, W, OH, OW, out, arg);
}

void launch_kpd_train_maxpool_backward(const float* dout, const int* arg, int planes, int H, int W, float* dx, hipStream_t s) {
    const int OH = kt_pool_out(H), OW = kt_pool_out(W);
    KT_LAUNCH(kt_maxpool_backward_kernel, kt_grid((size_t)planes * H * W), dout, arg, planes, H, W, OH, OW, dx);
}

void launch_kpd_train_rmsprop(const KpdTrainTensor* table, int tensors, int blocks, KpdTrainOpt o, hipStream_t s) {
    const KtOpt k = {o.lr, o.alpha, o.one_minus_alpha, o.eps, o.wd, o.momentum};
    KT_LAUNCH(kt_rmsprop_kernel, dim3(blocks), table, tensors, k);
}

}  // namespace bp
