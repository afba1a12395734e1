// Detector training batches and the yolo-layer loss on the device (include/betapose_hip.h bp_yolo_inputs,
// bp_yolo_truth, bp_yolo_loss).  The arithmetic of one input pixel, one sample's truth rows, one cell and one image's
// truth walk is yolo_train_math.inc, the text the host twins (yolo_train_host.cpp) compile too; here is who loops over what:
//   yt_inputs_kernel   one lane per 4 consecutive output columns of one row, all three channels (the HSV step needs the
//                      three together), grid-stride: the taps of both resize passes are read straight from the uint8
//                      frame through the crop (no cropped, `part` or flipped image exists), three 16-byte stores where
//                      the row allows it, scalar stores otherwise.  Every element of out is written.
//   yt_truth_kernel    one lane per sample: the work is tiny and sequential, it is here so a batch never leaves the device.
//   yt_cells_kernel    one lane per (image, anchor, cell): writes every entry of its cell in delta (and act); the block
//                      sums its objectness outputs in f64 (shuffle tree per wave, waves in order) into partial.
//   yt_walk_kernel     one wave per image, whose first lane walks the truth rows in order: later rows overwrite
//                      earlier ones and delta_yolo_class reads what is already written, so the walk is sequential.
//   yt_cost_kernel     one block per YT_CHUNK elements of delta: lane t sums the squares of elements t, t + 256, ... in
//                      f64, then the same block sum.  yt_finish_kernel (one block) adds each group of partial sums in
//                      index order from LDS, where all lanes stage them.
// No floating-point atomics: every sum has the same bits from run to run, on any stream, and the host twin's.  Every load
// of a frame is indexed by a pixel clamped into it and a frame index tested against [0, N); every cell index is below
// the launch's cell count; a truth row whose cell lies outside the grid is passed over; every store index is below the
// tensor's element count.
#include "bp_common.h"
#include "yolo_train.h"

#pragma clang fp contract(off)

namespace bp {

namespace {

#include "yolo_train_math.inc"

inline int yt_grid(long long n, int cap = 8192) {
    long long g = (n + YT_THREADS - 1) / YT_THREADS;
    return (int)(g < 1 ? 1 : (g > cap ? cap : g));
}

__global__ __launch_bounds__(YT_THREADS) void yt_inputs_kernel(const unsigned char* __restrict__ frames, int N, int H, int W,
                                                               const int* __restrict__ frame_index, const int* __restrict__ crop,
                                                               const unsigned char* __restrict__ flip,
                                                               const float* __restrict__ hsv, int B, int net_h, int net_w,
                                                               int base_aligned, float* __restrict__ out) {
    const int quads = (net_w + 3) / 4;
    const int total = B * net_h * quads;        // < 2^31 (checked by the caller)
    const size_t plane = (size_t)net_h * net_w;
    for (int i = blockIdx.x * YT_THREADS + threadIdx.x; i < total; i += gridDim.x * YT_THREADS) {
        const int q = i % quads, r = i / quads; // r = b * net_h + y
        const int y = r % net_h, b = r / net_h;
        const int fi = frame_index[b];
        const int x0 = q * 4;
        float v[3][4] = {{0.0f, 0.0f, 0.0f, 0.0f}, {0.0f, 0.0f, 0.0f, 0.0f}, {0.0f, 0.0f, 0.0f, 0.0f}};
        if (fi >= 0 && fi < N) {
            const unsigned char* frame = frames + (size_t)fi * H * W * 3;
            const YtCrop k = yt_crop(crop + (size_t)b * 4, net_h, net_w);
            const float* d = hsv ? hsv + (size_t)b * 3 : nullptr;
            const int f = flip[b] != 0;
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (x0 + j < net_w) {
                    float rgb[3];
                    yt_input_rgb(frame, H, W, k, net_h, net_w, f, d, y, x0 + j, rgb);
                    v[0][j] = rgb[0], v[1][j] = rgb[1], v[2][j] = rgb[2];
                }
        }
        const size_t off = (size_t)b * 3 * plane + (size_t)y * net_w + x0;     // channel 0; + c * plane stays inside the tensor
        const bool vec = base_aligned && (net_w & 3) == 0;      // then plane and every row offset are multiples of 4 floats
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            float* dst = out + off + c * plane;
            if (vec) {
                *reinterpret_cast<float4*>(dst) = make_float4(v[c][0], v[c][1], v[c][2], v[c][3]);
            } else {
                for (int j = 0; j < 4; ++j)
                    if (x0 + j < net_w) dst[j] = v[c][j];
            }
        }
    }
}

__global__ __launch_bounds__(YT_WAVE) void yt_truth_kernel(const float* __restrict__ labels, int M, const int* __restrict__ first,
                                                           const int* __restrict__ swap, const float* __restrict__ geom,
                                                           const unsigned char* __restrict__ flip, int B, int classes,
                                                           int max_boxes, int net_w, int net_h, int* __restrict__ order,
                                                           float* __restrict__ truth, int* __restrict__ kept) {
    const int b = blockIdx.x * YT_WAVE + threadIdx.x;
    if (b >= B) return;
    int f0 = first[b], f1 = first[b + 1];
    f0 = f0 < 0 ? 0 : (f0 > M ? M : f0);        // a slice always lies inside labels, swap and order
    f1 = f1 < f0 ? f0 : (f1 > M ? M : f1);
    const float* g = geom + (size_t)b * 4;
    kept[b] = yt_truth_rows(labels + (size_t)f0 * 5, f1 - f0, swap + f0, g[0], g[1], g[2], g[3], flip[b] != 0, classes, max_boxes,
                            net_w, net_h, order + f0, truth + (size_t)b * max_boxes * 5);
}

// the sum of one value per lane of the block, in the order yolo_train_host.cpp yt_block_sum fixes; valid on thread 0
__device__ __forceinline__ double yt_block_sum(double v, double* w_sum) {
    for (int o = YT_WAVE / 2; o > 0; o >>= 1) v = v + __shfl_down(v, o, YT_WAVE);
    if ((threadIdx.x & (YT_WAVE - 1)) == 0) w_sum[threadIdx.x / YT_WAVE] = v;
    __syncthreads();
    double t = w_sum[0];
    for (int w = 1; w < YT_THREADS / YT_WAVE; ++w) t = t + w_sum[w];
    return t;
}

__global__ __launch_bounds__(YT_THREADS) void yt_cells_kernel(YtHead L, const float* __restrict__ x,
                                                              const float* __restrict__ anchors, const int* __restrict__ mask,
                                                              const float* __restrict__ truth, float* __restrict__ act,
                                                              float* __restrict__ delta, double* __restrict__ p_any) {
    __shared__ double w_sum[YT_THREADS / YT_WAVE];
    const int wh = L.h * L.w;
    const size_t cells = (size_t)L.B * L.n * wh;
    const size_t g = (size_t)blockIdx.x * YT_THREADS + threadIdx.x;
    double v = 0.0;
    if (g < cells) {
        const int loc = (int)(g % wh), a = (int)(g / wh % L.n), b = (int)(g / wh / L.n);
        v = (double)yt_cell(L, x, anchors, mask, truth, b, a, loc, act, delta);
    }
    const double t = yt_block_sum(v, w_sum);    // (every lane of the block arrives: no early return above)
    if (threadIdx.x == 0) p_any[blockIdx.x] = t;
}

__global__ __launch_bounds__(YT_WAVE) void yt_walk_kernel(YtHead L, const float* __restrict__ x,
                                                          const float* __restrict__ anchors, const int* __restrict__ mask,
                                                          const float* __restrict__ truth, float* delta, double* __restrict__ p_img) {
    if (threadIdx.x != 0) return;
    const int b = blockIdx.x;                   // < B: the grid has B blocks
    double st[YT_IMAGE_STATS];
    yt_truth_walk(L, x, anchors, mask, truth, b, delta, st);
    for (int i = 0; i < YT_IMAGE_STATS; ++i) p_img[(size_t)b * YT_IMAGE_STATS + i] = st[i];
}

__global__ __launch_bounds__(YT_THREADS) void yt_cost_kernel(const float* __restrict__ delta, size_t elems,
                                                             double* __restrict__ p_cost) {
    __shared__ double w_sum[YT_THREADS / YT_WAVE];
    const size_t k = blockIdx.x;
    double s = 0.0;
    for (size_t e = k * YT_CHUNK + threadIdx.x; e < (k + 1) * YT_CHUNK && e < elems; e += YT_THREADS)
        s = s + (double)delta[e] * (double)delta[e];
    const double t = yt_block_sum(s, w_sum);
    if (threadIdx.x == 0) p_cost[k] = t;
}

constexpr int YT_TILE = 2048;                   // partial sums staged in LDS at a time by the finish kernel

// the n values of p in index order: every lane fetches, thread 0 adds (valid on thread 0)
__device__ __forceinline__ double yt_ordered_sum(const double* __restrict__ p, size_t n, size_t stride, double* tile) {
    double sum = 0.0;
    for (size_t base = 0; base < n; base += YT_TILE) {
        const int cnt = n - base < (size_t)YT_TILE ? (int)(n - base) : YT_TILE;
        for (int i = threadIdx.x; i < cnt; i += YT_THREADS) tile[i] = p[(base + i) * stride];
        __syncthreads();
        if (threadIdx.x == 0)
            for (int i = 0; i < cnt; ++i) sum = sum + tile[i];
        __syncthreads();
    }
    return sum;
}

__global__ __launch_bounds__(YT_THREADS) void yt_finish_kernel(const double* __restrict__ p_any, size_t nA,
                                                               const double* __restrict__ p_img, int B,
                                                               const double* __restrict__ p_cost, size_t nC,
                                                               double* __restrict__ cost, double* __restrict__ stats) {
    __shared__ double tile[YT_TILE];
    const double any = yt_ordered_sum(p_any, nA, 1, tile);
    double st[YT_IMAGE_STATS];
    for (int i = 0; i < YT_IMAGE_STATS; ++i) st[i] = yt_ordered_sum(p_img + i, (size_t)B, YT_IMAGE_STATS, tile);
    const double c = yt_ordered_sum(p_cost, nC, 1, tile);
    if (threadIdx.x == 0) {
        *cost = c;
        stats[0] = st[0], stats[1] = st[1], stats[2] = st[2], stats[3] = any, stats[4] = st[3], stats[5] = st[4], stats[6] = st[5];
    }
}

}  // namespace

void launch_yolo_inputs(const unsigned char* frames, int N, int H, int W, const int* frame_index, const int* crop,
                        const unsigned char* flip, const float* hsv, int B, int net_h, int net_w, float* out, hipStream_t s) {
    const long long total = (long long)B * net_h * ((net_w + 3) / 4);
    hipLaunchKernelGGL(yt_inputs_kernel, dim3(yt_grid(total)), dim3(YT_THREADS), 0, s, frames, N, H, W, frame_index, crop, flip,
                       hsv, B, net_h, net_w, (int)(((uintptr_t)out & 15) == 0), out);
}

void launch_yolo_truth(const float* labels, int M, const int* first, const int* swap, const float* geom, const unsigned char* flip,
                       int B, int classes, int max_boxes, int net_w, int net_h, int small_object, int* order, float* truth,
                       int* kept, hipStream_t s) {
    (void)small_object;                         // (changes no output: yolo_train_math.inc yt_truth_rows)
    hipLaunchKernelGGL(yt_truth_kernel, dim3((B + YT_WAVE - 1) / YT_WAVE), dim3(YT_WAVE), 0, s, labels, M, first, swap, geom, flip,
                       B, classes, max_boxes, net_w, net_h, order, truth, kept);
}

void launch_yolo_loss(const float* x, int B, int n, int classes, int h, int w, int net_w, int net_h, const float* anchors,
                      int total, const int* mask, const float* truth, int max_boxes, float ignore_thresh, float truth_thresh,
                      float* act, float* delta, double* cost, double* stats, double* partial, hipStream_t s) {
    const YtHead L = {B, n, classes, h, w, net_w, net_h, total, max_boxes, ignore_thresh, truth_thresh};
    const size_t nA = yt_any_blocks(B, n, h, w), nC = yt_cost_blocks(B, n, classes, h, w);
    const size_t elems = (size_t)B * n * (5 + classes) * h * w;
    double* p_any = partial;
    double* p_img = partial + nA;
    double* p_cost = p_img + (size_t)B * YT_IMAGE_STATS;
    hipLaunchKernelGGL(yt_cells_kernel, dim3((unsigned)nA), dim3(YT_THREADS), 0, s, L, x, anchors, mask, truth, act, delta, p_any);
    hipLaunchKernelGGL(yt_walk_kernel, dim3(B), dim3(YT_WAVE), 0, s, L, x, anchors, mask, truth, delta, p_img);
    hipLaunchKernelGGL(yt_cost_kernel, dim3((unsigned)nC), dim3(YT_THREADS), 0, s, delta, elems, p_cost);
    hipLaunchKernelGGL(yt_finish_kernel, dim3(1), dim3(YT_THREADS), 0, s, p_any, nA, p_img, B, p_cost, nC, cost, stats);
}

}  // namespace bp
