// KPD training samples on the device (include/betapose_hip.h bp_kpd_inputs, bp_kpd_augment, bp_heatmap_loss_acc).  The
// arithmetic of one input value, one augmented value, one residual and one distance is kpd_sample_math.inc, the text
// the host twins (kpd_sample_host.cpp) compile too; here is who loops over what:
//   ks_inputs_kernel     one lane per 4 consecutive floats of an input row, grid-stride: the four bilinear taps of each
//                        are read straight from the uint8 frame through the window (no padded image exists), a 16-byte
//                        store where the row allows it, scalar stores otherwise.  Every element of inp is written.
//   ks_augment_kernel    the same lane-to-output mapping over [B][C][H][W]; the taps are read through the flip and the
//                        channel table, so flip, shuffleLR and rotation are one pass.  Every element of y is written.
//   ks_loss_map_kernel   one block of KS_THREADS lanes per (sample, channel) map: each lane sums the squares of its
//                        elements in f64 and keeps the arg-max candidates of the masked output and of the label; a wave
//                        shuffle tree and thread 0 fold them in the order kpd_sample_math.inc fixes, and the gradient is
//                        stored on the way.  ks_loss_finish_kernel (one block) then makes dists and acc, one wave per
//                        channel (integer counts), and thread 0 adds the B * K partial sums in index order from LDS,
//                        where all lanes stage them.
// No floating-point atomics: the loss has the same bits from run to run, on any stream and for any grid size, and the
// host twin's.  Every load of a frame is indexed by a pixel that has been tested against [0, W) x [0, H) and a frame
// index tested against [0, N); every tap of a map uses indices clamped to it; every store index is below the launch's
// element count.
#include "bp_common.h"
#include "kpd_sample.h"

#pragma clang fp contract(off)

namespace bp {

namespace {

#include "kpd_sample_math.inc"

inline int ks_grid(long long n, int cap = 4096) {      // (aux_kernels.hip grid_for)
    long long g = (n + KS_THREADS - 1) / KS_THREADS;
    return (int)(g < 1 ? 1 : (g > cap ? cap : g));
}

// four floats of a row at x0: one 16-byte store when all four lie in the row and the address is 16-byte aligned (vec),
// scalar stores of those inside the row otherwise
__device__ __forceinline__ void ks_store_quad(float* __restrict__ dst, int x0, int rowW, bool vec, const float* v) {
    if (vec) {
        *reinterpret_cast<float4*>(dst) = make_float4(v[0], v[1], v[2], v[3]);
    } else {
        for (int j = 0; j < 4; ++j)
            if (x0 + j < rowW) dst[j] = v[j];
    }
}

// four floats of a map at element e0 of n: one 16-byte load (vec) or scalar loads of those below n, 0 for the others
__device__ __forceinline__ void ks_load_quad(const float* __restrict__ src, int e0, int n, bool vec, float* v) {
    if (vec) {
        const float4 t = *reinterpret_cast<const float4*>(src + e0);
        v[0] = t.x, v[1] = t.y, v[2] = t.z, v[3] = t.w;
    } else {
        for (int j = 0; j < 4; ++j) v[j] = e0 + j < n ? src[e0 + j] : 0.0f;
    }
}

__global__ __launch_bounds__(KS_THREADS) void ks_inputs_kernel(const unsigned char* __restrict__ frames, int N, int H, int W,
                                                               const int* __restrict__ frame_index, const float* __restrict__ ul,
                                                               const float* __restrict__ br, const float* __restrict__ gains,
                                                               const unsigned char* __restrict__ blank, int B, int inpH, int inpW,
                                                               int base_aligned, float* __restrict__ inp) {
    const int quads = (inpW + 3) / 4;
    const int total = B * 3 * inpH * quads;     // < 2^31 (checked by the caller)
    for (int i = blockIdx.x * KS_THREADS + threadIdx.x; i < total; i += gridDim.x * KS_THREADS) {
        const int q = i % quads, r = i / quads; // r = (b * 3 + c) * inpH + y
        const int y = r % inpH, bc = r / inpH;
        const int c = bc % 3, b = bc / 3;
        const int fi = frame_index[b];
        const bool zero = (blank && blank[b]) || fi < 0 || fi >= N;
        const int x0 = q * 4;
        float v[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        if (!zero) {
            const unsigned char* frame = frames + (size_t)fi * H * W * 3;
            const KsWindow k = ks_window(ul[b * 2], ul[b * 2 + 1], br[b * 2], br[b * 2 + 1], inpH, inpW);
            const float* gain = gains ? gains + (size_t)b * 3 : nullptr;
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (x0 + j < inpW) v[j] = ks_input_value(k, frame, H, W, gain, c, y, x0 + j);
        }
        const size_t off = (size_t)r * inpW + x0;       // < B * 3 * inpH * inpW: inside the tensor
        ks_store_quad(inp + off, x0, inpW, base_aligned && x0 + 4 <= inpW && (off & 3) == 0, v);
    }
}

__global__ __launch_bounds__(KS_THREADS) void ks_augment_kernel(const float* __restrict__ x, int B, int C, int H, int W,
                                                                const unsigned char* __restrict__ flip,
                                                                const double* __restrict__ cs, const int* __restrict__ perm,
                                                                int base_aligned, float* __restrict__ y) {
    const int quads = (W + 3) / 4;
    const int total = B * C * H * quads;        // < 2^31 (checked by the caller)
    const size_t HW = (size_t)H * W;
    for (int i = blockIdx.x * KS_THREADS + threadIdx.x; i < total; i += gridDim.x * KS_THREADS) {
        const int q = i % quads, r = i / quads; // r = (b * C + c) * H + row
        const int row = r % H, bc = r / H;
        const int c = bc % C, b = bc / C;
        const int f = flip[b] != 0;
        const float* src = x + ((size_t)b * C + ks_source_channel(perm, C, f, c)) * HW;
        const double a[2] = {cs[(size_t)b * 2], cs[(size_t)b * 2 + 1]};
        const int x0 = q * 4;
        float v[4] = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (x0 + j < W) v[j] = ks_augment_value(src, H, W, f, a, row, x0 + j);
        const size_t off = (size_t)r * W + x0;          // < B * C * H * W: inside the tensor
        ks_store_quad(y + off, x0, W, base_aligned && x0 + 4 <= W && (off & 3) == 0, v);
    }
}

__device__ __forceinline__ KsBest ks_best_shfl(KsBest a, int o) {
    KsBest b;
    b.v = __shfl_down(a.v, o, KS_WAVE);
    b.i = __shfl_down(a.i, o, KS_WAVE);
    return ks_best_of(a, b);
}

// aligned: out, labels, set_mask and grad (those given) start on a 16-byte boundary
__global__ __launch_bounds__(KS_THREADS) void ks_loss_map_kernel(const float* __restrict__ out, const float* __restrict__ labels,
                                                                 const float* __restrict__ set_mask, int maps, int H, int W,
                                                                 float norm, int aligned, double* __restrict__ partial,
                                                                 int* __restrict__ preds, int* __restrict__ gt,
                                                                 float* __restrict__ grad) {
    __shared__ double w_sum[KS_THREADS / KS_WAVE];
    __shared__ KsBest w_pred[KS_THREADS / KS_WAVE], w_gt[KS_THREADS / KS_WAVE];
    const int HW = H * W;                       // <= 2^24 (checked by the caller)
    const int quads = (HW + 3) / 4;
    const bool vec = aligned && (HW & 3) == 0;  // then every map starts on a 16-byte boundary too
    const int lane = threadIdx.x & (KS_WAVE - 1), wave = threadIdx.x / KS_WAVE;
    for (int m = blockIdx.x; m < maps; m += gridDim.x) {        // (uniform over the block: the shuffles see whole waves)
        const size_t base = (size_t)m * HW;
        double sum = 0.0;
        KsBest bp = ks_best_empty(), bg = ks_best_empty();
        for (int q = threadIdx.x; q < quads; q += KS_THREADS) {
            const int e0 = q * 4;
            float o[4], l[4], mk[4], g[4];
            ks_load_quad(out + base, e0, HW, vec, o);
            ks_load_quad(labels + base, e0, HW, vec, l);
            if (set_mask) ks_load_quad(set_mask + base, e0, HW, vec, mk);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                g[j] = 0.0f;
                if (e0 + j < HW) {
                    float p;
                    const float* pm = set_mask ? &mk[j] : nullptr;
                    const float d = ks_residual(o[j], pm, l[j], &p);
                    sum = sum + (double)d * (double)d;
                    bp = ks_best_of(bp, KsBest{p, e0 + j});
                    bg = ks_best_of(bg, KsBest{l[j], e0 + j});
                    g[j] = ks_gradient(norm, d, pm);
                }
            }
            if (grad) ks_store_quad(grad + base + e0, e0, HW, vec, g);     // (e0 + j < HW: inside this map)
        }
        for (int o = KS_WAVE / 2; o > 0; o >>= 1) {
            sum = sum + __shfl_down(sum, o, KS_WAVE);
            bp = ks_best_shfl(bp, o);
            bg = ks_best_shfl(bg, o);
        }
        if (lane == 0) {
            w_sum[wave] = sum;
            w_pred[wave] = bp;
            w_gt[wave] = bg;
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            double t = w_sum[0];
            KsBest p = w_pred[0], g = w_gt[0];
            for (int w = 1; w < KS_THREADS / KS_WAVE; ++w) {
                t = t + w_sum[w];
                p = ks_best_of(p, w_pred[w]);
                g = ks_best_of(g, w_gt[w]);
            }
            partial[m] = t;
            const int ip = ks_best_index(p), ig = ks_best_index(g);
            preds[(size_t)m * 2] = ip % W;
            preds[(size_t)m * 2 + 1] = ip / W;
            gt[(size_t)m * 2] = ig % W;
            gt[(size_t)m * 2 + 1] = ig / W;
        }
        __syncthreads();                        // the shared arrays are reused by the next map
    }
}

constexpr int KS_TILE = 2048;                   // partial sums staged in LDS at a time by the finish kernel

__global__ __launch_bounds__(KS_THREADS) void ks_loss_finish_kernel(const double* __restrict__ partial,
                                                                    const int* __restrict__ preds, const int* __restrict__ gt,
                                                                    int B, int K, int H, double count, double* __restrict__ loss,
                                                                    float* __restrict__ acc, float* __restrict__ dists) {
    __shared__ double tile[KS_TILE];
    const int lane = threadIdx.x & (KS_WAVE - 1), wave = threadIdx.x / KS_WAVE;
    // one wave per channel: the counts are integers, so the order of their sum does not matter
    for (int k = wave; k < K; k += KS_THREADS / KS_WAVE) {      // (uniform over the wave)
        int valid = 0, hits = 0;
        for (int b = lane; b < B; b += KS_WAVE) {
            const size_t m = (size_t)b * K + k;
            const float d = ks_dist(preds[m * 2], preds[m * 2 + 1], gt[m * 2], gt[m * 2 + 1], H);
            dists[(size_t)k * B + b] = d;
            if (d != -1.0f) {
                ++valid;
                hits += d <= 0.5f;
            }
        }
        for (int o = KS_WAVE / 2; o > 0; o >>= 1) {
            valid += __shfl_down(valid, o, KS_WAVE);
            hits += __shfl_down(hits, o, KS_WAVE);
        }
        if (lane == 0) acc[1 + k] = valid ? (float)hits / (float)valid : -1.0f;
    }
    // the B * K partial sums in index order: every lane fetches, thread 0 adds
    const int n = B * K;
    double sum = 0.0;
    for (int base = 0; base < n; base += KS_TILE) {
        const int cnt = n - base < KS_TILE ? n - base : KS_TILE;
        for (int i = threadIdx.x; i < cnt; i += KS_THREADS) tile[i] = partial[base + i];
        __syncthreads();
        if (threadIdx.x == 0)
            for (int i = 0; i < cnt; ++i) sum = sum + tile[i];
        __syncthreads();                        // (also: acc[1 ..] of this, the only, block is complete and visible)
    }
    if (threadIdx.x == 0) {
        *loss = sum / count;
        float avg = 0.0f;
        int cnt = 0;
        for (int k = 0; k < K; ++k) {
            const float a = acc[1 + k];
            if (a >= 0.0f) {
                avg = avg + a;
                ++cnt;
            }
        }
        acc[0] = cnt ? avg / (float)cnt : 0.0f;
    }
}

inline int ks_aligned(const void* p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace

void launch_kpd_inputs(const unsigned char* frames, int N, int H, int W, const int* frame_index, const float* ul,
                       const float* br, const float* gains, const unsigned char* blank, int B, int inpH, int inpW, float* inp,
                       hipStream_t s) {
    const long long total = (long long)B * 3 * inpH * ((inpW + 3) / 4);
    hipLaunchKernelGGL(ks_inputs_kernel, dim3(ks_grid(total)), dim3(KS_THREADS), 0, s, frames, N, H, W, frame_index, ul, br,
                       gains, blank, B, inpH, inpW, ks_aligned(inp), inp);
}

void launch_kpd_augment(const float* x, int B, int C, int H, int W, const unsigned char* flip, const double* cs, const int* perm,
                        float* y, hipStream_t s) {
    const long long total = (long long)B * C * H * ((W + 3) / 4);
    hipLaunchKernelGGL(ks_augment_kernel, dim3(ks_grid(total)), dim3(KS_THREADS), 0, s, x, B, C, H, W, flip, cs, perm,
                       ks_aligned(y), y);
}

void launch_heatmap_loss_acc(const float* out, const float* labels, const float* set_mask, int B, int K, int H, int W,
                             double* partial, double* loss, float* acc, int* preds, int* gt, float* dists, float* grad,
                             hipStream_t s) {
    const int maps = B * K;
    const double count = (double)maps * (double)(H * W);
    const int aligned = ks_aligned(out) && ks_aligned(labels) && (!set_mask || ks_aligned(set_mask)) && (!grad || ks_aligned(grad));
    hipLaunchKernelGGL(ks_loss_map_kernel, dim3(maps < 65535 ? maps : 65535), dim3(KS_THREADS), 0, s, out, labels, set_mask, maps,
                       H, W, (float)(2.0 / count), aligned, partial, preds, gt, grad);
    hipLaunchKernelGGL(ks_loss_finish_kernel, dim3(1), dim3(KS_THREADS), 0, s, partial, preds, gt, B, K, H, count, loss, acc, dists);
}

}  // namespace bp
