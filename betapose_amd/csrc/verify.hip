// Pose verification by gradient agreement on the device (gfx950; include/betapose_hip.h bp_image_gradients,
// bp_gradient_scores).  The arithmetic of one pixel is verify_math.inc, the text verify_host.cpp compiles
// too; here is who loops over what.
//   A block of 256 lanes owns a tile of 64 x 16 pixels of one image; a lane owns four consecutive pixels of one row.
//   vt_fill        the tile's gray with its 2-pixel halo, 20 rows x 68 columns of bytes, into LDS; border pixels are
//                  fetched through reflect-101.  Two paths, chosen per call:
//                    VEC   the row pitch 3 W is a multiple of 16 and the base is 16-byte aligned: every 16-byte word of a
//                          row lies wholly inside it, and a tile's left edge (3 * 64 k bytes) is aligned.  14 such words
//                          per halo row (the 16 bytes before the tile, its 192, the 16 after) are staged raw in LDS by one
//                          16-byte load each, and the grays are then made from LDS bytes.
//                    else  three byte loads per pixel straight from global memory.
//                  The gray rows have a pitch of 192 bytes = 48 dwords: a lane reads two dwords per row with ds_read_b32,
//                  whose banks are (a / 4) % 32 per 32-lane half; a half is 16 lanes of each of two rows, and 48 % 32 = 16
//                  puts the second row on the other 16 banks: conflict-free (pitch 72 would be 2-way on two banks).
//   vf_grad_kernel   one tile: unit gradients and magnitudes of its pixels (two 16-byte stores of gradients and one of
//                    magnitudes per lane where W % 4 == 0 and the outputs are 16-byte aligned, scalar stores otherwise).
//   vf_score_kernel  one tile of every render p = blockIdx.z, blockIdx.z + gridDim.z, ...: gray -> Sobel -> mask -> unit
//                    vector -> dot with the scene's -> sum and count.  A render's gradients never reach memory.  A tile
//                    whose gray with halo is one value has m2 = 0 everywhere: with min_sq > 0 nothing is kept and the
//                    block goes on to the next render before it touches the scene.  The lane's sum and count are combined
//                    by a wave shuffle tree, the four waves' through LDS, and lane 0 issues one 64-bit and one 32-bit
//                    integer atomicAdd into the pose's own output row (skipped when the block kept nothing).
//   vf_init_kernel / vf_finish_kernel   one lane per pose: the row is zeroed (count -1 for a frame index outside [0, T)),
//                    and afterwards score = sum / 2^24 / (count + 1) (NaN for such a row).  No workspace.
// Integer sums do not depend on the order of their operands: the same bytes from run to run, equal to the host twin's.
// No floating-point atomics.  Bounds: a fetched pixel index is reflected and then clamped into [max(tile origin - 2, 0),
// size - 1], which changes no value a pixel of the image needs (H, W >= 3) and keeps every read inside the image and,
// on the VEC path, inside the staged words; a lane writes and counts only pixels with x < W and y < H.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "bp_common.h"
#include "verify.h"

#pragma clang fp contract(off)

namespace bp {

namespace {

#include "verify_math.inc"

constexpr int VT_THREADS = 256;
constexpr int VT_W = 64, VT_H = 16;                          // pixels of a tile: 16 lanes x 4 pixels, 16 rows
constexpr int VT_GW = VT_W + 2 * VF_HALO, VT_GH = VT_H + 2 * VF_HALO;
constexpr int VT_PITCH = 192;                                // bytes between gray rows in LDS
constexpr int VT_RAW_WORDS = 14, VT_RAW = VT_RAW_WORDS * 16; // staged bytes per halo row on the VEC path, from 3 x0 - 16
static_assert(3 * (VT_W + VF_HALO + 1) + 16 + 3 <= VT_RAW, "the staged words must cover the right halo");
static_assert(VT_W % 16 == 0 && (VT_W * 3) % 16 == 0, "a tile's left edge must be 16-byte aligned");

// where pixel index i of a tile row / column is fetched from: reflect-101, clamped (see the header)
__device__ __forceinline__ int vt_src(int i, int n, int lo) { return min(max(vf_reflect(i, n), lo), n - 1); }

// the gray of entry j = r * VT_GW + c of the halo tile: from the staged words (VEC) or from global memory
template <bool VEC>
__device__ __forceinline__ int vt_gray_at(const uint8_t* __restrict__ img, int H, int W, int x0, int y0, int xlo, int ylo, int red,
                                          const uint8_t* raw, int j, int& r, int& c) {
    r = j / VT_GW, c = j - r * VT_GW;
    const int x = vt_src(x0 - VF_HALO + c, W, xlo);
    const uint8_t* p;
    if (VEC) {
        p = raw + r * VT_RAW + (3 * (x - x0) + 16);
    } else {
        const int y = vt_src(y0 - VF_HALO + r, H, ylo);
        p = img + ((size_t)y * W + x) * 3;
    }
    return vf_gray(p[red], p[1], p[2 - red]);
}

// The gray tile of image `img` at (x0, y0) into gray [VT_GH][VT_PITCH]; raw [VT_GH][VT_RAW] is the VEC path's stage.
// Returns whether this lane met a gray other than the tile's first.  Ends WITHOUT a barrier.
template <bool VEC>
__device__ __forceinline__ bool vt_fill(const uint8_t* __restrict__ img, int H, int W, int x0, int y0, int red, uint8_t* gray,
                                        uint8_t* raw) {
    const int xlo = max(x0 - VF_HALO, 0), ylo = max(y0 - VF_HALO, 0);
    if (VEC) {
        const size_t pitch = (size_t)W * 3;
        for (int i = threadIdx.x; i < VT_GH * VT_RAW_WORDS; i += VT_THREADS) {
            const int r = i / VT_RAW_WORDS, k = i - r * VT_RAW_WORDS;
            const int y = vt_src(y0 - VF_HALO + r, H, ylo);
            const long long off = 3ll * x0 - 16 + 16 * k;                  // a whole word of the row, or none of it
            if (off >= 0 && off + 16 <= (long long)pitch)
                *reinterpret_cast<uint4*>(raw + r * VT_RAW + 16 * k) = *reinterpret_cast<const uint4*>(img + (size_t)y * pitch + off);
        }
        __syncthreads();
    }
    int r, c;
    const int first = vt_gray_at<VEC>(img, H, W, x0, y0, xlo, ylo, red, raw, 0, r, c);
    bool differ = false;
    for (int i = threadIdx.x; i < VT_GH * VT_GW; i += VT_THREADS) {
        const int g = vt_gray_at<VEC>(img, H, W, x0, y0, xlo, ylo, red, raw, i, r, c);
        gray[r * VT_PITCH + c] = (uint8_t)g;
        differ |= g != first;
    }
    return differ;
}

// gx, gy of the lane's four pixels (columns 4 lx .. 4 lx + 3 of tile row ly) from the gray tile
__device__ __forceinline__ void vt_sobel4(const uint8_t* gray, int lx, int ly, int* gx, int* gy) {
    uint32_t w[5][2];
#pragma unroll
    for (int k = 0; k < 5; ++k) {
        const uint32_t* row = reinterpret_cast<const uint32_t*>(gray + (ly + k) * VT_PITCH + 4 * lx);
        w[k][0] = row[0];
        w[k][1] = row[1];
    }
    int vs[8], vd[8];
#pragma unroll
    for (int c = 0; c < 8; ++c) {
        const int sh = 8 * (c & 3), h = c >> 2;
        vf_column((int)((w[0][h] >> sh) & 255u), (int)((w[1][h] >> sh) & 255u), (int)((w[2][h] >> sh) & 255u),
                  (int)((w[3][h] >> sh) & 255u), (int)((w[4][h] >> sh) & 255u), vs[c], vd[c]);
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) vf_row(vs + j, vd + j, gx[j], gy[j]);
}

// grid (ceil(W / 64), ceil(H / 16), min(I, 65535))
template <bool VEC>
__global__ __launch_bounds__(VT_THREADS) void vf_grad_kernel(const uint8_t* __restrict__ images, int I, int H, int W, int red,
                                                            int min_sq, int quads, float* __restrict__ grad,
                                                            float* __restrict__ mag) {
    __shared__ __attribute__((aligned(16))) uint8_t raw[VEC ? VT_GH * VT_RAW : 16];
    __shared__ __attribute__((aligned(16))) uint8_t gray[VT_GH * VT_PITCH];
    const int x0 = blockIdx.x * VT_W, y0 = blockIdx.y * VT_H;
    const int lx = threadIdx.x & 15, ly = threadIdx.x >> 4;
    const int x = x0 + 4 * lx, y = y0 + ly;
    const size_t HW = (size_t)H * W;
    for (int i = blockIdx.z; i < I; i += gridDim.z) {
        vt_fill<VEC>(images + (size_t)i * HW * 3, H, W, x0, y0, red, gray, raw);
        __syncthreads();
        if (x < W && y < H) {
            int gx[4], gy[4];
            vt_sobel4(gray, lx, ly, gx, gy);
            VfUnit u[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) vf_unit(gx[j], gy[j], min_sq, u[j]);
            const size_t q = (size_t)i * HW + (size_t)y * W + x;
            if (quads) {                                                   // W % 4 == 0: x + 3 < W
                float4* g = reinterpret_cast<float4*>(grad + 2 * q);
                g[0] = make_float4(u[0].nx, u[0].ny, u[1].nx, u[1].ny);
                g[1] = make_float4(u[2].nx, u[2].ny, u[3].nx, u[3].ny);
                if (mag) *reinterpret_cast<float4*>(mag + q) = make_float4(u[0].mag, u[1].mag, u[2].mag, u[3].mag);
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (x + j < W) {
                        grad[2 * (q + j)] = u[j].nx;
                        grad[2 * (q + j) + 1] = u[j].ny;
                        if (mag) mag[q + j] = u[j].mag;
                    }
            }
        }
        __syncthreads();                                                   // the tile is free for the next image
    }
}

// grid (ceil(W / 64), ceil(H / 16), min(P, 65535))
template <bool VEC>
__global__ __launch_bounds__(VT_THREADS) void vf_score_kernel(const uint8_t* __restrict__ renders,
                                                             const float* __restrict__ scene_grad,
                                                             const int* __restrict__ frame_index, int P, int T, int H, int W,
                                                             int red, int min_sq, int quads, unsigned long long* __restrict__ sum,
                                                             int* __restrict__ count) {
    __shared__ __attribute__((aligned(16))) uint8_t raw[VEC ? VT_GH * VT_RAW : 16];
    __shared__ __attribute__((aligned(16))) uint8_t gray[VT_GH * VT_PITCH];
    __shared__ unsigned long long wsum[VT_THREADS / 64];
    __shared__ int wcount[VT_THREADS / 64];
    const int x0 = blockIdx.x * VT_W, y0 = blockIdx.y * VT_H;
    const int lx = threadIdx.x & 15, ly = threadIdx.x >> 4;
    const int x = x0 + 4 * lx, y = y0 + ly;
    const size_t HW = (size_t)H * W;
    for (int p = blockIdx.z; p < P; p += gridDim.z) {                      // (everything that leaves early is uniform over the block)
        const int fi = frame_index[p];
        if (fi < 0 || fi >= T) continue;
        const bool differ = vt_fill<VEC>(renders + (size_t)p * HW * 3, H, W, x0, y0, red, gray, raw);
        if (!__syncthreads_or(differ) && min_sq > 0) continue;             // one gray: m2 = 0 < min_sq at every pixel
        unsigned long long s = 0;
        int c = 0;
        if (x < W && y < H) {
            int gx[4], gy[4];
            vt_sobel4(gray, lx, ly, gx, gy);
            VfUnit u[4];
            bool kept[4], any = false;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                kept[j] = x + j < W && vf_unit(gx[j], gy[j], min_sq, u[j]);
                any |= kept[j];
            }
            if (any) {
                const float* sg = scene_grad + 2 * ((size_t)fi * HW + (size_t)y * W + x);
                float sn[8];
                if (quads) {                                               // W % 4 == 0: x + 3 < W
                    const float4 a = reinterpret_cast<const float4*>(sg)[0], b = reinterpret_cast<const float4*>(sg)[1];
                    sn[0] = a.x, sn[1] = a.y, sn[2] = a.z, sn[3] = a.w, sn[4] = b.x, sn[5] = b.y, sn[6] = b.z, sn[7] = b.w;
                } else {
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        sn[2 * j] = kept[j] ? sg[2 * j] : 0.0f;
                        sn[2 * j + 1] = kept[j] ? sg[2 * j + 1] : 0.0f;
                    }
                }
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (kept[j]) {
                        ++c;
                        s += vf_term(u[j].nx, u[j].ny, sn[2 * j], sn[2 * j + 1]);
                    }
            }
        }
        uint32_t lo = (uint32_t)s, hi = (uint32_t)(s >> 32);               // (a lane's sum fits 32 bits, a wave's need not)
        unsigned long long ws = s;
        for (int o = 32; o > 0; o >>= 1) {
            const uint32_t l2 = __shfl_down(lo, o, 64), h2 = __shfl_down(hi, o, 64);
            ws += ((unsigned long long)h2 << 32) | l2;
            lo = (uint32_t)ws, hi = (uint32_t)(ws >> 32);
            c += __shfl_down(c, o, 64);
        }
        if ((threadIdx.x & 63) == 0) {
            wsum[threadIdx.x >> 6] = ws;
            wcount[threadIdx.x >> 6] = c;
        }
        __syncthreads();                                                   // also: the tile is free for the next render
        if (threadIdx.x == 0) {
            unsigned long long bs = 0;
            int bc = 0;
#pragma unroll
            for (int w = 0; w < VT_THREADS / 64; ++w) bs += wsum[w], bc += wcount[w];
            if (bc > 0) {
                atomicAdd(&sum[p], bs);
                atomicAdd(&count[p], bc);
            }
        }
    }
}

__global__ __launch_bounds__(VT_THREADS) void vf_init_kernel(const int* __restrict__ frame_index, int P, int T,
                                                            unsigned long long* __restrict__ sum, int* __restrict__ count) {
    const int p = blockIdx.x * VT_THREADS + threadIdx.x;
    if (p >= P) return;
    const int fi = frame_index[p];
    sum[p] = 0;
    count[p] = fi < 0 || fi >= T ? -1 : 0;
}

__global__ __launch_bounds__(VT_THREADS) void vf_finish_kernel(int P, const unsigned long long* __restrict__ sum,
                                                              const int* __restrict__ count, double* __restrict__ score) {
    const int p = blockIdx.x * VT_THREADS + threadIdx.x;
    if (p >= P) return;
    score[p] = count[p] < 0 ? vf_no_score() : vf_score(sum[p], count[p]);
}

inline bool aligned_to(const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

inline dim3 tile_grid(int H, int W, int n) { return dim3((W + VT_W - 1) / VT_W, (H + VT_H - 1) / VT_H, n < 65535 ? n : 65535); }

}  // namespace

void launch_image_gradients(const uint8_t* d_images, int I, int H, int W, int red_channel, int min_sq, float* d_grad,
                            float* d_mag, hipStream_t s) {
    const bool vec = (3ll * W) % 16 == 0 && aligned_to(d_images, 16);
    const int quads = W % 4 == 0 && aligned_to(d_grad, 16) && (!d_mag || aligned_to(d_mag, 16));
    if (vec)
        hipLaunchKernelGGL(vf_grad_kernel<true>, tile_grid(H, W, I), dim3(VT_THREADS), 0, s, d_images, I, H, W, red_channel, min_sq,
                           quads, d_grad, d_mag);
    else
        hipLaunchKernelGGL(vf_grad_kernel<false>, tile_grid(H, W, I), dim3(VT_THREADS), 0, s, d_images, I, H, W, red_channel, min_sq,
                           quads, d_grad, d_mag);
    BP_HIP(hipGetLastError());
}

void launch_gradient_scores(const uint8_t* d_renders, const float* d_scene_grad, const int* d_frame_index, int P, int T, int H,
                            int W, int red_channel, int render_min_sq, unsigned long long* d_sum, int* d_count, double* d_score,
                            hipStream_t s) {
    const bool vec = (3ll * W) % 16 == 0 && aligned_to(d_renders, 16);
    const int quads = W % 4 == 0 && aligned_to(d_scene_grad, 16);
    const unsigned rows = (unsigned)((P + VT_THREADS - 1) / VT_THREADS);
    hipLaunchKernelGGL(vf_init_kernel, dim3(rows), dim3(VT_THREADS), 0, s, d_frame_index, P, T, d_sum, d_count);
    if (vec)
        hipLaunchKernelGGL(vf_score_kernel<true>, tile_grid(H, W, P), dim3(VT_THREADS), 0, s, d_renders, d_scene_grad, d_frame_index,
                           P, T, H, W, red_channel, render_min_sq, quads, d_sum, d_count);
    else
        hipLaunchKernelGGL(vf_score_kernel<false>, tile_grid(H, W, P), dim3(VT_THREADS), 0, s, d_renders, d_scene_grad, d_frame_index,
                           P, T, H, W, red_channel, render_min_sq, quads, d_sum, d_count);
    hipLaunchKernelGGL(vf_finish_kernel, dim3(rows), dim3(VT_THREADS), 0, s, P, d_sum, d_count, d_score);
    BP_HIP(hipGetLastError());
}

}  // namespace bp
