// Training-scene synthesiser on the device (gfx950; include/betapose_hip.h bp_synth_background, bp_synth_windows,
// bp_synth_compose, bp_synth_sensor_depth).  The arithmetic of one pixel is synth_math.inc, the text synth_host.cpp
// compiles too: integers and fixed point only, keyed by the pixel's own coordinates, so nothing depends on the launch
// geometry and the images equal the host twins' byte for byte.
//   1. background_kernel, one lane per pixel.  A block owns 256 consecutive pixels of an image = 768 output bytes; it
//      stages them in LDS and 48 lanes store them as 16-byte words when the image's byte range is 16-byte aligned.
//   2. windows_kernel, one lane per pixel, four taps of the photograph bank.
//   3. compose_kernel, the hot one: a block of 256 lanes (four wave64) owns a tile of 64 x 16 pixels.
//        A. colour and the depth > 0 flag of the tile plus a halo of r + 1, packed into one dword per pixel in LDS; every
//           colour and depth byte of the image is read once per block;
//        B. the pasted value (inside feather over the 3 x 3 flags) of the tile plus a halo of r, one dword per pixel;
//        C. the row pass of the binomial blur out of B's array, D. the column pass out of C's, then gain, offset, noise
//           and clamp in registers.
//      The arrays are dwords indexed by consecutive lanes: consecutive banks, no conflicts (ds_read_b32 / ds_write_b32
//      bank = dword index mod 32 within a 32-lane half).  16.7 KB of LDS per block.  A position outside the image holds
//      the value of the nearest pixel inside (clamped edges): it is computed FROM that pixel's coordinates, so the
//      paste, both blur passes and the host twin's whole-image loops agree.  Where W is a multiple of 16 the tile's
//      output rows (192 bytes) are staged in LDS and stored as 16-byte words.  No atomics.
//   4. sensor_depth_kernel, one lane per pixel, nine depth reads (eight of them cache hits).
// The per-image tables travel as kernel arguments, SY_CHUNK images per launch: no device allocation, no synchronisation.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "bp_common.h"
#include "synth.h"

#pragma clang fp contract(off)

namespace bp {

namespace {

#include "synth_math.inc"

constexpr int SY_THREADS = 256;
constexpr int SY_CHUNK = 64;                                  // images per launch: 64 x 9 ints of kernel arguments
constexpr int SY_TW = 64, SY_TH = 16;                         // the compose tile
constexpr int SY_H1 = SY_MAX_RADIUS + 1;                      // halo of the colour / flag array
constexpr int SY_SW = SY_TW + 2 * SY_H1, SY_SH = SY_TH + 2 * SY_H1;                        // 70 x 22
constexpr int SY_PW = SY_TW + 2 * SY_MAX_RADIUS, SY_PH = SY_TH + 2 * SY_MAX_RADIUS;        // 68 x 20
constexpr int SY_ROW_BYTES = SY_TW * 3;                       // 192 = 12 x 16
static_assert(SY_TH * SY_ROW_BYTES <= SY_SH * SY_SW * 4, "the output rows are staged in the colour / flag array");
static_assert(SY_THREADS == 4 * SY_TW && SY_TH == 16, "a lane keeps one column and four rows of the tile");

struct ComposeTable {
    int v[SY_CHUNK * SY_PARAMS];
};
struct SensorTable {
    int v[SY_CHUNK * SY_DEPTH_PARAMS];
};
struct WindowTable {
    int v[SY_CHUNK * SY_WINDOW];
};

__device__ __forceinline__ int sy_clamp0(int v, int hi) { return v < 0 ? 0 : (v > hi ? hi : v); }

// grid (ceil(H W / 256), images); vec: every image's byte range starts 16-byte aligned
__global__ __launch_bounds__(SY_THREADS) void background_kernel(int H, int W, uint32_t seed, uint32_t first_image, int vec,
                                                                unsigned char* __restrict__ out) {
    __shared__ __attribute__((aligned(16))) unsigned char stage[SY_THREADS * 3];
    const uint32_t image = first_image + blockIdx.y;
    const int px = H * W;
    const int first = blockIdx.x * SY_THREADS, at = first + threadIdx.x;
    unsigned char* o = out + (size_t)blockIdx.y * px * 3;
    const bool whole = vec && first + SY_THREADS <= px;         // block-uniform
    unsigned char v[3] = {0, 0, 0};
    if (at < px) {
        const SyBackground b = sy_background(seed, image);
        const uint32_t key = sy_image_key(seed, SY_STREAM_LATTICE, image);
        const int y = at / W, x = at - y * W;
#pragma unroll
        for (uint32_t c = 0; c < 3; ++c) v[c] = sy_background_pixel(b, key, x, y, c);
    }
    if (!whole) {
        if (at < px) {
#pragma unroll
            for (int c = 0; c < 3; ++c) o[(size_t)at * 3 + c] = v[c];
        }
        return;
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) stage[threadIdx.x * 3 + c] = v[c];
    __syncthreads();
    if (threadIdx.x < SY_THREADS * 3 / 16)
        reinterpret_cast<uint4*>(o + (size_t)first * 3)[threadIdx.x] = reinterpret_cast<const uint4*>(stage)[threadIdx.x];
}

// grid (ceil(H W / 256), images)
__global__ __launch_bounds__(SY_THREADS) void windows_kernel(const unsigned char* __restrict__ bank, int Hb, int Wb, WindowTable tab,
                                                             int H, int W, unsigned char* __restrict__ out) {
    const int* w = tab.v + blockIdx.y * SY_WINDOW;
    const int px = H * W, at = blockIdx.x * SY_THREADS + threadIdx.x;
    if (at >= px) return;
    const int y = at / W, x = at - y * W;
    const unsigned char* src = bank + (size_t)w[0] * Hb * Wb * 3;
    const int v = sy_window_coord(y, H, w[4]), u = sy_window_coord(w[5] ? W - 1 - x : x, W, w[3]);
    const int iy = w[2] + (v >> 16), iy1 = w[2] + ((v >> 16) + 1 < w[4] ? (v >> 16) + 1 : w[4] - 1), fy = (v & 65535) >> 8;
    const int ix = w[1] + (u >> 16), ix1 = w[1] + ((u >> 16) + 1 < w[3] ? (u >> 16) + 1 : w[3] - 1), fx = (u & 65535) >> 8;
    unsigned char* o = out + ((size_t)blockIdx.y * px + at) * 3;
#pragma unroll
    for (int c = 0; c < 3; ++c)
        o[c] = sy_bilinear(src[((size_t)iy * Wb + ix) * 3 + c], src[((size_t)iy * Wb + ix1) * 3 + c],
                           src[((size_t)iy1 * Wb + ix) * 3 + c], src[((size_t)iy1 * Wb + ix1) * 3 + c], fx, fy);
}

__device__ __forceinline__ uint32_t sy_pack(int c0, int c1, int c2) { return (uint32_t)c0 | ((uint32_t)c1 << 8) | ((uint32_t)c2 << 16); }
__device__ __forceinline__ int sy_chan(uint32_t p, int c) { return (int)((p >> (8 * c)) & 255u); }

// grid (ceil(W / 64), ceil(H / 16), images); vec: W is a multiple of 16 and `out` is 16-byte aligned
__global__ __launch_bounds__(SY_THREADS) void compose_kernel(const unsigned char* __restrict__ background,
                                                             const unsigned char* __restrict__ color,
                                                             const float* __restrict__ depth, int H, int W, ComposeTable tab,
                                                             uint32_t seed, uint32_t first_image, int vec,
                                                             unsigned char* __restrict__ out) {
    __shared__ __attribute__((aligned(16))) uint32_t S[SY_SH * SY_SW];    // flag << 24 | colour, halo r + 1
    __shared__ uint32_t P[SY_PH * SY_PW];                                  // pasted, halo r
    __shared__ uint32_t R[SY_PH * SY_TW];                                  // after the row pass, rows with halo r
    const int* pr = tab.v + blockIdx.z * SY_PARAMS;
    const int feather = pr[0], r = pr[1];
    const int x0 = blockIdx.x * SY_TW, y0 = blockIdx.y * SY_TH;
    const size_t base = (size_t)blockIdx.z * H * W;
    const int t = threadIdx.x;

    // A: colour and flag at the in-image positions within r + 1 of the tile
    for (int i = t; i < SY_SH * SY_SW; i += SY_THREADS) {
        const int ry = i / SY_SW, rx = i - ry * SY_SW;
        const int gy = y0 - SY_H1 + ry, gx = x0 - SY_H1 + rx;
        const int off = SY_H1 - (r + 1);                                  // positions the radius does not need
        if (ry < off || ry >= SY_SH - off || rx < off || rx >= SY_SW - off || gy < 0 || gy >= H || gx < 0 || gx >= W) continue;
        const size_t at = base + (size_t)gy * W + gx;
        const unsigned char* c = color + at * 3;
        S[i] = sy_pack(c[0], c[1], c[2]) | (depth[at] > 0.0f ? 1u << 24 : 0u);
    }
    __syncthreads();

    // B: the pasted value at every position within r of the tile; one outside the image is its nearest pixel's
    for (int i = t; i < SY_PH * SY_PW; i += SY_THREADS) {
        const int py = i / SY_PW, px = i - py * SY_PW;
        const int off = SY_MAX_RADIUS - r;
        if (py < off || py >= SY_PH - off || px < off || px >= SY_PW - off) continue;
        const int qy = sy_clamp0(y0 - SY_MAX_RADIUS + py, H - 1), qx = sy_clamp0(x0 - SY_MAX_RADIUS + px, W - 1);
        const unsigned char* b = background + (base + (size_t)qy * W + qx) * 3;
        const int b0 = b[0], b1 = b[1], b2 = b[2];
        const uint32_t s = S[(qy - y0 + SY_H1) * SY_SW + (qx - x0 + SY_H1)];
        uint32_t v = sy_pack(b0, b1, b2);
        if (s >> 24) {
            int a = 9;
            if (feather) {
                a = 0;
#pragma unroll
                for (int dy = -1; dy <= 1; ++dy)
#pragma unroll
                    for (int dx = -1; dx <= 1; ++dx)
                        a += (int)(S[(sy_clamp0(qy + dy, H - 1) - y0 + SY_H1) * SY_SW + (sy_clamp0(qx + dx, W - 1) - x0 + SY_H1)] >> 24);
            }
            v = sy_pack(sy_paste(a, sy_chan(s, 0), b0), sy_paste(a, sy_chan(s, 1), b1), sy_paste(a, sy_chan(s, 2), b2));
        }
        P[i] = v;
    }
    __syncthreads();

    // C: rows first
    for (int i = t; i < SY_PH * SY_TW; i += SY_THREADS) {
        const int py = i / SY_TW, x = i - py * SY_TW;
        const int off = SY_MAX_RADIUS - r;
        if (py < off || py >= SY_PH - off) continue;
        int s0 = 0, s1 = 0, s2 = 0;
        for (int k = -r; k <= r; ++k) {
            const uint32_t p = P[py * SY_PW + x + SY_MAX_RADIUS + k];
            const int w = sy_binomial(r, k);
            s0 += w * sy_chan(p, 0);
            s1 += w * sy_chan(p, 1);
            s2 += w * sy_chan(p, 2);
        }
        R[i] = sy_pack(sy_blur_round(s0, r), sy_blur_round(s1, r), sy_blur_round(s2, r));
    }
    __syncthreads();

    // D: then columns, and the rest in registers.  Lane t keeps column t % 64 and the rows t / 64 + 4 j.
    const bool whole = vec && x0 + SY_TW <= W;                             // block-uniform
    unsigned char* stage = reinterpret_cast<unsigned char*>(S);            // S is dead: every read of it was before C's barrier
    const uint32_t key = sy_image_key(seed, SY_STREAM_NOISE, first_image + blockIdx.z);
    const int x = t & (SY_TW - 1), gx = x0 + x;
#pragma unroll
    for (int j = 0; j < SY_TH / 4; ++j) {
        const int y = (t >> 6) + 4 * j, gy = y0 + y;
        if (gx >= W || gy >= H) continue;
        int s[3] = {0, 0, 0};
        for (int k = -r; k <= r; ++k) {
            const uint32_t p = R[(y + SY_MAX_RADIUS + k) * SY_TW + x];
            const int w = sy_binomial(r, k);
#pragma unroll
            for (int c = 0; c < 3; ++c) s[c] += w * sy_chan(p, c);
        }
        const uint32_t pixel = (uint32_t)(gy * W + gx);
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const unsigned char v = sy_finish(sy_blur_round(s[c], r), pr[2 + c], pr[5 + c], pr[8], key, pixel, (uint32_t)c);
            if (whole)
                stage[y * SY_ROW_BYTES + x * 3 + c] = v;
            else
                out[(base + pixel) * 3 + c] = v;
        }
    }
    if (!whole) return;
    __syncthreads();
    if (t < SY_TH * (SY_ROW_BYTES / 16)) {
        const int y = t / (SY_ROW_BYTES / 16), seg = t - y * (SY_ROW_BYTES / 16);
        if (y0 + y < H)
            reinterpret_cast<uint4*>(out + (base + (size_t)(y0 + y) * W + x0) * 3)[seg] =
                reinterpret_cast<const uint4*>(stage + y * SY_ROW_BYTES)[seg];
    }
}

// grid (ceil(H W / 256), images)
__global__ __launch_bounds__(SY_THREADS) void sensor_depth_kernel(const float* __restrict__ depth, int H, int W, double depth_scale,
                                                                  SensorTable tab, uint32_t seed, uint32_t first_image,
                                                                  uint16_t* __restrict__ out) {
    const int* p = tab.v + blockIdx.y * SY_DEPTH_PARAMS;
    const int px = H * W, at = blockIdx.x * SY_THREADS + threadIdx.x;
    if (at >= px) return;
    const int y = at / W, x = at - y * W;
    const float* d = depth + (size_t)blockIdx.y * px;
    uint32_t lo = 65535u, hi = 0, centre = 0;
#pragma unroll
    for (int dy = -1; dy <= 1; ++dy)
#pragma unroll
        for (int dx = -1; dx <= 1; ++dx) {
            const uint32_t v = sy_count(d[(size_t)sy_clamp0(y + dy, H - 1) * W + sy_clamp0(x + dx, W - 1)], depth_scale);
            lo = v < lo ? v : lo;
            hi = v > hi ? v : hi;
            if (dy == 0 && dx == 0) centre = v;
        }
    const uint32_t image = first_image + blockIdx.y;
    out[(size_t)blockIdx.y * px + at] = sy_sensor(centre, hi - lo, p[0], p[1], p[2], sy_image_key(seed, SY_STREAM_DEPTH, image),
                                                  sy_image_key(seed, SY_STREAM_HOLE, image), (uint32_t)at);
}

inline unsigned pixel_blocks(int H, int W) { return (unsigned)(((size_t)H * W + SY_THREADS - 1) / SY_THREADS); }
inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

}  // namespace

void launch_synth_background(int I, int H, int W, uint32_t seed, uint32_t first_image, unsigned char* out, hipStream_t s) {
    const int vec = aligned16(out) && ((size_t)H * W * 3) % 16 == 0;
    for (int i0 = 0; i0 < I; i0 += SY_CHUNK) {
        const int n = I - i0 < SY_CHUNK ? I - i0 : SY_CHUNK;
        hipLaunchKernelGGL(background_kernel, dim3(pixel_blocks(H, W), n), dim3(SY_THREADS), 0, s, H, W, seed,
                           first_image + (uint32_t)i0, vec, out + (size_t)i0 * H * W * 3);
    }
    BP_HIP(hipGetLastError());
}

void launch_synth_windows(const unsigned char* bank, int Hb, int Wb, const int* windows, int I, int H, int W, unsigned char* out,
                          hipStream_t s) {
    for (int i0 = 0; i0 < I; i0 += SY_CHUNK) {
        const int n = I - i0 < SY_CHUNK ? I - i0 : SY_CHUNK;
        WindowTable tab = {};
        for (int k = 0; k < n * SY_WINDOW; ++k) tab.v[k] = windows[(size_t)i0 * SY_WINDOW + k];
        hipLaunchKernelGGL(windows_kernel, dim3(pixel_blocks(H, W), n), dim3(SY_THREADS), 0, s, bank, Hb, Wb, tab, H, W,
                           out + (size_t)i0 * H * W * 3);
    }
    BP_HIP(hipGetLastError());
}

void launch_synth_compose(const unsigned char* background, const unsigned char* color, const float* depth, int I, int H, int W,
                          const int* params, uint32_t seed, uint32_t first_image, unsigned char* out, hipStream_t s) {
    const int vec = aligned16(out) && W % 16 == 0;
    for (int i0 = 0; i0 < I; i0 += SY_CHUNK) {
        const int n = I - i0 < SY_CHUNK ? I - i0 : SY_CHUNK;
        ComposeTable tab = {};
        for (int k = 0; k < n * SY_PARAMS; ++k) tab.v[k] = params[(size_t)i0 * SY_PARAMS + k];
        const size_t at = (size_t)i0 * H * W;
        hipLaunchKernelGGL(compose_kernel, dim3((W + SY_TW - 1) / SY_TW, (H + SY_TH - 1) / SY_TH, n), dim3(SY_THREADS), 0, s,
                           background + at * 3, color + at * 3, depth + at, H, W, tab, seed, first_image + (uint32_t)i0, vec,
                           out + at * 3);
    }
    BP_HIP(hipGetLastError());
}

void launch_synth_sensor_depth(const float* depth, int I, int H, int W, double depth_scale, const int* params, uint32_t seed,
                               uint32_t first_image, uint16_t* out, hipStream_t s) {
    for (int i0 = 0; i0 < I; i0 += SY_CHUNK) {
        const int n = I - i0 < SY_CHUNK ? I - i0 : SY_CHUNK;
        SensorTable tab = {};
        for (int k = 0; k < n * SY_DEPTH_PARAMS; ++k) tab.v[k] = params[(size_t)i0 * SY_DEPTH_PARAMS + k];
        const size_t at = (size_t)i0 * H * W;
        hipLaunchKernelGGL(sensor_depth_kernel, dim3(pixel_blocks(H, W), n), dim3(SY_THREADS), 0, s, depth + at, H, W, depth_scale,
                           tab, seed, first_image + (uint32_t)i0, out + at);
    }
    BP_HIP(hipGetLastError());
}

}  // namespace bp
