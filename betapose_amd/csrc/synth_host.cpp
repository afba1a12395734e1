// Host twins of the training-scene synthesiser (include/betapose_hip.h bp_synth_*_host): plain loops over images and
// pixels around the arithmetic of synth_math.inc, the text synth.hip compiles too.  Every value is an integer function
// of the inputs and the pixel's own coordinates, so these images and the kernels' are equal byte for byte.
#include <cstdint>
#include <vector>

#include "synth.h"

#pragma clang fp contract(off)

namespace bp {

namespace {
#include "synth_math.inc"

inline int clampi(int v, int hi) { return v < 0 ? 0 : (v > hi ? hi : v); }
}  // namespace

void synth_background_host(int I, int H, int W, uint32_t seed, uint32_t first_image, unsigned char* out) {
    for (int i = 0; i < I; ++i) {
        const SyBackground b = sy_background(seed, first_image + (uint32_t)i);
        const uint32_t key = sy_image_key(seed, SY_STREAM_LATTICE, first_image + (uint32_t)i);
        unsigned char* o = out + (size_t)i * H * W * 3;
        for (int y = 0; y < H; ++y)
            for (int x = 0; x < W; ++x)
                for (uint32_t c = 0; c < 3; ++c) o[((size_t)y * W + x) * 3 + c] = sy_background_pixel(b, key, x, y, c);
    }
}

void synth_windows_host(const unsigned char* bank, int Hb, int Wb, const int* windows, int I, int H, int W, unsigned char* out) {
    for (int i = 0; i < I; ++i) {
        const int* w = windows + (size_t)i * SY_WINDOW;
        const unsigned char* src = bank + (size_t)w[0] * Hb * Wb * 3;
        unsigned char* o = out + (size_t)i * H * W * 3;
        for (int y = 0; y < H; ++y) {
            const int v = sy_window_coord(y, H, w[4]);
            const int iy = w[2] + (v >> 16), iy1 = w[2] + ((v >> 16) + 1 < w[4] ? (v >> 16) + 1 : w[4] - 1), fy = (v & 65535) >> 8;
            for (int x = 0; x < W; ++x) {
                const int u = sy_window_coord(w[5] ? W - 1 - x : x, W, w[3]);
                const int ix = w[1] + (u >> 16), ix1 = w[1] + ((u >> 16) + 1 < w[3] ? (u >> 16) + 1 : w[3] - 1), fx = (u & 65535) >> 8;
                for (int c = 0; c < 3; ++c)
                    o[((size_t)y * W + x) * 3 + c] =
                        sy_bilinear(src[((size_t)iy * Wb + ix) * 3 + c], src[((size_t)iy * Wb + ix1) * 3 + c],
                                    src[((size_t)iy1 * Wb + ix) * 3 + c], src[((size_t)iy1 * Wb + ix1) * 3 + c], fx, fy);
            }
        }
    }
}

void synth_compose_host(const unsigned char* background, const unsigned char* color, const float* depth, int I, int H, int W,
                        const int* params, uint32_t seed, uint32_t first_image, unsigned char* out) {
    const size_t px = (size_t)H * W;
    std::vector<unsigned char> pasted(px * 3), rows(px * 3);
    for (int i = 0; i < I; ++i) {
        const int* p = params + (size_t)i * SY_PARAMS;
        const int feather = p[0], r = p[1];
        const unsigned char* bg = background + (size_t)i * px * 3;
        const unsigned char* fg = color + (size_t)i * px * 3;
        const float* d = depth + (size_t)i * px;
        for (int y = 0; y < H; ++y)
            for (int x = 0; x < W; ++x) {
                const size_t at = (size_t)y * W + x;
                int a = 9;
                if (d[at] > 0.0f && feather) {
                    a = 0;
                    for (int dy = -1; dy <= 1; ++dy)
                        for (int dx = -1; dx <= 1; ++dx) a += d[(size_t)clampi(y + dy, H - 1) * W + clampi(x + dx, W - 1)] > 0.0f;
                }
                for (int c = 0; c < 3; ++c)
                    pasted[at * 3 + c] = d[at] > 0.0f ? (unsigned char)sy_paste(a, fg[at * 3 + c], bg[at * 3 + c]) : bg[at * 3 + c];
            }
        for (int y = 0; y < H; ++y)                   // rows first
            for (int x = 0; x < W; ++x)
                for (int c = 0; c < 3; ++c) {
                    int s = 0;
                    for (int k = -r; k <= r; ++k) s += sy_binomial(r, k) * pasted[((size_t)y * W + clampi(x + k, W - 1)) * 3 + c];
                    rows[((size_t)y * W + x) * 3 + c] = (unsigned char)sy_blur_round(s, r);
                }
        const uint32_t key = sy_image_key(seed, SY_STREAM_NOISE, first_image + (uint32_t)i);
        unsigned char* o = out + (size_t)i * px * 3;
        for (int y = 0; y < H; ++y)                   // then columns, gain, offset, noise, clamp
            for (int x = 0; x < W; ++x)
                for (int c = 0; c < 3; ++c) {
                    int s = 0;
                    for (int k = -r; k <= r; ++k) s += sy_binomial(r, k) * rows[((size_t)clampi(y + k, H - 1) * W + x) * 3 + c];
                    o[((size_t)y * W + x) * 3 + c] =
                        sy_finish(sy_blur_round(s, r), p[2 + c], p[5 + c], p[8], key, (uint32_t)(y * W + x), (uint32_t)c);
                }
    }
}

void synth_sensor_depth_host(const float* depth, int I, int H, int W, double depth_scale, const int* params, uint32_t seed,
                             uint32_t first_image, uint16_t* out) {
    const size_t px = (size_t)H * W;
    std::vector<uint32_t> counts(px);
    for (int i = 0; i < I; ++i) {
        const int* p = params + (size_t)i * SY_DEPTH_PARAMS;
        for (size_t at = 0; at < px; ++at) counts[at] = sy_count(depth[(size_t)i * px + at], depth_scale);
        const uint32_t nkey = sy_image_key(seed, SY_STREAM_DEPTH, first_image + (uint32_t)i);
        const uint32_t hkey = sy_image_key(seed, SY_STREAM_HOLE, first_image + (uint32_t)i);
        for (int y = 0; y < H; ++y)
            for (int x = 0; x < W; ++x) {
                uint32_t lo = 65535u, hi = 0;
                for (int dy = -1; dy <= 1; ++dy)
                    for (int dx = -1; dx <= 1; ++dx) {
                        const uint32_t v = counts[(size_t)clampi(y + dy, H - 1) * W + clampi(x + dx, W - 1)];
                        lo = v < lo ? v : lo;
                        hi = v > hi ? v : hi;
                    }
                out[(size_t)i * px + (size_t)y * W + x] =
                    sy_sensor(counts[(size_t)y * W + x], hi - lo, p[0], p[1], p[2], nkey, hkey, (uint32_t)(y * W + x));
            }
    }
}

}  // namespace bp
