// The training-scene synthesiser's per-pixel arithmetic, ONE source for the host twins (synth_host.cpp) and the device
// kernels (synth.hip): the stateless random source, the lattice-noise background, the window resampler, the paste with
// its inside feather, the binomial blur weights, gain / offset / noise, and the depth-sensor model (DESIGN.md 3.15).
// Everything is integer or fixed point: no libm, no floating-point reduction, nothing that depends on who computes a
// pixel or in which order, so host and device agree byte for byte by construction.  The ONE place a float is read is
// sy_count (depth in metres -> sensor counts); its rounding is pinned there.
// Plain C++17, no HIP header.  Included inside `namespace bp { namespace {` after <cstdint> and synth.h, in a unit that
// has `#pragma clang fp contract(off)` in force.
#ifndef BP_HD
#if defined(__HIPCC__)
#define BP_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define BP_HD inline
#endif
#endif

// ---- the random source: a 32-bit mix keyed by (seed, stream, image, pixel, channel).  `image` is the GLOBAL scene
// number (first_image + index within the call), so a scene's bytes do not depend on how the scenes are chunked.
constexpr uint32_t SY_STREAM_NOISE = 0;      // camera noise of compose
constexpr uint32_t SY_STREAM_LATTICE = 1;    // lattice values of the procedural background
constexpr uint32_t SY_STREAM_BG = 2;         // per-image background parameters (octave weights, base colour, contrast)
constexpr uint32_t SY_STREAM_DEPTH = 3;      // depth-sensor noise
constexpr uint32_t SY_STREAM_HOLE = 4;       // depth-sensor holes
constexpr int SY_NOISE_MEAN = 1530;          // 12 bytes x 127.5
constexpr int SY_OCTAVES = 4;                // lattice cells of 64, 32, 16 and 8 pixels

BP_HD uint32_t sy_fmix(uint32_t h) {         // MurmurHash3's 32-bit finaliser: a bijection of the 32-bit words
    h ^= h >> 16;
    h *= 0x85EBCA6Bu;
    h ^= h >> 13;
    h *= 0xC2B2AE35u;
    h ^= h >> 16;
    return h;
}
BP_HD uint32_t sy_absorb(uint32_t h, uint32_t k) { return sy_fmix(h ^ k) + 0x9E3779B9u; }
// the part of a draw's key that a whole image shares
BP_HD uint32_t sy_image_key(uint32_t seed, uint32_t stream, uint32_t image) {
    return sy_absorb(sy_absorb(sy_absorb(0x243F6A88u, seed), stream), image);
}
BP_HD uint32_t sy_draw(uint32_t image_key, uint32_t pixel, uint32_t channel) {
    return sy_fmix(sy_absorb(sy_absorb(image_key, pixel), channel));
}
BP_HD int sy_byte_sum(uint32_t u) { return (int)((u & 255u) + ((u >> 8) & 255u) + ((u >> 16) & 255u) + (u >> 24)); }
// The Gaussian-like noise value: the 12 bytes of the draws (pixel, channel), (pixel, channel + 3), (pixel, channel + 6)
// summed, minus 1530 (Irwin-Hall of 12 uniform bytes): an integer in -1530 .. 1530 of mean exactly 0 and variance
// 12 (256^2 - 1) / 12 = 65 535, so value / 256 has the standard deviation 0.999992.
BP_HD int sy_noise(uint32_t image_key, uint32_t pixel, uint32_t channel) {
    int s = -SY_NOISE_MEAN;
#pragma unroll
    for (uint32_t j = 0; j < 3; ++j) s += sy_byte_sum(sy_draw(image_key, pixel, channel + 3u * j));
    return s;
}
// noise value times a Q8 sigma in units of 1/256 of the value, rounded half up (the shift of a negative is arithmetic)
BP_HD int sy_scale_noise(int noise, long long sigma_q8) { return (int)(((long long)noise * sigma_q8 + 32768) >> 16); }

BP_HD int sy_clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// ---- the procedural background: SY_OCTAVES octaves of lattice value noise.  Octave o has cells of 2^(6 - o) pixels;
// the lattice value at node (gx, gy) of channel c is the low byte of the draw (SY_STREAM_LATTICE, image,
// pixel = o << 28 | gy << 14 | gx, c).  Inside a cell the four corner bytes are mixed bilinearly with Q8 fractions, which
// gives a Q16 value, rounded half up to Q8.
BP_HD int sy_lattice(uint32_t key, int o, int gx, int gy, uint32_t c) {
    return (int)(sy_draw(key, ((uint32_t)o << 28) | ((uint32_t)gy << 14) | (uint32_t)gx, c) & 255u);
}
BP_HD int sy_octave_q8(uint32_t key, int o, int x, int y, uint32_t c) {
    const int sh = 6 - o, mask = (1 << sh) - 1;
    const int gx = x >> sh, gy = y >> sh, fx = (x & mask) << (8 - sh), fy = (y & mask) << (8 - sh);
    const int v00 = sy_lattice(key, o, gx, gy, c), v10 = sy_lattice(key, o, gx + 1, gy, c);
    const int v01 = sy_lattice(key, o, gx, gy + 1, c), v11 = sy_lattice(key, o, gx + 1, gy + 1, c);
    const int q16 = (256 - fx) * (256 - fy) * v00 + fx * (256 - fy) * v10 + (256 - fx) * fy * v01 + fx * fy * v11;
    return (q16 + 128) >> 8;
}
// per-image parameters, from (SY_STREAM_BG, image): octave weight w_o = ((byte of pixel o) + 1) >> o, base colour of
// channel c the byte of (pixel 8, channel c), amplitude 64 + (low 7 bits of pixel 9) in units of 1 / 128
struct SyBackground {
    int w[SY_OCTAVES], wsum, base[3], amp;
};
BP_HD SyBackground sy_background(uint32_t seed, uint32_t image) {
    const uint32_t key = sy_image_key(seed, SY_STREAM_BG, image);
    SyBackground b;
    b.wsum = 0;
#pragma unroll
    for (int o = 0; o < SY_OCTAVES; ++o) {
        b.w[o] = (int)((sy_draw(key, (uint32_t)o, 0) & 255u) + 1u) >> o;
        b.wsum += b.w[o];
    }
#pragma unroll
    for (uint32_t c = 0; c < 3; ++c) b.base[c] = (int)(sy_draw(key, 8, c) & 255u);
    b.amp = 64 + (int)(sy_draw(key, 9, 0) & 127u);
    return b;
}
// t = sum_o w_o octave_o / wsum (Q8, integer division); the byte is base + ((t - 127.5 * 256) amp / 128) / 256, rounded
// half up, clamped
BP_HD unsigned char sy_background_pixel(const SyBackground& b, uint32_t lattice_key, int x, int y, uint32_t c) {
    int sum = 0;
#pragma unroll
    for (int o = 0; o < SY_OCTAVES; ++o) sum += b.w[o] * sy_octave_q8(lattice_key, o, x, y, c);
    const int t = sum / b.wsum;
    return (unsigned char)sy_clampi(b.base[c] + (((t - 32640) * b.amp + 16384) >> 15), 0, 255);
}

// ---- a window of a photograph resampled to W output pixels along one axis: the Q16 source coordinate of output pixel x
// (centres aligned: (x + 1/2) w / W - 1/2), clamped to the window
BP_HD int sy_window_coord(int x, int W, int w) {
    const long long u = ((long long)(2 * x + 1) * w * 32768) / W - 32768;
    const long long hi = (long long)(w - 1) << 16;
    return (int)(u < 0 ? 0 : (u > hi ? hi : u));
}
// bilinear mix of four bytes with Q8 fractions, rounded half up
BP_HD unsigned char sy_bilinear(int v00, int v10, int v01, int v11, int fx, int fy) {
    return (unsigned char)(((256 - fx) * (256 - fy) * v00 + fx * (256 - fy) * v10 + (256 - fx) * fy * v01 + fx * fy * v11 + 32768) >> 16);
}

// ---- compose.  params row of an image (SY_PARAMS ints): feather flag, blur radius r, gain[3] (Q8), offset[3], sigma (Q8)
// paste with the inside feather: a of the 9 neighbourhood pixels carry a fragment
BP_HD int sy_paste(int a, int fg, int bg) { return (a * fg + (9 - a) * bg + 4) / 9; }
// binomial weight k = -r .. r of radius r: [1], [1 2 1], [1 4 6 4 1]; a pass divides by 4^r = 1 << 2r, rounded half up
BP_HD int sy_binomial(int r, int k) {
    if (r == 0) return 1;
    if (r == 1) return k == 0 ? 2 : 1;
    return k == 0 ? 6 : ((k == 1 || k == -1) ? 4 : 1);
}
BP_HD int sy_blur_round(int sum, int r) { return r ? (sum + (1 << (2 * r - 1))) >> (2 * r) : sum; }
// gain, offset, noise, clamp of one blurred byte
BP_HD unsigned char sy_finish(int v, int gain_q8, int offset, int sigma_q8, uint32_t noise_key, uint32_t pixel, uint32_t c) {
    v = ((gain_q8 * v + 128) >> 8) + offset;
    if (sigma_q8) v += sy_scale_noise(sy_noise(noise_key, pixel, c), sigma_q8);
    return (unsigned char)sy_clampi(v, 0, 255);
}

// ---- the depth sensor.  params row (SY_DEPTH_PARAMS ints): noise_k, edge_counts, hole_p
// counts of a depth in metres: depth / depth_scale in f64 (one IEEE division), plus one half, truncated: round half up.
// Not positive (or NaN): 0, the missing value.  65 535 and above: 65 535.
BP_HD uint32_t sy_count(float depth, double depth_scale) {
    if (!(depth > 0.0f)) return 0;
    const double q = (double)depth / depth_scale + 0.5;
    return q >= 65535.0 ? 65535u : (uint32_t)q;
}
// sigma of the noise at `count`, in 1/256 count: noise_k count^2 / 2^20
BP_HD long long sy_depth_sigma_q8(int noise_k, uint32_t count) {
    return (long long)(((unsigned long long)noise_k * count * count) >> 20);
}
// the sensor's value of a pixel whose ideal count is `count` (> 0) and whose neighbourhood spans `span` counts
BP_HD uint16_t sy_sensor(uint32_t count, uint32_t span, int noise_k, int edge_counts, int hole_p, uint32_t noise_key,
                         uint32_t hole_key, uint32_t pixel) {
    if (count == 0) return 0;
    if (span > (uint32_t)edge_counts && hole_p > 0 && (int)(sy_draw(hole_key, pixel, 0) & 255u) < hole_p) return 0;
    long long v = count;
    if (noise_k) v += sy_scale_noise(sy_noise(noise_key, pixel, 0), sy_depth_sigma_q8(noise_k, count));
    return (uint16_t)(v < 0 ? 0 : (v > 65535 ? 65535 : v));
}
