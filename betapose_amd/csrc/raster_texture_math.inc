// The textured resolve's arithmetic of O(1) size, ONE source for the host twin (raster_texture_host.cpp) and the device
// kernels (raster_texture.hip): the packed mip pyramid's layout and box filter, the UV of a fragment and of its two
// neighbouring rays, the level rule, the fixed-point bilinear sampler and the shading of a textured fragment.  Host and
// device compile this text and do the same f64 / integer operations in the same order, without FMA contraction, so
// their images agree byte for byte.  Plain C++17, f64 and integers only, no libm call but floor and fabs.  Included right
// after raster_color_math.inc (it uses RcFrag, rc_fragment, rc_sub_area and rc_lit), in a unit that has
// `#pragma clang fp contract(off)` in force.  DESIGN.md §3.17 has the definition in words.

// ---- the pyramid: level 0 is the image, level l + 1 has ceil(w / 2) x ceil(h / 2) texels, down to 1 x 1.  A texel is
// one dword, channel k in byte k (the fourth byte is 0); the levels follow each other, level l at tx_level_offset.
constexpr int TX_MAX_SIZE = 8192;               // Wt, Ht above this are refused
constexpr int TX_MAX_LEVELS = 14;               // 8192 = 2^13: 14 levels
constexpr double TX_UV_RANGE = 1073741824.0;    // |u|, |v| are limited to 2^30 before the wrap: floor() stays exact

BP_HD int tx_half(int w) { return (w + 1) >> 1; }

// levels of the full chain of a w x h image: 1 + ceil(log2(max(w, h)))
BP_HD int tx_full_levels(int w, int h) {
    int levels = 1;
    while (w > 1 || h > 1) {
        w = tx_half(w);
        h = tx_half(h);
        ++levels;
    }
    return levels;
}

// texels before level `level`, and that level's size
BP_HD size_t tx_level_offset(int w, int h, int level, int* lw, int* lh) {
    size_t at = 0;
    for (int l = 0; l < level; ++l) {
        at += (size_t)w * h;
        w = tx_half(w);
        h = tx_half(h);
    }
    *lw = w;
    *lh = h;
    return at;
}

BP_HD uint32_t tx_pack(unsigned c0, unsigned c1, unsigned c2) { return c0 | (c1 << 8) | (c2 << 16); }

// texel (x, y) of the level below `src` [sh][sw]: (a + b + c + d + 2) >> 2 per channel over the 2 x 2 block, the partner
// index clamped to the edge where a dimension is odd
BP_HD uint32_t tx_box(const uint32_t* src, int sw, int sh, int x, int y) {
    const int x0 = 2 * x, y0 = 2 * y;                       // < sw, < sh: x < ceil(sw / 2)
    const int x1 = x0 + 1 < sw ? x0 + 1 : sw - 1, y1 = y0 + 1 < sh ? y0 + 1 : sh - 1;
    const uint32_t a = src[(size_t)y0 * sw + x0], b = src[(size_t)y0 * sw + x1];
    const uint32_t c = src[(size_t)y1 * sw + x0], d = src[(size_t)y1 * sw + x1];
    uint32_t out = 0;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const int s = 8 * k;
        out |= (((((a >> s) & 255u) + ((b >> s) & 255u)) + (((c >> s) & 255u) + ((d >> s) & 255u)) + 2u) >> 2) << s;
    }
    return out;
}

// ---- the fragment's texture coordinates
// (u, v) of the point where the ray (dx, dy, 1) meets the plane of the fragment's triangle, from the corner coordinates
// uv [3][2] by UNCLAMPED barycentrics: what the footprint is measured with.  A ray parallel to the plane gives
// infinities or NaNs, which the level rule and the sampler take.
BP_HD void tx_plane_uv(const RcFrag& g, const double* A, const double* B, const double* C, const double* uv, double dx, double dy,
                       double* u, double* v) {
    const double z = g.nd / ((g.nx * dx + g.ny * dy) + g.nz);
    const double X[3] = {z * dx, z * dy, z};
    const double a = rc_sub_area(B, C, X, g.nx, g.ny, g.nz) / g.nn;
    const double b = rc_sub_area(C, A, X, g.nx, g.ny, g.nz) / g.nn;
    const double c = rc_sub_area(A, B, X, g.nx, g.ny, g.nz) / g.nn;
    *u = (a * uv[0] + b * uv[2]) + c * uv[4];
    *v = (a * uv[1] + b * uv[3]) + c * uv[5];
}

// The level of a fragment: its footprint is the change of (u Wt, v Ht), level-0 texels, from the ray of pixel (x, y) to
// those of (x + 1, y) and (x, y + 1); rx, ry are the squared lengths of the two.  level = the number of l < levels - 1
// with rx > 4^l or ry > 4^l: ceil(log2 rho) of the longer one, limited to the pyramid.  Comparisons against exact powers
// of four only; every comparison with a NaN is false, so a NaN length counts for nothing (both NaN: level 0).
BP_HD int tx_level(double rx, double ry, int levels) {
    int level = 0;
    double t = 1.0;
    for (int l = 0; l < levels - 1; ++l) {
        level += (rx > t || ry > t) ? 1 : 0;
        t = t * 4.0;
    }
    return level;
}

BP_HD int tx_fragment_level(const RsCam& cam, const RcFrag& g, const double* A, const double* B, const double* C, const double* uv,
                            int x, int y, int Wt, int Ht, int levels) {
    if (levels <= 1) return 0;
    const double dx0 = (((double)x + cam.c) - cam.cx) / cam.fx, dy0 = (((double)y + cam.c) - cam.cy) / cam.fy;
    const double dx1 = (((double)(x + 1) + cam.c) - cam.cx) / cam.fx, dy1 = (((double)(y + 1) + cam.c) - cam.cy) / cam.fy;
    double u0, v0, ux, vx, uy, vy;
    tx_plane_uv(g, A, B, C, uv, dx0, dy0, &u0, &v0);
    tx_plane_uv(g, A, B, C, uv, dx1, dy0, &ux, &vx);
    tx_plane_uv(g, A, B, C, uv, dx0, dy1, &uy, &vy);
    const double ax = (ux - u0) * (double)Wt, bx = (vx - v0) * (double)Ht;
    const double ay = (uy - u0) * (double)Wt, by = (vy - v0) * (double)Ht;
    return tx_level(ax * ax + bx * bx, ay * ay + by * by, levels);
}

// ---- the sampler
// a coordinate into [0, 1]: NaN -> 0, the magnitude limited to 2^30, then u - floor(u) (1.0 itself can come out of a
// tiny negative u; the taps are wrapped again as integers)
BP_HD double tx_wrap01(double u) {
    if (!(u == u)) u = 0.0;
    if (u > TX_UV_RANGE) u = TX_UV_RANGE;
    if (u < -TX_UV_RANGE) u = -TX_UV_RANGE;
    return u - floor(u);
}

BP_HD int tx_mod(long long i, int n) {      // n > 0; the result lies in [0, n) whatever i
    const int r = (int)(i % (long long)n);
    return r < 0 ? r + n : r;
}

// Bilinear sample of one level (texels [h][w]) at (u, v), v upwards (v = 1 is the top row): s = u w - 0.5,
// t = (1 - v) h - 0.5, floor(256 s) and floor(256 t) give the texel index and an 8-bit fraction per axis, the four taps
// are wrapped modulo the level's size BEFORE the loads, a channel is
// ((c00 (256 - fx) + c10 fx) (256 - fy) + (c01 (256 - fx) + c11 fx) fy + 32768) >> 16.
BP_HD void tx_sample(const uint32_t* texels, int w, int h, double u, double v, int* out) {
    const double s = tx_wrap01(u) * (double)w - 0.5;            // [-0.5, w - 0.5]
    const double t = (1.0 - tx_wrap01(v)) * (double)h - 0.5;    // [-0.5, h - 0.5]
    const long long si = (long long)floor(256.0 * s), ti = (long long)floor(256.0 * t);     // >= -128
    const long long xi = (si + 256) >> 8, yi = (ti + 256) >> 8;                           // floor(s) + 1, >= 0
    const int fx = (int)((si + 256) & 255), fy = (int)((ti + 256) & 255);
    const int x0 = tx_mod(xi - 1, w), x1 = tx_mod(xi, w), y0 = tx_mod(yi - 1, h), y1 = tx_mod(yi, h);
    const uint32_t c00 = texels[(size_t)y0 * w + x0], c10 = texels[(size_t)y0 * w + x1];
    const uint32_t c01 = texels[(size_t)y1 * w + x0], c11 = texels[(size_t)y1 * w + x1];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const int sh = 8 * k;
        const int top = (int)((c00 >> sh) & 255u) * (256 - fx) + (int)((c10 >> sh) & 255u) * fx;
        const int bot = (int)((c01 >> sh) & 255u) * (256 - fx) + (int)((c11 >> sh) & 255u) * fx;
        out[k] = (top * (256 - fy) + bot * fy + 32768) >> 16;
    }
}

// Colour of the fragment of pixel (x, y) on the triangle A, B, C with corner texture coordinates uv [3][2]: rc_shade with
// the sampled texel in the place of the mixed vertex colour.  mips: the packed pyramid of a Wt x Ht image, of which the
// first `levels` levels may be read (1: the image alone).
BP_HD void tx_shade(const RsCam& cam, const double* A, const double* B, const double* C, const double* uv, const uint32_t* mips,
                    int Wt, int Ht, int levels, int x, int y, const ColorLight& lt, unsigned char* out) {
    RcFrag g;
    rc_fragment(cam, A, B, C, x, y, lt, &g);
    const double u = (g.wa * uv[0] + g.wb * uv[2]) + g.wc * uv[4];
    const double v = (g.wa * uv[1] + g.wb * uv[3]) + g.wc * uv[5];
    const int level = tx_fragment_level(cam, g, A, B, C, uv, x, y, Wt, Ht, levels);
    int lw, lh, base[3];
    const size_t at = tx_level_offset(Wt, Ht, level, &lw, &lh);
    tx_sample(mips + at, lw, lh, u, v, base);
#pragma unroll
    for (int k = 0; k < 3; ++k) out[k] = rc_lit(g.light_w, (double)base[k]);
}
