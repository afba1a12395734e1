// The KPD training sample's arithmetic of O(1) size, ONE source for the host twins (kpd_sample_host.cpp) and the device
// kernels (kpd_sample.hip): one value of the network input (colour gain, mean, cropBox window, bilinear resize), one
// value of an augmented map (flip, channel swap, rotation), one element of the masked squared error and its gradient,
// the combination of two arg-max candidates and one normalised distance.  Host and device compile this text and do the
// same f64 / f32 / integer operations in the same order, without FMA contraction, so their outputs agree bit for bit;
// only who loops over what differs per side.
// Plain C++17, no HIP header.  Included inside `namespace bp { namespace {` after <cmath> and <cstdint>, in a unit that
// has `#pragma clang fp contract(off)` in force.
//
// Conventions (DESIGN.md §3.10): frames are uint8 [N][H][W][3] RGB; maps are float32 [B][C][H][W]; a window is the pair
// (ul, br) of float32 corners (x, y) that bp_kpd_targets takes, truncated toward zero here as cropBox's .int() does.
#ifndef BP_HD
#if defined(__HIPCC__)
#define BP_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define BP_HD inline
#endif
#endif

constexpr int KS_THREADS = 256;             // lanes of one block of the loss reduction (the host twin sums in their order)
constexpr int KS_WAVE = 64;

// ---------------------------------------------------------------------------------------------------- inputs
// The window of one sample in the reference's padded image: the crop [y0, y0 + h) x [x0, x0 + w) of the frame sits at
// rows [oy, oy + h), columns [ox, ox + w) of a PH x PW image whose other pixels are 0 (SpecialCrop at the top left,
// then Pad's centred np.pad: ceil before, floor after).  ok = 0: the window is empty or not finite and the sample is 0.
struct KsWindow {
    int x0, y0, w, h, PW, PH, ox, oy, ok;
    float sx, sy;                           // align_corners = True source steps
};

BP_HD int ks_trunc(float v) {               // .int(): toward zero; what does not fit an image coordinate makes the window empty
    return (v > -1.0e6f && v < 1.0e6f) ? (int)v : -(1 << 30);
}

BP_HD KsWindow ks_window(float ulx, float uly, float brx, float bry, int inpH, int inpW) {
    KsWindow k;
    k.x0 = ks_trunc(ulx);
    k.y0 = ks_trunc(uly);
    const int x1 = ks_trunc(brx), y1 = ks_trunc(bry);
    k.ok = k.x0 > -(1 << 30) && k.y0 > -(1 << 30) && x1 > k.x0 && y1 > k.y0;
    if (!k.ok) {
        k.w = k.h = k.PW = k.PH = 1;
        k.ox = k.oy = 0;
        k.sx = k.sy = 0.0f;
        return k;
    }
    k.w = x1 - k.x0;
    k.h = y1 - k.y0;
    const float wide = ((float)k.w * (float)inpH) / (float)inpW;
    const float lenH = (float)k.h > wide ? (float)k.h : wide;
    const float lenW = (lenH * (float)inpW) / (float)inpH;
    const int iH = (int)lenH, iW = (int)lenW;
    k.PH = iH > k.h ? iH : k.h;
    k.PW = iW > k.w ? iW : k.w;
    k.oy = (k.PH - k.h + 1) / 2;            // ceil((PH - h) / 2)
    k.ox = (k.PW - k.w + 1) / 2;
    k.sy = inpH > 1 ? (float)(k.PH - 1) / (float)(inpH - 1) : 0.0f;
    k.sx = inpW > 1 ? (float)(k.PW - 1) / (float)(inpW - 1) : 0.0f;
    return k;
}

BP_HD float ks_mean(int c) { return c == 0 ? 0.406f : (c == 1 ? 0.457f : 0.480f); }

// load_image + generateSampleBox:21-28 of one byte: u8 / 255, (gain, clamp), - mean.  gain == nullptr skips the
// multiply as the reference's evaluation mode does (x * 1.0f == x for every float, so the bits are the same).
BP_HD float ks_pixel(unsigned char u, const float* gain, int c) {
    float v = (float)u / 255.0f;
    if (gain) v = v * gain[c];
    v = v < 0.0f ? 0.0f : (v > 1.0f ? 1.0f : v);
    return v - ks_mean(c);
}

// one tap of the padded image; frame [H][W][3] of this sample.  The frame index is formed only after the pixel has
// been tested against the frame.
BP_HD float ks_tap(const KsWindow& k, const unsigned char* frame, int H, int W, const float* gain, int c, int py, int px) {
    const int ry = py - k.oy, rx = px - k.ox;
    if (ry < 0 || ry >= k.h || rx < 0 || rx >= k.w) return 0.0f;
    const int y = k.y0 + ry, x = k.x0 + rx;
    if (y < 0 || y >= H || x < 0 || x >= W) return 0.0f;
    return ks_pixel(frame[((size_t)y * W + x) * 3 + c], gain, c);
}

// F.interpolate(bilinear, align_corners = True) at output pixel (y, x) of channel c
BP_HD float ks_input_value(const KsWindow& k, const unsigned char* frame, int H, int W, const float* gain, int c, int y, int x) {
    if (!k.ok) return 0.0f;
    const float fy = k.sy * (float)y, fx = k.sx * (float)x;
    int y0 = (int)fy, x0 = (int)fx;
    y0 = y0 > k.PH - 1 ? k.PH - 1 : y0;
    x0 = x0 > k.PW - 1 ? k.PW - 1 : x0;
    const int y1 = y0 + 1 < k.PH ? y0 + 1 : k.PH - 1;
    const int x1 = x0 + 1 < k.PW ? x0 + 1 : k.PW - 1;
    const float ly = fy - (float)y0, lx = fx - (float)x0;
    const float t00 = ks_tap(k, frame, H, W, gain, c, y0, x0), t01 = ks_tap(k, frame, H, W, gain, c, y0, x1);
    const float t10 = ks_tap(k, frame, H, W, gain, c, y1, x0), t11 = ks_tap(k, frame, H, W, gain, c, y1, x1);
    const float top = (1.0f - lx) * t00 + lx * t01;
    const float bot = (1.0f - lx) * t10 + lx * t11;
    return (1.0f - ly) * top + ly * bot;
}

// ---------------------------------------------------------------------------------------------------- augmentation
// the map the flipped sample reads for channel c: perm [C] (shuffleLR as a source-channel table) or the identity; an
// entry outside [0, C) counts as the identity
BP_HD int ks_source_channel(const int* perm, int C, int flip, int c) {
    if (!flip || !perm) return c;
    const int p = perm[c];
    return p >= 0 && p < C ? p : c;
}

// one value of the flipped map: src is the chosen channel [H][W]
BP_HD float ks_flipped(const float* src, int W, int flip, int r, int q) { return src[(size_t)r * W + (flip ? W - 1 - q : q)]; }

BP_HD int ks_is_identity(const double* cs) { return cs[0] == 1.0 && cs[1] == 0.0; }

// the clamped floor index, its neighbour and the weight of the neighbour along one axis of n pixels
BP_HD void ks_axis(double coord, int n, int* i0, int* i1, float* d) {
    double c = coord < 0.0 ? 0.0 : coord;   // (NaN stays NaN here and lands on index 0 below)
    c = c > (double)(n - 1) ? (double)(n - 1) : c;
    const double f = floor(c);
    int a = f >= 0.0 ? (int)f : 0;
    a = a > n - 1 ? n - 1 : a;
    *i0 = a;
    *i1 = a + 1 < n ? a + 1 : n - 1;
    *d = f >= 0.0 ? (float)(c - f) : 0.0f;
}

// Rotate of one output pixel (i, j): cs = (cos, sin) of the angle, A = [[cos, -sin], [sin, cos]] on (row, col) about
// (H/2 - 0.5, W/2 - 0.5), coordinates in f64, blend in f32; the taps are read through the flip
BP_HD float ks_augment_value(const float* src, int H, int W, int flip, const double* cs, int i, int j) {
    if (ks_is_identity(cs)) return ks_flipped(src, W, flip, i, j);
    const double cr = (double)H / 2.0 - 0.5, cq = (double)W / 2.0 - 0.5;
    const double dr = (double)i - cr, dq = (double)j - cq;
    const double r = (cs[0] * dr - cs[1] * dq) + cr;
    const double q = (cs[1] * dr + cs[0] * dq) + cq;
    int r0, r1, q0, q1;
    float rd, qd;
    ks_axis(r, H, &r0, &r1, &rd);
    ks_axis(q, W, &q0, &q1, &qd);
    const float v00 = ks_flipped(src, W, flip, r0, q0), v10 = ks_flipped(src, W, flip, r1, q0);
    const float v01 = ks_flipped(src, W, flip, r0, q1), v11 = ks_flipped(src, W, flip, r1, q1);
    const float rm = 1.0f - rd, qm = 1.0f - qd;
    return ((v00 * rm * qm + v10 * rd * qm) + v01 * rm * qd) + v11 * rd * qd;
}

// ---------------------------------------------------------------------------------------------------- loss, accuracy
// out * mask - label in f32 (mask == nullptr: out - label); *pred is the masked output, what getPreds sees
BP_HD float ks_residual(float o, const float* m, float l, float* pred) {
    const float p = m ? o * *m : o;
    *pred = p;
    return p - l;
}

// d(loss)/d(out): the MSE's (2 / N) * residual, then the product's mask; norm = (float)(2.0 / N)
BP_HD float ks_gradient(float norm, float residual, const float* m) {
    const float g = norm * residual;
    return m ? g * *m : g;
}

// arg-max candidate: the larger value wins, the lower flat index among equal values; a NaN never wins
struct KsBest {
    float v;
    int i;
};
BP_HD KsBest ks_best_empty() { return KsBest{-INFINITY, INT32_MAX}; }
BP_HD KsBest ks_best_of(KsBest a, KsBest b) { return (b.v > a.v || (b.v == a.v && b.i < a.i)) ? b : a; }
BP_HD int ks_best_index(KsBest a) { return a.i == INT32_MAX ? 0 : a.i; }   // (a map of NaNs only)

// calc_dists of one (sample, channel): -1 unless both ground-truth coordinates are positive
BP_HD float ks_dist(int px, int py, int gx, int gy, int H) {
    if (!(gx > 0 && gy > 0)) return -1.0f;
    const long long dx = (long long)px - gx, dy = (long long)py - gy;
    const float d = (float)sqrt((double)(dx * dx + dy * dy));      // == sqrtf of the f32 sum below 2^24
    return d / ((float)H / 10.0f);
}

// The order in which one map's squares are summed, for both sides: element e belongs to lane (e / 4) % KS_THREADS and
// every lane adds its elements in ascending order; each wave of KS_WAVE lanes is folded by the shuffle tree
// (lane l += lane l + o, o = 32 .. 1), and the block's waves are added in ascending order.
