// The detector's training arithmetic of O(1) size, ONE source for the host twins (yolo_train_host.cpp) and the device
// kernels (yolo_train.hip): the three channels of one network-input pixel (crop, two-pass bilinear resize, flip, HSV
// distortion), the truth rows of one sample, exp / log / logistic, box_iou, the deltas of one cell and of one truth row.
// Host and device compile this text and do the same f64 / f32 / integer operations in the same order, without FMA
// contraction, so their outputs agree bit for bit; only who loops over what differs per side.
// Plain C++17, no HIP header.  Included inside `namespace bp { namespace {` after <cmath> and <cstdint>, in a unit that
// has `#pragma clang fp contract(off)` in force.
//
// Conventions (DESIGN.md §3.11): frames are uint8 [N][H][W][3] RGB; the network input is float32 [B][3][net_h][net_w];
// a head's output is float32 [B][n * (5 + classes)][h][w]; a truth row is (x, y, w, h, id), a row with x == 0 ends a
// sample's list.
#ifndef BP_HD
#if defined(__HIPCC__)
#define BP_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define BP_HD inline
#endif
#endif

constexpr int YT_THREADS = 256;             // lanes of one block of a reduction (the host twin sums in their order)
constexpr int YT_WAVE = 64;
constexpr int YT_CHUNK = 16384;             // delta elements whose squares one block sums
constexpr int YT_IMAGE_STATS = 6;           // per-image sums of the truth walk: IoU, class, obj, recall .5, recall .75, count

// blocks of the cell step (one lane per cell) and of the cost step (YT_CHUNK elements each): one partial sum per block
BP_HD size_t yt_any_blocks(int B, int n, int h, int w) { return ((size_t)B * n * h * w + YT_THREADS - 1) / YT_THREADS; }
BP_HD size_t yt_cost_blocks(int B, int n, int classes, int h, int w) {
    return ((size_t)B * n * (5 + classes) * h * w + YT_CHUNK - 1) / YT_CHUNK;
}

// ---------------------------------------------------------------------------------------------------- inputs
struct YtCrop {
    int pleft, ptop, sw, sh;                // crop_image(orig, pleft, ptop, sw, sh); sw, sh >= 2 (checked by the caller)
    float w_scale, h_scale;                 // resize_image's source steps
};

BP_HD YtCrop yt_crop(const int* c, int net_h, int net_w) {
    YtCrop k;
    k.pleft = c[0], k.ptop = c[1], k.sw = c[2], k.sh = c[3];
    k.w_scale = (float)(k.sw - 1) / (float)(net_w - 1);
    k.h_scale = (float)(k.sh - 1) / (float)(net_h - 1);
    return k;
}

// one value of the cropped image: load_image's u8 / 255 (a division in double rounded to float there; with 53 >= 2 * 24
// + 2 bits that double rounding is innocuous, so the float division has the same bits) of the frame pixel that
// crop_image clamps the position to.  The clamp makes every position safe to read.
BP_HD float yt_pixel(const unsigned char* frame, int H, int W, const YtCrop& k, int col, int row, int ch) {
    int r = row + k.ptop, c = col + k.pleft;
    r = r < 0 ? 0 : (r > H - 1 ? H - 1 : r);
    c = c < 0 ? 0 : (c > W - 1 ? W - 1 : c);
    return (float)frame[((size_t)r * W + c) * 3 + ch] / 255.0f;
}

// resize_image's first pass: column c of the net_w wide `part` image at source row r
BP_HD float yt_part(const unsigned char* frame, int H, int W, const YtCrop& k, int net_w, int c, int r, int ch) {
    if (c == net_w - 1 || k.sw == 1) return yt_pixel(frame, H, W, k, k.sw - 1, r, ch);
    const float sx = (float)c * k.w_scale;
    const int ix = (int)sx;
    const float dx = sx - (float)ix;
    return (1.0f - dx) * yt_pixel(frame, H, W, k, ix, r, ch) + dx * yt_pixel(frame, H, W, k, ix + 1, r, ch);
}

// ... and its second: (1 - dy) * part[iy], then += dy * part[iy + 1] except on the last row
BP_HD float yt_resized(const unsigned char* frame, int H, int W, const YtCrop& k, int net_h, int net_w, int c, int r, int ch) {
    const float sy = (float)r * k.h_scale;
    const int iy = (int)sy;
    const float dy = sy - (float)iy;
    float val = (1.0f - dy) * yt_part(frame, H, W, k, net_w, c, iy, ch);
    if (!(r == net_h - 1 || k.sh == 1)) val = val + dy * yt_part(frame, H, W, k, net_w, c, iy + 1, ch);
    return val;
}

BP_HD float yt_max3(float a, float b, float c) { return (a > b) ? ((a > c) ? a : c) : ((b > c) ? b : c); }
BP_HD float yt_min3(float a, float b, float c) { return (a < b) ? ((a < c) ? a : c) : ((b < c) ? b : c); }
BP_HD float yt_unit(float a) { return a < 0.0f ? 0.0f : (a > 1.0f ? 1.0f : a); }

// distort_image on one pixel: rgb_to_hsv, saturation and value scaled, hue shifted and wrapped once either way,
// hsv_to_rgb, constrain_image.  A grey pixel has hue 0 / 0 = NaN there as here; its saturation 0 keeps the NaN out of
// the result.  (h / 6. is a double division rounded to float in the reference: innocuous as above.)
BP_HD void yt_distort(float* rgb, float dhue, float dsat, float dexp) {
    const float r = rgb[0], g = rgb[1], b = rgb[2];
    const float mx = yt_max3(r, g, b), mn = yt_min3(r, g, b);
    const float delta = mx - mn;
    float h, s, v = mx;
    if (mx == 0.0f) {
        s = 0.0f;
        h = 0.0f;
    } else {
        s = delta / mx;
        if (r == mx) h = (g - b) / delta;
        else if (g == mx) h = 2.0f + (b - r) / delta;
        else h = 4.0f + (r - g) / delta;
        if (h < 0.0f) h = h + 6.0f;
        h = h / 6.0f;
    }
    s = s * dsat;
    v = v * dexp;
    h = h + dhue;
    if (h > 1.0f) h = h - 1.0f;
    if (h < 0.0f) h = h + 1.0f;
    float R, G, B;
    if (s == 0.0f) {
        R = G = B = v;
    } else {
        const float h6 = 6.0f * h;
        const float fl = floorf(h6);
        const int index = (fl > -8.0f && fl < 8.0f) ? (int)fl : 7;     // (outside 0 .. 4 every index takes the last branch)
        const float f = h6 - (float)index;
        const float p = v * (1.0f - s);
        const float q = v * (1.0f - s * f);
        const float t = v * (1.0f - s * (1.0f - f));
        if (index == 0) R = v, G = t, B = p;
        else if (index == 1) R = q, G = v, B = p;
        else if (index == 2) R = p, G = v, B = t;
        else if (index == 3) R = p, G = q, B = v;
        else if (index == 4) R = t, G = p, B = v;
        else R = v, G = p, B = q;
    }
    rgb[0] = yt_unit(R), rgb[1] = yt_unit(G), rgb[2] = yt_unit(B);
}

// the three channels of output pixel (y, x) of one sample; hsv = (dhue, dsat, dexp) or null for no distortion
BP_HD void yt_input_rgb(const unsigned char* frame, int H, int W, const YtCrop& k, int net_h, int net_w, int flip,
                        const float* hsv, int y, int x, float* rgb) {
    const int c = flip ? net_w - 1 - x : x;
    for (int ch = 0; ch < 3; ++ch) rgb[ch] = yt_resized(frame, H, W, k, net_h, net_w, c, y, ch);
    if (hsv) yt_distort(rgb, hsv[0], hsv[1], hsv[2]);
}

// ---------------------------------------------------------------------------------------------------- truth rows
BP_HD float yt_constrain(float mn, float mx, float a) { return a < mn ? mn : (a > mx ? mx : a); }

// fill_truth_detection for one sample: labels [n][5] = (id, x, y, w, h), swap [n] the index randomize_boxes draws at
// each step (one outside [0, n) swaps nothing), order [n] scratch, truth [max_boxes][5] zero-filled past the kept rows.
// Returns the rows kept.  small_object == 1 raises w and h to one pixel BEFORE correct_boxes, which then overwrites
// both on every path: as in the reference it changes no output, so it is accepted and not evaluated.
BP_HD int yt_truth_rows(const float* labels, int n, const int* swap, float dx, float dy, float sx, float sy, int flip,
                        int classes, int max_boxes, int net_w, int net_h, int* order, float* truth) {
    for (int i = 0; i < max_boxes * 5; ++i) truth[i] = 0.0f;
    for (int i = 0; i < n; ++i) order[i] = i;
    for (int i = 0; i < n; ++i) {
        const int j = swap[i];
        if (j < 0 || j >= n) continue;
        const int t = order[i];
        order[i] = order[j];
        order[j] = t;
    }
    const float lowest_w = 1.0f / (float)net_w, lowest_h = 1.0f / (float)net_h;
    const int count = n > max_boxes ? max_boxes : n;    // truncated before the filter
    int sub = 0;
    for (int i = 0; i < count; ++i) {
        const float* L = labels + (size_t)order[i] * 5;
        const int id = (int)L[0];
        float x = L[1], y = L[2], w = L[3], h = L[4];
        if (x == 0.0f && y == 0.0f) {
            x = y = w = h = 999999.0f;
        } else {
            float left = x - w / 2.0f, right = x + w / 2.0f, top = y - h / 2.0f, bottom = y + h / 2.0f;    // (read_boxes)
            left = left * sx - dx;
            right = right * sx - dx;
            top = top * sy - dy;
            bottom = bottom * sy - dy;
            if (flip) {
                const float s = left;
                left = (float)(1.0 - (double)right);
                right = (float)(1.0 - (double)s);
            }
            left = yt_constrain(0.0f, 1.0f, left);
            right = yt_constrain(0.0f, 1.0f, right);
            top = yt_constrain(0.0f, 1.0f, top);
            bottom = yt_constrain(0.0f, 1.0f, bottom);
            x = (left + right) / 2.0f;
            y = (top + bottom) / 2.0f;
            w = yt_constrain(0.0f, 1.0f, right - left);
            h = yt_constrain(0.0f, 1.0f, bottom - top);
        }
        if (id >= classes || w < lowest_w || h < lowest_h || x == 999999.0f || y == 999999.0f || x <= 0.0f || x > 1.0f ||
            y <= 0.0f || y > 1.0f) {
            ++sub;
            continue;
        }
        if (w > 1.0f) w = 1.0f;
        if (h > 1.0f) h = 1.0f;
        float* T = truth + (size_t)(i - sub) * 5;
        T[0] = x, T[1] = y, T[2] = w, T[3] = h, T[4] = (float)id;
    }
    return count - sub;
}

// ---------------------------------------------------------------------------------------------------- exp, log, logistic
BP_HD double yt_bits(uint64_t b) {
    double d;
    __builtin_memcpy(&d, &b, sizeof d);
    return d;
}

// exp(x) for any x (clamped to [-700, 700], whose results round to 0 and inf in float32 as the true ones do; NaN stays)
// from + - * and a bit-built power of two, built as ds_exp of designate_math.inc, whose domain stops at 0.3: x = k ln2 + r
// with |r| <= 0.35 (ln2 split into a 32-bit head, so k * head is exact, and a tail), the degree-13 Taylor polynomial of
// exp(r) by Horner's rule (truncation below 2^-57, thirteen rounded steps below 3e-15 relative), times 2^k.  Neither
// libm's nor ocml's exp: the two differ, and the host's and the device's must not.
BP_HD double yt_exp(double x) {
    if (!(x == x)) return x;
    x = x > 700.0 ? 700.0 : (x < -700.0 ? -700.0 : x);
    const double t = x * 1.44269504088896338700e+00;
    const int k = (int)(t < 0.0 ? t - 0.5 : t + 0.5);
    const double kd = (double)k;
    const double r = (x - kd * 6.93147180369123816490e-01) - kd * 1.90821492927058770002e-10;
    double p = 1.0 / 6227020800.0;
    p = p * r + 1.0 / 479001600.0;
    p = p * r + 1.0 / 39916800.0;
    p = p * r + 1.0 / 3628800.0;
    p = p * r + 1.0 / 362880.0;
    p = p * r + 1.0 / 40320.0;
    p = p * r + 1.0 / 5040.0;
    p = p * r + 1.0 / 720.0;
    p = p * r + 1.0 / 120.0;
    p = p * r + 1.0 / 24.0;
    p = p * r + 1.0 / 6.0;
    p = p * r + 0.5;
    p = p * r + 1.0;
    p = p * r + 1.0;
    return p * yt_bits((uint64_t)(1023 + k) << 52);     // 2^k, k in [-1010, 1010]
}

// log(a): -inf for 0, NaN for a negative or NaN argument, a for +inf; otherwise a = m 2^e with m in (sqrt(1/2), sqrt 2],
// s = (m - 1) / (m + 1) (|s| <= 0.1716), log m = 2 s (1 + s^2/3 + ... + s^22/23) by Horner's rule (truncation below
// 2^-60 relative, the rounded steps below 4e-16 relative), plus e ln2 with the split of yt_exp.
BP_HD double yt_log(double a) {
    if (!(a == a) || a < 0.0) return (a - a) / (a - a);
    if (a == 0.0) return yt_bits(0xfff0000000000000ull);
    uint64_t b;
    __builtin_memcpy(&b, &a, sizeof b);
    if ((b >> 52) == 0x7ff) return a;
    int e = 0;
    if ((b >> 52) == 0) {                   // subnormal: scale by 2^54 first
        a = a * 18014398509481984.0;
        __builtin_memcpy(&b, &a, sizeof b);
        e = -54;
    }
    e += (int)(b >> 52) - 1023;
    double m = yt_bits((b & 0x000fffffffffffffull) | 0x3ff0000000000000ull);
    if (m > 1.41421356237309514547) {
        m = m * 0.5;
        e += 1;
    }
    const double s = (m - 1.0) / (m + 1.0), z = s * s;
    double p = 1.0 / 23.0;
    p = p * z + 1.0 / 21.0;
    p = p * z + 1.0 / 19.0;
    p = p * z + 1.0 / 17.0;
    p = p * z + 1.0 / 15.0;
    p = p * z + 1.0 / 13.0;
    p = p * z + 1.0 / 11.0;
    p = p * z + 1.0 / 9.0;
    p = p * z + 1.0 / 7.0;
    p = p * z + 1.0 / 5.0;
    p = p * z + 1.0 / 3.0;
    p = p * z + 1.0;
    const double ed = (double)e;
    return ed * 6.93147180369123816490e-01 + ((2.0 * s) * p + ed * 1.90821492927058770002e-10);
}

// logistic_activate: 1. / (1. + exp(-x)) in double, stored as float
BP_HD float yt_logistic(float x) { return (float)(1.0 / (1.0 + yt_exp(-(double)x))); }

// ---------------------------------------------------------------------------------------------------- boxes
struct YtBox {
    float x, y, w, h;
};

BP_HD float yt_overlap(float x1, float w1, float x2, float w2) {
    const float l1 = x1 - w1 / 2.0f, l2 = x2 - w2 / 2.0f;
    const float left = l1 > l2 ? l1 : l2;
    const float r1 = x1 + w1 / 2.0f, r2 = x2 + w2 / 2.0f;
    const float right = r1 < r2 ? r1 : r2;
    return right - left;
}

// box_iou as box.c has it: two empty boxes give 0 / 0 = NaN, which no `>` accepts
BP_HD float yt_box_iou(const YtBox& a, const YtBox& b) {
    const float w = yt_overlap(a.x, a.w, b.x, b.w), h = yt_overlap(a.y, a.h, b.y, b.h);
    const float inter = (w < 0.0f || h < 0.0f) ? 0.0f : w * h;
    const float uni = (a.w * a.h + b.w * b.h) - inter;
    return inter / uni;
}

// ---------------------------------------------------------------------------------------------------- the yolo layer
// One head.  x and delta are [B][n * (5 + classes)][h][w]; a cell's entries lie `wh` apart from `x + base`.
struct YtHead {
    int B, n, classes, h, w, net_w, net_h, total, max_boxes;
    float ignore_thresh, truth_thresh;
};

BP_HD size_t yt_cell_base(const YtHead& L, int b, int a, int loc) {
    return ((size_t)b * L.n + a) * (size_t)(5 + L.classes) * ((size_t)L.h * L.w) + loc;
}

// l.output's entry e of a cell: logistic on x, y, objectness and classes, the raw value on w and h
BP_HD float yt_output(const float* x, size_t base, size_t wh, int e) {
    const float v = x[base + e * wh];
    return (e == 2 || e == 3) ? v : yt_logistic(v);
}

// get_yolo_box: exp() is the double one, so w and h are formed in double and stored as float
BP_HD YtBox yt_pred_box(float ox, float oy, float ow, float oh, float aw, float ah, int i, int j, const YtHead& L) {
    YtBox b;
    b.x = ((float)i + ox) / (float)L.w;
    b.y = ((float)j + oy) / (float)L.h;
    b.w = (float)(yt_exp((double)ow) * (double)aw / (double)L.net_w);
    b.h = (float)(yt_exp((double)oh) * (double)ah / (double)L.net_h);
    return b;
}

// delta_yolo_box's four deltas (scale = 2 - w * h of the truth); o = the cell's four outputs
BP_HD void yt_box_delta(const YtBox& truth, const float* o, float aw, float ah, int i, int j, const YtHead& L, float* d) {
    const float scale = 2.0f - truth.w * truth.h;
    const float tx = truth.x * (float)L.w - (float)i;
    const float ty = truth.y * (float)L.h - (float)j;
    const float tw = (float)yt_log((double)(truth.w * (float)L.net_w / aw));
    const float th = (float)yt_log((double)(truth.h * (float)L.net_h / ah));
    d[0] = scale * (tx - o[0]);
    d[1] = scale * (ty - o[1]);
    d[2] = scale * (tw - o[2]);
    d[3] = scale * (th - o[3]);
}

// the class id of a truth row, or -1 where the row is passed over: an id >= classes as in the reference, and a negative
// one, with which the reference would index before the tensor
BP_HD int yt_class_id(const float* row, int classes) {
    const float v = row[4];
    if (!(v > -1.0f && v < (float)classes)) return -1;
    return (int)v;
}

// Step 1, one (b, anchor a, cell loc): writes every entry of the cell in delta (and act), returns the objectness output.
BP_HD float yt_cell(const YtHead& L, const float* x, const float* anchors, const int* mask, const float* truth, int b, int a,
                    int loc, float* act, float* delta) {
    const size_t wh = (size_t)L.h * L.w, base = yt_cell_base(L, b, a, loc);
    const int i = loc % L.w, j = loc / L.w;
    const int entries = 5 + L.classes;
    float o[5];
    for (int e = 0; e < 5; ++e) o[e] = yt_output(x, base, wh, e);
    const float aw = anchors[2 * mask[a]], ah = anchors[2 * mask[a] + 1];
    const YtBox pred = yt_pred_box(o[0], o[1], o[2], o[3], aw, ah, i, j, L);
    float best_iou = 0.0f;
    int best_t = 0;
    const float* rows = truth + (size_t)b * L.max_boxes * 5;
    for (int t = 0; t < L.max_boxes; ++t) {
        const float* row = rows + t * 5;
        if (yt_class_id(row, L.classes) < 0) continue;
        if (!row[0]) break;
        const YtBox tb = {row[0], row[1], row[2], row[3]};
        const float iou = yt_box_iou(pred, tb);
        if (iou > best_iou) {
            best_iou = iou;
            best_t = t;
        }
    }
    float d[5] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f - o[4]};
    if (best_iou > L.ignore_thresh) d[4] = 0.0f;
    const bool match = best_iou > L.truth_thresh;
    int cls = -1;
    if (match) {
        const float* row = rows + best_t * 5;
        d[4] = 1.0f - o[4];
        cls = yt_class_id(row, L.classes);      // (>= 0: best_t was accepted above)
        const YtBox tb = {row[0], row[1], row[2], row[3]};
        yt_box_delta(tb, o, aw, ah, i, j, L, d);
    }
    for (int e = 0; e < 5; ++e) {
        delta[base + e * wh] = d[e];
        if (act) act[base + e * wh] = o[e];
    }
    for (int e = 5; e < entries; ++e) {
        const float oc = yt_output(x, base, wh, e);
        // delta_yolo_class on a cell whose deltas are still zero: its second branch
        delta[base + e * wh] = match ? (e - 5 == cls ? 1.0f : 0.0f) - oc : 0.0f;
        if (act) act[base + e * wh] = oc;
    }
    return o[4];
}

// Step 2, the truth rows of image b in order (later rows overwrite earlier ones); st [YT_IMAGE_STATS] gets the sums.
// A row whose cell lies outside the grid (x or y of 1 exactly puts it one past, where the reference writes into the
// neighbouring row or past the tensor) is passed over.
BP_HD void yt_truth_walk(const YtHead& L, const float* x, const float* anchors, const int* mask, const float* truth, int b,
                         float* delta, double* st) {
    const size_t wh = (size_t)L.h * L.w;
    double s_iou = 0.0, s_cat = 0.0, s_obj = 0.0, r50 = 0.0, r75 = 0.0, count = 0.0;
    const float* rows = truth + (size_t)b * L.max_boxes * 5;
    for (int t = 0; t < L.max_boxes; ++t) {
        const float* row = rows + t * 5;
        const int cls = yt_class_id(row, L.classes);
        if (cls < 0) continue;
        if (!row[0]) break;
        const YtBox tb = {row[0], row[1], row[2], row[3]};
        const float fi = tb.x * (float)L.w, fj = tb.y * (float)L.h;
        if (!(fi >= 0.0f && fi < (float)L.w && fj >= 0.0f && fj < (float)L.h)) continue;
        const int i = (int)fi, j = (int)fj;
        float best_iou = 0.0f;
        int best_n = 0;
        const YtBox shift = {0.0f, 0.0f, tb.w, tb.h};
        for (int n = 0; n < L.total; ++n) {
            const YtBox p = {0.0f, 0.0f, anchors[2 * n] / (float)L.net_w, anchors[2 * n + 1] / (float)L.net_h};
            const float iou = yt_box_iou(p, shift);
            if (iou > best_iou) {
                best_iou = iou;
                best_n = n;
            }
        }
        int a = -1;
        for (int m = 0; m < L.n; ++m)
            if (mask[m] == best_n) {
                a = m;
                break;
            }
        if (a < 0) continue;
        const size_t base = yt_cell_base(L, b, a, j * L.w + i);
        float o[5], d[4];
        for (int e = 0; e < 5; ++e) o[e] = yt_output(x, base, wh, e);
        const float aw = anchors[2 * best_n], ah = anchors[2 * best_n + 1];
        const float iou = yt_box_iou(yt_pred_box(o[0], o[1], o[2], o[3], aw, ah, i, j, L), tb);
        yt_box_delta(tb, o, aw, ah, i, j, L, d);
        for (int e = 0; e < 4; ++e) delta[base + e * wh] = d[e];
        s_obj = s_obj + (double)o[4];
        delta[base + 4 * wh] = 1.0f - o[4];
        // delta_yolo_class: its first branch keys on the delta already written being non-zero
        const size_t ci = base + (size_t)(5 + cls) * wh;
        if (delta[ci]) {
            const float oc = yt_output(x, base, wh, 5 + cls);
            delta[ci] = 1.0f - oc;
            s_cat = s_cat + (double)oc;
        } else {
            for (int c = 0; c < L.classes; ++c) {
                const float oc = yt_output(x, base, wh, 5 + c);
                delta[base + (size_t)(5 + c) * wh] = (c == cls ? 1.0f : 0.0f) - oc;
                if (c == cls) s_cat = s_cat + (double)oc;
            }
        }
        count = count + 1.0;
        if (iou > 0.5f) r50 = r50 + 1.0;
        if (iou > 0.75f) r75 = r75 + 1.0;
        s_iou = s_iou + (double)iou;
    }
    st[0] = s_iou, st[1] = s_cat, st[2] = s_obj, st[3] = r50, st[4] = r75, st[5] = count;
}
