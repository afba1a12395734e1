// The arithmetic of one Darknet training iteration, ONE source for the host twins (darknet_train_host.cpp) and the device
// kernels (darknet_train.hip): which element of which tensor is operand (m, k) / (k, j) of the implicit GEMM in each of
// its three roles and in which order k runs, the batch-norm statistics and their per-element forms, forward and
// backward, and the three steps of the update.  Host and device compile this text and do the same f64 / f32 / integer
// operations in the same order, without FMA contraction (the GEMM's chain is an explicit fmaf on the host and the fp32
// MFMA on the device), so their outputs agree bit for bit; only who loops over what differs per side.
// Plain C++17, no HIP header.  Included inside `namespace bp { namespace {` after <cmath> and <cstdint>, in a unit that
// has `#pragma clang fp contract(off)` in force.
//
// Conventions (DESIGN.md 3.13): activations and deltas are float32 [N][C][H][W], filters and their updates
// [Cout][Cin][ky][kx] (Darknet's order, the order of a .weights file), padding size / 2.
#ifndef BP_HD
#if defined(__HIPCC__)
#define BP_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define BP_HD inline
#endif
#endif

constexpr int DT_THREADS = 256;             // lanes of one block (the host twin sums a reduction in their order)
constexpr int DT_WAVE = 64;
constexpr int DT_BM = 64, DT_BN = 64;       // the block tile of the GEMM core: 2 x 2 waves of one 32 x 32 MFMA tile each
constexpr int DT_BK = 16;                   // k values staged in LDS per step: 8 MFMAs of k = 2
constexpr int DT_SLICE = 2048;              // k values of one reduction slice of the filter gradient (a multiple of DT_BK)
constexpr int DT_UPD_CHUNK = 1024;          // elements one block of the update handles

enum { DT_FORWARD = 0, DT_FILTER_GRAD = 1, DT_INPUT_GRAD = 2 };

// One convolution as a GEMM  D[M][Ncol] = sum_k A(m, k) B(k, j):
//   forward        M = Cout, j = (n, oy, ox), k = (ky, kx, c)     A = filters, B = im2col(input),   D = output
//   filter grad    M = Cout, j = (ky, kx, c), k = (n, oy, ox)     A = delta,   B = im2col(input)^T, D = a slice's partial sum
//   input grad     M = Cin,  j = (n, iy, ix), k = (ky, kx, cout)  A = filters, B = col2im's gather of delta, D += input's delta
// k ascending in the order written; a tap outside the image, an m, j or k past the end is the value 0 IN the chain.
struct DtG {
    int role, N, C, H, W, K, size, stride, pad, OH, OW;
    int M, Ncol, Kdim, slices;
};

BP_HD DtG dt_geom(int role, int N, int C, int H, int W, int K, int size, int stride) {
    DtG g;
    g.role = role, g.N = N, g.C = C, g.H = H, g.W = W, g.K = K, g.size = size, g.stride = stride, g.pad = size / 2;
    g.OH = (H + 2 * g.pad - size) / stride + 1, g.OW = (W + 2 * g.pad - size) / stride + 1;
    if (role == DT_FORWARD) g.M = K, g.Ncol = N * g.OH * g.OW, g.Kdim = size * size * C;
    else if (role == DT_FILTER_GRAD) g.M = K, g.Ncol = size * size * C, g.Kdim = N * g.OH * g.OW;
    else g.M = C, g.Ncol = N * H * W, g.Kdim = size * size * K;
    g.slices = role == DT_FILTER_GRAD ? (g.Kdim + DT_SLICE - 1) / DT_SLICE : 1;
    return g;
}

// the k range of slice s: bounds that depend on the shape only
BP_HD int dt_slice_begin(const DtG& g, int s) { return g.role == DT_FILTER_GRAD ? s * DT_SLICE : 0; }
BP_HD int dt_slice_end(const DtG& g, int s) {
    if (g.role != DT_FILTER_GRAD) return g.Kdim;
    const int e = (s + 1) * DT_SLICE;
    return e < g.Kdim ? e : g.Kdim;
}

BP_HD float dt_a(const DtG& g, const float* __restrict__ a, int m, int k) {
    if (m >= g.M || k >= g.Kdim) return 0.0f;
    if (g.role == DT_FILTER_GRAD) {
        const int sp = g.OH * g.OW, n = k / sp, r = k - n * sp;
        return a[((size_t)n * g.K + m) * sp + r];
    }
    const int inner = g.role == DT_FORWARD ? g.C : g.K;
    const int t = k / inner, ch = k - t * inner;            // t = ky * size + kx
    const int co = g.role == DT_FORWARD ? m : ch, ci = g.role == DT_FORWARD ? ch : m;
    return a[((size_t)co * g.C + ci) * (g.size * g.size) + t];
}

// the input's value under tap (ky, kx) of output position (oy, ox): 0 outside the image
BP_HD float dt_tap(const DtG& g, const float* __restrict__ x, int n, int c, int oy, int ox, int t) {
    const int ky = t / g.size, kx = t - ky * g.size;
    const int iy = oy * g.stride + ky - g.pad, ix = ox * g.stride + kx - g.pad;
    if (iy < 0 || iy >= g.H || ix < 0 || ix >= g.W) return 0.0f;
    return x[(((size_t)n * g.C + c) * g.H + iy) * g.W + ix];
}

BP_HD float dt_b(const DtG& g, const float* __restrict__ b, int k, int j) {
    if (k >= g.Kdim || j >= g.Ncol) return 0.0f;
    if (g.role == DT_INPUT_GRAD) {
        const int sp = g.H * g.W, n = j / sp, r = j - n * sp, iy = r / g.W, ix = r - iy * g.W;
        const int t = k / g.K, co = k - t * g.K, ky = t / g.size, kx = t - ky * g.size;
        const int ty = iy + g.pad - ky, tx = ix + g.pad - kx;
        if (ty < 0 || tx < 0 || ty % g.stride || tx % g.stride) return 0.0f;
        const int oy = ty / g.stride, ox = tx / g.stride;
        if (oy >= g.OH || ox >= g.OW) return 0.0f;
        return b[(((size_t)n * g.K + co) * g.OH + oy) * g.OW + ox];
    }
    const int pos = g.role == DT_FORWARD ? j : k, tc = g.role == DT_FORWARD ? k : j;
    const int sp = g.OH * g.OW, n = pos / sp, r = pos - n * sp, oy = r / g.OW, ox = r - oy * g.OW;
    const int t = tc / g.C, c = tc - t * g.C;
    return dt_tap(g, b, n, c, oy, ox, t);
}

// where D(m, j) lies: the output / the input's delta [n][m][spatial], or a partial sum [slice][m][j]
BP_HD size_t dt_d_index(const DtG& g, int m, int j, int slice) {
    if (g.role == DT_FILTER_GRAD) return ((size_t)slice * g.M + m) * g.Ncol + j;
    const int sp = g.role == DT_FORWARD ? g.OH * g.OW : g.H * g.W, n = j / sp, r = j - n * sp;
    return ((size_t)n * g.M + m) * sp + r;
}
// ... and column j = (ky, kx, c) of filter m in [Cout][Cin][ky][kx]
BP_HD size_t dt_filter_index(const DtG& g, int m, int j) {
    const int t = j / g.C, c = j - t * g.C;
    return ((size_t)m * g.C + c) * (g.size * g.size) + t;
}

// ---------------------------------------------------------------------------------------------------- batch norm
// mean_cpu / variance_cpu with the sums in f64 (declared deviation: Darknet's are float32 running sums)
BP_HD float dt_mean(double sum, int count) { return (float)sum * (float)(1. / count); }
BP_HD float dt_variance(double sum, int count) { return (float)sum * (float)(1. / (count - 1)); }
BP_HD double dt_sq(float x, float mean) {
    const double d = (double)(x - mean);
    return d * d;
}
// scal_cpu(.9) then axpy_cpu(.1): two rounded steps
BP_HD float dt_roll(float rolling, float v) {
    const float r = rolling * .9f;
    return r + .1f * v;
}
// normalize_cpu: the float difference over the double sqrt(var) + .000001f, rounded to float once
BP_HD double dt_norm_den(float var) { return sqrt((double)var) + (double).000001f; }
BP_HD float dt_norm(float x, float mean, double den) { return (float)((double)(x - mean) / den); }
BP_HD float dt_scale_bias(float xn, float scale, float bias) {
    const float v = xn * scale;
    return v + bias;
}
BP_HD float dt_activate(float v, int leaky) { return leaky ? (v > 0 ? v : .1f * v) : v; }
BP_HD float dt_gradient(float out, int leaky) { return leaky ? (out > 0 ? 1.0f : .1f) : 1.0f; }

// mean_delta_cpu, variance_delta_cpu: the f64 sum rounded to float as Darknet's accumulator is, then its double factor.
// pow(v, -3/2) is 1 / (v sqrt v) here (no math library's pow on either side).
BP_HD float dt_mean_delta(double sum, float var) { return (float)((double)(float)sum * (-1. / sqrt((double)(var + .00001f)))); }
BP_HD float dt_variance_delta(double sum, float var) {
    const double v = (double)(var + .00001f);
    return (float)((double)(float)sum * (-.5 * (1. / (v * sqrt(v)))));
}
// normalize_delta_cpu, term by term in its precedence: d * 1. / (sqrt(var) + .00001f) + vd * 2. * (x - mean) / count +
// md / count, the last a float division
BP_HD float dt_normalize_delta(float d, float x, float mean, float var, float md, float vd, int count) {
    const double a = (double)d * 1. / (sqrt((double)var) + (double).00001f);
    const double b = (double)vd * 2. * (double)(x - mean) / (double)count;
    const double c = (double)(md / (float)count);
    return (float)(a + b + c);
}

// ---------------------------------------------------------------------------------------------------- update
// update_convolutional_layer for one element: kind 1 (filters) takes the decay step first; three rounded steps
BP_HD void dt_update(float& p, float& u, int kind, float rate_over_batch, float decay_term, float momentum) {
    if (kind) u = u + decay_term * p;
    p = p + rate_over_batch * u;
    u = u * momentum;
}
