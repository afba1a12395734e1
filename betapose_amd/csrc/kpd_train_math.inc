// The arithmetic of one key-point-detector training iteration outside its convolutions (DESIGN.md 3.14), ONE source for
// the host twins (kpd_train_host.cpp) and the device kernels (kpd_train.hip): PyTorch's batch norm forward and backward
// with the fused ReLU, the bottleneck's tail, the SE gate's pool and sigmoid, the 3 x 3 / 2 max-pool's window, and
// torch.optim.RMSprop's element step.  Host and device compile this text and do the same f64 / f32 / integer operations
// in the same order, without FMA contraction, so their outputs agree bit for bit; only who loops over what differs per
// side.  The convolutions and Linears are darknet_train_math.inc's GEMM core, unchanged.
// Plain C++17, no HIP header.  Included inside `namespace bp { namespace {` after darknet_train_math.inc (DT_THREADS,
// DT_WAVE, BP_HD) and yolo_train_math.inc's yt_exp, in a unit that has `#pragma clang fp contract(off)` in force.
//
// Conventions: activations and gradients are float32 [N][C][S]; a gradient is the loss's (torch's sign).

constexpr int KT_UPD_CHUNK = 1024;          // elements one block of the RMSprop launch handles

// ---------------------------------------------------------------------------------------------------- batch norm
// The statistics stay in f64 until they are stored: mean = sum / n; var = sum((x - mean)^2) / n with the difference
// formed in f64 from the f64 mean; invstd = 1 / sqrt(var + eps).
BP_HD double kt_sq(float x, double mean) {
    const double d = (double)x - mean;
    return d * d;
}
BP_HD float kt_invstd(double var) { return (float)(1.0 / sqrt(var + 1e-5)); }
// running = (1 - momentum) running + momentum batch in f64, rounded once (momentum 0.1)
BP_HD float kt_running(float running, double v) { return (float)(0.9 * (double)running + 0.1 * v); }
// y = ((x - mean) * invstd) * w + b in four rounded f32 steps, then the ReLU
BP_HD float kt_bn(float x, float mean, float invstd, float w, float b, int relu) {
    float v = x - mean;
    v = v * invstd;
    v = v * w;
    v = v + b;
    return relu && !(v > 0.0f) ? 0.0f : v;
}
BP_HD float kt_bias(float x, float b, int relu) {
    const float v = x + b;
    return relu && !(v > 0.0f) ? 0.0f : v;
}
// the ReLU's backward keyed on the stored output
BP_HD float kt_mask(float dy, float out, int relu) { return relu && !(out > 0.0f) ? 0.0f : dy; }
BP_HD double kt_dot(float d, float x, float mean) { return (double)d * ((double)x - (double)mean); }
// dx = (dy - sum / n - (x - mean) * dotp * invstd^2 / n) * invstd * w: gm = sum / n and k = dotp * invstd * invstd / n
// are formed once per channel in f64; the element is f64 throughout and rounded once
BP_HD double kt_bn_k(double dotp, float invstd, int n) { return dotp * (double)invstd * (double)invstd / (double)n; }
BP_HD float kt_bn_dx(float d, float x, float mean, double gm, double k, float invstd, float w) {
    return (float)((((double)d - gm) - ((double)x - (double)mean) * k) * (double)invstd * (double)w);
}

// ---------------------------------------------------------------------------------------------------- block tail
// out = relu(y * s + residual): two rounded steps; s is 1 (no multiply) in a block without SE
BP_HD float kt_tail(float y, float s, int has_s, float r) {
    float v = has_s ? y * s : y;
    v = v + r;
    return v > 0.0f ? v : 0.0f;
}

// ---------------------------------------------------------------------------------------------------- SE gate
BP_HD float kt_pool(double sum, int S) { return (float)(sum * (1.0 / (double)S)); }
BP_HD float kt_pool_back(float dy, float dpool, int S) { return dy + dpool * (float)(1.0 / (double)S); }
BP_HD float kt_sigmoid(float x) { return (float)(1.0 / (1.0 + yt_exp(-(double)x))); }
// torch's sigmoid_backward: grad * (1 - s) * s, left to right
BP_HD float kt_sigmoid_back(float g, float s) {
    const float t = g * (1.0f - s);
    return t * s;
}

// ---------------------------------------------------------------------------------------------------- max-pool 3 / 2 / 1
BP_HD int kt_pool_out(int n) { return (n - 1) / 2 + 1; }
// the window of output (oy, ox) scanned rows first: the first maximum wins (`val > maxval` from -inf); the padding is
// never read, so it is -inf.  Returns the flat index iy * W + ix of the maximum.
BP_HD int kt_window(const float* __restrict__ x, int H, int W, int oy, int ox, float* best) {
    float m = -__builtin_inff();
    int at = -1;
    for (int ky = 0; ky < 3; ++ky) {
        const int iy = 2 * oy - 1 + ky;
        if (iy < 0 || iy >= H) continue;
        for (int kx = 0; kx < 3; ++kx) {
            const int ix = 2 * ox - 1 + kx;
            if (ix < 0 || ix >= W) continue;
            const float v = x[iy * W + ix];
            if (v > m || at < 0) m = v, at = iy * W + ix;
        }
    }
    *best = m;
    return at;
}
// the gradient of input (iy, ix): the outputs whose window holds it (at most two per axis), rows first, added in that
// order from zero where their arg-max is this position
BP_HD float kt_pool_gather(const float* __restrict__ dout, const int* __restrict__ arg, int H, int W, int OH, int OW, int iy, int ix) {
    float t = 0.0f;
    const int me = iy * W + ix;
    for (int oy = iy / 2; oy <= (iy + 1) / 2; ++oy) {
        if (oy >= OH) continue;
        for (int ox = ix / 2; ox <= (ix + 1) / 2; ++ox) {
            if (ox >= OW) continue;
            if (arg[oy * OW + ox] == me) t = t + dout[oy * OW + ox];
        }
    }
    return t;
}

// ---------------------------------------------------------------------------------------------------- RMSprop
// torch.optim.RMSprop (_single_tensor_rmsprop, not centred) for one element, each line's roundings as torch's CPU
// kernels make them.  Those kernels are compiled with contraction on, so `add(alpha=)` and `addcmul` come out as fused
// multiply-adds (one rounding); measured against the installed torch on 20 000 elements per setting, this text gives
// square_avg bit for bit, and the parameter and the momentum buffer but for under 1 % of the elements, by one ulp (torch's
// vector division).  kt_fma is the explicit fused step on both sides.
//   g = fma(wd, p, g)                                      (weight_decay != 0)
//   v = v * alpha;  v = fma((1 - alpha) * g, g, v)
//   a = sqrt(v) + eps
//   b = b * m;  b = b + g / a;  p = fma(-lr, b, p)         (momentum > 0)
//   p = p + ((-lr) * g) / a                                (otherwise)
// f32 sqrt and division through f64 (53 >= 2 * 24 + 2 bits: the double rounding is innocuous, the result the correctly
// rounded f32 one on both sides, whatever the compiler's f32 division and sqrt options are)
BP_HD float kt_sqrt(float v) { return (float)sqrt((double)v); }
BP_HD float kt_div(float a, float b) { return (float)((double)a / (double)b); }
struct KtOpt {
    float lr, alpha, one_minus_alpha, eps, wd, momentum;
};
BP_HD float kt_fma(float a, float b, float c) { return __builtin_fmaf(a, b, c); }
BP_HD void kt_rmsprop(float& p, float g, float& v, float& b, const KtOpt& o) {
    if (o.wd != 0.0f) g = kt_fma(o.wd, p, g);
    v = v * o.alpha;
    float t = o.one_minus_alpha * g;
    v = kt_fma(t, g, v);
    const float a = kt_sqrt(v) + o.eps;
    if (o.momentum > 0.0f) {
        b = b * o.momentum;
        b = b + kt_div(g, a);
        p = kt_fma(-o.lr, b, p);
    } else {
        t = -o.lr * g;
        t = kt_div(t, a);
        p = p + t;
    }
}

// ---------------------------------------------------------------------------------------------------- who reads what
// A pass over the N * S values of channel f of a [N][C][S] tensor, over the S values of one row, or over a flat tensor
// is cut into units of V values: V = 4 where S (or the flat count) is a multiple of 4, so a unit never straddles a row
// and is one 16-byte access on the device, else V = 1.  Lane t of the block takes units t, t + DT_THREADS, ... ascending
// and the values of a unit in order; that fixes the order of every sum below on both sides.  kt_ld4 / kt_st4 are the
// side's 16-byte (device) or four scalar (host) accesses, defined before this text is included.
BP_HD int kt_vec(long long n) { return n % 4 == 0 ? 4 : 1; }
BP_HD size_t kt_at(int e, int f, int C, int S) { return ((size_t)(e / S) * C + f) * S + e % S; }
template <int V>
BP_HD void kt_ld(const float* p, float* r) {
    if constexpr (V == 4) kt_ld4(p, r);
    else r[0] = p[0];
}
template <int V>
BP_HD void kt_st(float* p, const float* r) {
    if constexpr (V == 4) kt_st4(p, r);
    else p[0] = r[0];
}

// batch-norm forward, lane t of channel f: pass 0 sums x, pass 1 the squared distances from the f64 mean
template <int V>
BP_HD double kt_bnf_sum(const float* x, int f, int C, int S, int count, int t, int pass, double mean) {
    double s = 0.0;
    for (int u = t; u < count / V; u += DT_THREADS) {
        float r[V];
        kt_ld<V>(x + kt_at(u * V, f, C, S), r);
        for (int i = 0; i < V; ++i) s = s + (pass ? kt_sq(r[i], mean) : (double)r[i]);
    }
    return s;
}
template <int V>
BP_HD void kt_bnf_apply(const float* x, float* out, int f, int C, int S, int count, int t, float mean, float invstd, float w,
                        float b, int bn, int relu) {
    for (int u = t; u < count / V; u += DT_THREADS) {
        float r[V];
        const size_t at = kt_at(u * V, f, C, S);
        kt_ld<V>(x + at, r);
        for (int i = 0; i < V; ++i) r[i] = bn ? kt_bn(r[i], mean, invstd, w, b, relu) : kt_bias(r[i], b, relu);
        kt_st<V>(out + at, r);
    }
}
// batch-norm backward, lane t of channel f: sum(d) and sum(d * (x - mean)) of the masked gradient in one read
template <int V>
BP_HD void kt_bnb_sum(const float* out, const float* d, const float* x, int f, int C, int S, int count, int t, float mean, int bn,
                      int relu, double* s0, double* s1) {
    double a = 0.0, b = 0.0;
    for (int u = t; u < count / V; u += DT_THREADS) {
        float rd[V], ro[V], rx[V];
        const size_t at = kt_at(u * V, f, C, S);
        kt_ld<V>(d + at, rd);
        if (relu) kt_ld<V>(out + at, ro);
        if (bn) kt_ld<V>(x + at, rx);
        for (int i = 0; i < V; ++i) {
            const float m = kt_mask(rd[i], relu ? ro[i] : 1.0f, relu);
            a = a + (double)m;
            if (bn) b = b + kt_dot(m, rx[i], mean);
        }
    }
    *s0 = a, *s1 = b;
}
template <int V>
BP_HD void kt_bnb_apply(const float* out, float* d, const float* x, int f, int C, int S, int count, int t, float mean, double gm,
                        double k, float invstd, float w, int bn, int relu) {
    for (int u = t; u < count / V; u += DT_THREADS) {
        float rd[V], ro[V], rx[V];
        const size_t at = kt_at(u * V, f, C, S);
        kt_ld<V>(d + at, rd);
        if (relu) kt_ld<V>(out + at, ro);
        if (bn) kt_ld<V>(x + at, rx);
        for (int i = 0; i < V; ++i) {
            const float m = kt_mask(rd[i], relu ? ro[i] : 1.0f, relu);
            rd[i] = bn ? kt_bn_dx(m, rx[i], mean, gm, k, invstd, w) : m;
        }
        kt_st<V>(d + at, rd);
    }
}
// one row of S values, lane t: mode 0 sums y (the SE pool), mode 1 sums mask(dout, out) * y (the gate's gradient)
template <int V>
BP_HD double kt_row_sum(const float* y, const float* out, const float* dout, int S, int t, int mode) {
    double s = 0.0;
    for (int u = t; u < S / V; u += DT_THREADS) {
        float ry[V], ro[V], rd[V];
        kt_ld<V>(y + u * V, ry);
        if (mode) kt_ld<V>(out + u * V, ro), kt_ld<V>(dout + u * V, rd);
        for (int i = 0; i < V; ++i) s = s + (mode ? (double)kt_mask(rd[i], ro[i], 1) * (double)ry[i] : (double)ry[i]);
    }
    return s;
}
// unit u of the flat element-wise passes; row = element / S picks the per-row factor
template <int V>
BP_HD void kt_tail_fwd_unit(const float* y, const float* s, const float* res, float* out, int S, size_t u) {
    float ry[V], rr[V];
    const size_t at = u * V;
    kt_ld<V>(y + at, ry), kt_ld<V>(res + at, rr);
    const float sv = s ? s[at / S] : 1.0f;
    for (int i = 0; i < V; ++i) ry[i] = kt_tail(ry[i], sv, s != nullptr, rr[i]);
    kt_st<V>(out + at, ry);
}
template <int V>
BP_HD void kt_tail_bwd_unit(const float* out, const float* dout, const float* s, float* dres, float* dy, int S, size_t u) {
    float ro[V], rd[V], rr[V];
    const size_t at = u * V;
    kt_ld<V>(out + at, ro), kt_ld<V>(dout + at, rd), kt_ld<V>(dres + at, rr);
    const float sv = s ? s[at / S] : 1.0f;
    for (int i = 0; i < V; ++i) {
        const float m = kt_mask(rd[i], ro[i], 1);
        rr[i] = rr[i] + m;
        rd[i] = s ? m * sv : m;
    }
    kt_st<V>(dres + at, rr), kt_st<V>(dy + at, rd);
}
template <int V>
BP_HD void kt_pool_bwd_unit(const float* dpool, float* dy, int S, size_t u) {
    float r[V];
    const size_t at = u * V;
    kt_ld<V>(dy + at, r);
    const float g = dpool[at / S];
    for (int i = 0; i < V; ++i) r[i] = kt_pool_back(r[i], g, S);
    kt_st<V>(dy + at, r);
}
