// Host twins of the training iteration (include/betapose_hip.h bp_train_conv_host, bp_train_bn_forward_host,
// bp_train_bn_backward_host, bp_train_update_host): plain loops around the arithmetic of darknet_train_math.inc, the
// text darknet_train.hip compiles too.  A GEMM element is one fmaf chain over k in the order the .inc fixes, started
// from zero per reduction slice, the slices added in order; a reduction over floating-point values is summed in the
// order the kernels' lanes and waves fix.  So these results and the kernels' are meant to be equal bit for bit.
#include <cmath>
#include <cstdint>
#include <vector>

#include "darknet_train.h"

#pragma clang fp contract(off)

namespace bp {

namespace {
#include "darknet_train_math.inc"

// what one block of DT_THREADS lanes makes of its lanes' values: a shuffle tree per wave, then the waves in order
double dt_block_sum(double* lane) {
    double total = 0.0;
    for (int w = 0; w < DT_THREADS / DT_WAVE; ++w) {
        double* l = lane + w * DT_WAVE;
        for (int o = DT_WAVE / 2; o > 0; o >>= 1)
            for (int t = 0; t < o; ++t) l[t] = l[t] + l[t + o];
        total = w == 0 ? l[0] : total + l[0];
    }
    return total;
}

// element e = b * S + k of channel f of a [N][C][S] tensor
inline size_t dt_at(int e, int f, int C, int S) { return ((size_t)(e / S) * C + f) * S + e % S; }
}  // namespace

size_t train_conv_scratch(int N, int C, int H, int W, int K, int size, int stride) {
    const DtG g = dt_geom(DT_FILTER_GRAD, N, C, H, W, K, size, stride);
    return (size_t)g.slices * g.M * g.Ncol;
}

int train_update_chunk() { return DT_UPD_CHUNK; }

void train_conv_host(int role, float* x, float* w, float* y, int N, int C, int H, int W, int K, int size, int stride,
                     float* scratch) {
    const DtG g = dt_geom(role, N, C, H, W, K, size, stride);
    const float* a = role == DT_FILTER_GRAD ? y : w;
    const float* b = role == DT_INPUT_GRAD ? y : x;
    float* d = role == DT_FORWARD ? y : (role == DT_FILTER_GRAD ? scratch : x);
    std::vector<float> av, bv;
    for (int s = 0; s < g.slices; ++s) {
        const int k0 = dt_slice_begin(g, s), k1 = dt_slice_end(g, s);
        const int kp = k0 + (k1 - k0 + DT_BK - 1) / DT_BK * DT_BK;    // the device's last step is padded with zeros
        const size_t L = (size_t)(kp - k0);
        av.resize(L * g.M), bv.resize(L);
        for (int m = 0; m < g.M; ++m)
            for (int k = k0; k < kp; ++k) av[m * L + (size_t)(k - k0)] = k < k1 ? dt_a(g, a, m, k) : 0.0f;
        for (int j = 0; j < g.Ncol; ++j) {
            for (int k = k0; k < kp; ++k) bv[(size_t)(k - k0)] = k < k1 ? dt_b(g, b, k, j) : 0.0f;
            for (int m = 0; m < g.M; ++m) {
                float acc = 0.0f;
                for (size_t k = 0; k < L; ++k) acc = std::fmaf(av[m * L + k], bv[k], acc);
                const size_t i = dt_d_index(g, m, j, s);
                d[i] = role == DT_INPUT_GRAD ? d[i] + acc : acc;
            }
        }
    }
    if (role == DT_FILTER_GRAD)
        for (int m = 0; m < g.M; ++m)
            for (int j = 0; j < g.Ncol; ++j) {
                float t = scratch[dt_d_index(g, m, j, 0)];
                for (int s = 1; s < g.slices; ++s) t = t + scratch[dt_d_index(g, m, j, s)];
                const size_t i = dt_filter_index(g, m, j);
                w[i] = w[i] + t;
            }
}

void train_bn_forward_host(const float* x, int N, int C, int S, const float* scales, const float* biases, float* rolling_mean,
                           float* rolling_var, float* mean, float* var, float* x_norm, float* out, int bn, int leaky, int train) {
    const int count = N * S;
    double lane[DT_THREADS];
    for (int f = 0; f < C; ++f) {
        float mu = 0.0f, v = 0.0f;
        if (bn && train) {
            for (int t = 0; t < DT_THREADS; ++t) {
                double s = 0.0;
                for (int e = t; e < count; e += DT_THREADS) s = s + (double)x[dt_at(e, f, C, S)];
                lane[t] = s;
            }
            mu = dt_mean(dt_block_sum(lane), count);
            for (int t = 0; t < DT_THREADS; ++t) {
                double s = 0.0;
                for (int e = t; e < count; e += DT_THREADS) s = s + dt_sq(x[dt_at(e, f, C, S)], mu);
                lane[t] = s;
            }
            v = dt_variance(dt_block_sum(lane), count);
            mean[f] = mu, var[f] = v;
            rolling_mean[f] = dt_roll(rolling_mean[f], mu), rolling_var[f] = dt_roll(rolling_var[f], v);
        } else if (bn) {
            mu = rolling_mean[f], v = rolling_var[f];
        }
        const double den = bn ? dt_norm_den(v) : 1.0;
        for (int e = 0; e < count; ++e) {
            const size_t i = dt_at(e, f, C, S);
            float val;
            if (bn) {
                const float xn = dt_norm(x[i], mu, den);
                if (train) x_norm[i] = xn;
                val = dt_scale_bias(xn, scales[f], biases[f]);
            } else {
                val = x[i] + biases[f];
            }
            out[i] = dt_activate(val, leaky);
        }
    }
}

void train_bn_backward_host(const float* out, float* delta, const float* x, const float* x_norm, const float* mean,
                            const float* var, const float* scales, int N, int C, int S, float* bias_updates,
                            float* scale_updates, float* stat, int bn, int leaky) {
    const int count = N * S;
    double l0[DT_THREADS], l1[DT_THREADS], l2[DT_THREADS], l3[DT_THREADS];
    for (int f = 0; f < C; ++f) {
        for (int t = 0; t < DT_THREADS; ++t) {
            double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
            for (int e = t; e < count; e += DT_THREADS) {
                const size_t i = dt_at(e, f, C, S);
                const float d1 = delta[i] * dt_gradient(out[i], leaky);
                s0 = s0 + (double)d1;
                if (bn) {
                    const float d2 = d1 * scales[f];
                    s1 = s1 + (double)d1 * (double)x_norm[i];
                    s2 = s2 + (double)d2;
                    s3 = s3 + (double)d2 * (double)(x[i] - mean[f]);
                }
            }
            l0[t] = s0, l1[t] = s1, l2[t] = s2, l3[t] = s3;
        }
        bias_updates[f] = bias_updates[f] + (float)dt_block_sum(l0);
        float md = 0.0f, vd = 0.0f;
        if (bn) {
            scale_updates[f] = scale_updates[f] + (float)dt_block_sum(l1);
            md = dt_mean_delta(dt_block_sum(l2), var[f]);
            vd = dt_variance_delta(dt_block_sum(l3), var[f]);
            stat[f] = md, stat[C + f] = vd;
        }
        for (int e = 0; e < count; ++e) {
            const size_t i = dt_at(e, f, C, S);
            const float d1 = delta[i] * dt_gradient(out[i], leaky);
            delta[i] = bn ? dt_normalize_delta(d1 * scales[f], x[i], mean[f], var[f], md, vd, count) : d1;
        }
    }
}

void train_update_host(const TrainTensor* table, int tensors, float rate_over_batch, float decay_term, float momentum) {
    for (int t = 0; t < tensors; ++t)
        for (long long i = 0; i < table[t].count; ++i)
            dt_update(table[t].p[i], table[t].u[i], (int)table[t].kind, rate_over_batch, decay_term, momentum);
}

}  // namespace bp
