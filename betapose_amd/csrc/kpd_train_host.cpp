// Host twins of the key-point detector's training kernels (include/betapose_hip.h bp_kpd_train_*_host): plain loops around
// the lane and unit functions of kpd_train_math.inc, the text kpd_train.hip compiles too.  A reduction is summed in the
// order the kernels' lanes and waves fix, so these results and the kernels' are meant to be equal bit for bit.
#include <cmath>
#include <cstdint>
#include <vector>

#include "kpd_train.h"

#pragma clang fp contract(off)

namespace bp {

namespace {
#include "darknet_train_math.inc"
#include "yolo_train_math.inc"

inline void kt_ld4(const float* p, float* r) { r[0] = p[0], r[1] = p[1], r[2] = p[2], r[3] = p[3]; }
inline void kt_st4(float* p, const float* r) { p[0] = r[0], p[1] = r[1], p[2] = r[2], p[3] = r[3]; }

#include "kpd_train_math.inc"

// what one block of DT_THREADS lanes makes of its lanes' values: a shuffle tree per wave, then the waves in order
double kt_block_sum(double* lane) {
    double total = 0.0;
    for (int w = 0; w < DT_THREADS / DT_WAVE; ++w) {
        double* l = lane + w * DT_WAVE;
        for (int o = DT_WAVE / 2; o > 0; o >>= 1)
            for (int t = 0; t < o; ++t) l[t] = l[t] + l[t + o];
        total = w == 0 ? l[0] : total + l[0];
    }
    return total;
}

template <int V>
void bn_forward(const float* x, int N, int C, int S, const float* w, const float* b, float* running_mean, float* running_var,
                float* mean, float* invstd, float* out, int bn, int relu, int train) {
    const int count = N * S;
    double lane[DT_THREADS];
    for (int f = 0; f < C; ++f) {
        float mu = 0.0f, is = 1.0f;
        if (bn && train) {
            for (int t = 0; t < DT_THREADS; ++t) lane[t] = kt_bnf_sum<V>(x, f, C, S, count, t, 0, 0.0);
            const double m = kt_block_sum(lane) / (double)count;
            for (int t = 0; t < DT_THREADS; ++t) lane[t] = kt_bnf_sum<V>(x, f, C, S, count, t, 1, m);
            const double ss = kt_block_sum(lane), var = ss / (double)count;
            mu = (float)m, is = kt_invstd(var);
            mean[f] = mu, invstd[f] = is;
            running_mean[f] = kt_running(running_mean[f], m), running_var[f] = kt_running(running_var[f], ss / (double)(count - 1));
        } else if (bn) {
            mu = running_mean[f], is = kt_invstd((double)running_var[f]);
        }
        for (int t = 0; t < DT_THREADS; ++t)
            kt_bnf_apply<V>(x, out, f, C, S, count, t, mu, is, bn ? w[f] : 1.0f, b[f], bn, relu);
    }
}

template <int V>
void bn_backward(const float* out, float* d, const float* x, const float* mean, const float* invstd, const float* w, int N, int C,
                 int S, float* grad_w, float* grad_b, int bn, int relu) {
    const int count = N * S;
    double l0[DT_THREADS], l1[DT_THREADS];
    for (int f = 0; f < C; ++f) {
        const float mu = bn ? mean[f] : 0.0f, is = bn ? invstd[f] : 1.0f, wf = bn ? w[f] : 1.0f;
        for (int t = 0; t < DT_THREADS; ++t) kt_bnb_sum<V>(out, d, x, f, C, S, count, t, mu, bn, relu, &l0[t], &l1[t]);
        const double sum = kt_block_sum(l0);
        grad_b[f] = grad_b[f] + (float)sum;
        double k = 0.0;
        if (bn) {
            const double dotp = kt_block_sum(l1);
            grad_w[f] = grad_w[f] + (float)(dotp * (double)is);
            k = kt_bn_k(dotp, is, count);
        }
        for (int t = 0; t < DT_THREADS; ++t) kt_bnb_apply<V>(out, d, x, f, C, S, count, t, mu, sum / (double)count, k, is, wf, bn, relu);
    }
}

template <int V>
void rows(const float* y, const float* out, const float* dout, int nrows, int S, int mode, float* dst) {
    double lane[DT_THREADS];
    for (int r = 0; r < nrows; ++r) {
        const size_t at = (size_t)r * S;
        for (int t = 0; t < DT_THREADS; ++t) lane[t] = kt_row_sum<V>(y + at, mode ? out + at : nullptr, mode ? dout + at : nullptr, S, t, mode);
        const double sum = kt_block_sum(lane);
        dst[r] = mode ? (float)sum : kt_pool(sum, S);
    }
}
}  // namespace

int kpd_train_update_chunk() { return KT_UPD_CHUNK; }

void kpd_train_bn_forward_host(const float* x, int N, int C, int S, const float* w, const float* b, float* running_mean,
                               float* running_var, float* mean, float* invstd, float* out, int bn, int relu, int train) {
    if (kt_vec(S) == 4) bn_forward<4>(x, N, C, S, w, b, running_mean, running_var, mean, invstd, out, bn, relu, train);
    else bn_forward<1>(x, N, C, S, w, b, running_mean, running_var, mean, invstd, out, bn, relu, train);
}

void kpd_train_bn_backward_host(const float* out, float* d, const float* x, const float* mean, const float* invstd, const float* w,
                                int N, int C, int S, float* grad_w, float* grad_b, int bn, int relu) {
    if (kt_vec(S) == 4) bn_backward<4>(out, d, x, mean, invstd, w, N, C, S, grad_w, grad_b, bn, relu);
    else bn_backward<1>(out, d, x, mean, invstd, w, N, C, S, grad_w, grad_b, bn, relu);
}

void kpd_train_tail_forward_host(const float* y, const float* s, const float* res, float* out, int N, int C, int S) {
    const size_t total = (size_t)N * C * S;
    if (kt_vec(S) == 4) for (size_t u = 0; u < total / 4; ++u) kt_tail_fwd_unit<4>(y, s, res, out, S, u);
    else for (size_t u = 0; u < total; ++u) kt_tail_fwd_unit<1>(y, s, res, out, S, u);
}

void kpd_train_tail_backward_host(const float* out, const float* dout, const float* y, const float* s, float* dres, float* dy,
                                  float* ds, int N, int C, int S) {
    if (s) {            // (before dy is written: dy may be any buffer but out, dout and y)
        if (kt_vec(S) == 4) rows<4>(y, out, dout, N * C, S, 1, ds);
        else rows<1>(y, out, dout, N * C, S, 1, ds);
    }
    const size_t total = (size_t)N * C * S;
    if (kt_vec(S) == 4) for (size_t u = 0; u < total / 4; ++u) kt_tail_bwd_unit<4>(out, dout, s, dres, dy, S, u);
    else for (size_t u = 0; u < total; ++u) kt_tail_bwd_unit<1>(out, dout, s, dres, dy, S, u);
}

void kpd_train_pool_forward_host(const float* y, int nrows, int S, float* pool) {
    if (kt_vec(S) == 4) rows<4>(y, nullptr, nullptr, nrows, S, 0, pool);
    else rows<1>(y, nullptr, nullptr, nrows, S, 0, pool);
}

void kpd_train_pool_backward_host(const float* dpool, float* dy, int nrows, int S) {
    const size_t total = (size_t)nrows * S;
    if (kt_vec(S) == 4) for (size_t u = 0; u < total / 4; ++u) kt_pool_bwd_unit<4>(dpool, dy, S, u);
    else for (size_t u = 0; u < total; ++u) kt_pool_bwd_unit<1>(dpool, dy, S, u);
}

void kpd_train_sigmoid_forward_host(const float* x, float* s, long long n) {
    for (long long i = 0; i < n; ++i) s[i] = kt_sigmoid(x[i]);
}

void kpd_train_sigmoid_backward_host(const float* s, float* g, long long n) {
    for (long long i = 0; i < n; ++i) g[i] = kt_sigmoid_back(g[i], s[i]);
}

void kpd_train_maxpool_forward_host(const float* x, int planes, int H, int W, float* out, int* arg) {
    const int OH = kt_pool_out(H), OW = kt_pool_out(W);
    for (int p = 0; p < planes; ++p)
        for (int oy = 0; oy < OH; ++oy)
            for (int ox = 0; ox < OW; ++ox) {
                const size_t o = ((size_t)p * OH + oy) * OW + ox;
                arg[o] = kt_window(x + (size_t)p * H * W, H, W, oy, ox, &out[o]);
            }
}

void kpd_train_maxpool_backward_host(const float* dout, const int* arg, int planes, int H, int W, float* dx) {
    const int OH = kt_pool_out(H), OW = kt_pool_out(W);
    for (int p = 0; p < planes; ++p)
        for (int iy = 0; iy < H; ++iy)
            for (int ix = 0; ix < W; ++ix)
                dx[((size_t)p * H + iy) * W + ix] =
                    kt_pool_gather(dout + (size_t)p * OH * OW, arg + (size_t)p * OH * OW, H, W, OH, OW, iy, ix);
}

void kpd_train_rmsprop_host(const KpdTrainTensor* table, int tensors, KpdTrainOpt o) {
    const KtOpt k = {o.lr, o.alpha, o.one_minus_alpha, o.eps, o.wd, o.momentum};
    for (int t = 0; t < tensors; ++t)
        for (long long i = 0; i < table[t].count; ++i) {
            float b = k.momentum > 0.0f ? table[t].b[i] : 0.0f;
            kt_rmsprop(table[t].p[i], table[t].g[i], table[t].v[i], b, k);
            if (k.momentum > 0.0f) table[t].b[i] = b;
        }
}

}  // namespace bp
