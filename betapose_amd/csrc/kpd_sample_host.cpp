// Host twins of the KPD training sample calls (include/betapose_hip.h bp_kpd_inputs_host, bp_kpd_augment_host,
// bp_heatmap_loss_acc_host): plain loops around the arithmetic of kpd_sample_math.inc, the text kpd_sample.hip compiles
// too.  The one reduction over floating-point values, the loss, is summed in the order that file fixes for both sides,
// so these results and the kernels' are equal bit for bit.
#include <cmath>
#include <cstdint>

#include "kpd_sample.h"

#pragma clang fp contract(off)

namespace bp {

namespace {
#include "kpd_sample_math.inc"
}  // namespace

void kpd_inputs_host(const unsigned char* frames, int N, int H, int W, const int* frame_index, const float* ul, const float* br,
                     const float* gains, const unsigned char* blank, int B, int inpH, int inpW, float* inp) {
    for (int b = 0; b < B; ++b) {
        const int fi = frame_index[b];
        const bool zero = (blank && blank[b]) || fi < 0 || fi >= N;
        const unsigned char* frame = zero ? nullptr : frames + (size_t)fi * H * W * 3;
        const KsWindow k = ks_window(ul[b * 2], ul[b * 2 + 1], br[b * 2], br[b * 2 + 1], inpH, inpW);
        const float* gain = gains ? gains + (size_t)b * 3 : nullptr;
        for (int c = 0; c < 3; ++c)
            for (int y = 0; y < inpH; ++y)
                for (int x = 0; x < inpW; ++x)
                    inp[(((size_t)b * 3 + c) * inpH + y) * inpW + x] = zero ? 0.0f : ks_input_value(k, frame, H, W, gain, c, y, x);
    }
}

void kpd_augment_host(const float* x, int B, int C, int H, int W, const unsigned char* flip, const double* cs, const int* perm,
                      float* y) {
    const size_t HW = (size_t)H * W;
    for (int b = 0; b < B; ++b)
        for (int c = 0; c < C; ++c) {
            const int f = flip[b] != 0;
            const float* src = x + ((size_t)b * C + ks_source_channel(perm, C, f, c)) * HW;
            float* dst = y + ((size_t)b * C + c) * HW;
            for (int i = 0; i < H; ++i)
                for (int j = 0; j < W; ++j) dst[(size_t)i * W + j] = ks_augment_value(src, H, W, f, cs + (size_t)b * 2, i, j);
        }
}

void heatmap_loss_acc_host(const float* out, const float* labels, const float* set_mask, int B, int K, int H, int W,
                           double* partial, double* loss, float* acc, int* preds, int* gt, float* dists, float* grad) {
    const int HW = H * W, maps = B * K;
    const double count = (double)maps * (double)HW;
    const float norm = (float)(2.0 / count);
    for (int m = 0; m < maps; ++m) {
        const size_t base = (size_t)m * HW;
        double lane[KS_THREADS];
        for (int t = 0; t < KS_THREADS; ++t) lane[t] = 0.0;
        KsBest bp = ks_best_empty(), bg = ks_best_empty();
        for (int e = 0; e < HW; ++e) {
            float p;
            const float* mk = set_mask ? set_mask + base + e : nullptr;
            const float d = ks_residual(out[base + e], mk, labels[base + e], &p);
            double& a = lane[(e / 4) % KS_THREADS];
            a = a + (double)d * (double)d;
            bp = ks_best_of(bp, KsBest{p, e});
            bg = ks_best_of(bg, KsBest{labels[base + e], e});
            if (grad) grad[base + e] = ks_gradient(norm, d, mk);
        }
        double total = 0.0;
        for (int w = 0; w < KS_THREADS / KS_WAVE; ++w) {
            double* l = lane + w * KS_WAVE;
            for (int o = KS_WAVE / 2; o > 0; o >>= 1)
                for (int t = 0; t < o; ++t) l[t] = l[t] + l[t + o];
            total = w == 0 ? l[0] : total + l[0];
        }
        partial[m] = total;
        const int ip = ks_best_index(bp), ig = ks_best_index(bg);
        preds[(size_t)m * 2] = ip % W;
        preds[(size_t)m * 2 + 1] = ip / W;
        gt[(size_t)m * 2] = ig % W;
        gt[(size_t)m * 2 + 1] = ig / W;
    }
    double sum = 0.0;
    for (int m = 0; m < maps; ++m) sum = sum + partial[m];
    *loss = sum / count;
    float avg = 0.0f;
    int cnt = 0;
    for (int k = 0; k < K; ++k) {
        int valid = 0, hits = 0;
        for (int b = 0; b < B; ++b) {
            const size_t m = (size_t)b * K + k;
            const float d = ks_dist(preds[m * 2], preds[m * 2 + 1], gt[m * 2], gt[m * 2 + 1], H);
            dists[(size_t)k * B + b] = d;
            if (d != -1.0f) {
                ++valid;
                hits += d <= 0.5f;
            }
        }
        const float a = valid ? (float)hits / (float)valid : -1.0f;
        acc[1 + k] = a;
        if (a >= 0.0f) {
            avg = avg + a;
            ++cnt;
        }
    }
    acc[0] = cnt ? avg / (float)cnt : 0.0f;
}

}  // namespace bp
