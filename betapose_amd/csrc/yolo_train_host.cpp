// Host twins of the detector training calls (include/betapose_hip.h bp_yolo_inputs_host, bp_yolo_truth_host,
// bp_yolo_loss_host): plain loops around the arithmetic of yolo_train_math.inc, the text yolo_train.hip compiles too.
// The reductions over floating-point values (the any-obj sum, the statistics and the cost) are summed in the order the
// kernels' blocks, waves and lanes fix, so these results and the kernels' are equal bit for bit.
#include <cmath>
#include <cstdint>

#include "yolo_train.h"

#pragma clang fp contract(off)

namespace bp {

namespace {
#include "yolo_train_math.inc"

// what one block of YT_THREADS lanes makes of its lanes' values: a shuffle tree per wave, then the waves in order
double yt_block_sum(double* lane) {
    double total = 0.0;
    for (int w = 0; w < YT_THREADS / YT_WAVE; ++w) {
        double* l = lane + w * YT_WAVE;
        for (int o = YT_WAVE / 2; o > 0; o >>= 1)
            for (int t = 0; t < o; ++t) l[t] = l[t] + l[t + o];
        total = w == 0 ? l[0] : total + l[0];
    }
    return total;
}
}  // namespace

size_t yolo_loss_partials(int B, int n, int classes, int h, int w) {
    return yt_any_blocks(B, n, h, w) + (size_t)B * YT_IMAGE_STATS + yt_cost_blocks(B, n, classes, h, w);
}

void yolo_inputs_host(const unsigned char* frames, int N, int H, int W, const int* frame_index, const int* crop,
                      const unsigned char* flip, const float* hsv, int B, int net_h, int net_w, float* out) {
    const size_t plane = (size_t)net_h * net_w;
    for (int b = 0; b < B; ++b) {
        const int fi = frame_index[b];
        const bool zero = fi < 0 || fi >= N;
        const unsigned char* frame = zero ? nullptr : frames + (size_t)fi * H * W * 3;
        const YtCrop k = yt_crop(crop + (size_t)b * 4, net_h, net_w);
        const float* d = hsv ? hsv + (size_t)b * 3 : nullptr;
        float* o = out + (size_t)b * 3 * plane;
        for (int y = 0; y < net_h; ++y)
            for (int x = 0; x < net_w; ++x) {
                float rgb[3] = {0.0f, 0.0f, 0.0f};
                if (!zero) yt_input_rgb(frame, H, W, k, net_h, net_w, flip[b] != 0, d, y, x, rgb);
                for (int c = 0; c < 3; ++c) o[c * plane + (size_t)y * net_w + x] = rgb[c];
            }
    }
}

void yolo_truth_host(const float* labels, int M, const int* first, const int* swap, const float* geom, const unsigned char* flip,
                     int B, int classes, int max_boxes, int net_w, int net_h, int small_object, int* order, float* truth,
                     int* kept) {
    (void)small_object;
    for (int b = 0; b < B; ++b) {
        int f0 = first[b], f1 = first[b + 1];
        f0 = f0 < 0 ? 0 : (f0 > M ? M : f0);
        f1 = f1 < f0 ? f0 : (f1 > M ? M : f1);
        const float* g = geom + (size_t)b * 4;
        kept[b] = yt_truth_rows(labels + (size_t)f0 * 5, f1 - f0, swap + f0, g[0], g[1], g[2], g[3], flip[b] != 0, classes,
                                max_boxes, net_w, net_h, order + f0, truth + (size_t)b * max_boxes * 5);
    }
}

void yolo_loss_host(const float* x, int B, int n, int classes, int h, int w, int net_w, int net_h, const float* anchors, int total,
                    const int* mask, const float* truth, int max_boxes, float ignore_thresh, float truth_thresh, float* act,
                    float* delta, double* cost, double* stats, double* partial) {
    const YtHead L = {B, n, classes, h, w, net_w, net_h, total, max_boxes, ignore_thresh, truth_thresh};
    const int wh = h * w;
    const size_t cells = (size_t)B * n * wh, elems = cells * (5 + classes);
    const size_t nA = yt_any_blocks(B, n, h, w), nC = yt_cost_blocks(B, n, classes, h, w);
    double* p_any = partial;
    double* p_img = partial + nA;
    double* p_cost = p_img + (size_t)B * YT_IMAGE_STATS;
    double lane[YT_THREADS];
    // 1. cells
    for (size_t k = 0; k < nA; ++k) {
        for (int t = 0; t < YT_THREADS; ++t) {
            const size_t g = k * YT_THREADS + t;
            lane[t] = 0.0;
            if (g < cells) {
                const int loc = (int)(g % wh), a = (int)(g / wh % n), b = (int)(g / wh / n);
                lane[t] = (double)yt_cell(L, x, anchors, mask, truth, b, a, loc, act, delta);
            }
        }
        p_any[k] = yt_block_sum(lane);
    }
    // 2. truths
    for (int b = 0; b < B; ++b) yt_truth_walk(L, x, anchors, mask, truth, b, delta, p_img + (size_t)b * YT_IMAGE_STATS);
    // 3. cost
    for (size_t k = 0; k < nC; ++k) {
        for (int t = 0; t < YT_THREADS; ++t) {
            double s = 0.0;
            for (size_t e = k * YT_CHUNK + t; e < (k + 1) * YT_CHUNK && e < elems; e += YT_THREADS)
                s = s + (double)delta[e] * (double)delta[e];
            lane[t] = s;
        }
        p_cost[k] = yt_block_sum(lane);
    }
    double any = 0.0, c = 0.0, st[YT_IMAGE_STATS] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (size_t k = 0; k < nA; ++k) any = any + p_any[k];
    for (int b = 0; b < B; ++b)
        for (int i = 0; i < YT_IMAGE_STATS; ++i) st[i] = st[i] + p_img[(size_t)b * YT_IMAGE_STATS + i];
    for (size_t k = 0; k < nC; ++k) c = c + p_cost[k];
    *cost = c;
    stats[0] = st[0], stats[1] = st[1], stats[2] = st[2], stats[3] = any, stats[4] = st[3], stats[5] = st[4], stats[6] = st[5];
}

}  // namespace bp
