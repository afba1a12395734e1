// Host twins of the detector validation calls (include/betapose_hip.h bp_yolo_detections_host,
// bp_detector_map_match_host, bp_detector_map_reduce_host): plain loops around the arithmetic of yolo_map_math.inc, the
// text yolo_map.hip compiles too.  Every order the kernels fix by a key (the class passes of the NMS, the ranks) is the
// same total order here, and the one sum over floating-point values (an image's IoU sum) runs in the order the
// kernel's lanes and waves fix, so these results and the kernels' are equal bit for bit.
#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

#include "yolo_map.h"

#pragma clang fp contract(off)

namespace bp {

namespace {
#include "yolo_map_math.inc"

YmHeads ym_heads(const int* heads, int nheads) {
    YmHeads H = {};
    H.nheads = nheads;
    for (int h = 0; h < nheads; ++h) {
        H.off[h] = heads[h * 4], H.n[h] = heads[h * 4 + 1], H.cells[h] = heads[h * 4 + 2] * heads[h * 4 + 3];
        H.off[h + 1] = H.off[h] + H.n[h] * H.cells[h];
    }
    return H;
}

// what one block of YM_THREADS lanes makes of its lanes' values: a shuffle tree per wave, then the waves in order
double ym_block_sum(double* lane) {
    double total = 0.0;
    for (int w = 0; w < YM_THREADS / YT_WAVE; ++w) {
        double* l = lane + w * YT_WAVE;
        for (int o = YT_WAVE / 2; o > 0; o >>= 1)
            for (int t = 0; t < o; ++t) l[t] = l[t] + l[t + o];
        total = w == 0 ? l[0] : total + l[0];
    }
    return total;
}
}  // namespace

int yolo_map_max_dets() { return YM_MAX_DETS; }
int yolo_map_max_heads() { return YM_MAX_HEADS; }
size_t yolo_detections_scratch(int B, int max_dets, int classes) { return (size_t)B * max_dets * (6 + classes) * sizeof(float); }
size_t map_reduce_scratch(int D, int truths) {
    size_t P = YM_SORT_TILE;
    while (P < (size_t)D) P *= 2;
    return P * 2 * sizeof(unsigned long long) + ((size_t)truths + 1) * sizeof(int);
}

void yolo_detections_host(const float* pred, int B, int rows, const int* heads, int nheads, int net_w, int net_h, int classes,
                          float thresh, float nms, int max_dets, float* dets, int* count) {
    const YmHeads H = ym_heads(heads, nheads);
    const int attrs = 5 + classes, S = 6 + classes;
    std::vector<float> stage;
    std::vector<int> order, next;
    for (int b = 0; b < B; ++b) {
        const float* p = pred + (size_t)b * rows * attrs;
        float* out = dets + (size_t)b * max_dets * S;
        std::memset(out, 0, (size_t)max_dets * S * sizeof(float));
        stage.clear();
        int n = 0;
        for (int c = 0; c < rows; ++c) {
            const float* r = p + (size_t)ym_cand_row(H, c) * attrs;
            if (!(r[4] > thresh)) continue;
            stage.resize((size_t)(n + 1) * S);
            ym_det_row(r, c, classes, (float)net_w, (float)net_h, thresh, stage.data() + (size_t)n * S);
            ++n;
        }
        count[b] = n;
        if (n > max_dets) continue;         // reported by the count; the block stays zero
        order.resize(n);
        for (int i = 0; i < n; ++i) order[i] = i;
        for (int k = 0; nms > 0.0f && k < classes; ++k) {
            // the stable sort by prob[k] descending: the previous position breaks ties
            std::stable_sort(order.begin(), order.end(), [&](int a, int c) {
                return ym_bits(stage[(size_t)a * S + 6 + k]) > ym_bits(stage[(size_t)c * S + 6 + k]);
            });
            for (int i = 0; i < n; ++i) {
                const float* a = stage.data() + (size_t)order[i] * S;
                if (a[6 + k] == 0.0f) continue;
                const YtBox ba = {a[0], a[1], a[2], a[3]};
                for (int j = i + 1; j < n; ++j) {
                    float* c = stage.data() + (size_t)order[j] * S;
                    const YtBox bc = {c[0], c[1], c[2], c[3]};
                    if (yt_box_iou(ba, bc) > nms) c[6 + k] = 0.0f;
                }
            }
        }
        for (int i = 0; i < n; ++i) std::memcpy(out + (size_t)i * S, stage.data() + (size_t)order[i] * S, S * sizeof(float));
    }
}

void map_match_host(const float* dets, const int* count, int B, int max_dets, int classes, const float* labels, int M,
                    const int* first, float iou_thresh, float thresh_calc, int truth_base, int image_base, int rec_stride,
                    float* rec, int* rec_count, int* truth_classes_count, double* img_stats) {
    const int S = 6 + classes;
    std::vector<int> claim;
    double lane[YM_THREADS];
    for (int b = 0; b < B; ++b) {
        int f0 = first[b], f1 = first[b + 1];
        f0 = f0 < 0 ? 0 : (f0 > M ? M : f0);
        f1 = f1 < f0 ? f0 : (f1 > M ? M : f1);
        const int m = f1 - f0;
        const float* lab = labels + (size_t)f0 * 5;
        for (int j = 0; j < m; ++j) {
            const int k = ym_label_class(lab[(size_t)j * 5], classes);
            if (k >= 0) truth_classes_count[k]++;
        }
        const int n = count[b] > max_dets || count[b] < 0 ? 0 : count[b];
        float* out = rec + (size_t)b * rec_stride * YM_REC;
        std::memset(out, 0, (size_t)rec_stride * YM_REC * sizeof(float));
        claim.assign(m, INT_MAX);
        int r = 0;
        for (int i = 0; i < n; ++i) {
            const float* d = dets + ((size_t)b * max_dets + i) * S;
            for (int k = 0; k < classes; ++k) {
                if (!(d[6 + k] > 0.0f)) continue;
                if (r < rec_stride) {
                    float mx;
                    const int j = ym_match(d, k, lab, m, iou_thresh, &mx);
                    float* o = out + (size_t)r * YM_REC;
                    o[0] = d[6 + k], o[1] = ym_float((unsigned)(image_base + b)), o[2] = ym_float((unsigned)k);
                    o[3] = ym_float((unsigned)(j < 0 ? -1 : truth_base + f0 + j)), o[4] = mx, o[5] = ym_float((unsigned)r);
                    if (j >= 0 && r < claim[j]) claim[j] = r;
                }
                ++r;
            }
        }
        rec_count[b] = r;
        const int R = r < rec_stride ? r : rec_stride;
        int tp = 0, fp = 0;
        for (int t = 0; t < YM_THREADS; ++t) {
            double s = 0.0;
            for (int e = t; e < R; e += YM_THREADS) {
                const float* o = out + (size_t)e * YM_REC;
                if (!(o[0] > thresh_calc)) continue;
                const int truth = (int)ym_bits(o[3]);
                if (truth >= 0 && claim[truth - truth_base - f0] == e) ++tp, s = s + (double)o[4];
                else ++fp;
            }
            lane[t] = s;
        }
        img_stats[(size_t)b * 3] = (double)tp, img_stats[(size_t)b * 3 + 1] = (double)fp, img_stats[(size_t)b * 3 + 2] = ym_block_sum(lane);
    }
}

void map_reduce_host(const float* rec, int D, const int* truth_classes_count, int classes, int truths, const double* img_stats,
                     int N, double* ap, double* stats, double* pr) {
    std::vector<unsigned long long> hi(D), lo(D);
    std::vector<int> rank(D);
    for (int i = 0; i < D; ++i) {
        hi[i] = ym_rank_hi(rec + (size_t)i * YM_REC), lo[i] = ym_rank_lo(rec + (size_t)i * YM_REC, (unsigned)i);
        rank[i] = i;
    }
    std::sort(rank.begin(), rank.end(), [&](int a, int b) { return hi[a] != hi[b] ? hi[a] > hi[b] : lo[a] > lo[b]; });
    std::vector<int> first_claim((size_t)truths + 1, INT_MAX);
    for (int r = 0; r < D; ++r) {
        const int t = (int)ym_bits(rec[(size_t)rank[r] * YM_REC + 3]);
        if (t >= 0 && t < truths && r < first_claim[t]) first_claim[t] = r;
    }
    for (int c = 0; c < classes; ++c) {
        double best[YM_POINTS] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
        int tp = 0, fp = 0;
        for (int r = 0; r < D; ++r) {
            const float* o = rec + (size_t)rank[r] * YM_REC;
            const int t = (int)ym_bits(o[3]);
            if ((int)ym_bits(o[2]) == c) {
                if (t < 0) ++fp;
                else if (t < truths && first_claim[t] == r) ++tp;
            }
            double precision, recall;
            ym_pr(tp, fp, truth_classes_count[c], &precision, &recall);
            ym_points(precision, recall, best);
            if (pr) pr[((size_t)c * D + r) * 2] = precision, pr[((size_t)c * D + r) * 2 + 1] = recall;
        }
        ap[c] = ym_ap(best);
    }
    double tp = 0.0, fp = 0.0, iou = 0.0;
    for (int i = 0; i < N; ++i) tp = tp + img_stats[(size_t)i * 3], fp = fp + img_stats[(size_t)i * 3 + 1], iou = iou + img_stats[(size_t)i * 3 + 2];
    ym_stats(ap, classes, tp, fp, iou, truths, stats);
}

}  // namespace bp
