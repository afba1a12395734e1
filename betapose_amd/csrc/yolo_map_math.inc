// Detector validation (Darknet's `detector map`), the arithmetic of O(1) size: ONE source for the host twins
// (yolo_map_host.cpp) and the device kernels (yolo_map.hip).  One candidate row of get_yolo_detections, the sort key of
// do_nms_sort's per-class qsort, the truth match of one detection record, precision / recall of one rank and the
// reported statistics.  box_iou is yolo_train_math.inc's, included here and not restated.  Host and device compile this
// text without FMA contraction and do the same f32 / f64 / integer operations in the same order; only who loops over
// what differs per side.  Plain C++17, no HIP header.  Included inside `namespace bp { namespace {` after <cmath> and
// <cstdint>, in a unit that has `#pragma clang fp contract(off)` in force.
//
// Conventions (DESIGN.md 3.12): pred is float32 [B][rows][attrs], attrs = 5 + classes, (x, y, w, h) in detector-input
// pixels, row order head, anchor, gy, gx; a detection row is (x, y, w, h, objectness, candidate index as int bits,
// prob[classes]); a record is 6 words (p, image, class, truth, max_iou, position within the image), ints as bits.
#include "yolo_train_math.inc"

constexpr int YM_MAX_HEADS = 8;
constexpr int YM_MAX_DETS = 4096;           // the device's cap on max_dets: keys, boxes and probs of one image live in LDS
constexpr int YM_DET_THREADS = 1024;        // lanes of the block that owns one image in bp_yolo_detections
constexpr int YM_THREADS = 256;             // lanes of every other block; the f64 sums run in their order
constexpr int YM_REC = 6;                   // words of a record
constexpr int YM_SORT_TILE = 2048;          // records one block of the rank sort holds in LDS
constexpr int YM_POINTS = 11;
constexpr int YM_STATS = 8;                 // mAP, precision, recall, F1, average IoU, TP, FP, FN

struct YmHeads {
    int nheads;
    int off[YM_MAX_HEADS + 1];              // first row of each head = first candidate index of it; off[nheads] = rows
    int n[YM_MAX_HEADS], cells[YM_MAX_HEADS];
};

BP_HD unsigned ym_bits(float v) {
    union { float f; unsigned u; } c;
    c.f = v;
    return c.u;
}
BP_HD float ym_float(unsigned u) {
    union { float f; unsigned u; } c;
    c.u = u;
    return c.f;
}

// Darknet's order is head, cell, anchor; the tensor's is head, anchor, cell.  c in [0, rows).
BP_HD int ym_cand_row(const YmHeads& H, int c) {
    int h = 0;
    while (h + 1 < H.nheads && c >= H.off[h + 1]) ++h;
    const int q = c - H.off[h];
    const int cell = q / H.n[h], a = q - cell * H.n[h];
    return H.off[h] + a * H.cells[h] + cell;
}

// one candidate: row `r` of one image's pred -> a detection row of 6 + classes words
BP_HD void ym_det_row(const float* r, int cand, int classes, float net_w, float net_h, float thresh, float* out) {
    const float obj = r[4];
    out[0] = r[0] / net_w, out[1] = r[1] / net_h, out[2] = r[2] / net_w, out[3] = r[3] / net_h;
    out[4] = obj;
    out[5] = ym_float((unsigned)cand);
    for (int k = 0; k < classes; ++k) {
        const float p = obj * r[5 + k];
        out[6 + k] = p > thresh ? p : 0.0f;
    }
}

// The key of one entry in a class pass: descending keys are nms_comparator_v3's order under a stable sort.  prob >= +0
// (its bits grow with its value), pos = where the previous pass left the entry, src = its row in candidate order; a real
// key is never 0, which is what the padding holds.
BP_HD unsigned long long ym_nms_key(float prob, int pos, int src) {
    return ((unsigned long long)ym_bits(prob) << 32) | (1ull << 24) | ((unsigned long long)(YM_MAX_DETS - 1 - pos) << 12) |
           (unsigned long long)src;
}
BP_HD int ym_key_src(unsigned long long key) { return (int)(key & (YM_MAX_DETS - 1)); }

// The two words of a record's rank key: descending (hi, lo) is p descending, then image, position and index ascending
BP_HD unsigned long long ym_rank_hi(const float* rec) {
    return ((unsigned long long)ym_bits(rec[0]) << 32) | (unsigned long long)(0xffffffffu - ym_bits(rec[1]));
}
BP_HD unsigned long long ym_rank_lo(const float* rec, unsigned index) {
    return ((unsigned long long)(0xffffffffu - ym_bits(rec[5])) << 32) | (unsigned long long)(0xffffffffu - index);
}
BP_HD unsigned ym_rank_index(unsigned long long lo) { return 0xffffffffu - (unsigned)(lo & 0xffffffffu); }

// detector.c:704-718 for one (detection, class): the label of class k with the greatest IoU above iou_thresh, the first
// on ties; labels [m][5] = (id, x, y, w, h).  Returns the label's index or -1.
BP_HD int ym_match(const float* det, int k, const float* labels, int m, float iou_thresh, float* max_iou) {
    const YtBox d = {det[0], det[1], det[2], det[3]};
    int best = -1;
    float mx = 0.0f;
    for (int j = 0; j < m; ++j) {
        const float* l = labels + (size_t)j * 5;
        const YtBox t = {l[1], l[2], l[3], l[4]};
        const float iou = yt_box_iou(d, t);
        if (iou > iou_thresh && (float)k == l[0] && iou > mx) mx = iou, best = j;
    }
    *max_iou = mx;
    return best;
}

// a label counts for its class when its id is a whole number in [0, classes)
BP_HD int ym_label_class(float id, int classes) {
    if (!(id >= 0.0f && id < (float)classes)) return -1;
    const int k = (int)id;
    return (float)k == id ? k : -1;
}

// detector.c:825-834
BP_HD void ym_pr(int tp, int fp, int truths, double* precision, double* recall) {
    const int fn = truths - tp;
    *precision = (tp + fp) > 0 ? (double)tp / (double)(tp + fp) : 0.0;
    *recall = (tp + fn) > 0 ? (double)tp / (double)(tp + fn) : 0.0;
}

// best[point] = max(best[point], precision) where recall >= point * 0.1 (the double product, as the reference has it)
BP_HD void ym_points(double precision, double recall, double* best) {
    for (int point = 0; point < YM_POINTS; ++point) {
        const double cur = point * 0.1;
        if (recall >= cur && precision > best[point]) best[point] = precision;
    }
}

BP_HD double ym_ap(const double* best) {
    double avg = 0.0;
    for (int point = 0; point < YM_POINTS; ++point) avg = avg + best[point];
    return avg / 11;
}

// detector.c:774-775, 866-876: tp, fp and iou_sum are the run's totals, truths = unique_truth_count
BP_HD void ym_stats(const double* ap, int classes, double tp, double fp, double iou_sum, long long truths, double* stats) {
    double m = 0.0;
    for (int i = 0; i < classes; ++i) m = m + ap[i];
    const float ftp = (float)tp, ffp = (float)fp, ffn = (float)((double)truths - tp);
    const float precision = ftp / (ftp + ffp);
    const float recall = ftp / (ftp + ffn);
    const float f1 = 2.0f * precision * recall / (precision + recall);
    stats[0] = m / classes;
    stats[1] = (double)precision, stats[2] = (double)recall, stats[3] = (double)f1;
    stats[4] = (tp + fp) > 0.0 ? iou_sum / (tp + fp) : iou_sum;
    stats[5] = tp, stats[6] = fp, stats[7] = (double)truths - tp;
}
