// Detector validation on the device (include/betapose_hip.h bp_yolo_detections, bp_detector_map_match,
// bp_detector_map_reduce).  The arithmetic of one candidate row, one truth match, one rank's precision / recall and the
// reported statistics is yolo_map_math.inc, the text the host twins (yolo_map_host.cpp) compile too; here is who loops over what:
//   ym_dets_kernel     one block of 1 024 lanes per image.  Compaction: the lanes walk the candidate indices in Darknet's
//                      order (head, cell, anchor; the row comes from the head table by 32-bit division), a wave ballot and
//                      the waves' counts in LDS give every candidate its place, so the list order never depends on timing.
//                      Per class: a bitonic sort in LDS on a 64-bit key (prob bits, previous position, source row), then
//                      the greedy sweep with the sorted boxes and probs in LDS (28 bytes per entry of max_dets rounded up to a
//                      power of two: 28 KB at the default 1 024, 112 KB at the cap): a live entry is compared with every later
//                      one by all lanes, one barrier per live entry, none for a suppressed one.
//   ym_match_kernel    one block per image: a lane per (detection, class) pair, ballot + prefix again for the record's
//                      place, the first claimant of a label by an integer minimum, tp / fp by integer adds in LDS, the
//                      IoU sum in f64 by lane, wave tree and waves in order.
//   ym_rank_*          the sort of all records: keys (p, image, position, index), a bitonic sort whose steps below
//                      YM_SORT_TILE run in LDS and whose wider steps are one launch each.
//   ym_claim_kernel    the first rank that claims each truth: an integer minimum.
//   ym_pr_kernel       one block per class: running tp / fp over the ranks by ballot + prefix, precision and recall per
//                      rank, the 11 maxima per lane and then over the block (a maximum has no order).
//   ym_final_kernel    the images' (tp, fp, IoU sum) added in index order, mAP and the reported statistics.
// No floating-point atomics; integer minima and adds only, whose results have no order.  Every index into pred is below
// B * rows * attrs, every detection and stage row below max_dets, every record below rec_stride or D, every label
// index inside the clamped slice of its image, every truth below `truths` before it indexes the claim array.
#include "bp_common.h"
#include "yolo_map.h"

#pragma clang fp contract(off)

namespace bp {

namespace {

#include "yolo_map_math.inc"

constexpr int YM_DET_WAVES = YM_DET_THREADS / YT_WAVE;

// place of this lane's flagged item among the block's, in lane order; *total = the block's count.  All lanes call it.
template <int WAVES>
__device__ __forceinline__ int ym_block_place(bool flag, int* w_cnt, int* total) {
    const unsigned long long m = __ballot(flag);
    const int lane = threadIdx.x & (YT_WAVE - 1), wave = threadIdx.x / YT_WAVE;
    const int before = __popcll(m & ((1ull << lane) - 1ull));
    __syncthreads();                            // (the previous round's readers are done with w_cnt)
    if (lane == 0) w_cnt[wave] = __popcll(m);
    __syncthreads();
    int off = 0, all = 0;
    for (int w = 0; w < WAVES; ++w) {
        const int c = w_cnt[w];
        off += w < wave ? c : 0;
        all += c;
    }
    *total = all;
    return off + before;
}

// descending bitonic sort of P (a power of two) keys in LDS by the whole block
__device__ __forceinline__ void ym_bitonic_desc(unsigned long long* key, int P, int threads) {
    for (int k = 2; k <= P; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            __syncthreads();
            for (int t = threadIdx.x; t < P / 2; t += threads) {
                const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1)), l = i | j;
                const unsigned long long a = key[i], b = key[l];
                const bool up = (i & k) != 0;   // this run ascends
                if (up ? a > b : a < b) key[i] = b, key[l] = a;
            }
        }
    __syncthreads();
}

__global__ __launch_bounds__(YM_DET_THREADS) void ym_dets_kernel(const float* __restrict__ pred, int rows, YmHeads H, float net_w,
                                                                 float net_h, int classes, float thresh, float nms, int max_dets, int cap,
                                                                 float* stage_all, float* __restrict__ dets_all,
                                                                 int* __restrict__ count) {
    extern __shared__ __align__(16) unsigned char ym_lds[];    // cap = max_dets rounded up to a power of two: 28 bytes each
    float4* box = reinterpret_cast<float4*>(ym_lds);
    unsigned long long* key = reinterpret_cast<unsigned long long*>(box + cap);
    float* prob = reinterpret_cast<float*>(key + cap);
    __shared__ int w_cnt[YM_DET_WAVES];
    const int b = blockIdx.x, attrs = 5 + classes, S = 6 + classes;
    const float* p = pred + (size_t)b * rows * attrs;
    float* stage = stage_all + (size_t)b * max_dets * S;
    float* dets = dets_all + (size_t)b * max_dets * S;

    // 1. candidates, in candidate-index order
    int n = 0;
    for (int base = 0; base < rows; base += YM_DET_THREADS) {
        const int c = base + threadIdx.x;
        const float* r = nullptr;
        bool flag = false;
        if (c < rows) {
            r = p + (size_t)ym_cand_row(H, c) * attrs;
            flag = r[4] > thresh;
        }
        int total;
        const int pos = n + ym_block_place<YM_DET_WAVES>(flag, w_cnt, &total);
        if (flag && pos < max_dets) ym_det_row(r, c, classes, net_w, net_h, thresh, stage + (size_t)pos * S);
        n += total;
    }
    if (threadIdx.x == 0) count[b] = n;
    const int kept = n > max_dets ? 0 : n;      // an overflowing image is reported by its count; its block is zero
    for (int e = kept * S + threadIdx.x; e < max_dets * S; e += YM_DET_THREADS) dets[e] = 0.0f;
    if (kept == 0) return;
    __syncthreads();                            // the stage rows are written

    // 2. per class: sort, sweep
    int P = 2;
    while (P < kept) P <<= 1;
    const bool sorted = nms > 0.0f;
    for (int k = 0; sorted && k < classes; ++k) {
        for (int i = threadIdx.x; i < P; i += YM_DET_THREADS) {
            unsigned long long v = 0ull;
            if (i < kept) {
                const int src = k == 0 ? i : ym_key_src(key[i]);
                v = ym_nms_key(stage[(size_t)src * S + 6 + k], i, src);
            }
            key[i] = v;                         // (a lane reads and writes its own entries only)
        }
        ym_bitonic_desc(key, P, YM_DET_THREADS);
        for (int i = threadIdx.x; i < kept; i += YM_DET_THREADS) {
            const float* d = stage + (size_t)ym_key_src(key[i]) * S;
            box[i] = make_float4(d[0], d[1], d[2], d[3]);
            prob[i] = ym_float((unsigned)(key[i] >> 32));
        }
        __syncthreads();
        for (int i = 0; i + 1 < kept; ++i) {
            if (prob[i] == 0.0f) continue;      // the same value on every lane: written before the last barrier
            const float4 a4 = box[i];
            const YtBox a = {a4.x, a4.y, a4.z, a4.w};
            for (int j = i + 1 + threadIdx.x; j < kept; j += YM_DET_THREADS) {
                if (prob[j] == 0.0f) continue;
                const float4 c4 = box[j];
                const YtBox c = {c4.x, c4.y, c4.z, c4.w};
                if (yt_box_iou(a, c) > nms) prob[j] = 0.0f;
            }
            __syncthreads();
        }
        for (int i = threadIdx.x; i < kept; i += YM_DET_THREADS) stage[(size_t)ym_key_src(key[i]) * S + 6 + k] = prob[i];
        __syncthreads();                        // the next pass reads other lanes' stage entries
    }

    // 3. the rows, in the order the last pass left
    for (int e = threadIdx.x; e < kept * S; e += YM_DET_THREADS) {
        const int i = e / S, f = e - i * S;
        const int src = sorted ? ym_key_src(key[i]) : i;
        dets[e] = stage[(size_t)src * S + f];
    }
}

// the sum of one value per lane of a YM_THREADS block, in the order yolo_map_host.cpp ym_block_sum fixes; valid on thread 0
__device__ __forceinline__ double ym_block_sum(double v, double* w_sum) {
    for (int o = YT_WAVE / 2; o > 0; o >>= 1) v = v + __shfl_down(v, o, YT_WAVE);
    if ((threadIdx.x & (YT_WAVE - 1)) == 0) w_sum[threadIdx.x / YT_WAVE] = v;
    __syncthreads();
    double t = w_sum[0];
    for (int w = 1; w < YM_THREADS / YT_WAVE; ++w) t = t + w_sum[w];
    return t;
}

__global__ __launch_bounds__(YM_THREADS) void ym_match_kernel(const float* __restrict__ dets_all, const int* __restrict__ count,
                                                              int max_dets, int classes, const float* __restrict__ labels, int M,
                                                              const int* __restrict__ first, float iou_thresh, float thresh_calc,
                                                              int truth_base, int image_base, int rec_stride, float* rec_all,
                                                              int* __restrict__ rec_count, int* truth_classes_count,
                                                              double* __restrict__ img_stats, int* claim) {
    __shared__ int w_cnt[YM_THREADS / YT_WAVE];
    __shared__ double w_sum[YM_THREADS / YT_WAVE];
    __shared__ int s_tp, s_fp;
    const int b = blockIdx.x, S = 6 + classes;
    int f0 = first[b], f1 = first[b + 1];
    f0 = f0 < 0 ? 0 : (f0 > M ? M : f0);        // a slice always lies inside labels and claim
    f1 = f1 < f0 ? f0 : (f1 > M ? M : f1);
    const int m = f1 - f0;
    const float* lab = labels + (size_t)f0 * 5;
    if (threadIdx.x == 0) s_tp = 0, s_fp = 0;
    for (int j = threadIdx.x; j < m; j += YM_THREADS) {
        const int k = ym_label_class(lab[(size_t)j * 5], classes);
        if (k >= 0) atomicAdd(truth_classes_count + k, 1);
    }
    const int cnt = count[b];
    const int n = cnt > max_dets || cnt < 0 ? 0 : cnt;
    const float* dets = dets_all + (size_t)b * max_dets * S;
    float* rec = rec_all + (size_t)b * rec_stride * YM_REC;

    const int pairs = n * classes;              // <= 2^31 / 6 (checked by the caller)
    int r0 = 0;
    for (int base = 0; base < pairs; base += YM_THREADS) {
        const int e = base + threadIdx.x;
        int i = 0, k = 0;
        bool flag = false;
        if (e < pairs) {
            i = e / classes, k = e - i * classes;
            flag = dets[(size_t)i * S + 6 + k] > 0.0f;
        }
        int total;
        const int r = r0 + ym_block_place<YM_THREADS / YT_WAVE>(flag, w_cnt, &total);
        if (flag && r < rec_stride) {
            const float* d = dets + (size_t)i * S;
            float mx;
            const int j = ym_match(d, k, lab, m, iou_thresh, &mx);
            float* o = rec + (size_t)r * YM_REC;
            o[0] = d[6 + k], o[1] = ym_float((unsigned)(image_base + b)), o[2] = ym_float((unsigned)k);
            o[3] = ym_float((unsigned)(j < 0 ? -1 : truth_base + f0 + j)), o[4] = mx, o[5] = ym_float((unsigned)r);
            if (j >= 0) atomicMin(claim + f0 + j, r);
        }
        r0 += total;
    }
    if (threadIdx.x == 0) rec_count[b] = r0;
    const int R = r0 < rec_stride ? r0 : rec_stride;
    for (int e = R * YM_REC + threadIdx.x; e < rec_stride * YM_REC; e += YM_THREADS) rec[e] = 0.0f;
    __threadfence();
    __syncthreads();                            // records and claims of this image are complete

    int tp = 0, fp = 0;
    double s = 0.0;
    for (int e = threadIdx.x; e < R; e += YM_THREADS) {
        const float* o = rec + (size_t)e * YM_REC;
        if (!(o[0] > thresh_calc)) continue;
        const int truth = (int)ym_bits(o[3]);
        if (truth >= 0 && __hip_atomic_load(claim + (truth - truth_base), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == e)
            ++tp, s = s + (double)o[4];
        else
            ++fp;
    }
    if (tp) atomicAdd(&s_tp, tp);
    if (fp) atomicAdd(&s_fp, fp);
    const double sum = ym_block_sum(s, w_sum);  // (its barrier also completes the two counts)
    if (threadIdx.x == 0) img_stats[(size_t)b * 3] = (double)s_tp, img_stats[(size_t)b * 3 + 1] = (double)s_fp, img_stats[(size_t)b * 3 + 2] = sum;
}

// ---------------------------------------------------------------------------------------------------- ranks
struct YmKey {
    unsigned long long hi, lo;
};
__device__ __forceinline__ bool ym_key_less(const YmKey& a, const YmKey& b) { return a.hi != b.hi ? a.hi < b.hi : a.lo < b.lo; }

__global__ __launch_bounds__(YM_THREADS) void ym_rank_keys_kernel(const float* __restrict__ rec, int D, int P,
                                                                  unsigned long long* __restrict__ hi, unsigned long long* __restrict__ lo) {
    const int i = blockIdx.x * YM_THREADS + threadIdx.x;
    if (i >= P) return;
    hi[i] = i < D ? ym_rank_hi(rec + (size_t)i * YM_REC) : 0ull;
    lo[i] = i < D ? ym_rank_lo(rec + (size_t)i * YM_REC, (unsigned)i) : 0ull;
}

// the steps j = j0, j0 / 2, .. 1 of stage k on one tile of YM_SORT_TILE keys in LDS; full: every stage k = 2 .. tile
__global__ __launch_bounds__(YM_DET_THREADS) void ym_rank_tile_kernel(unsigned long long* __restrict__ hi, unsigned long long* __restrict__ lo,
                                                                      int k_only, int full) {
    __shared__ YmKey key[YM_SORT_TILE];
    const int base = blockIdx.x * YM_SORT_TILE;
    for (int i = threadIdx.x; i < YM_SORT_TILE; i += YM_DET_THREADS) key[i] = {hi[base + i], lo[base + i]};
    for (int k = full ? 2 : k_only; k <= (full ? YM_SORT_TILE : k_only); k <<= 1) {
        for (int j = (k >> 1) < YM_SORT_TILE ? (k >> 1) : YM_SORT_TILE >> 1; j > 0; j >>= 1) {
            __syncthreads();
            const int t = threadIdx.x;          // YM_SORT_TILE / 2 pairs, one per lane
            const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1)), l = i | j;
            const YmKey a = key[i], c = key[l];
            const bool up = ((base + i) & k) != 0;
            if (up ? ym_key_less(c, a) : ym_key_less(a, c)) key[i] = c, key[l] = a;
        }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < YM_SORT_TILE; i += YM_DET_THREADS) hi[base + i] = key[i].hi, lo[base + i] = key[i].lo;
}

// one step (k, j) with j >= YM_SORT_TILE over all P / 2 pairs
__global__ __launch_bounds__(YM_THREADS) void ym_rank_step_kernel(unsigned long long* __restrict__ hi, unsigned long long* __restrict__ lo,
                                                                  int P, int k, int j) {
    const int t = blockIdx.x * YM_THREADS + threadIdx.x;
    if (t >= P / 2) return;
    const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1)), l = i | j;
    const YmKey a = {hi[i], lo[i]}, c = {hi[l], lo[l]};
    const bool up = (i & k) != 0;
    if (up ? ym_key_less(c, a) : ym_key_less(a, c)) hi[i] = c.hi, lo[i] = c.lo, hi[l] = a.hi, lo[l] = a.lo;
}

__global__ __launch_bounds__(YM_THREADS) void ym_fill_kernel(int* __restrict__ p, int n, int v) {
    const int i = blockIdx.x * YM_THREADS + threadIdx.x;
    if (i < n) p[i] = v;
}

__global__ __launch_bounds__(YM_THREADS) void ym_claim_kernel(const float* __restrict__ rec, const unsigned long long* __restrict__ lo,
                                                              int D, int truths, int* first_claim) {
    const int r = blockIdx.x * YM_THREADS + threadIdx.x;
    if (r >= D) return;
    const unsigned idx = ym_rank_index(lo[r]);
    if (idx >= (unsigned)D) return;
    const int t = (int)ym_bits(rec[(size_t)idx * YM_REC + 3]);
    if (t >= 0 && t < truths) atomicMin(first_claim + t, r);
}

__global__ __launch_bounds__(YM_THREADS) void ym_pr_kernel(const float* __restrict__ rec, const unsigned long long* __restrict__ lo, int D,
                                                           int truths, const int* __restrict__ first_claim,
                                                           const int* __restrict__ truth_classes_count, double* __restrict__ ap,
                                                           double* __restrict__ pr) {
    __shared__ int w_cnt[YM_THREADS / YT_WAVE];
    __shared__ double s_best[YM_THREADS / YT_WAVE][YM_POINTS];
    const int c = blockIdx.x;
    const int tcc = truth_classes_count[c];
    double best[YM_POINTS];
    for (int q = 0; q < YM_POINTS; ++q) best[q] = 0.0;
    int tp0 = 0, fp0 = 0;
    for (int base = 0; base < D; base += YM_THREADS) {
        const int r = base + threadIdx.x;
        bool is_tp = false, is_fp = false;
        if (r < D) {
            const unsigned idx = ym_rank_index(lo[r]);
            if (idx < (unsigned)D) {
                const float* o = rec + (size_t)idx * YM_REC;
                const int t = (int)ym_bits(o[3]);
                if ((int)ym_bits(o[2]) == c) {
                    if (t < 0) is_fp = true;
                    else if (t < truths && first_claim[t] == r) is_tp = true;
                }
            }
        }
        int tot_tp, tot_fp;
        const int tp = tp0 + ym_block_place<YM_THREADS / YT_WAVE>(is_tp, w_cnt, &tot_tp) + (is_tp ? 1 : 0);    // inclusive
        const int fp = fp0 + ym_block_place<YM_THREADS / YT_WAVE>(is_fp, w_cnt, &tot_fp) + (is_fp ? 1 : 0);
        if (r < D) {
            double precision, recall;
            ym_pr(tp, fp, tcc, &precision, &recall);
            ym_points(precision, recall, best);
            if (pr) pr[((size_t)c * D + r) * 2] = precision, pr[((size_t)c * D + r) * 2 + 1] = recall;
        }
        tp0 += tot_tp, fp0 += tot_fp;
    }
    for (int q = 0; q < YM_POINTS; ++q) {
        double v = best[q];
        for (int o = YT_WAVE / 2; o > 0; o >>= 1) {
            const double w = __shfl_down(v, o, YT_WAVE);
            v = w > v ? w : v;
        }
        if ((threadIdx.x & (YT_WAVE - 1)) == 0) s_best[threadIdx.x / YT_WAVE][q] = v;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int q = 0; q < YM_POINTS; ++q) {
            double v = s_best[0][q];
            for (int w = 1; w < YM_THREADS / YT_WAVE; ++w) v = s_best[w][q] > v ? s_best[w][q] : v;
            best[q] = v;
        }
        ap[c] = ym_ap(best);
    }
}

__global__ __launch_bounds__(YM_THREADS) void ym_final_kernel(const double* ap, int classes, int truths, const double* __restrict__ img_stats,
                                                              int N, double* __restrict__ stats) {
    __shared__ double tile[YM_THREADS * 3];
    double tp = 0.0, fp = 0.0, iou = 0.0;
    for (int base = 0; base < N; base += YM_THREADS) {
        const int cnt = N - base < YM_THREADS ? N - base : YM_THREADS;
        for (int i = threadIdx.x; i < cnt * 3; i += YM_THREADS) tile[i] = img_stats[(size_t)base * 3 + i];
        __syncthreads();
        if (threadIdx.x == 0)
            for (int i = 0; i < cnt; ++i) tp = tp + tile[i * 3], fp = fp + tile[i * 3 + 1], iou = iou + tile[i * 3 + 2];
        __syncthreads();
    }
    if (threadIdx.x == 0) ym_stats(ap, classes, tp, fp, iou, truths, stats);
}

inline unsigned ym_blocks(long long n) { return (unsigned)((n + YM_THREADS - 1) / YM_THREADS); }

}  // namespace

void launch_yolo_detections(const float* pred, int B, int rows, const int* heads, int nheads, int net_w, int net_h, int classes,
                            float thresh, float nms, int max_dets, float* dets, int* count, void* scratch, hipStream_t s) {
    YmHeads H = {};
    H.nheads = nheads;
    for (int h = 0; h < nheads; ++h) {
        H.off[h] = heads[h * 4], H.n[h] = heads[h * 4 + 1], H.cells[h] = heads[h * 4 + 2] * heads[h * 4 + 3];
        H.off[h + 1] = H.off[h] + H.n[h] * H.cells[h];
    }
    int cap = 2;
    while (cap < max_dets) cap <<= 1;           // <= YM_MAX_DETS (checked by the caller)
    const size_t lds = (size_t)cap * (sizeof(float4) + sizeof(unsigned long long) + sizeof(float));
    if (lds > 64 * 1024) allow_big_lds(reinterpret_cast<const void*>(ym_dets_kernel));
    hipLaunchKernelGGL(ym_dets_kernel, dim3(B), dim3(YM_DET_THREADS), lds, s, pred, rows, H, (float)net_w, (float)net_h, classes,
                       thresh, nms, max_dets, cap, (float*)scratch, dets, count);
}

void launch_map_match(const float* dets, const int* count, int B, int max_dets, int classes, const float* labels, int M,
                      const int* first, float iou_thresh, float thresh_calc, int truth_base, int image_base, int rec_stride,
                      float* rec, int* rec_count, int* truth_classes_count, double* img_stats, int* claim, hipStream_t s) {
    hipLaunchKernelGGL(ym_fill_kernel, dim3(ym_blocks(M + 1)), dim3(YM_THREADS), 0, s, claim, M + 1, 0x7fffffff);
    hipLaunchKernelGGL(ym_match_kernel, dim3(B), dim3(YM_THREADS), 0, s, dets, count, max_dets, classes, labels, M, first, iou_thresh,
                       thresh_calc, truth_base, image_base, rec_stride, rec, rec_count, truth_classes_count, img_stats, claim);
}

void launch_map_reduce(const float* rec, int D, const int* truth_classes_count, int classes, int truths, const double* img_stats,
                       int N, double* ap, double* stats, double* pr, void* scratch, hipStream_t s) {
    int P = YM_SORT_TILE;
    while (P < D) P *= 2;
    unsigned long long* hi = (unsigned long long*)scratch;
    unsigned long long* lo = hi + P;
    int* first_claim = (int*)(lo + P);
    if (D > 0) {
        hipLaunchKernelGGL(ym_rank_keys_kernel, dim3(ym_blocks(P)), dim3(YM_THREADS), 0, s, rec, D, P, hi, lo);
        hipLaunchKernelGGL(ym_rank_tile_kernel, dim3(P / YM_SORT_TILE), dim3(YM_DET_THREADS), 0, s, hi, lo, 0, 1);
        for (int k = YM_SORT_TILE * 2; k <= P; k *= 2) {
            for (int j = k / 2; j >= YM_SORT_TILE; j /= 2)
                hipLaunchKernelGGL(ym_rank_step_kernel, dim3(ym_blocks(P / 2)), dim3(YM_THREADS), 0, s, hi, lo, P, k, j);
            hipLaunchKernelGGL(ym_rank_tile_kernel, dim3(P / YM_SORT_TILE), dim3(YM_DET_THREADS), 0, s, hi, lo, k, 0);
        }
        hipLaunchKernelGGL(ym_fill_kernel, dim3(ym_blocks(truths + 1)), dim3(YM_THREADS), 0, s, first_claim, truths + 1, 0x7fffffff);
        hipLaunchKernelGGL(ym_claim_kernel, dim3(ym_blocks(D)), dim3(YM_THREADS), 0, s, rec, lo, D, truths, first_claim);
    }
    hipLaunchKernelGGL(ym_pr_kernel, dim3(classes), dim3(YM_THREADS), 0, s, rec, lo, D, truths, first_claim, truth_classes_count, ap, pr);
    hipLaunchKernelGGL(ym_final_kernel, dim3(1), dim3(YM_THREADS), 0, s, ap, classes, truths, img_stats, N, stats);
}

}  // namespace bp
