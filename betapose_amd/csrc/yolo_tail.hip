// The detector's tail (gfx950): everything between the YOLO head tensors and the select records the per-frame chains read.
// Three things vary, and each is stated once:
//   row source      PredRows (the decoded [rows][attrs] tensor) or HeadRows (the head tensors, decoded on the fly with
//                   yolo_decode_kernel's float operations, so both write identical records)
//   selection rule  select_classes (write_results with nms=False: per class slot the arg-max objectness row) or
//                   select_nms (its NMS branch live: up to C survivors of one class)
//   slot count S    of select_classes: 1 with the list {0} is the single select of the per-frame pipeline,
//                   BP_MAX_SCENE_CLASSES serves the shared detector
// A kernel is one instantiation of rule<source[, S]>; a launcher picks the source from its YoloRowSource.
#include "bp_common.h"

namespace bp {

// ---------------------------------------------------------------- row sources: launch arguments, and the rows of one image
__device__ __forceinline__ float sigmoidf_(float x) { return 1.f / (1.f + expf(-x)); }

struct PredRows {
    const float* P;   // this image's [rows][attrs]
    int attrs;
    __device__ __forceinline__ const float* row(int r) const { return P + (long long)r * attrs; }
    __device__ __forceinline__ float attr(const float* q, int k) const { return q[k]; }   // k >= 4: objectness, class scores
    __device__ __forceinline__ void box(int, const float* q, float* b) const { b[0] = q[0]; b[1] = q[1]; b[2] = q[2]; b[3] = q[3]; }
};
struct YoloPred {
    const float* pred;   // [N][rows][attrs]
    int rows, attrs;
    __device__ __forceinline__ PredRows image(int n) const { return {pred + (long long)n * rows * attrs, attrs}; }
};

struct YoloHeads;
struct HeadRows {   // DetectionLayer.forward (yolo/darknet.py:129-169) on one row at a time
    const YoloHeads* hs;
    int n;
    struct Addr {
        const YoloHead* H;
        const float* t;   // the row's attrs raw head values
        int a, gx, gy;
        float stride;
    };
    __device__ __forceinline__ Addr addr(int r) const;
    __device__ __forceinline__ const float* row(int r) const { return addr(r).t; }
    __device__ __forceinline__ float attr(const float* t, int k) const { return sigmoidf_(t[k]); }
    __device__ __forceinline__ void box(int r, const float* t, float* b) const { box(addr(r), t, b); }
    __device__ __forceinline__ void box(const Addr& A, const float* t, float* b) const {
        // anchors are divided by the stride then the box is multiplied back (darknet.py:151,165)
        b[0] = (sigmoidf_(t[0]) + (float)A.gx) * A.stride;
        b[1] = (sigmoidf_(t[1]) + (float)A.gy) * A.stride;
        b[2] = (expf(t[2]) * (A.H->aw[A.a] / A.stride)) * A.stride;
        b[3] = (expf(t[3]) * (A.H->ah[A.a] / A.stride)) * A.stride;
    }
};
struct YoloHeads {
    YoloHead h[4];
    int n, rows, attrs, reso;
    __device__ __forceinline__ HeadRows image(int img) const { return {this, img}; }
};
// row -> head -> anchor -> gy -> gx (the row order of the [rows][attrs] tensor)
__device__ __forceinline__ HeadRows::Addr HeadRows::addr(int r) const {
    int hi = 0;
    for (int k = 1; k < hs->n; ++k)
        if (r >= hs->h[k].row_off) hi = k;
    Addr A;
    A.H = &hs->h[hi];
    const int g = A.H->g, rr = r - A.H->row_off;
    A.a = rr / (g * g);
    const int cell = rr - A.a * g * g;
    A.gy = cell / g;
    A.gx = cell - A.gy * g;
    A.stride = (float)(hs->reso / g);
    A.t = A.H->t + ((long long)n * g * g + cell) * (3 * hs->attrs) + A.a * hs->attrs;
    return A;
}

static YoloHeads pack_heads(const YoloRowSource& src) {
    BP_CHECK(src.heads && src.nheads <= 4, "at most 4 yolo heads");
    YoloHeads hs;
    hs.n = src.nheads; hs.rows = src.rows; hs.attrs = src.attrs; hs.reso = src.reso;
    for (int i = 0; i < src.nheads; ++i) hs.h[i] = src.heads[i];
    return hs;
}
// f(the source's launch argument): YoloPred when the tensor is there, YoloHeads otherwise
template <class F>
static void with_source(const YoloRowSource& src, F f) {
    if (src.pred) f(YoloPred{src.pred, src.rows, src.attrs});
    else f(pack_heads(src));
}

// ---------------------------------------------------------------- decode: the [rows][attrs] tensor from the heads
__global__ void yolo_decode_kernel(YoloHeads hs, int N, float* __restrict__ pred) {
    const long long total = (long long)N * hs.rows;
    // 32-bit index math: every tensor on this path has < 2^31 elements (checked by the launchers), and 64-bit
    // div/mod costs ~100 instructions on gfx950
    for (int e = blockIdx.x * blockDim.x + threadIdx.x; e < (int)total; e += gridDim.x * blockDim.x) {
        const int row = (int)(e % hs.rows);
        const HeadRows src = hs.image((int)(e / hs.rows));
        const HeadRows::Addr A = src.addr(row);
        float* o = pred + e * hs.attrs;
        src.box(A, A.t, o);
        for (int k = 4; k < hs.attrs; ++k) o[k] = src.attr(A.t, k);
    }
}
void launch_yolo_decode(const YoloRowSource& src, int N, float* pred, hipStream_t s) {
    hipLaunchKernelGGL(yolo_decode_kernel, dim3(grid_for((long long)N * src.rows)), dim3(256), 0, s, pack_heads(src), N, pred);
}

// ---------------------------------------------------------------- what the selection rules share
// class arg-max over the masked row (first max wins)
template <class Rows>
__device__ __forceinline__ int first_max_class(const Rows& src, const float* q, int ncls) {
    int cls = 0;
    float cm = src.attr(q, 5);
    for (int k = 1; k < ncls; ++k) {
        const float v = src.attr(q, 5 + k);
        if (v > cm) { cm = v; cls = k; }
    }
    return cls;
}
// (ov, oi) replaces (v, i) when its objectness is higher, or equal with the lower row: the first maximum in row order
__device__ __forceinline__ void take_better(float& v, int& i, float ov, int oi) {
    if (ov > v || (ov == v && oi < i)) { v = ov; i = oi; }
}
// lane 0 of each wave ends with the wave's first maximum (64-lane shuffles) ...
__device__ __forceinline__ void wave_first_max(float& v, int& i) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const float ov = __shfl_down(v, off, 64);
        const int oi = __shfl_down(i, off, 64);
        take_better(v, i, ov, oi);
    }
}
// ... and the block's is the first maximum of the waves' partials in LDS
__device__ __forceinline__ void combine_partials(const float* sv, const int* si, int waves, float& v, int& i) {
    v = sv[0];
    i = si[0];
    for (int k = 1; k < waves; ++k) take_better(v, i, sv[k], si[k]);
}
// the select record: row (int bits), corners x1 y1 x2 y2, objectness, class score, class id; row -1 and zeros = no detection
__device__ __forceinline__ void write_empty(float* o) {
    o[0] = __int_as_float(-1);
    for (int k = 1; k < 8; ++k) o[k] = 0.f;
}
__device__ __forceinline__ void to_corners(const float* x, float* c) {   // centre, size -> corners
#pragma clang fp contract(off)   // (select_nms: bit-identical to an f32 host restatement)
    c[0] = x[0] - x[2] / 2;
    c[1] = x[1] - x[3] / 2;
    c[2] = x[0] + x[2] / 2;
    c[3] = x[1] + x[3] / 2;
}
__device__ __forceinline__ void write_record(float* o, int row, const float* c, float obj, float score, int id) {
    o[0] = __int_as_float(row);
    o[1] = c[0]; o[2] = c[1]; o[3] = c[2]; o[4] = c[3];
    o[5] = obj;
    o[6] = score;
    o[7] = (float)id;
}

// ---------------------------------------------------------------- select per class slot
// write_results with nms=False (yolo/util.py:118-223), its class filter generalised: a row with objectness > conf competes
// for the slot of the class list that holds its arg-max class, and per slot the arg-max objectness row wins (first on
// ties).  ONE pass over the rows, one block per image: every thread keeps a (objectness, row) pair per slot in registers
// (constant indices: the slot loops are unrolled, S is the register budget), the slots are reduced wave by wave with
// shuffles and across waves through LDS, and thread k writes slot k's record.  No atomics: the reduction order is fixed.
template <int S, class Rows>
__device__ __forceinline__ void select_classes(const Rows& src, int rows, float conf, int ncls, const YoloClassList& cl,
                                               float* __restrict__ out, int ld_slot) {
    __shared__ float sv[S][16];
    __shared__ int si[S][16];
    float best[S];
    int bi[S];
#pragma unroll
    for (int k = 0; k < S; ++k) { best[k] = -1.f; bi[k] = 0x7fffffff; }
    for (int r = threadIdx.x; r < rows; r += blockDim.x) {
        const float* q = src.row(r);
        const float obj = src.attr(q, 4);
        if (!(obj > conf)) continue;
        const int cls = first_max_class(src, q, ncls);
#pragma unroll
        for (int k = 0; k < S; ++k)
            if (k < cl.n && cl.id[k] == cls) take_better(best[k], bi[k], obj, r);
    }
    const int w = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < S; ++k) {
        if (k < cl.n) {   // uniform
            wave_first_max(best[k], bi[k]);
            if ((threadIdx.x & 63) == 0) { sv[k][w] = best[k]; si[k][w] = bi[k]; }
        }
    }
    __syncthreads();
    if ((int)threadIdx.x < cl.n) {
        const int k = threadIdx.x;
        int id = 0;
#pragma unroll
        for (int j = 0; j < S; ++j)
            if (j == k) id = cl.id[j];
        float b;
        int i;
        combine_partials(sv[k], si[k], blockDim.x >> 6, b, i);
        float* o = out + (long long)k * ld_slot;
        if (b < 0.f) {
            write_empty(o);
        } else {
            const float* q = src.row(i);
            float x[4], c[4];
            src.box(i, q, x);
            to_corners(x, c);
            write_record(o, i, c, src.attr(q, 4), src.attr(q, 5 + id), id);
        }
    }
}
template <class Src, int S>
__global__ __launch_bounds__(1024) void yolo_select_classes_kernel(Src src, float conf, int num_classes, YoloClassList cl,
                                                                    float* __restrict__ sel, int ld_image, int ld_slot) {
    select_classes<S>(src.image(blockIdx.x), src.rows, conf, min(num_classes, src.attrs - 5), cl, sel + (long long)blockIdx.x * ld_image,
                      ld_slot);
}
YoloClassList make_class_list(const int* class_ids, int K, int num_classes, int attrs) {
    BP_CHECK(K >= 1 && K <= BP_MAX_SCENE_CLASSES, "class list: 1 to 16 class ids (BP_MAX_SCENE_CLASSES)");
    BP_CHECK(class_ids, "class list: null class ids");
    const int ncls = num_classes < attrs - 5 ? num_classes : attrs - 5;
    YoloClassList cl{};
    cl.n = K;
    for (int k = 0; k < K; ++k) {
        if (class_ids[k] < 0 || class_ids[k] >= ncls)
            throw Error("class list: class id " + std::to_string(class_ids[k]) + " is not below the detector's class count " + std::to_string(ncls));
        for (int j = 0; j < k; ++j)
            if (class_ids[j] == class_ids[k]) throw Error("class list: duplicate class id " + std::to_string(class_ids[k]));
        cl.id[k] = class_ids[k];
    }
    return cl;
}
template <int S>
static void launch_select_slots(const YoloRowSource& src, int N, float conf, int num_classes, const YoloClassList& cl, float* sel,
                                hipStream_t s, int ld_image, int ld_slot) {
    with_source(src, [&](auto arg) {
        hipLaunchKernelGGL(HIP_KERNEL_NAME(yolo_select_classes_kernel<decltype(arg), S>), dim3(N), dim3(1024), 0, s, arg, conf, num_classes,
                           cl, sel, ld_image, ld_slot);
    });
}
void launch_yolo_select_classes(const YoloRowSource& src, int N, float conf, int num_classes, const YoloClassList& cl, float* sel,
                                hipStream_t s, int ld_image, int ld_slot) {
    launch_select_slots<BP_MAX_SCENE_CLASSES>(src, N, conf, num_classes, cl, sel, s, ld_image, ld_slot);
}
// the single select: only rows whose arg-max class is 0 are kept, [6] = the score of class 0, [7] = 0
void launch_yolo_select(const YoloRowSource& src, int N, float conf, int num_classes, float* sel, hipStream_t s, int sel_ld) {
    YoloClassList cl{};
    cl.n = 1;
    launch_select_slots<1>(src, N, conf, num_classes, cl, sel, s, sel_ld, sel_ld);
}

// ---------------------------------------------------------------- select with box NMS (candidate boxes per frame)
// write_results with its NMS branch live and the final arg-max removed (yolo/util.py:176-196, bbox_iou yolo/bbox.py:51-77):
// the rows with objectness > conf whose first-max class is class_id, visited by descending objectness (lower row on ties);
// each visited survivor is kept and removes every later row whose IoU with it is NOT < nms_conf (a NaN IoU removes); stop
// after C <= BP_MAX_CANDIDATES survivors.  IoU in f32 on corner boxes in detector-input pixels, with the reference's + 1 on
// widths and heights.  dynamic_write_results' second pass at nms_conf - 0.05 when more than 100 boxes survive is not
// reproduced: at most 8 survivors are ever kept, so it is moot.
// One block of 1 024 threads per image: a thread owns rows tid, tid + 1024, ... (at most NMS_RPT; 11 at 10 647 rows), their
// liveness as a bit mask and their corners in registers.  C rounds of: block arg-max over the live rows (wave shuffles, 16
// partials through LDS), the winner's box broadcast through LDS, every thread clears the rows that fail the IoU test.  A
// round without a live row ends the loop, uniformly.  No atomics, nothing uploaded: the launch captures as it is.  No FMA
// contraction: +, -, x, max / min and one correctly rounded division, bit-identical to an f32 host restatement.
constexpr int NMS_RPT = 12;   // rows per thread: rows <= 12 288
__device__ __forceinline__ float nms_max(float a, float b) { return (a != a) ? a : ((b != b) ? b : (a >= b ? a : b)); }   // torch.max
__device__ __forceinline__ float nms_min(float a, float b) { return (a != a) ? a : ((b != b) ? b : (a <= b ? a : b)); }   // torch.min
// bbox_iou(box1 = the kept box w, box2 = a later row b)
__device__ __forceinline__ float nms_iou(const float* w, const float* b) {
#pragma clang fp contract(off)
    const float ix1 = nms_max(w[0], b[0]), iy1 = nms_max(w[1], b[1]);
    const float ix2 = nms_min(w[2], b[2]), iy2 = nms_min(w[3], b[3]);
    const float inter = nms_max(ix2 - ix1 + 1.f, 0.f) * nms_max(iy2 - iy1 + 1.f, 0.f);
    const float a1 = (w[2] - w[0] + 1.f) * (w[3] - w[1] + 1.f);
    const float a2 = (b[2] - b[0] + 1.f) * (b[3] - b[1] + 1.f);
    return inter / (a1 + a2 - inter);
}
template <class Rows>
__device__ __forceinline__ void select_nms(const Rows& src, int rows, float conf, int ncls, int class_id, float nms_conf, int C,
                                           float* __restrict__ out, int ld_slot, int* __restrict__ count) {
#pragma clang fp contract(off)
    __shared__ float sv[16];
    __shared__ int si[16];
    __shared__ float sbox[4];
    float bx[NMS_RPT][4], ob[NMS_RPT];
    unsigned live = 0;
    const int tid = threadIdx.x;
#pragma unroll
    for (int j = 0; j < NMS_RPT; ++j) {
        const int r = tid + j * 1024;
        ob[j] = -1.f;
        bx[j][0] = bx[j][1] = bx[j][2] = bx[j][3] = 0.f;
        if (r < rows) {
            const float* q = src.row(r);
            const float obj = src.attr(q, 4);
            if (obj > conf && first_max_class(src, q, ncls) == class_id) {
                float x[4];
                src.box(r, q, x);
                to_corners(x, bx[j]);
                ob[j] = obj;
                live |= 1u << j;
            }
        }
    }
    const int w = tid >> 6;
    int kept = 0;
    for (int c = 0; c < C; ++c) {
        float best = -1.f;
        int bi = 0x7fffffff;
#pragma unroll
        for (int j = 0; j < NMS_RPT; ++j)   // ascending rows: the first maximum stays
            if (((live >> j) & 1u) && ob[j] > best) { best = ob[j]; bi = tid + j * 1024; }
        wave_first_max(best, bi);
        if ((tid & 63) == 0) { sv[w] = best; si[w] = bi; }
        __syncthreads();
        combine_partials(sv, si, 16, best, bi);   // every thread reads the 16 partials
        if (best < 0.f) break;   // no live row left: the same on every thread
        if ((bi & 1023) == tid) {   // the winner's owner: broadcast its box, write its record, retire it
            const int jw = bi >> 10;
            float wb[4] = {0.f, 0.f, 0.f, 0.f}, wo = 0.f;
#pragma unroll
            for (int j = 0; j < NMS_RPT; ++j)
                if (j == jw) { wb[0] = bx[j][0]; wb[1] = bx[j][1]; wb[2] = bx[j][2]; wb[3] = bx[j][3]; wo = ob[j]; }
            sbox[0] = wb[0]; sbox[1] = wb[1]; sbox[2] = wb[2]; sbox[3] = wb[3];
            write_record(out + (long long)c * ld_slot, bi, wb, wo, src.attr(src.row(bi), 5 + class_id), class_id);
            live &= ~(1u << jw);
        }
        __syncthreads();   // (also: every thread has read sv / si before the next round rewrites them)
        const float wb[4] = {sbox[0], sbox[1], sbox[2], sbox[3]};
#pragma unroll
        for (int j = 0; j < NMS_RPT; ++j)
            if ((live >> j) & 1u) {
                const float iou = nms_iou(wb, bx[j]);
                if (!(iou < nms_conf)) live &= ~(1u << j);
            }
        ++kept;
        __syncthreads();   // sbox is read before the next winner overwrites it
    }
    if (tid < C && tid >= kept) write_empty(out + (long long)tid * ld_slot);   // unused slots
    if (tid == 0) *count = kept;
}
template <class Src>
__global__ __launch_bounds__(1024) void yolo_select_nms_kernel(Src src, float conf, int num_classes, int class_id, float nms_conf, int C,
                                                                float* __restrict__ sel, int* __restrict__ count, int ld_image,
                                                                int ld_slot) {
    select_nms(src.image(blockIdx.x), src.rows, conf, min(num_classes, src.attrs - 5), class_id, nms_conf, C,
               sel + (long long)blockIdx.x * ld_image, ld_slot, count + blockIdx.x);
}
void launch_yolo_select_nms(const YoloRowSource& src, int N, float conf, int num_classes, int class_id, float nms_conf, int C,
                            float* sel, int* count, hipStream_t s, int ld_image, int ld_slot) {
    BP_CHECK(C >= 1 && C <= BP_MAX_CANDIDATES, "select with NMS: 1 to 8 candidates (BP_MAX_CANDIDATES)");
    BP_CHECK(src.rows >= 1 && src.rows <= NMS_RPT * 1024, "select with NMS: at most 12 288 rows per image");
    const int ncls = num_classes < src.attrs - 5 ? num_classes : src.attrs - 5;
    BP_CHECK(class_id >= 0 && class_id < ncls, "select with NMS: class id is not below the detector's class count");
    with_source(src, [&](auto arg) {
        hipLaunchKernelGGL(HIP_KERNEL_NAME(yolo_select_nms_kernel<decltype(arg)>), dim3(N), dim3(1024), 0, s, arg, conf, num_classes, class_id,
                           nms_conf, C, sel, count, ld_image, ld_slot);
    });
}

}  // namespace bp
