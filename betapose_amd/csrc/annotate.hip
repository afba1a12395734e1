// Key-point annotator on the device (include/betapose_hip.h bp_annotate_keypoints, bp_mask_boxes, bp_vertex_boxes,
// bp_kpd_targets).  The arithmetic of one key point, one pixel, one vertex and one map value is annotate_math.inc, the
// text the host twins (annotate_host.cpp) compile too; here is who loops over what:
//   annot_keypoints_kernel   one lane per (pose, key point), grid-stride.
//   annot_mask_boxes_kernel  one block per (pose, band of AN_BAND rows): every lane keeps the min / max / count of the
//                            covered and of the visible pixels it meets, a wave shuffle tree combines them, and lane 0 of
//                            each wave folds them into the pose's accumulator with integer atomicMin / atomicMax /
//                            atomicAdd.  annot_boxes_init_kernel sets the accumulators before, annot_boxes_finish_kernel
//                            turns them into boxes (-1 x4 when the count is 0) after.
//   annot_vertex_boxes_kernel  the same reduction over (pose, slice of AN_VERTS vertices).
//   annot_centres_kernel     one lane per (sample, part): the heat-map centre.
//   annot_targets_kernel     one lane per 4 consecutive floats of a map row, grid-stride: a 16-byte store where the row
//                            starts on a 16-byte boundary and the four floats lie inside it, scalar stores otherwise.
//                            Every element of the maps is written, so the caller does not clear them.
// Minimum, maximum and sum over integers do not depend on the order of their operands, so every result is the same
// whatever the scheduling, and equal to the host twin's bit for bit.  Every load of an image is indexed by a pixel that
// has been tested against [0, W) x [0, H); every store index is below the launch's element count.
#include "bp_common.h"
#include "annotate.h"

#pragma clang fp contract(off)

namespace bp {

namespace {

#include "annotate_math.inc"

static_assert(AN_BOX_INTS == ANNOT_BOX_INTS, "annotate.h and annotate_math.inc disagree");

constexpr int AN_THREADS = 256;
constexpr int AN_BAND = 16;                     // rows per block of the mask reduction
constexpr int AN_VERTS = AN_THREADS * 8;        // vertices per block of the vertex reduction

inline int an_grid(long long n, int cap = 4096) {     // (aux_kernels.hip grid_for)
    long long g = (n + AN_THREADS - 1) / AN_THREADS;
    return (int)(g < 1 ? 1 : (g > cap ? cap : g));
}

__global__ __launch_bounds__(AN_THREADS) void annot_keypoints_kernel(const double* __restrict__ poses, int P,
                                                                     const double* __restrict__ kp, int Kp, AnCam cam, int H,
                                                                     int W, const float* __restrict__ model_depth,
                                                                     const float* __restrict__ scene_depth,
                                                                     const int* __restrict__ scene_index, double self_tol,
                                                                     double delta, double* __restrict__ xy,
                                                                     double* __restrict__ z, unsigned char* __restrict__ flags) {
    const int total = P * Kp;                   // < 2^31 (checked by the caller)
    const size_t HW = (size_t)H * W;
    for (int i = blockIdx.x * AN_THREADS + threadIdx.x; i < total; i += gridDim.x * AN_THREADS) {
        const int p = i / Kp, k = i - p * Kp;
        const float* md = model_depth ? model_depth + (size_t)p * HW : nullptr;
        const float* sc = scene_depth ? scene_depth + (size_t)scene_index[p] * HW : nullptr;
        double o[2], zz;
        const unsigned f = an_keypoint(cam, poses + (size_t)p * 12, kp + (size_t)k * 3, H, W, md, sc, self_tol, delta, o, &zz);
        xy[(size_t)i * 2] = o[0];
        xy[(size_t)i * 2 + 1] = o[1];
        z[i] = zz;
        flags[i] = (unsigned char)f;
    }
}

struct AnBox {
    int xmin, xmax, ymin, ymax, count;
};

__device__ __forceinline__ AnBox an_box_empty() {
    return AnBox{AN_BOX_EMPTY_MIN, AN_BOX_EMPTY_MAX, AN_BOX_EMPTY_MIN, AN_BOX_EMPTY_MAX, 0};
}

__device__ __forceinline__ void an_box_add(AnBox& b, int x, int y) {
    b.xmin = min(b.xmin, x);
    b.xmax = max(b.xmax, x);
    b.ymin = min(b.ymin, y);
    b.ymax = max(b.ymax, y);
    ++b.count;
}

// the wave's box in lane 0, folded into acc [AN_BOX_INTS] by integer atomics (skipped when the wave met nothing)
__device__ __forceinline__ void an_box_commit(AnBox b, int* __restrict__ acc) {
    for (int o = 32; o > 0; o >>= 1) {
        b.xmin = min(b.xmin, __shfl_down(b.xmin, o, 64));
        b.xmax = max(b.xmax, __shfl_down(b.xmax, o, 64));
        b.ymin = min(b.ymin, __shfl_down(b.ymin, o, 64));
        b.ymax = max(b.ymax, __shfl_down(b.ymax, o, 64));
        b.count += __shfl_down(b.count, o, 64);
    }
    if ((threadIdx.x & 63) == 0 && b.count > 0) {
        atomicMin(&acc[0], b.xmin);
        atomicMax(&acc[1], b.xmax);
        atomicMin(&acc[2], b.ymin);
        atomicMax(&acc[3], b.ymax);
        atomicAdd(&acc[4], b.count);
    }
}

__global__ __launch_bounds__(AN_THREADS) void annot_boxes_init_kernel(int* __restrict__ acc, int boxes) {
    const int i = blockIdx.x * AN_THREADS + threadIdx.x;
    if (i >= boxes) return;
    int* a = acc + (size_t)i * AN_BOX_INTS;
    a[0] = AN_BOX_EMPTY_MIN;
    a[1] = AN_BOX_EMPTY_MAX;
    a[2] = AN_BOX_EMPTY_MIN;
    a[3] = AN_BOX_EMPTY_MAX;
    a[4] = 0;
}

// boxes [n][4] and (counts non-null) counts [n] from acc [n][AN_BOX_INTS]
__global__ __launch_bounds__(AN_THREADS) void annot_boxes_finish_kernel(const int* __restrict__ acc, int boxes,
                                                                        int* __restrict__ out, int* __restrict__ counts) {
    const int i = blockIdx.x * AN_THREADS + threadIdx.x;
    if (i >= boxes) return;
    const int* a = acc + (size_t)i * AN_BOX_INTS;
    const int cnt = a[4];
    for (int k = 0; k < 4; ++k) out[(size_t)i * 4 + k] = cnt > 0 ? a[k] : -1;
    if (counts) counts[i] = cnt;
}

__global__ __launch_bounds__(AN_THREADS) void annot_mask_boxes_kernel(const float* __restrict__ depth, int P, int H, int W,
                                                                      AnCam cam, const float* __restrict__ scene_depth,
                                                                      const int* __restrict__ scene_index, double delta,
                                                                      int* __restrict__ acc) {
    const int y0 = blockIdx.x * AN_BAND, y1 = min(H, y0 + AN_BAND);
    const int i0 = y0 * W, i1 = y1 * W;         // H * W <= 2^24
    const size_t HW = (size_t)H * W;
    for (int p = blockIdx.y; p < P; p += gridDim.y) {   // (uniform over the block: the shuffles below see whole waves)
        const float* d = depth + (size_t)p * HW;
        const float* sc = scene_depth ? scene_depth + (size_t)scene_index[p] * HW : nullptr;
        AnBox full = an_box_empty(), vis = an_box_empty();
        for (int i = i0 + (int)threadIdx.x; i < i1; i += AN_THREADS) {
            const float D = d[i];
            if (!(D > 0.0f)) continue;
            const int y = i / W, x = i - y * W;
            an_box_add(full, x, y);
            if (!sc || an_pixel_visible(cam, x, y, D, sc[i], delta)) an_box_add(vis, x, y);
        }
        an_box_commit(full, acc + (size_t)p * 2 * AN_BOX_INTS);
        an_box_commit(vis, acc + ((size_t)p * 2 + 1) * AN_BOX_INTS);
    }
}

__global__ __launch_bounds__(AN_THREADS) void annot_vertex_boxes_kernel(const double* __restrict__ poses, int P,
                                                                        const double* __restrict__ vertices, int n, AnCam cam,
                                                                        int H, int W, int* __restrict__ acc) {
    const int v0 = blockIdx.x * AN_VERTS, v1 = min(n, v0 + AN_VERTS);
    for (int p = blockIdx.y; p < P; p += gridDim.y) {   // (uniform over the block)
        AnBox b = an_box_empty();
        for (int i = v0 + (int)threadIdx.x; i < v1; i += AN_THREADS) {
            int ix, iy;
            if (an_splat(cam, poses + (size_t)p * 12, vertices + (size_t)i * 3, H, W, &ix, &iy)) an_box_add(b, ix, iy);
        }
        an_box_commit(b, acc + (size_t)p * AN_BOX_INTS);
    }
}

__global__ __launch_bounds__(AN_THREADS) void annot_centres_kernel(const double* __restrict__ parts, const float* __restrict__ ul,
                                                                   const float* __restrict__ br, int B, int Kp, int inpH,
                                                                   int inpW, int resH, int* __restrict__ centres) {
    const int i = blockIdx.x * AN_THREADS + threadIdx.x;
    if (i >= B * Kp) return;
    const int b = i / Kp;
    int cx, cy;
    an_target_centre(parts[(size_t)i * 2], parts[(size_t)i * 2 + 1], ul[b * 2], ul[b * 2 + 1], br[b * 2], br[b * 2 + 1], inpH,
                     inpW, resH, &cx, &cy);
    centres[(size_t)i * 2] = cx;
    centres[(size_t)i * 2 + 1] = cy;
}

// four floats of a map row at x0: one 16-byte store when all four lie in the row and the address is 16-byte aligned
// (vec), scalar stores of those inside the row otherwise
__device__ __forceinline__ void an_store_quad(float* __restrict__ dst, int x0, int resW, bool vec, const float* v) {
    if (vec) {
        *reinterpret_cast<float4*>(dst) = make_float4(v[0], v[1], v[2], v[3]);
    } else {
        for (int j = 0; j < 4; ++j)
            if (x0 + j < resW) dst[j] = v[j];
    }
}

// base_aligned: out (and set_mask, when given) start on a 16-byte boundary
__global__ __launch_bounds__(AN_THREADS) void annot_targets_kernel(const int* __restrict__ centres, int maps, int resH, int resW,
                                                                   const float* __restrict__ g, int size, int base_aligned,
                                                                   float* __restrict__ out, float* __restrict__ set_mask) {
    const int quads = (resW + 3) / 4;
    const int total = maps * resH * quads;      // < 2^31 (checked by the caller)
    for (int i = blockIdx.x * AN_THREADS + threadIdx.x; i < total; i += gridDim.x * AN_THREADS) {
        const int q = i % quads, r = i / quads; // r = map * resH + y
        const int y = r % resH, m = r / resH;
        const int cx = centres[(size_t)m * 2], cy = centres[(size_t)m * 2 + 1];
        const int x0 = q * 4;
        float v[4], one[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            v[j] = x0 + j < resW ? an_target_value(g, size, cx, cy, x0 + j, y) : 0.0f;
            one[j] = 1.0f;
        }
        const size_t off = (size_t)r * resW + x0;       // < maps * resH * resW: inside the tensor
        const bool vec = base_aligned && x0 + 4 <= resW && (off & 3) == 0;
        an_store_quad(out + off, x0, resW, vec, v);
        if (set_mask) an_store_quad(set_mask + off, x0, resW, vec, one);
    }
}

}  // namespace

void launch_annotate_keypoints(const double* poses, int P, const double* kp, int Kp, const double* K, int H, int W,
                               double pixel_center, double near, const float* model_depth, const float* scene_depth,
                               const int* scene_index, double self_tol, double delta, double* xy, double* z,
                               unsigned char* flags, hipStream_t s) {
    const AnCam cam = an_cam(K, pixel_center, near);
    hipLaunchKernelGGL(annot_keypoints_kernel, dim3(an_grid((long long)P * Kp)), dim3(AN_THREADS), 0, s, poses, P, kp, Kp, cam, H,
                       W, model_depth, scene_depth, scene_index, self_tol, delta, xy, z, flags);
}

void launch_mask_boxes(const float* depth, int P, int H, int W, const double* K, double pixel_center, const float* scene_depth,
                       const int* scene_index, double delta, int* acc, int* boxes, int* counts, hipStream_t s) {
    const AnCam cam = an_cam(K, pixel_center, 0.0);
    const int nb = 2 * P;
    hipLaunchKernelGGL(annot_boxes_init_kernel, dim3((nb + AN_THREADS - 1) / AN_THREADS), dim3(AN_THREADS), 0, s, acc, nb);
    hipLaunchKernelGGL(annot_mask_boxes_kernel, dim3((H + AN_BAND - 1) / AN_BAND, P < 65535 ? P : 65535), dim3(AN_THREADS), 0, s,
                       depth, P, H, W, cam, scene_depth, scene_index, delta, acc);
    hipLaunchKernelGGL(annot_boxes_finish_kernel, dim3((nb + AN_THREADS - 1) / AN_THREADS), dim3(AN_THREADS), 0, s, acc, nb,
                       boxes, counts);
}

void launch_vertex_boxes(const double* poses, int P, const double* vertices, int n, const double* K, int H, int W, int* acc,
                         int* boxes, hipStream_t s) {
    const AnCam cam = an_cam(K, 0.0, 0.0);
    hipLaunchKernelGGL(annot_boxes_init_kernel, dim3((P + AN_THREADS - 1) / AN_THREADS), dim3(AN_THREADS), 0, s, acc, P);
    hipLaunchKernelGGL(annot_vertex_boxes_kernel, dim3((n + AN_VERTS - 1) / AN_VERTS, P < 65535 ? P : 65535), dim3(AN_THREADS), 0,
                       s, poses, P, vertices, n, cam, H, W, acc);
    hipLaunchKernelGGL(annot_boxes_finish_kernel, dim3((P + AN_THREADS - 1) / AN_THREADS), dim3(AN_THREADS), 0, s, acc, P, boxes,
                       (int*)nullptr);
}

void launch_kpd_targets(const double* parts, const float* ul, const float* br, int B, int Kp, int inpH, int inpW, int resH,
                        int resW, const float* g, int size, float* out, int* centres, float* set_mask, hipStream_t s) {
    const int maps = B * Kp;
    hipLaunchKernelGGL(annot_centres_kernel, dim3((maps + AN_THREADS - 1) / AN_THREADS), dim3(AN_THREADS), 0, s, parts, ul, br, B,
                       Kp, inpH, inpW, resH, centres);
    const long long total = (long long)maps * resH * ((resW + 3) / 4);
    const int aligned = ((uintptr_t)out & 15) == 0 && (!set_mask || ((uintptr_t)set_mask & 15) == 0);
    hipLaunchKernelGGL(annot_targets_kernel, dim3(an_grid(total)), dim3(AN_THREADS), 0, s, centres, maps, resH, resW, g, size,
                       aligned, out, set_mask);
}

}  // namespace bp
