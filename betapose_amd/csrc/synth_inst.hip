// Instance ownership of a multi-object scene on the device (gfx950; include/betapose_hip.h bp_synth_instances).  The
// arithmetic of one (pixel, object) is synth_inst_math.inc, the text synth_inst_host.cpp compiles too; here is who
// loops over what.  An image is a flat run of H W pixels; plane (j, i) of `alone` starts at (j I + i) H W floats.
//   1. inst_init_kernel     one lane per (image, object): the row of `stats` becomes an empty accumulator.  `stats`
//                           itself is the accumulator, so the call needs no workspace.
//   2. inst_winner_kernel   one lane per four consecutive pixels of an image, a loop over the present objects: the
//                           nearest positive depth wins, the higher j on a tie.  Where H W is a multiple of 4 and a
//                           tensor's base is aligned (16 bytes for the floats, 4 for the ids) every plane and every
//                           quad of it is aligned too, and the lane moves 16-byte words and one 4-byte word of ids;
//                           each tensor falls back to scalar accesses on its own otherwise (chosen per call).
//   3. inst_stats_kernel    one block per (span of SI_SPAN pixels, (image, object)): every lane keeps count and extrema
//                           of the object's covered and of its owned pixels, a wave shuffle tree combines them and lane
//                           0 of each wave folds them into the row of `stats` with integer atomicMin / atomicMax /
//                           atomicAdd (the reduction of annot_mask_boxes_kernel).
//   4. inst_finish_kernel   one lane per (image, object): a box whose count is 0 becomes -1 x4.
// Minimum, maximum and sum over integers do not depend on the order of their operands: the results are the same
// whatever the scheduling and equal the host twin's bit for bit.  No floating-point atomics.  Bounds: a quad's pixels
// are tested against H W unless H W % 4 == 0 (then 4 q + 3 < H W for every quad q); every plane index is below J I.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "bp_common.h"
#include "synth.h"

namespace bp {

namespace {

#include "synth_inst_math.inc"

constexpr int SI_THREADS = 256;
constexpr int SI_SPAN = SI_THREADS * 16;          // pixels per block of the reduction: four quads per lane
constexpr int SI_VEC_ALONE = 1, SI_VEC_DEPTH = 2, SI_VEC_IDS = 4;

__global__ __launch_bounds__(SI_THREADS) void inst_init_kernel(int* __restrict__ stats, int rows) {
    const int o = blockIdx.x * SI_THREADS + threadIdx.x;
    if (o >= rows) return;
    int* s = stats + (size_t)o * SY_INST_STATS;
    s[SI_PX_ALL] = 0;
    s[SI_PX_VISIB] = 0;
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        int* b = s + (k ? SI_BOX_VISIB : SI_BOX_FULL);
        b[0] = SI_EMPTY_MIN;
        b[1] = SI_EMPTY_MAX;
        b[2] = SI_EMPTY_MIN;
        b[3] = SI_EMPTY_MAX;
    }
}

__global__ __launch_bounds__(SI_THREADS) void inst_finish_kernel(int* __restrict__ stats, int rows) {
    const int o = blockIdx.x * SI_THREADS + threadIdx.x;
    if (o >= rows) return;
    int* s = stats + (size_t)o * SY_INST_STATS;
    si_box_finish(s + SI_BOX_FULL, s[SI_PX_ALL]);
    si_box_finish(s + SI_BOX_VISIB, s[SI_PX_VISIB]);
}

// four depths of a plane at pixel p0 (a multiple of 4): one 16-byte load, or those below HW one by one (0 beyond)
__device__ __forceinline__ void si_load_quad(const float* __restrict__ a, int p0, int HW, bool vec, float* d) {
    if (vec) {
        const float4 v = *reinterpret_cast<const float4*>(a + p0);
        d[0] = v.x, d[1] = v.y, d[2] = v.z, d[3] = v.w;
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) d[k] = p0 + k < HW ? a[p0 + k] : 0.0f;
    }
}

// grid (ceil(ceil(HW / 4) / 256), min(I, 65535))
__global__ __launch_bounds__(SI_THREADS) void inst_winner_kernel(const float* __restrict__ alone, int J, int I, int HW,
                                                                 const unsigned char* __restrict__ present, int vec,
                                                                 unsigned char* __restrict__ ids, float* __restrict__ depth) {
    const int p0 = (blockIdx.x * SI_THREADS + (int)threadIdx.x) * 4;      // HW <= 2^24
    if (p0 >= HW) return;
    for (int i = blockIdx.y; i < I; i += gridDim.y) {
        const unsigned char* pr = present + (size_t)i * J;
        float best[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        int id[4] = {0, 0, 0, 0};
        for (int j = 0; j < J; ++j) {
            if (!pr[j]) continue;                                          // (uniform over the block)
            float d[4];
            si_load_quad(alone + ((size_t)j * I + i) * HW, p0, HW, vec & SI_VEC_ALONE, d);
#pragma unroll
            for (int k = 0; k < 4; ++k) si_pick(d[k], j, best[k], id[k]);
        }
        float* z = depth + (size_t)i * HW + p0;
        unsigned char* m = ids + (size_t)i * HW + p0;
        if (vec & SI_VEC_DEPTH) {
            *reinterpret_cast<float4*>(z) = make_float4(best[0], best[1], best[2], best[3]);
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (p0 + k < HW) z[k] = best[k];
        }
        if (vec & SI_VEC_IDS) {
            *reinterpret_cast<uint32_t*>(m) = (uint32_t)id[0] | ((uint32_t)id[1] << 8) | ((uint32_t)id[2] << 16) | ((uint32_t)id[3] << 24);
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (p0 + k < HW) m[k] = (unsigned char)id[k];
        }
    }
}

// the wave's box in lane 0, folded into the row's count and box by integer atomics (skipped when the wave met nothing)
__device__ __forceinline__ void si_box_commit(SiBox b, int* __restrict__ count, int* __restrict__ box) {
    for (int o = 32; o > 0; o >>= 1) {
        b.xmin = min(b.xmin, __shfl_down(b.xmin, o, 64));
        b.xmax = max(b.xmax, __shfl_down(b.xmax, o, 64));
        b.ymin = min(b.ymin, __shfl_down(b.ymin, o, 64));
        b.ymax = max(b.ymax, __shfl_down(b.ymax, o, 64));
        b.count += __shfl_down(b.count, o, 64);
    }
    if ((threadIdx.x & 63) == 0 && b.count > 0) {
        atomicMin(&box[0], b.xmin);
        atomicMax(&box[1], b.xmax);
        atomicMin(&box[2], b.ymin);
        atomicMax(&box[3], b.ymax);
        atomicAdd(count, b.count);
    }
}

// grid (ceil(HW / SI_SPAN), min(I J, 65535))
__global__ __launch_bounds__(SI_THREADS) void inst_stats_kernel(const float* __restrict__ alone, int J, int I, int H, int W,
                                                                const unsigned char* __restrict__ ids, int vec,
                                                                int* __restrict__ stats) {
    const int HW = H * W;                                                  // <= 2^24
    const int begin = blockIdx.x * SI_SPAN, end = min(HW, begin + SI_SPAN);
    for (int o = blockIdx.y; o < I * J; o += gridDim.y) {                  // (uniform over the block: the shuffles see whole waves)
        const int i = o / J, j = o - i * J;
        const float* a = alone + ((size_t)j * I + i) * HW;
        const unsigned char* m = ids + (size_t)i * HW;
        SiBox full = si_box_empty(), vis = si_box_empty();
        for (int p0 = begin + (int)threadIdx.x * 4; p0 < end; p0 += SI_THREADS * 4) {
            float d[4];
            si_load_quad(a, p0, HW, vec & SI_VEC_ALONE, d);
            if (!(d[0] > 0.0f || d[1] > 0.0f || d[2] > 0.0f || d[3] > 0.0f)) continue;
            int owner[4];
            if (vec & SI_VEC_IDS) {
                const uint32_t w = *reinterpret_cast<const uint32_t*>(m + p0);
#pragma unroll
                for (int k = 0; k < 4; ++k) owner[k] = (int)((w >> (8 * k)) & 255u);
            } else {
#pragma unroll
                for (int k = 0; k < 4; ++k) owner[k] = p0 + k < HW ? m[p0 + k] : 0;
            }
            int y = p0 / W, x = p0 - y * W;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                si_stats_add(full, vis, d[k], owner[k], j, x, y);
                if (++x == W) x = 0, ++y;
            }
        }
        int* s = stats + (size_t)o * SY_INST_STATS;
        si_box_commit(full, s + SI_PX_ALL, s + SI_BOX_FULL);
        si_box_commit(vis, s + SI_PX_VISIB, s + SI_BOX_VISIB);
    }
}

inline bool aligned_to(const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

}  // namespace

void launch_synth_instances(const float* alone, int J, int I, int H, int W, const unsigned char* present, unsigned char* ids,
                            float* depth, int* stats, hipStream_t s) {
    const int HW = H * W, rows = I * J;
    const bool quads = HW % 4 == 0;
    const int vec = (quads && aligned_to(alone, 16) ? SI_VEC_ALONE : 0) | (quads && aligned_to(depth, 16) ? SI_VEC_DEPTH : 0) |
                    (quads && aligned_to(ids, 4) ? SI_VEC_IDS : 0);
    const unsigned row_blocks = (unsigned)((rows + SI_THREADS - 1) / SI_THREADS);
    hipLaunchKernelGGL(inst_init_kernel, dim3(row_blocks), dim3(SI_THREADS), 0, s, stats, rows);
    hipLaunchKernelGGL(inst_winner_kernel, dim3(((HW + 3) / 4 + SI_THREADS - 1) / SI_THREADS, I < 65535 ? I : 65535), dim3(SI_THREADS),
                       0, s, alone, J, I, HW, present, vec, ids, depth);
    hipLaunchKernelGGL(inst_stats_kernel, dim3((HW + SI_SPAN - 1) / SI_SPAN, rows < 65535 ? rows : 65535), dim3(SI_THREADS), 0, s,
                       alone, J, I, H, W, ids, vec, stats);
    hipLaunchKernelGGL(inst_finish_kernel, dim3(row_blocks), dim3(SI_THREADS), 0, s, stats, rows);
    BP_HIP(hipGetLastError());
}

}  // namespace bp
