// Colour images of posed meshes, 3-D bounding boxes and their blend over a frame (include/betapose_hip.h
// bp_render_color, bp_draw_boxes, bp_overlay).  The arithmetic of one fragment, one box edge and one blended pixel is
// raster_math.inc + raster_color_math.inc, the text the host twin (raster_color_host.cpp) compiles too; here is who
// loops over what:
//   1. color_clear_kernel, one lane per pixel: the empty key, or the kept key of a pixel an earlier call drew.
//   2. raster.hip's transform (launch_raster_transform), then color_visibility_kernel, one lane per (pose, triangle):
//      rs_walk (raster_walk.inc, the walk raster_tri_kernel and the host twins run too) with the key buffer as its sink.
//      Every covered pixel takes ONE 64-bit atomicMin of (depth bits << 32 | pose slot * F + face) on global memory.
//   3. color_resolve_kernel, one lane per pixel, no atomics: decodes the key and shades the winner from the model, the
//      faces and the pose (never from the per-chunk vertex workspace), keeps an accumulated pixel, or writes background.
//   4. box_mark_kernel, one lane per (pose, edge): an integer DDA over major-axis positions clamped to the image, each
//      pixel an atomicMax of (pose slot * 12 + edge + 1) into a scratch plane; box_paint_kernel, one lane per pixel,
//      colours the marked pixels.  The highest (pose slot, edge) wins whatever the scheduling.
//   5. overlay_kernel, one lane per pixel.
// A minimum and a maximum do not depend on the order of their operands, so every image is the same from run to run and
// equal to the host twin's byte for byte.  Every pixel loop runs over a range clamped to the image before the loop.
#include "bp_common.h"
#include "raster.h"

#pragma clang fp contract(off)

namespace bp {

namespace {

#include "raster_math.inc"
#define RS_WALK_DEVICE      // the kernels' walk too, not only the host's
#include "raster_walk.inc"
#include "raster_color_math.inc"

constexpr int RC_THREADS = 256;

inline unsigned rc_blocks(size_t count) {
    size_t blocks = (count + RC_THREADS - 1) / RC_THREADS;
    return (unsigned)(blocks > 65535 ? 65535 : (blocks ? blocks : 1));
}

__global__ __launch_bounds__(RC_THREADS) void color_clear_kernel(unsigned long long* __restrict__ keys,
                                                                 const float* __restrict__ depth, int accumulate, size_t count) {
    for (size_t i = (size_t)blockIdx.x * RC_THREADS + threadIdx.x; i < count; i += (size_t)gridDim.x * RC_THREADS) {
        unsigned long long key = RC_EMPTY_KEY;
        if (accumulate) {
            const float d = depth[i];
            if (d > 0.0f) key = rc_key(__float_as_uint(d), RC_KEEP);
        }
        keys[i] = key;
    }
}

struct KeySink {       // smaller key wins: nearest, then the lowest pose slot, then the lowest face
    unsigned long long* __restrict__ kb;
    uint32_t id0;       // fragment id of the pose slot's face 0
    __device__ __forceinline__ void operator()(size_t at, uint32_t bits, int face) const {
        atomicMin(&kb[at], rc_key(bits, id0 + (uint32_t)face));
    }
};

__global__ __launch_bounds__(RC_THREADS) void color_visibility_kernel(const int* __restrict__ faces, int F, int n,
                                                                      const double* __restrict__ xyz, const int* __restrict__ uv,
                                                                      int q0, int poses, const int* __restrict__ image_index,
                                                                      int img0, RsCam cam, int H, int W,
                                                                      unsigned long long* __restrict__ keys,
                                                                      int* __restrict__ skipped) {
    const RsFace face = rs_face(faces, F, blockIdx.x * RC_THREADS + threadIdx.x);
    for (int qc = blockIdx.y; qc < poses; qc += gridDim.y) {   // (uniform over the block: the walk's ballots see whole waves)
        const int q = q0 + qc;                                 // the call's pose slot
        const int image = (image_index ? image_index[q] : q) - img0;    // in range: the host chose the chunk by it
        rs_walk(cam, face, F, n, xyz + (size_t)qc * n * 3, uv + (size_t)qc * n * 2, H, W, skipped + q,
                KeySink{keys + (size_t)image * H * W, (uint32_t)((unsigned long long)q * F)});
    }
}

__global__ __launch_bounds__(RC_THREADS) void color_resolve_kernel(const unsigned long long* __restrict__ keys, size_t count,
                                                                   const double* __restrict__ model,
                                                                   const int* __restrict__ faces, int F,
                                                                   const unsigned char* __restrict__ colors,
                                                                   const double* __restrict__ poses, RsCam cam, ColorLight lt, int H,
                                                                   int W, unsigned char* __restrict__ color,
                                                                   float* __restrict__ depth) {
    const size_t HW = (size_t)H * W;
    for (size_t at = (size_t)blockIdx.x * RC_THREADS + threadIdx.x; at < count; at += (size_t)gridDim.x * RC_THREADS) {
        const unsigned long long key = keys[at];
        const uint32_t id = (uint32_t)key;
        if (key == RC_EMPTY_KEY) {
            color[at * 3 + 0] = 0;
            color[at * 3 + 1] = 0;
            color[at * 3 + 2] = 0;
            depth[at] = 0.0f;
            continue;
        }
        if (id == RC_KEEP) continue;
        const size_t pix = at % HW;
        const int x = (int)(pix % W), y = (int)(pix / W);
        const int q = (int)(id / (uint32_t)F), f = (int)(id % (uint32_t)F);
        const double* pose = poses + (size_t)q * 12;
        const int i0 = faces[(size_t)f * 3 + 0], i1 = faces[(size_t)f * 3 + 1], i2 = faces[(size_t)f * 3 + 2];   // a winner's are in range
        double A[3], B[3], C[3];
        rs_transform(pose, model[(size_t)i0 * 3 + 0], model[(size_t)i0 * 3 + 1], model[(size_t)i0 * 3 + 2], A);
        rs_transform(pose, model[(size_t)i1 * 3 + 0], model[(size_t)i1 * 3 + 1], model[(size_t)i1 * 3 + 2], B);
        rs_transform(pose, model[(size_t)i2 * 3 + 0], model[(size_t)i2 * 3 + 1], model[(size_t)i2 * 3 + 2], C);
        unsigned char ca[3], cb[3], cc[3], out[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            ca[k] = colors[(size_t)i0 * 3 + k];
            cb[k] = colors[(size_t)i1 * 3 + k];
            cc[k] = colors[(size_t)i2 * 3 + k];
        }
        rc_shade(cam, A, B, C, ca, cb, cc, x, y, lt, out);
        color[at * 3 + 0] = out[0];
        color[at * 3 + 1] = out[1];
        color[at * 3 + 2] = out[2];
        depth[at] = __uint_as_float((uint32_t)(key >> 32));
    }
}

__global__ __launch_bounds__(RC_THREADS) void box_mark_kernel(const double* __restrict__ poses, int q0, int count,
                                                              const double* __restrict__ corners,
                                                              const int* __restrict__ image_index, int img0, RsCam cam, int H,
                                                              int W, uint32_t* __restrict__ ids) {
    const int i = blockIdx.x * RC_THREADS + threadIdx.x;
    if (i >= count * RC_BOX_EDGES) return;
    const int q = q0 + i / RC_BOX_EDGES, e = i % RC_BOX_EDGES;
    RcEdge g;
    if (!rc_edge_setup(cam, poses + (size_t)q * 12, corners, e, H, W, &g)) return;
    uint32_t* plane = ids + (size_t)((image_index ? image_index[q] : q) - img0) * H * W;
    const uint32_t id = (uint32_t)q * RC_BOX_EDGES + e + 1;
    const long long minor_size = g.major_x ? H : W;
    for (int p = g.p0; p <= g.p1; ++p) {        // 0 <= p0, p1 < W (or H): clamped by rc_edge_setup
        const long long j = rc_edge_minor(g, p);
        if (j < 0 || j >= minor_size) continue;
        atomicMax(&plane[g.major_x ? (size_t)j * W + p : (size_t)p * W + j], id);
    }
}

__global__ __launch_bounds__(RC_THREADS) void box_paint_kernel(const uint32_t* __restrict__ ids, size_t count,
                                                               const double* __restrict__ poses,
                                                               const double* __restrict__ corners,
                                                               const unsigned char* __restrict__ corner_colors, RsCam cam, int H,
                                                               int W, unsigned char* __restrict__ color) {
    const size_t HW = (size_t)H * W;
    for (size_t at = (size_t)blockIdx.x * RC_THREADS + threadIdx.x; at < count; at += (size_t)gridDim.x * RC_THREADS) {
        const uint32_t id = ids[at];
        if (!id) continue;
        const size_t pix = at % HW;
        const int x = (int)(pix % W), y = (int)(pix / W);
        const int q = (int)((id - 1) / RC_BOX_EDGES), e = (int)((id - 1) % RC_BOX_EDGES);
        RcEdge g;
        if (!rc_edge_setup(cam, poses + (size_t)q * 12, corners, e, H, W, &g)) continue;   // (it marked the pixel: it is valid)
        unsigned char out[3];
        rc_edge_color(g, g.major_x ? x : y, corner_colors, out);
        color[at * 3 + 0] = out[0];
        color[at * 3 + 1] = out[1];
        color[at * 3 + 2] = out[2];
    }
}

// (out may be frames: every byte is read before it is written, by the lane that writes it)
__global__ __launch_bounds__(RC_THREADS) void overlay_kernel(const unsigned char* frames, const unsigned char* __restrict__ color,
                                                             const float* __restrict__ depth, size_t pixels, int alpha,
                                                             unsigned char* out) {
    for (size_t i = (size_t)blockIdx.x * RC_THREADS + threadIdx.x; i < pixels; i += (size_t)gridDim.x * RC_THREADS) {
        const bool drawn = depth[i] > 0.0f;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const unsigned char fr = frames[i * 3 + k];
            out[i * 3 + k] = drawn ? rc_blend(alpha, color[i * 3 + k], fr) : fr;
        }
    }
}

}  // namespace

void launch_color_clear(unsigned long long* keys, const float* depth, int accumulate, size_t count, hipStream_t s) {
    hipLaunchKernelGGL(color_clear_kernel, dim3(rc_blocks(count)), dim3(RC_THREADS), 0, s, keys, depth, accumulate, count);
}

void launch_color_visibility(const int* faces, int F, int n, const void* vertex_ws, int q0, int count,
                             const int* d_image_index, int img0, const RsCam& cam, int H, int W, unsigned long long* keys,
                             int* skipped, hipStream_t s) {
    const double* xyz = (const double*)vertex_ws;
    const int* uv = (const int*)(xyz + (size_t)count * n * 3);
    const int gy = count < 65535 ? count : 65535;
    hipLaunchKernelGGL(color_visibility_kernel, dim3((F + RC_THREADS - 1) / RC_THREADS, gy), dim3(RC_THREADS), 0, s, faces, F, n,
                       xyz, uv, q0, count, d_image_index, img0, cam, H, W, keys, skipped);
}

void launch_color_resolve(const unsigned long long* keys, int images, const double* model, const int* faces, int F,
                          const unsigned char* colors, const double* poses, const RsCam& cam, int H, int W,
                          const ColorLight& light, unsigned char* color, float* depth, hipStream_t s) {
    const size_t count = (size_t)images * H * W;
    hipLaunchKernelGGL(color_resolve_kernel, dim3(rc_blocks(count)), dim3(RC_THREADS), 0, s, keys, count, model, faces, F,
                       colors, poses, cam, light, H, W, color, depth);
}

void launch_draw_boxes(const double* poses, int q0, int count, const double* corners, const unsigned char* corner_colors,
                       const int* d_image_index, int img0, int images, const RsCam& cam, int H, int W, uint32_t* ids,
                       unsigned char* color, hipStream_t s) {
    const size_t pixels = (size_t)images * H * W;
    BP_HIP(hipMemsetAsync(ids, 0, pixels * sizeof(uint32_t), s));
    if (count > 0)
        hipLaunchKernelGGL(box_mark_kernel, dim3((count * RC_BOX_EDGES + RC_THREADS - 1) / RC_THREADS), dim3(RC_THREADS), 0, s,
                           poses, q0, count, corners, d_image_index, img0, cam, H, W, ids);
    hipLaunchKernelGGL(box_paint_kernel, dim3(rc_blocks(pixels)), dim3(RC_THREADS), 0, s, ids, pixels, poses, corners,
                       corner_colors, cam, H, W, color);
}

void launch_overlay(const unsigned char* frames, const unsigned char* color, const float* depth, size_t pixels, int alpha,
                    unsigned char* out, hipStream_t s) {
    hipLaunchKernelGGL(overlay_kernel, dim3(rc_blocks(pixels)), dim3(RC_THREADS), 0, s, frames, color, depth, pixels, alpha, out);
}

}  // namespace bp
