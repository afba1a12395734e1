// Textured colour images of posed meshes (include/betapose_hip.h bp_texture_mips, bp_render_color_textured).  Steps 1, 2
// and 4 of raster_color.hip's header (clear, visibility, boxes) are that file's, unchanged: coverage, depth and the
// 64-bit z-test know nothing of colour.  Here are the two things a texture adds:
//   texture_pack_kernel, one lane per texel: the [Ht][Wt][3] u8 image into level 0 of the packed pyramid, one dword a
//     texel; texture_mip_kernel, one lane per texel of a level, one launch per level: the 2 x 2 box filter of the level
//     above (tx_box).  A level is a few per cent of the one before, so the chain costs about a third of the pack.
//   color_resolve_tex_kernel, one lane per pixel, no atomics: color_resolve_kernel's loop with the textured fragment
//     (tx_shade): the winner's three corner UVs, the level from the footprint, four aligned dword loads of that level.
// The arithmetic is raster_math.inc + raster_color_math.inc + raster_texture_math.inc, the text the host twin
// (raster_texture_host.cpp) compiles too: integers and f64 in a fixed order, so the images are equal byte for byte.
// Every texel index is wrapped into its level before the load (tx_mod), whatever the UVs hold.
#include "bp_common.h"
#include "raster.h"

#pragma clang fp contract(off)

namespace bp {

namespace {

#include "raster_math.inc"
#include "raster_color_math.inc"
#include "raster_texture_math.inc"

constexpr int TX_THREADS = 256;

inline unsigned tx_blocks(size_t count) {
    size_t blocks = (count + TX_THREADS - 1) / TX_THREADS;
    return (unsigned)(blocks > 65535 ? 65535 : (blocks ? blocks : 1));
}

__global__ __launch_bounds__(TX_THREADS) void texture_pack_kernel(const unsigned char* __restrict__ image, size_t texels,
                                                                  uint32_t* __restrict__ level0) {
    for (size_t i = (size_t)blockIdx.x * TX_THREADS + threadIdx.x; i < texels; i += (size_t)gridDim.x * TX_THREADS)
        level0[i] = tx_pack(image[i * 3 + 0], image[i * 3 + 1], image[i * 3 + 2]);
}

__global__ __launch_bounds__(TX_THREADS) void texture_mip_kernel(const uint32_t* __restrict__ src, int sw, int sh,
                                                                 uint32_t* __restrict__ dst, int dw, int dh) {
    const size_t texels = (size_t)dw * dh;
    for (size_t i = (size_t)blockIdx.x * TX_THREADS + threadIdx.x; i < texels; i += (size_t)gridDim.x * TX_THREADS)
        dst[i] = tx_box(src, sw, sh, (int)(i % dw), (int)(i / dw));
}

__global__ __launch_bounds__(TX_THREADS) void color_resolve_tex_kernel(const unsigned long long* __restrict__ keys, size_t count,
                                                                       const double* __restrict__ model,
                                                                       const int* __restrict__ faces, int F,
                                                                       const double* __restrict__ uv,
                                                                       const uint32_t* __restrict__ mips, int Wt, int Ht,
                                                                       int levels, const double* __restrict__ poses, RsCam cam,
                                                                       ColorLight lt, int H, int W,
                                                                       unsigned char* __restrict__ color,
                                                                       float* __restrict__ depth) {
    const size_t HW = (size_t)H * W;
    for (size_t at = (size_t)blockIdx.x * TX_THREADS + threadIdx.x; at < count; at += (size_t)gridDim.x * TX_THREADS) {
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
        double A[3], B[3], C[3], t[6];
        rs_transform(pose, model[(size_t)i0 * 3 + 0], model[(size_t)i0 * 3 + 1], model[(size_t)i0 * 3 + 2], A);
        rs_transform(pose, model[(size_t)i1 * 3 + 0], model[(size_t)i1 * 3 + 1], model[(size_t)i1 * 3 + 2], B);
        rs_transform(pose, model[(size_t)i2 * 3 + 0], model[(size_t)i2 * 3 + 1], model[(size_t)i2 * 3 + 2], C);
#pragma unroll
        for (int k = 0; k < 6; ++k) t[k] = uv[(size_t)f * 6 + k];
        unsigned char out[3];
        tx_shade(cam, A, B, C, t, mips, Wt, Ht, levels, x, y, lt, out);
        color[at * 3 + 0] = out[0];
        color[at * 3 + 1] = out[1];
        color[at * 3 + 2] = out[2];
        depth[at] = __uint_as_float((uint32_t)(key >> 32));
    }
}

}  // namespace

void launch_texture_mips(const unsigned char* image, int Wt, int Ht, int levels, uint32_t* mips, hipStream_t s) {
    const size_t texels = (size_t)Wt * Ht;
    hipLaunchKernelGGL(texture_pack_kernel, dim3(tx_blocks(texels)), dim3(TX_THREADS), 0, s, image, texels, mips);
    int sw = Wt, sh = Ht;
    uint32_t* src = mips;
    for (int l = 1; l < levels; ++l) {
        const int dw = tx_half(sw), dh = tx_half(sh);
        uint32_t* dst = src + (size_t)sw * sh;
        hipLaunchKernelGGL(texture_mip_kernel, dim3(tx_blocks((size_t)dw * dh)), dim3(TX_THREADS), 0, s, src, sw, sh, dst, dw, dh);
        src = dst;
        sw = dw;
        sh = dh;
    }
}

void launch_color_resolve_tex(const unsigned long long* keys, int images, const double* model, const int* faces, int F,
                              const ColorTexture& tex, const double* poses, const RsCam& cam, int H, int W,
                              const ColorLight& light, unsigned char* color, float* depth, hipStream_t s) {
    const size_t count = (size_t)images * H * W;
    hipLaunchKernelGGL(color_resolve_tex_kernel, dim3(tx_blocks(count)), dim3(TX_THREADS), 0, s, keys, count, model, faces, F,
                       tex.uv, tex.mips, tex.Wt, tex.Ht, tex.levels, poses, cam, light, H, W, color, depth);
}

}  // namespace bp
