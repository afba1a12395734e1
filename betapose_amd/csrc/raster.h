// Depth and colour rasterisers and VSD: the declarations shared by raster_host.cpp, raster.hip, raster_color_host.cpp,
// raster_color.hip, raster_texture_host.cpp, raster_texture.hip, vsd.hip, eval_device.cpp and c_api_eval.cpp, so a signature that drifts fails to compile.  Needs no HIP
// header (the host twins are plain C++): the stream type is declared as hip_runtime_api.h declares it.  The loop over a
// pose's triangles and their pixels belongs to none of those files: it is raster_walk.inc, which the four raster units
// include.
#pragma once
#include <cstddef>
#include <cstdint>

typedef struct ihipStream_t* hipStream_t;

namespace bp {

constexpr int VSD_MAX_TAUS = 16;
constexpr int VSD_ACC = 4 + VSD_MAX_TAUS;      // ints per pair: rendered_gt, visib_gt, inter, union, one count per tau

struct VsdTaus {
    double tau[VSD_MAX_TAUS];
};

// the rasterisers' camera (raster_math.inc), built here and nowhere else
struct RsCam {
    double fx, fy, cx, cy;
    double c;       // pixel_center
    double near;    // vertices with z < near make their triangles skipped
};
inline RsCam raster_cam(const double* K, double pixel_center, double near) {      // K 3x3 row-major
    return RsCam{K[0], K[4], K[2], K[5], pixel_center, near};
}

// ---- raster_host.cpp: the host twin of launch_render_depth.  poses [P][12], vertices [n][3], faces [F][3], K 3x3, all
// host; depth [P][H][W] (0 where nothing was drawn), skipped [P].  Returns -1 for a face index outside [0, n), else 0.
int render_depth_host(const double* poses, int P, const double* vertices, int n, const int* faces, int F, const double* K,
                      int H, int W, double pixel_center, double near, float* depth, int* skipped);

// ---- raster.hip
// bytes of the per-vertex workspace (camera-space xyz + snapped uv) of `poses` poses of an n-vertex mesh
size_t raster_vertex_bytes(int n, int poses);
// Draws poses_a[0 .. na) and then poses_b[0 .. nb) (poses_b may be NULL with nb == 0) into zbuf [(na + nb)][H][W], f32
// bit patterns that the caller has cleared to +inf, and ADDS the skipped triangles of each to skipped [(na + nb)].
void launch_raster(const double* model, int n, const int* faces, int F, const double* poses_a, int na, const double* poses_b,
                   int nb, const RsCam& cam, int H, int W, void* vertex_ws, uint32_t* zbuf, int* skipped, hipStream_t s);
// +inf -> 0 over `count` values, in place: the z-buffer becomes the public depth image
void launch_raster_finish(uint32_t* zbuf, size_t count, hipStream_t s);
// launch_raster's first half, which the colour renderer launches alone: the camera-space xyz and the snapped uv of the
// na + nb poses into vertex_ws (raster_vertex_bytes(n, na + nb): xyz [na + nb][n][3] f64, then uv [na + nb][n][2] i32)
void launch_raster_transform(const double* model, int n, const double* poses_a, int na, const double* poses_b, int nb,
                             const RsCam& cam, void* vertex_ws, hipStream_t s);

// ---- raster_color_host.cpp: the host twins of the colour renderer (raster_color.hip), all pointers host.  colors
// [n][3] u8, image_index [P] or NULL (pose p -> image p), light [3]; color [I][H][W][3] u8, depth [I][H][W] f32.
// render_color_host returns -1 for a face index outside [0, n), else 0.
int render_color_host(const double* poses, int P, const double* vertices, int n, const int* faces, int F,
                      const unsigned char* colors, const int* image_index, int I, const double* K, int H, int W,
                      double pixel_center, double near, double ambient, const double* light, int accumulate,
                      unsigned char* color, float* depth, int* skipped);
// render_color_host's first half, which the textured twin runs too: keys [I][H][W] <- the z-test of every pose (with
// `accumulate` over the kept keys of depth [I][H][W]), skipped [P].  The face indices have been checked.
void color_visibility_host(const double* poses, int P, const double* vertices, int n, const int* faces, int F,
                           const int* image_index, int I, const RsCam& cam, int H, int W, int accumulate, const float* depth,
                           unsigned long long* keys, int* skipped);
void draw_boxes_host(const double* poses, int P, const double* corners, const unsigned char* corner_colors,
                     const int* image_index, int I, const double* K, int H, int W, double pixel_center, double near,
                     unsigned char* color);
void overlay_host(const unsigned char* frames, const unsigned char* color, const float* depth, int I, int H, int W, int alpha,
                  unsigned char* out);

// ---- raster_color.hip
struct ColorLight {
    double ambient;
    double x, y, z;     // light position in camera space
};
constexpr unsigned long long COLOR_MAX_IDS = 0xFFFFFFFEull;     // P * F above this is refused: fragment ids stay below 2^32 - 1
// keys [images][H][W] u64 <- the empty key, or with `accumulate` the kept key of every pixel of depth [images][H][W]
// that holds something
void launch_color_clear(unsigned long long* keys, const float* depth, int accumulate, size_t count, hipStream_t s);
// z-test of poses [q0, q0 + count) of the call (vertex_ws: their launch_raster_transform) into keys, whose first image is
// image img0 of the call; d_image_index [P] of the call or NULL; fragment ids are (call's pose slot) * F + face.  ADDS the
// skipped triangles to skipped[q0 ..].
void launch_color_visibility(const int* faces, int F, int n, const void* vertex_ws, int q0, int count,
                             const int* d_image_index, int img0, const RsCam& cam, int H, int W, unsigned long long* keys,
                             int* skipped, hipStream_t s);
// colour and depth of `images` images from their keys: the winner shaded from model, faces, colors and the call's poses
void launch_color_resolve(const unsigned long long* keys, int images, const double* model, const int* faces, int F,
                          const unsigned char* colors, const double* poses, const RsCam& cam, int H, int W,
                          const ColorLight& light, unsigned char* color, float* depth, hipStream_t s);
// the 12 box edges of poses [q0, q0 + count) of the call over color, whose first image is image img0 of the call; ids
// [images][H][W] u32 is scratch that the call clears itself
void launch_draw_boxes(const double* poses, int q0, int count, const double* corners, const unsigned char* corner_colors,
                       const int* d_image_index, int img0, int images, const RsCam& cam, int H, int W, uint32_t* ids,
                       unsigned char* color, hipStream_t s);
void launch_overlay(const unsigned char* frames, const unsigned char* color, const float* depth, size_t pixels, int alpha,
                    unsigned char* out, hipStream_t s);

// ---- raster_texture_host.cpp / raster_texture.hip: a texture in the place of the vertex colours
struct ColorTexture {
    const double* uv;        // [F][3][2]: (u, v) of every face corner, v upwards
    const uint32_t* mips;    // the packed pyramid of a Wt x Ht image, one dword a texel
    int Wt, Ht;
    int levels;              // levels the resolve may read, 1 .. texture_full_levels (1: the image alone)
};
int texture_max_size();                                     // Wt, Ht above this are refused
int texture_full_levels(int Wt, int Ht);                    // 1 + ceil(log2(max(Wt, Ht)))
size_t texture_mips_texels(int Wt, int Ht, int levels);     // dwords of the first `levels` levels
// mips <- the first `levels` levels of image [Ht][Wt][3] u8
void texture_mips_host(const unsigned char* image, int Wt, int Ht, int levels, uint32_t* mips);
void launch_texture_mips(const unsigned char* image, int Wt, int Ht, int levels, uint32_t* mips, hipStream_t s);
// render_color_host with the textured resolve
int render_color_textured_host(const double* poses, int P, const double* vertices, int n, const int* faces, int F,
                               const ColorTexture& tex, const int* image_index, int I, const double* K, int H, int W,
                               double pixel_center, double near, double ambient, const double* light, int accumulate,
                               unsigned char* color, float* depth, int* skipped);
// launch_color_resolve with the textured fragment
void launch_color_resolve_tex(const unsigned long long* keys, int images, const double* model, const int* faces, int F,
                              const ColorTexture& tex, const double* poses, const RsCam& cam, int H, int W,
                              const ColorLight& light, unsigned char* color, float* depth, hipStream_t s);

// ---- vsd.hip
// acc [pairs][VSD_ACC] (zeroed by the caller) += the counts of pairs [0, pairs): zbuf holds the ground-truth renders
// [pairs][H][W] followed by the estimates' [pairs][H][W] (cleared value +inf = nothing drawn)
void launch_vsd_reduce(const uint32_t* zbuf, int pairs, const uint16_t* depth_test, int T, const int* test_index, int H, int W,
                       const double* K, double pixel_center, double depth_scale, double delta, const VsdTaus& taus, int n_tau,
                       double diameter, int* acc, hipStream_t s);
// err [P][n_tau], counts [P][4] from acc [P][VSD_ACC]; a pair whose test_index lies outside [0, T) gets NaN and -1
void launch_vsd_finish(const int* acc, const int* test_index, int T, int P, int n_tau, double* err, int* counts, hipStream_t s);

// ---- eval_device.cpp: the device drivers, one per device call of include/betapose_hip.h (arguments checked by the
// caller).  The host twins' arguments on device pointers (image_index, K, light and taus stay host) plus the stream;
// chunk: poses per pass, 0 = as many as keep the workspaces under 256 MB.  A driver that needs a workspace returns when its work is done; the others only enqueue.
#pragma GCC visibility push(hidden)     // the library's own: not in its dynamic symbol table
void render_depth(const double* poses, int P, const double* model, int n, const int* faces, int F, const double* K, int H,
                  int W, double pixel_center, double near, float* depth, int* skipped, hipStream_t s);
// (tex: NULL shades from colors, otherwise from the texture and colors is not read)
void render_color(const double* poses, int P, const double* model, int n, const int* faces, int F, const unsigned char* colors,
                  const int* image_index, int I, const double* K, int H, int W, double pixel_center, double near,
                  double ambient, const double* light, int accumulate, unsigned char* color, float* depth, int* skipped,
                  hipStream_t s, const ColorTexture* tex = nullptr);
void draw_boxes(const double* poses, int P, const double* corners, const unsigned char* corner_colors, const int* image_index,
                int I, const double* K, int H, int W, double pixel_center, double near, unsigned char* color, hipStream_t s);
void overlay(const unsigned char* frames, const unsigned char* color, const float* depth, int I, int H, int W, int alpha,
             unsigned char* out, hipStream_t s);
void vsd_errors(const double* model, int n, const int* faces, int F, const double* gt, const double* est, int P, const double* K,
                const uint16_t* depth_test, int T, int H, int W, double depth_scale, const int* test_index, double delta,
                const double* taus, int n_tau, double diameter, double pixel_center, double near, int chunk, double* err,
                int* counts, hipStream_t s);
#pragma GCC visibility pop

}  // namespace bp
