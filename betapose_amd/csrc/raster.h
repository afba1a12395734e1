// Depth rasteriser and VSD: the declarations shared by raster_host.cpp, raster.hip, vsd.hip and c_api.cpp, so a signature
// that drifts fails to compile.  Needs no HIP header (raster_host.cpp is plain C++): the stream type is declared as
// hip_runtime_api.h declares it.
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
                   int nb, const double* K, int H, int W, double pixel_center, double near, void* vertex_ws, uint32_t* zbuf,
                   int* skipped, hipStream_t s);
// +inf -> 0 over `count` values, in place: the z-buffer becomes the public depth image
void launch_raster_finish(uint32_t* zbuf, size_t count, hipStream_t s);

// ---- vsd.hip
// acc [pairs][VSD_ACC] (zeroed by the caller) += the counts of pairs [0, pairs): zbuf holds the ground-truth renders
// [pairs][H][W] followed by the estimates' [pairs][H][W] (cleared value +inf = nothing drawn)
void launch_vsd_reduce(const uint32_t* zbuf, int pairs, const uint16_t* depth_test, int T, const int* test_index, int H, int W,
                       const double* K, double pixel_center, double depth_scale, double delta, const VsdTaus& taus, int n_tau,
                       double diameter, int* acc, hipStream_t s);
// err [P][n_tau], counts [P][4] from acc [P][VSD_ACC]; a pair whose test_index lies outside [0, T) gets NaN and -1
void launch_vsd_finish(const int* acc, const int* test_index, int T, int P, int n_tau, double* err, int* counts, hipStream_t s);

}  // namespace bp
