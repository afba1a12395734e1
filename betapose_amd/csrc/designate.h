// Key-point designator (stage 1 of the reference): the declarations shared by designate_host.cpp, designate.hip,
// eval_device.cpp and c_api_eval.cpp, so a signature that drifts fails to compile.  Needs no HIP header
// (designate_host.cpp is plain C++): the stream type is declared as hip_runtime_api.h declares it.
#pragma once
#include <cstddef>
#include <cstdint>

typedef struct ihipStream_t* hipStream_t;

#define DESIGNATE_MAX_SCALES 12     // scales of one octave (the kernels keep 2 accumulators per scale in registers)

namespace bp {

constexpr int DESIGNATE_MAX_K = 64;             // neighbours of the extremum test (64 lists of (d2, index) in LDS)
constexpr int DESIGNATE_MAX_OCTAVE = 1 << 17;   // points of one octave: all pairs, 2^34 at the limit
constexpr int DESIGNATE_MAX_FPS = 1 << 20;      // points of farthest_points
constexpr int DESIGNATE_MAX_THIN = 1 << 14;     // points of thin_points

// ---- designate_host.cpp: the host twins, all pointers host
// out [n][3], *n_out <= n
void voxel_grid_host(const double* points, int n, double leaf, double* out, int* n_out);
// dog [n][ns-1], flags [n][ns-3]
void sift_octave_host(const double* points, int n, int field, const double* scales, int ns, int k, double min_contrast,
                      double* dog, signed char* flags);
// start < 0: the point farthest from the centroid.  idx [K], d2 [K]
void farthest_points_host(const double* points, int n, int K, int start, int* idx, double* d2);
// alive [n] (1 = survivor), state [2] = (rounds done, carried position)
void thin_points_host(const double* points, int n, int keep, unsigned char* alive, int* state);

// ---- designate.hip: the same on device pointers, enqueued on s (scales stays host)
void launch_sift_octave(const double* points, int n, int field, const double* scales, int ns, int k, double min_contrast,
                        double* dog, signed char* flags, hipStream_t s);
// mind [n] is scratch that the launch initialises itself
void launch_farthest_points(const double* points, int n, int K, int start, double* mind, int* idx, double* d2, hipStream_t s);
// nn_d [n], nn_j [n], list [n] likewise
void launch_thin_points(const double* points, int n, int keep, double* nn_d, int* nn_j, int* list, unsigned char* alive,
                        int* state, hipStream_t s);

// ---- eval_device.cpp: the device drivers (arguments checked by the caller).  The octave only enqueues; the other two
// bring their scratch and return when their work is done.
#pragma GCC visibility push(hidden)     // the library's own: not in its dynamic symbol table
void sift_octave(const double* d_points, int n, int field, const double* scales, int ns, int k, double min_contrast,
                 double* d_dog, signed char* d_flags, hipStream_t s);
void farthest_points(const double* d_points, int n, int K, int start, int* d_idx, double* d_d2, hipStream_t s);
void thin_points(const double* d_points, int n, int keep, unsigned char* d_alive, int* d_state, hipStream_t s);
#pragma GCC visibility pop

}  // namespace bp
