// Depth refinement of estimated poses (projective point-to-plane ICP against the test depth image): the declarations
// shared by icp_host.cpp, icp.hip, eval_device.cpp and c_api_eval.cpp, so a signature that drifts fails to compile.  Needs
// no HIP header (icp_host.cpp is plain C++): the stream type is declared as hip_runtime_api.h declares it.
#pragma once
#include <cstddef>
#include <cstdint>

typedef struct ihipStream_t* hipStream_t;

namespace bp {

constexpr int ICP_ACC = 29;        // one accumulation: A's upper triangle row by row (21), b (6), N, E = sum r^2
constexpr int ICP_STATS = 6;       // N_first, rms_first, N_last, rms_last, iterations_done, status

// what one refinement is run with (include/betapose_hip.h bp_refine_depth)
struct IcpParams {
    double fx, fy, cx, cy, c;      // K and pixel_center
    double depth_scale;            // test depth = raw uint16 * depth_scale, 0 = missing
    double max_dist, min_cos;
    int min_pixels, iterations;
};

// ---- icp_host.cpp: the host twins.  depth_test [T][H][W]; test_index [P]; everything host memory.  Both return -1 for
// a face index outside [0, n), else 0.
int icp_normal_equations_host(const double* poses, int P, const double* vertices, int n, const int* faces, int F,
                              const double* K, const uint16_t* depth_test, int T, const int* test_index, int H, int W,
                              const IcpParams& prm, double near, double* out);
int refine_depth_host(const double* poses, int P, const double* vertices, int n, const int* faces, int F, const double* K,
                      const uint16_t* depth_test, int T, const int* test_index, int H, int W, const IcpParams& prm, double near,
                      double* poses_out, double* stats);

// ---- icp.hip
int icp_slices(int H, int W);      // pixel slices (blocks) per pose of the accumulate kernel
// poses_out [P][12] = poses_in, stats [P][ICP_STATS] = 0 with status RUNNING, or NO_IMAGE when test_index[p] is outside [0, T)
void launch_icp_init(const double* poses_in, const int* test_index, int T, int P, double* poses_out, double* stats,
                     hipStream_t s);
// partial [P][slices][ICP_ACC] of the renders zbuf [P][H][W] (cleared value +inf = nothing drawn) at poses [P][12].  A pose
// whose test index lies outside [0, T), or (stats != NULL) whose status is final, is skipped and its partials left alone.
void launch_icp_accumulate(const uint32_t* zbuf, const double* poses, int P, const uint16_t* depth_test, int T,
                           const int* test_index, int H, int W, const IcpParams& prm, const double* stats, double* partial,
                           hipStream_t s);
// out [P][ICP_ACC] = the slices of each pose summed in index order; zeros for a test index outside [0, T)
void launch_icp_sum(const double* partial, const int* test_index, int T, int P, int slices, double* out, hipStream_t s);
// accumulation number k (0 .. iterations) of every pose still running: sum, guards, solve, update of poses [P][12] and stats
void launch_icp_step(const double* partial, int P, int slices, int k, const IcpParams& prm, const double* poses_in,
                     double* poses, double* stats, hipStream_t s);

// ---- eval_device.cpp: the device drivers (arguments checked by the caller): the host twins' arguments on device
// pointers (K stays host) plus chunk (poses per pass, 0 = as many as keep the workspaces under 256 MB) and the stream.
// refine_depth enqueues the whole iteration loop of a chunk (render, accumulate, step) without a host round trip; both
// return when their work is done.
#pragma GCC visibility push(hidden)     // the library's own: not in its dynamic symbol table
void icp_normal_equations(const double* poses, int P, const double* model, int n, const int* faces, int F, const double* K,
                          const uint16_t* depth_test, int T, const int* test_index, int H, int W, const IcpParams& prm,
                          double near, int chunk, double* out, hipStream_t s);
void refine_depth(const double* poses, int P, const double* model, int n, const int* faces, int F, const double* K,
                  const uint16_t* depth_test, int T, const int* test_index, int H, int W, const IcpParams& prm, double near,
                  int chunk, double* poses_out, double* stats, hipStream_t s);
#pragma GCC visibility pop

}  // namespace bp
