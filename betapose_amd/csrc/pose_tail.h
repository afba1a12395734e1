// The pose tail's shared declarations: record constants (from include/betapose_hip.h), the launch-argument structs, the
// host solvers of host_post.cpp and the launchers of the pose units.  Included by the units that call them (c_api.cpp
// through frame_chain.h, c_api_pose.cpp, c_api_eval.cpp, eval_device.cpp) and by every unit that defines one of these
// functions, so a signature that drifts fails to compile.  Needs no HIP header (host_post.cpp also builds as plain C++):
// the stream type is declared as hip_runtime_api.h declares it.
#pragma once
#include <cmath>
#include <cstddef>

#include "../../include/betapose_hip.h"

typedef struct ihipStream_t* hipStream_t;

namespace bp {

constexpr int PT_MAXN = BP_PNP_MAX_POINTS;     // points per problem (one per lane)
constexpr int PT_K = 50;                       // key points per frame record
constexpr int PT_REC = BP_RESULT_FLOATS;       // floats per frame record
constexpr int PT_POSE = BP_POSE_DOUBLES;       // doubles per pose row
constexpr int PT_MERGED = BP_MERGED_FLOATS;    // floats per merged pose: pick (int bits), proposal score, 50 x (x, y, score)
constexpr int PT_MAXC = BP_MAX_CANDIDATES;     // candidates per frame
static_assert(PT_MAXN == 64, "one point per lane of a wave64");
static_assert(PT_REC == 16 + PT_K * BP_KP_FLOATS && PT_POSE == 16 + PT_K * 3 && PT_MERGED == 2 + PT_K * 3, "record layouts");

// camera and damping table of the PnP minimiser, host and device: lam[lg + 16] = 10^lg for lg = -16 .. 16, computed on the
// host by the one expression below so that every solver damps by the same numbers
struct PnpCam {
    double fx, fy, cx, cy;
    double lam[33];
};
inline PnpCam make_pnp_cam(const double* K) {   // K: 3x3 row-major, host memory
    PnpCam c;
    c.fx = K[0]; c.fy = K[4]; c.cx = K[2]; c.cy = K[5];
    for (int lg = -16; lg <= 16; ++lg) c.lam[lg + 16] = std::exp(lg * std::log(10.0));
    return c;
}

// launch arguments of the device RANSAC (pnp_ransac.hip), both filled on the host: the sample indices of up to TRIALS
// consecutive trials (pnp_ransac_samples; below 64, so a byte each) and the trials-needed table
// (pnp_ransac_trials_needed), passed by value so that a launch needs no upload and can be captured in a graph
struct RansacSamples {
    static constexpr int TRIALS = 256;
    unsigned char idx[TRIALS * 6];
};
struct RansacNeed {
    int need[PT_MAXN + 1];
};

// ---- host_post.cpp
int solve_pnp(const double* P, const double* U, int n, const double* K, double* R, double* t);
int solve_pnp_refined(const double* P, const double* U, int n, const double* K, double* R, double* t);
int solve_pnp_ransac(const double* P, const double* U, int n, const double* K, double reproj_err, int max_trials,
                     double confidence, double* R, double* t, unsigned char* inlier_mask);
void pnp_ransac_samples(int n, int max_trials, int* idx);
void pnp_ransac_trials_needed(int n, double confidence, int* need);
int pose_nms(const float* bboxes, const float* bbox_scores, const float* preds, const float* scores, int n, int K,
             int* out_pick, float* out_pose, float* out_score, float* out_prop);
// ---- pose_metrics.hip, pose_metrics_sym.hip
int pose_error_blocks(int n);
void launch_pose_errors(const double* model, int n, const double* gt, const double* est, int P, const double* K,
                        int want, double* partial, double* out, hipStream_t s);
size_t pose_errors_sym_scratch_bytes(int n, int P, int S);
void launch_pose_errors_sym(const double* model, int n, const double* gt, const double* est, int P, const double* sym,
                            int S, const double* K, int want, double* scratch, double* out, hipStream_t s);
// ---- eval_device.cpp: the two launches above with their scratch brought along (arguments checked by the caller); they
// return when the work is done
#pragma GCC visibility push(hidden)     // the library's own: not in its dynamic symbol table
void pose_errors(const double* model, int n, const double* gt, const double* est, int P, const double* K, int want,
                 double* out, hipStream_t s);
void pose_errors_sym(const double* model, int n, const double* gt, const double* est, int P, const double* sym, int S,
                     const double* K, int want, double* out, hipStream_t s);
#pragma GCC visibility pop
// ---- pose_tail.hip
void launch_solve_pnp_batch(const double* pts3d, int shared_3d, const double* pts2d, int n, int P, const PnpCam& cam,
                            double* Rt, int* status, hipStream_t s);
void launch_pose_tail(const float* records, int batch, const double* kp3d, const PnpCam& cam, int left_number,
                      double* poses, hipStream_t s);
void launch_pose_tail_prepare(const float* records, int batch, const double* kp3d, const PnpCam& cam, int left_number,
                              double* poses, double* ws3d, double* ws2d, int* active, hipStream_t s);
// ---- pose_tail_cands.hip
void launch_pose_tail_cands(const float* records, const int* counts, int frames, int C, const double* kp3d, const PnpCam& cam,
                            int left_number, double* poses, float* merged, int* info, hipStream_t s);
// ---- pose_tail_inst.hip
void launch_pose_instances(const float* merged, const int* info, const double* poses, int frames, int C, const double* kp3d,
                           const PnpCam& cam, int left_number, double* inst_poses, hipStream_t s);
// ---- pnp_ransac.hip
size_t pnp_ransac_workspace_bytes(int P, int max_trials);
void launch_pnp_ransac(const double* pts3d, size_t stride3d, const double* pts2d, size_t stride2d, const int* active, int n,
                       int P, const PnpCam& cam, double reproj_err, int max_trials, const int* samples, const int* need,
                       void* workspace, double* Rt, int* status, unsigned char* inliers, double* poses, hipStream_t s);

}  // namespace bp
