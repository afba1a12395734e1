// extern "C" boundary, the pose solvers: host PnP / RANSAC / pose NMS (host_post.cpp) and the stand-alone device pose
// tails (pose_tail*.hip, pnp_ransac.hip) -- see include/betapose_hip.h.
#include <vector>

#include "c_api_util.h"
#include "frame_chain.h"
#include "pose_tail.h"

extern "C" {

// ------------------------------------------------------------------ host post-processing
int bp_solve_pnp(const double* pts3d, const double* pts2d, int n, const double* K, double* R, double* t) {
    BP_TRY
    BP_CHECK(pts3d && pts2d && K && R && t, "null argument");
    const int rc = bp::solve_pnp(pts3d, pts2d, n, K, R, t);
    if (rc != 0) throw bp::Error("solve_pnp failed (need >= 6 non-degenerate points, or >= 4 coplanar ones)");
    return 0;
    BP_CATCH
}

int bp_solve_pnp_status(const double* pts3d, const double* pts2d, int n, const double* K, double* R, double* t, int* status) {
    BP_TRY
    BP_CHECK(pts3d && pts2d && K && R && t && status, "null argument");
    *status = bp::solve_pnp(pts3d, pts2d, n, K, R, t);
    return 0;
    BP_CATCH
}

int bp_solve_pnp_refined(const double* pts3d, const double* pts2d, int n, const double* K, double* R, double* t) {
    BP_TRY
    BP_CHECK(pts3d && pts2d && K && R && t, "null argument");
    const int rc = bp::solve_pnp_refined(pts3d, pts2d, n, K, R, t);
    if (rc != 0) throw bp::Error("solve_pnp_refined failed (need >= 6 non-degenerate points)");
    return 0;
    BP_CATCH
}

int bp_solve_pnp_ransac(const double* pts3d, const double* pts2d, int n, const double* K, double reproj_err,
                        int max_trials, double confidence, double* R, double* t, unsigned char* inliers) {
    BP_TRY
    BP_CHECK(pts3d && pts2d && K && R && t, "null argument");
    bp::check_ransac_params(reproj_err, max_trials, confidence);
    const int rc = bp::solve_pnp_ransac(pts3d, pts2d, n, K, reproj_err, max_trials, confidence, R, t, inliers);
    if (rc != 0) throw bp::Error("solve_pnp_ransac failed (need >= 6 points and a 6-point consensus)");
    return 0;
    BP_CATCH
}

int bp_pose_nms(const float* bboxes, const float* bbox_scores, const float* preds, const float* scores, int n, int K,
                int* out_pick, float* out_pose, float* out_score, float* out_prop) {
    BP_TRY
    BP_CHECK(n >= 0 && K >= 1, "bad sizes");
    BP_CHECK(n == 0 || (bboxes && bbox_scores && preds && scores && out_pick && out_pose && out_score && out_prop), "null argument");
    return bp::pose_nms(bboxes, bbox_scores, preds, scores, n, K, out_pick, out_pose, out_score, out_prop);
    BP_CATCH
}

// ------------------------------------------------------------------ device pose tails
int bp_pose_from_records(const float* d_records, int batch, const double* d_kp3d, int n_kp, const double* K,
                         int left_number, double* d_poses, void* stream) {
    BP_TRY
    BP_CHECK(d_records && d_kp3d && K && d_poses, "null argument");
    BP_CHECK(batch >= 0, "batch must be >= 0");
    bp::check_pose_points(n_kp, left_number);
    if (batch == 0) return 0;
    bp::launch_pose_tail(d_records, batch, d_kp3d, bp::make_pnp_cam(K), left_number, d_poses, (hipStream_t)stream);
    BP_HIP(hipGetLastError());
    return 0;
    BP_CATCH
}

int bp_pose_from_candidate_records(const float* d_records, const int* d_counts, int frames, int C, const double* d_kp3d, int n_kp,
                                   const double* K, int left_number, double* d_poses, float* d_merged, int* d_info, void* stream) {
    BP_TRY
    BP_CHECK(d_records && d_counts && d_kp3d && K && d_poses && d_merged && d_info, "null argument");
    BP_CHECK(frames >= 0, "frames must be >= 0");
    BP_CHECK(C >= 1 && C <= BP_MAX_CANDIDATES, "1 to 8 candidates per frame (BP_MAX_CANDIDATES)");
    bp::check_pose_points(n_kp, left_number);
    if (frames == 0) return 0;
    bp::launch_pose_tail_cands(d_records, d_counts, frames, C, d_kp3d, bp::make_pnp_cam(K), left_number, d_poses, d_merged, d_info,
                               (hipStream_t)stream);
    BP_HIP(hipGetLastError());
    return 0;
    BP_CATCH
}

int bp_pose_instances_from_merged(const float* d_merged, const int* d_info, const double* d_poses, int frames, int C,
                                  const double* d_kp3d, int n_kp, const double* K, int left_number, double* d_inst_poses,
                                  void* stream) {
    BP_TRY
    BP_CHECK(C >= 1 && C <= BP_MAX_CANDIDATES, "1 to 8 candidates per frame (BP_MAX_CANDIDATES)");
    BP_CHECK(d_merged && d_info && d_poses && d_kp3d && K && d_inst_poses, "null argument");
    BP_CHECK(frames >= 0 && frames <= 65535, "frames must be in [0, 65535]");
    bp::check_pose_points(n_kp, left_number);
    if (frames == 0) return 0;
    bp::launch_pose_instances(d_merged, d_info, d_poses, frames, C, d_kp3d, bp::make_pnp_cam(K), left_number, d_inst_poses,
                              (hipStream_t)stream);
    BP_HIP(hipGetLastError());
    return 0;
    BP_CATCH
}

int bp_solve_pnp_batch(const double* d_pts3d, int shared_3d, const double* d_pts2d, int n, int P, const double* K,
                       double* d_Rt, int* d_status, void* stream) {
    BP_TRY
    BP_CHECK(d_pts3d && d_pts2d && K && d_Rt && d_status, "null argument");
    BP_CHECK(n >= 0 && n <= BP_PNP_MAX_POINTS, "bp_solve_pnp_batch: n must be in [0, 64] points per problem");
    BP_CHECK(P >= 0, "P must be >= 0");
    if (P == 0) return 0;
    bp::launch_solve_pnp_batch(d_pts3d, shared_3d, d_pts2d, n, P, bp::make_pnp_cam(K), d_Rt, d_status, (hipStream_t)stream);
    BP_HIP(hipGetLastError());
    return 0;
    BP_CATCH
}

int bp_pnp_ransac_samples(int n, int max_trials, int* idx) {
    BP_TRY
    BP_CHECK(idx, "null argument");
    BP_CHECK(n >= 6 && max_trials >= 1, "bp_pnp_ransac_samples: needs n >= 6 points and max_trials >= 1");
    bp::pnp_ransac_samples(n, max_trials, idx);
    return 0;
    BP_CATCH
}

int bp_pnp_ransac_trials_needed(int n, double confidence, int* need) {
    BP_TRY
    BP_CHECK(need, "null argument");
    BP_CHECK(n >= 1 && confidence > 0 && confidence < 1, "bp_pnp_ransac_trials_needed: needs n >= 1 and a confidence in (0, 1)");
    bp::pnp_ransac_trials_needed(n, confidence, need);
    return 0;
    BP_CATCH
}

size_t bp_pnp_ransac_workspace_bytes(int P, int max_trials) {
    return P > 0 && max_trials > 0 ? bp::pnp_ransac_workspace_bytes(P, max_trials) : 0;
}

int bp_solve_pnp_ransac_batch(const double* d_pts3d, int shared_3d, const double* d_pts2d, int n, int P, const double* K,
                              double reproj_err, int max_trials, double confidence, double* d_Rt, int* d_status,
                              unsigned char* d_inliers, void* d_workspace, size_t workspace_bytes, void* stream) {
    BP_TRY
    BP_CHECK(d_pts3d && d_pts2d && K && d_Rt && d_status, "null argument");
    BP_CHECK(n >= 0 && n <= BP_PNP_MAX_POINTS, "bp_solve_pnp_ransac_batch: n must be in [0, 64] points per problem");
    BP_CHECK(P >= 0, "P must be >= 0");
    bp::check_ransac_params(reproj_err, max_trials, confidence);
    if (P == 0) return 0;
    BP_CHECK(d_workspace && workspace_bytes >= bp::pnp_ransac_workspace_bytes(P, max_trials),
             "bp_solve_pnp_ransac_batch: workspace smaller than bp_pnp_ransac_workspace_bytes(P, max_trials)");
    BP_CHECK(((uintptr_t)d_workspace & 7) == 0, "bp_solve_pnp_ransac_batch: workspace must be 8-byte aligned");
    std::vector<int> samples, need;
    bp::ransac_tables(n, max_trials, confidence, samples, need);
    bp::launch_pnp_ransac(d_pts3d, shared_3d ? 0 : (size_t)n * 3, d_pts2d, (size_t)n * 2, nullptr, n, P, bp::make_pnp_cam(K), reproj_err,
                          max_trials, samples.data(), need.data(), d_workspace, d_Rt, d_status, d_inliers, nullptr,
                          (hipStream_t)stream);
    BP_HIP(hipGetLastError());
    return 0;
    BP_CATCH
}

size_t bp_pose_ransac_workspace_bytes(int batch, int max_trials) {
    return batch > 0 && max_trials > 0 ? bp::pose_ransac_ws_bytes(batch, max_trials) : 0;
}

int bp_pose_from_records_ransac(const float* d_records, int batch, const double* d_kp3d, int n_kp, const double* K,
                                int left_number, double reproj_err, int max_trials, double confidence, double* d_poses,
                                void* d_workspace, size_t workspace_bytes, void* stream) {
    BP_TRY
    BP_CHECK(d_records && d_kp3d && K && d_poses, "null argument");
    BP_CHECK(batch >= 0, "batch must be >= 0");
    bp::check_pose_points(n_kp, left_number);
    bp::check_ransac_params(reproj_err, max_trials, confidence);
    if (batch == 0) return 0;
    BP_CHECK(d_workspace && workspace_bytes >= bp::pose_ransac_ws_bytes(batch, max_trials),
             "bp_pose_from_records_ransac: workspace smaller than bp_pose_ransac_workspace_bytes(batch, max_trials)");
    BP_CHECK(((uintptr_t)d_workspace & 7) == 0, "bp_pose_from_records_ransac: workspace must be 8-byte aligned");
    std::vector<int> samples, need;
    bp::ransac_tables(bp::pose_points(left_number), max_trials, confidence, samples, need);
    bp::pose_tail_ransac(d_records, batch, d_kp3d, bp::make_pnp_cam(K), left_number, reproj_err, max_trials, samples.data(), need.data(),
                     d_poses, d_workspace, (hipStream_t)stream);
    BP_HIP(hipGetLastError());
    return 0;
    BP_CATCH
}

}  // extern "C"
