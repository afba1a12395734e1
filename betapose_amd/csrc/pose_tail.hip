// Device pose tail (include/betapose_hip.h bp_pose_from_records, bp_pipeline_set_pose_solver, bp_solve_pnp_batch): the
// twin of pipeline.finish_record, one frame (or one PnP problem) per wave64 workgroup.
//
//   a. key-point decode, f32 -- eval.decode_keypoints (KPD/src/utils/eval.py:113-147, img.py:216-239) op for op
//   b. pPose-NMS at n = 1, f32 -- the n == 1 path of bp::pose_nms (host_post.cpp, pPose_nms.py:24-122)
//   c. pruning to left_number key points: the first minimum goes each time (np.argmin + np.delete, dataloader.py:718-722)
//   d. PnP, f64 -- solve_pnp_iterative of host_post.cpp (utils/utils.py:17-41): its O(1) arithmetic is the very text the
//      host compiles (pnp_math.inc), its sums over the points run in the host's order (pnp_wave.inc)
//
// Numerical contract: no FMA contraction (fp contract(off) on both sides), every sum accumulates in the host's order, and
// the eigen-solvers are the host's cyclic Jacobi with the same rotation order.  Only the transcendental functions (sin, cos,
// acos, hypot) may round differently from the host's libm; lambda = 10^lg of the minimiser comes from the one table both
// sides read (pose_tail.h make_pnp_cam).  So decode / NMS / pruning are bit-identical to the host and R, t agree to the
// rounding that the minimiser's FLT_EPSILON stop leaves.
//
// Wave layout: one lane per accumulator (a normal-matrix entry, a JtJ / JtErr entry), looping over the points in host
// order; one lane per point for the residuals and Jacobian rows (J in LDS); each Jacobi rotation's three k-loops spread
// over lanes; everything of O(1) size (3x3 polar factors, Rodrigues, the damped 6x6 solve, error norms) computed by
// every lane redundantly on the same LDS inputs, which keeps control flow uniform.
#include "bp_common.h"
#include "pose_tail.h"

#pragma clang fp contract(off)

namespace bp {

namespace {

#include "pnp_wave.inc"

// ---------------------------------------------------------------- kernels
__global__ __launch_bounds__(64) void solve_pnp_batch_kernel(const double* __restrict__ pts3d, int shared_3d,
                                                             const double* __restrict__ pts2d, int n, int P, PnpCam cam,
                                                             double* __restrict__ Rt, int* __restrict__ status) {
    __shared__ PnpShared sh;
    const int lane = threadIdx.x;
    const int p = blockIdx.x;
    if (p >= P) return;
    const double* p3 = pts3d + (shared_3d ? 0 : (size_t)p * n * 3);
    const double* p2 = pts2d + (size_t)p * n * 2;
    if (lane < n) {
#pragma unroll
        for (int k = 0; k < 3; ++k) sh.P[3 * lane + k] = p3[3 * lane + k];
        sh.U[2 * lane] = p2[2 * lane];
        sh.U[2 * lane + 1] = p2[2 * lane + 1];
    }
    wsync();
    double R[9], t[3];
    const int rc = pnp_wave(sh, n, cam, R, t);
    if (lane < 12) {
        const int r = lane / 4, c = lane % 4;
        const double v = c < 3 ? R[r * 3 + c] : t[r];
        Rt[(size_t)p * 12 + lane] = rc == 0 ? v : __builtin_nan("");
    }
    if (lane == 0) status[p] = rc;
}

#include "pose_decode.inc"

// one frame per workgroup: record [316] f32 -> pose row [166] f64 (layout: include/betapose_hip.h BP_POSE_DOUBLES).
// PREP (the RANSAC tail's first launch, pnp_ransac.hip): steps a-c as ever, then instead of step d the kept points go to
// ws3d [batch][64][3] / ws2d [batch][64][2] and active[frame] says whether a PnP problem was left (status 0 so far); the
// row is complete but for status / R / t / inlier set, which the select-and-refit launch writes.
template <bool PREP>
__global__ __launch_bounds__(64) void pose_tail_kernel(const float* __restrict__ records, const double* __restrict__ kp3d,
                                                       PnpCam cam, int left_number, double* __restrict__ poses,
                                                       double* __restrict__ ws3d, double* __restrict__ ws2d,
                                                       int* __restrict__ active) {
    __shared__ PnpShared sh;
    __shared__ float kx[PT_K], ky[PT_K], ks[PT_K];
    __shared__ int kept[PT_K];
    const int lane = threadIdx.x;
    const float* rec = records + (size_t)blockIdx.x * PT_REC;
    double* out = poses + (size_t)blockIdx.x * PT_POSE;
    const double qnan = __builtin_nan("");
    const int det = __float_as_int(rec[0]);
    if (det < 0) {                     // no detection
        write_status_row(out, lane, 1);
        if (PREP && lane == 0) active[blockIdx.x] = 0;
        return;
    }
    // ---- a. decode (eval.decode_keypoints, resH 80, resW 64, inpH 320, inpW 256)
    if (lane < PT_K) {
        decode_kp(rec, lane, &kx[lane], &ky[lane], &ks[lane]);
        kept[lane] = 1;
    }
    wsync();
    // ---- b. pPose-NMS, n = 1 (host pose_nms): the same sequential scans on every lane
    float mx = -HUGE_VALF;
    for (int k = 0; k < PT_K; ++k) mx = fmaxs(mx, ks[k]);
    float ssum, smax;
    const bool keep = merged_pose_scan(kx, ky, ks, &ssum, &smax) && !(mx < 0.3f);
    if (!keep) {                       // dropped by pPose-NMS
        write_status_row(out, lane, 2);
        if (PREP && lane == 0) active[blockIdx.x] = 0;
        return;
    }
    const float prop = proposal_score(ssum, smax, rec[5]);
    if (lane < PT_K) {
        kx[lane] = kx[lane] - 0.3f;
        ky[lane] = ky[lane] - 0.3f;
    }
    wsync();
    // ---- c. pruning: drop the first minimum score (np.argmin: a NaN is the minimum) until left_number remain
    const int cnt = prune_and_compact(sh, kx, ky, ks, kept, kp3d, left_number, lane);
    // ---- d. PnP (PREP: left to the RANSAC launches)
    double R[9], t[3];
    int rc = 0;
    if (PREP) {
        double* o3 = ws3d + (size_t)blockIdx.x * PT_MAXN * 3;
        double* o2 = ws2d + (size_t)blockIdx.x * PT_MAXN * 2;
        if (lane < cnt) {
#pragma unroll
            for (int k = 0; k < 3; ++k) o3[3 * lane + k] = sh.P[3 * lane + k];
            o2[2 * lane] = sh.U[2 * lane];
            o2[2 * lane + 1] = sh.U[2 * lane + 1];
        }
        if (lane == 0) active[blockIdx.x] = 1;
#pragma unroll
        for (int e = 0; e < 9; ++e) R[e] = qnan;
        t[0] = t[1] = t[2] = qnan;
        rc = -2;
    } else {
        rc = pnp_wave(sh, cnt, cam, R, t);
    }
    write_pose_row(out, lane, rc, cnt, R, t, prop, kx, ky, ks);
}

}  // namespace

void launch_solve_pnp_batch(const double* pts3d, int shared_3d, const double* pts2d, int n, int P, const PnpCam& cam,
                            double* Rt, int* status, hipStream_t s) {
    hipLaunchKernelGGL(solve_pnp_batch_kernel, dim3(P), dim3(64), 0, s, pts3d, shared_3d, pts2d, n, P, cam, Rt, status);
}

void launch_pose_tail(const float* records, int batch, const double* kp3d, const PnpCam& cam, int left_number,
                      double* poses, hipStream_t s) {
    hipLaunchKernelGGL(pose_tail_kernel<false>, dim3(batch), dim3(64), 0, s, records, kp3d, cam, left_number, poses,
                       (double*)nullptr, (double*)nullptr, (int*)nullptr);
}

void launch_pose_tail_prepare(const float* records, int batch, const double* kp3d, const PnpCam& cam, int left_number,
                              double* poses, double* ws3d, double* ws2d, int* active, hipStream_t s) {
    hipLaunchKernelGGL(pose_tail_kernel<true>, dim3(batch), dim3(64), 0, s, records, kp3d, cam, left_number, poses, ws3d,
                       ws2d, active);
}

}  // namespace bp
