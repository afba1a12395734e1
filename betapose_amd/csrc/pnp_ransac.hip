// Device RANSAC PnP (include/betapose_hip.h bp_solve_pnp_ransac_batch, bp_pose_from_records_ransac,
// bp_pipeline_set_pose_ransac): the result of the host's sequential loop (host_post.cpp solve_pnp_ransac) with the
// hypotheses evaluated in parallel.
//
//   1. hypothesis kernel, grid (trials, P), one wave64 per (trial, problem): the trial's six sampled points -> pnp_wave
//      -> reprojection error of all n points -> 64-bit inlier mask and its count into the workspace.  Every trial up to
//      max_trials is evaluated, also those the host's early stop would not have run: they are independent of each other.
//   2. select-and-refit kernel, one wave per problem: replays the host loop over the recorded counts in trial order
//      (strict > keeps the first best; after each improvement the trial limit shrinks by the host's table need[cnt]),
//      so the trials past the host's stop are ignored; then compacts the winner's inliers in index order and runs
//      pnp_wave on them.
//
// What must equal the host exactly is integer: the sample indices (the host's table, passed by value in the launch
// arguments) and the trials-needed table (computed on the host with its own log / pow / ceil).  The f64 arithmetic is
// pnp_wave's and project_residuals', in the host's operation order without FMA contraction; the inlier test is written
// as the host writes it.  No atomics: each (problem, trial) owns its workspace slot.
#include "bp_common.h"
#include "pose_tail.h"

#pragma clang fp contract(off)

namespace bp {

namespace {

#include "pnp_wave.inc"

constexpr int RS_MS = 6;                   // sample size (the DLT initialiser needs six points)

// ---- 1. one hypothesis per wave.  masks / counts [P][max_trials]; active (may be null): problems with 0 are skipped.
__global__ __launch_bounds__(64) void pnp_ransac_hypothesis_kernel(const double* __restrict__ pts3d, size_t stride3d,
                                                                    const double* __restrict__ pts2d, size_t stride2d,
                                                                    const int* __restrict__ active, int n, PnpCam cam,
                                                                    double reproj_err, RansacSamples smp, int trial0,
                                                                    int max_trials, unsigned long long* __restrict__ masks,
                                                                    int* __restrict__ counts) {
    __shared__ PnpShared sh;
    __shared__ double fP[PT_MAXN * 3], fU[PT_MAXN * 2];
    const int lane = threadIdx.x;
    const int it = trial0 + blockIdx.x, p = blockIdx.y;
    if (it >= max_trials) return;
    if (active && !active[p]) return;
    const double* p3 = pts3d + (size_t)p * stride3d;
    const double* p2 = pts2d + (size_t)p * stride2d;
    if (lane < n) {
#pragma unroll
        for (int k = 0; k < 3; ++k) fP[3 * lane + k] = p3[3 * lane + k];
        fU[2 * lane] = p2[2 * lane];
        fU[2 * lane + 1] = p2[2 * lane + 1];
    }
    wsync();
    if (lane < RS_MS) {
        int src = smp.idx[blockIdx.x * RS_MS + lane];
        src = src < n ? src : 0;           // (the host's table holds indices below n)
#pragma unroll
        for (int k = 0; k < 3; ++k) sh.P[3 * lane + k] = fP[3 * src + k];
        sh.U[2 * lane] = fU[2 * src];
        sh.U[2 * lane + 1] = fU[2 * src + 1];
    }
    wsync();
    double R[9], t[3], prm[6];
    const int rc = pnp_wave(sh, RS_MS, cam, R, t);
    unsigned long long mask = 0;
    if (rc == 0) {                         // (a failed hypothesis counts as no inliers: the host's `continue`)
        pose_to_params(R, t, prm);
        wsync();
        if (lane < n) {
#pragma unroll
            for (int k = 0; k < 3; ++k) sh.P[3 * lane + k] = fP[3 * lane + k];
            sh.U[2 * lane] = fU[2 * lane];
            sh.U[2 * lane + 1] = fU[2 * lane + 1];
        }
        wsync();
        project_residuals(sh, n, cam, prm, false);
        bool in = false;
        if (lane < n) {
            const double ex = sh.err[2 * lane], ey = sh.err[2 * lane + 1];
            in = ex * ex + ey * ey <= reproj_err * reproj_err;
        }
        mask = __ballot(in);
    }
    if (lane == 0) {
        masks[(size_t)p * max_trials + it] = mask;
        counts[(size_t)p * max_trials + it] = __popcll(mask);
    }
}

// ---- 2. the host's loop over the counts, then the refit on the winner's inliers.
// Rt [P][12] / status [P] / inliers [P][n] (may be null): the batch form.  poses (non-null): the pose-tail form, which
// writes slots 0 (status), 2..13 (R, t) and 15 (inlier set) of the frame's pose row instead: a partial write of the layout
// that write_pose_row (pose_decode.inc) documents; the prepare launch wrote the whole row through it.
__global__ __launch_bounds__(64) void pnp_ransac_select_kernel(const double* __restrict__ pts3d, size_t stride3d,
                                                                const double* __restrict__ pts2d, size_t stride2d,
                                                                const int* __restrict__ active, int n, PnpCam cam,
                                                                RansacNeed need, int max_trials,
                                                                const unsigned long long* __restrict__ masks,
                                                                const int* __restrict__ counts, double* __restrict__ Rt,
                                                                int* __restrict__ status, unsigned char* __restrict__ inliers,
                                                                double* __restrict__ poses) {
    __shared__ PnpShared sh;
    __shared__ int s_cnt[64], s_need[PT_MAXN + 1];
    const int lane = threadIdx.x;
    const int p = blockIdx.x;
    if (active && !active[p]) return;      // pose-tail form: the row of a frame without a PnP problem is complete
    const double* p3 = pts3d + (size_t)p * stride3d;
    const double* p2 = pts2d + (size_t)p * stride2d;
    int rc;
    unsigned long long mask = 0;
    double R[9], t[3];
    if (n < RS_MS) {
        rc = -1;
    } else {
        int m = n;                         // points of the refit
        if (n == RS_MS) {                  // the host skips the trials
            mask = (1ull << RS_MS) - 1;
        } else {
            for (int e = lane; e <= n; e += 64) s_need[e] = need.need[e];
            int best_cnt = 0, best_it = -1, trials = max_trials;
            for (int c0 = 0; c0 < trials; c0 += 64) {
                wsync();
                s_cnt[lane] = c0 + lane < max_trials ? counts[(size_t)p * max_trials + c0 + lane] : 0;
                wsync();
                for (int j = 0; j < 64 && c0 + j < trials; ++j) {
                    const int it = c0 + j, cnt = s_cnt[j];
                    if (cnt > best_cnt) {
                        best_cnt = cnt;
                        best_it = it;
                        const int nd = s_need[cnt];
                        if (nd < trials) trials = it + 1 > nd ? it + 1 : nd;
                    }
                }
            }
            m = best_cnt;
            if (best_cnt >= RS_MS) mask = masks[(size_t)p * max_trials + best_it];
        }
        if (m < RS_MS) {
            rc = -2;
            mask = 0;
        } else {
            wsync();
            if (lane < n && ((mask >> lane) & 1ull)) {
                const int j = __popcll(mask & ((1ull << lane) - 1ull));
#pragma unroll
                for (int k = 0; k < 3; ++k) sh.P[3 * j + k] = p3[3 * lane + k];
                sh.U[2 * j] = p2[2 * lane];
                sh.U[2 * j + 1] = p2[2 * lane + 1];
            }
            wsync();
            rc = pnp_wave(sh, m, cam, R, t);
        }
    }
    const double qnan = __builtin_nan("");
    if (poses) {
        double* out = poses + (size_t)p * PT_POSE;
        if (lane < 12) out[2 + lane] = rc == 0 ? (lane < 9 ? R[lane] : t[lane - 9]) : qnan;
        if (lane == 12) out[0] = (double)rc;
        if (lane == 13) out[15] = (double)mask;        // at most 50 bits: exact
        return;
    }
    if (lane < 12) {
        const int r = lane / 4, c = lane % 4;
        const double v = c < 3 ? R[r * 3 + c] : t[r];
        Rt[(size_t)p * 12 + lane] = rc == 0 ? v : qnan;
    }
    if (lane == 0) status[p] = rc;
    if (inliers && lane < n) inliers[(size_t)p * n + lane] = (unsigned char)((mask >> lane) & 1ull);
}

}  // namespace

// masks [P][max_trials] u64, then counts [P][max_trials] i32
size_t pnp_ransac_workspace_bytes(int P, int max_trials) {
    return (size_t)P * max_trials * (sizeof(unsigned long long) + sizeof(int));
}

// samples: the host's table [max_trials][6] (pnp_ransac_samples for this n); need: [n + 1] (pnp_ransac_trials_needed).
// stride3d = 0 shares one set of 3-D points.  Nothing but launches: capturable, no allocation, no host round trip.
void launch_pnp_ransac(const double* pts3d, size_t stride3d, const double* pts2d, size_t stride2d, const int* active, int n,
                       int P, const PnpCam& cam, double reproj_err, int max_trials, const int* samples, const int* need,
                       void* workspace, double* Rt, int* status, unsigned char* inliers, double* poses, hipStream_t s) {
    unsigned long long* masks = (unsigned long long*)workspace;
    int* counts = (int*)(masks + (size_t)P * max_trials);
    if (n > RS_MS) {
        for (int t0 = 0; t0 < max_trials; t0 += RansacSamples::TRIALS) {
            const int nt = max_trials - t0 < RansacSamples::TRIALS ? max_trials - t0 : RansacSamples::TRIALS;
            RansacSamples smp;
            for (int e = 0; e < nt * RS_MS; ++e) smp.idx[e] = (unsigned char)samples[(size_t)t0 * RS_MS + e];
            for (int e = nt * RS_MS; e < RansacSamples::TRIALS * RS_MS; ++e) smp.idx[e] = 0;
            hipLaunchKernelGGL(pnp_ransac_hypothesis_kernel, dim3(nt, P), dim3(64), 0, s, pts3d, stride3d, pts2d, stride2d,
                               active, n, cam, reproj_err, smp, t0, max_trials, masks, counts);
        }
    }
    RansacNeed nd;
    for (int e = 0; e <= PT_MAXN; ++e) nd.need[e] = e <= n && need ? need[e] : 0x7fffffff;
    hipLaunchKernelGGL(pnp_ransac_select_kernel, dim3(P), dim3(64), 0, s, pts3d, stride3d, pts2d, stride2d, active, n, cam,
                       nd, max_trials, masks, counts, Rt, status, inliers, poses);
}

}  // namespace bp
