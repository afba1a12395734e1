// A pose for every merged candidate (include/betapose_hip.h bp_pose_instances_from_merged, bp_cands_set_instance_poses): the
// step after pose_tail_cands.hip, which solves result[0] alone.  One wave64 workgroup per (frame, slot j):
//
//   j = 0             the frame's existing pose row, copied whatever its status -- the PnP of result[0] is not repeated
//   0 < j < m         merged pose j: the left_number pruning (pose_decode.inc), pnp_wave (pnp_wave.inc), the row written as
//                     pose_tail_cands_kernel writes its own
//   j >= max(m, 1)    the "no candidate" row: status 1, NaN in R and t, zeros elsewhere
//
// No atomics, no traffic between waves: the instances of a frame run side by side.  Numerical contract: no FMA
// contraction; the same prune_and_compact and pnp_wave as the tail that produced `merged`, so an instance's R and t are
// what bp_solve_pnp_batch gives on its pruned points, bit for bit.
#include "bp_common.h"
#include "pose_tail.h"

#pragma clang fp contract(off)

namespace bp {

namespace {

#include "pnp_wave.inc"
#include "pose_decode.inc"

// merged [frames][C][152] f32, info [frames][4] i32, poses [frames][166] f64 -> inst [frames][C][166] f64
__global__ __launch_bounds__(64) void pose_instances_kernel(const float* __restrict__ merged, const int* __restrict__ info,
                                                            const double* __restrict__ poses, int C,
                                                            const double* __restrict__ kp3d, PnpCam cam, int left_number,
                                                            double* __restrict__ inst) {
    __shared__ PnpShared sh;
    __shared__ float kx[PT_K], ky[PT_K], ks[PT_K];
    __shared__ int kept[PT_K];
    const int lane = threadIdx.x;
    const int j = blockIdx.x, f = blockIdx.y;
    double* out = inst + ((size_t)f * C + j) * PT_POSE;
    int m = info[(size_t)f * 4 + 1];
    m = m < 0 ? 0 : (m > C ? C : m);
    if (j == 0) {
        const double* src = poses + (size_t)f * PT_POSE;
        for (int e = lane; e < PT_POSE; e += 64) out[e] = src[e];
        return;
    }
    if (j >= m) {                      // no merged pose in this slot
        write_status_row(out, lane, 1);
        return;
    }
    const float* mg = merged + ((size_t)f * C + j) * PT_MERGED;
    if (lane < PT_K) {
        kx[lane] = mg[2 + 3 * lane]; ky[lane] = mg[3 + 3 * lane]; ks[lane] = mg[4 + 3 * lane];
        kept[lane] = 1;
    }
    wsync();
    const int cnt = prune_and_compact(sh, kx, ky, ks, kept, kp3d, left_number, lane);
    double R[9], t[3];
    const int rc = pnp_wave(sh, cnt, cam, R, t);
    write_pose_row(out, lane, rc, cnt, R, t, mg[1], kx, ky, ks);
}

}  // namespace

void launch_pose_instances(const float* merged, const int* info, const double* poses, int frames, int C, const double* kp3d,
                           const PnpCam& cam, int left_number, double* inst_poses, hipStream_t s) {
    BP_CHECK(C >= 1 && C <= PT_MAXC, "instance poses: 1 to 8 candidates per frame (BP_MAX_CANDIDATES)");
    hipLaunchKernelGGL(pose_instances_kernel, dim3(C, frames), dim3(64), 0, s, merged, info, poses, C, kp3d, cam, left_number,
                       inst_poses);
}

}  // namespace bp
