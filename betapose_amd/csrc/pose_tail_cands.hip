// Device pose tail over candidates (include/betapose_hip.h bp_pose_from_candidate_records, bp_cands_set_pose_solver): the
// twin of pipeline.finish_candidate_records, one frame per wave64 workgroup.
//
//   a. key-point decode of the frame's n valid candidates, f32 -- eval.decode_keypoints op for op (pose_decode.inc)
//   b. pPose-NMS over them, f32 -- bp::pose_nms (host_post.cpp, pPose_nms.py:24-122) for any n: the 0 -> 1e-5 score fix,
//      ref_dists and mean scores, the greedy loop (first-max pick; per remaining candidate the similarity
//      sum[d <= 1] tanh tanh + mu sum exp(-d / delta2) and the match count; the "nothing deleted" rule), the score-weighted
//      merge over the cluster with its min(ref_dist, 15) mask, the three filters and the proposal score
//   c. result[0] = the first merged pose that survives the filters; pruning to left_number key points
//   d. PnP, f64 -- pnp_wave (pnp_wave.inc)
//
// Numerical contract: no FMA contraction; one lane per key point for the per-point terms, which go to LDS and are summed
// in k order by every lane; sums over candidates run in cluster order (ascending candidate index: the host's id list only
// ever loses entries, so it stays sorted).  Pick, merged x / y / score and proposal score are bit-identical to bp_pose_nms.
// Only tanhf and expf may round differently from the host's libm, and they feed the comparison simi > gamma alone.
#include "bp_common.h"
#include "pose_tail.h"

#pragma clang fp contract(off)

namespace bp {

namespace {

#include "pnp_wave.inc"
#include "pose_decode.inc"

// records [frames][C][316] f32, counts [frames] -> poses [frames][166] f64, merged [frames][C][152] f32, info [frames][4] i32
__global__ __launch_bounds__(64) void pose_tail_cands_kernel(const float* __restrict__ records, const int* __restrict__ counts, int C,
                                                             const double* __restrict__ kp3d, PnpCam cam, int left_number,
                                                             double* __restrict__ poses, float* __restrict__ merged,
                                                             int* __restrict__ info) {
    __shared__ PnpShared sh;
    __shared__ float cx[PT_MAXC][PT_K], cy[PT_MAXC][PT_K], cs[PT_MAXC][PT_K];
    __shared__ float kx[PT_K], ky[PT_K], ks[PT_K];        // result[0]
    __shared__ float mx_[PT_K], my_[PT_K], ms_[PT_K];     // the merged pose being built
    __shared__ float t_sd[PT_K], t_ex[PT_K];
    __shared__ int t_near[PT_K], t_match[PT_K];
    __shared__ int kept[PT_K];
    const int lane = threadIdx.x;
    const float* recs = records + (size_t)blockIdx.x * C * PT_REC;
    double* out = poses + (size_t)blockIdx.x * PT_POSE;
    float* mrg = merged + (size_t)blockIdx.x * C * PT_MERGED;
    int* inf = info + (size_t)blockIdx.x * 4;
    int n = counts[blockIdx.x];
    n = n < 0 ? 0 : (n > C ? C : n);
    if (n == 0) {                      // no candidate
        write_status_row(out, lane, 1);
        if (lane < 4) inf[lane] = lane == 2 ? -1 : 0;
        return;
    }
    // ---- a. decode
    if (lane < PT_K)
        for (int c = 0; c < n; ++c) decode_kp(recs + (size_t)c * PT_REC, lane, &cx[c][lane], &cy[c][lane], &cs[c][lane]);
    wsync();
    // ---- b. pPose-NMS: the same sequential scans on every lane (uniform control flow)
    float ref_dists[PT_MAXC], human[PT_MAXC];
#pragma unroll
    for (int c = 0; c < PT_MAXC; ++c) {
        ref_dists[c] = 0.f;
        human[c] = 0.f;
        if (c < n) {
            const float* r = recs + (size_t)c * PT_REC;
            const float w = r[14] - r[12], h = r[15] - r[13];
            ref_dists[c] = 0.1f * fmaxs(w, h);
            float s = 0.f;
            for (int k = 0; k < PT_K; ++k) s += cs[c][k];
            human[c] = s / (float)PT_K;
        }
    }
    // greedy clustering: `ids` as a bit mask (ascending index = the host's list order)
    int pick[PT_MAXC], cluster[PT_MAXC], npick = 0;
#pragma unroll
    for (int j = 0; j < PT_MAXC; ++j) { pick[j] = 0; cluster[j] = 0; }
    if (n == 1) {
        pick[0] = 0; cluster[0] = 1; npick = 1;
    } else {
        unsigned ids = (1u << n) - 1u;
        while (ids) {
            int ref = -1;
            float hbest = 0.f, rd = 0.f;
#pragma unroll
            for (int c = 0; c < PT_MAXC; ++c)       // first maximum (a NaN never wins, as the host's >)
                if (((ids >> c) & 1u) && (ref < 0 || human[c] > hbest)) { hbest = human[c]; ref = c; rd = ref_dists[c]; }
            const float mlim = fmins(rd, 7.f);
            unsigned dele = 0;
            for (int c = 0; c < n; ++c) {
                if (!((ids >> c) & 1u)) continue;
                if (lane < PT_K) {
                    const float dx = cx[ref][lane] - cx[c][lane], dy = cy[ref][lane] - cy[c][lane];
                    const float d = sqrtf(dx * dx + dy * dy);
                    t_near[lane] = d <= 1.f;
                    t_sd[lane] = tanhf(cs[ref][lane] / 1.f) * tanhf(cs[c][lane] / 1.f);
                    t_ex[lane] = expf(-d / 2.65f);
                    t_match[lane] = (d / mlim) <= 1.f;
                }
                wsync();
                float sd = 0.f, ex = 0.f;
                int nmatch = 0;
                for (int k = 0; k < PT_K; ++k) {
                    if (t_near[k]) sd += t_sd[k];
                    ex += t_ex[k];
                    nmatch += t_match[k];
                }
                const float simi = sd + 1.7f * ex;
                if (simi > 22.48f || nmatch >= 5) dele |= 1u << c;
                wsync();
            }
            if (!dele) dele = 1u << ref;                                    // pPose_nms.py:63-64
#pragma unroll
            for (int j = 0; j < PT_MAXC; ++j)
                if (j == npick) { pick[j] = ref; cluster[j] = (int)dele; }
            ++npick;
            ids &= ~dele;
        }
    }
    // merge, filters, proposal score
    int m = 0, mask0 = 0;
    float prop0 = 0.f;
    for (int j = 0; j < npick; ++j) {
        int pk = 0, mid = 0;
#pragma unroll
        for (int q = 0; q < PT_MAXC; ++q)
            if (q == j) { pk = pick[q]; mid = cluster[q]; }
        float rd = 0.f;
#pragma unroll
        for (int c = 0; c < PT_MAXC; ++c)
            if (c == pk) rd = ref_dists[c];
        float mx = -HUGE_VALF;
        for (int k = 0; k < PT_K; ++k) mx = fmaxs(mx, cs[pk][k]);
        if (mx < 0.3f) continue;
        wsync();                       // the previous pose's scans are done before its terms are overwritten
        if (lane < PT_K) {
            if (n == 1) {
                mx_[lane] = cx[0][lane]; my_[lane] = cy[0][lane]; ms_[lane] = cs[0][lane];
            } else {
                const float lim = fmins(rd, 15.f);
                float wsum = 0.f;
                for (int c = 0; c < n; ++c) {
                    if (!((mid >> c) & 1)) continue;
                    const float dx = cx[pk][lane] - cx[c][lane], dy = cy[pk][lane] - cy[c][lane];
                    if (sqrtf(dx * dx + dy * dy) <= lim) wsum += cs[c][lane];
                }
                float px = 0.f, py = 0.f, sc = 0.f;
                for (int c = 0; c < n; ++c) {
                    if (!((mid >> c) & 1)) continue;
                    const float dx = cx[pk][lane] - cx[c][lane], dy = cy[pk][lane] - cy[c][lane];
                    const float msk = sqrtf(dx * dx + dy * dy) <= lim ? cs[c][lane] : 0.f;
                    const float nw = msk / wsum;
                    px += cx[c][lane] * nw;
                    py += cy[c][lane] * nw;
                    sc += msk * nw;
                }
                mx_[lane] = px; my_[lane] = py; ms_[lane] = sc;
            }
        }
        wsync();
        float ssum, smax;
        if (!merged_pose_scan(mx_, my_, ms_, &ssum, &smax)) continue;
        const float prop = proposal_score(ssum, smax, recs[(size_t)pk * PT_REC + 5]);
        float* o = mrg + (size_t)m * PT_MERGED;
        if (lane == 0) { o[0] = __int_as_float(pk); o[1] = prop; }
        if (lane < PT_K) {
            const float x = mx_[lane] - 0.3f, y = my_[lane] - 0.3f;
            o[2 + 3 * lane] = x; o[3 + 3 * lane] = y; o[4 + 3 * lane] = ms_[lane];
            if (m == 0) { kx[lane] = x; ky[lane] = y; ks[lane] = ms_[lane]; kept[lane] = 1; }
        }
        if (m == 0) { mask0 = mid; prop0 = prop; }
        ++m;
    }
    if (lane == 0) { inf[0] = n; inf[1] = m; inf[2] = m > 0 ? 0 : -1; inf[3] = mask0; }
    if (m == 0) {                      // every merged pose was filtered out
        write_status_row(out, lane, 2);
        return;
    }
    wsync();
    // ---- c. pruning, d. PnP on result[0]
    const int cnt = prune_and_compact(sh, kx, ky, ks, kept, kp3d, left_number, lane);
    double R[9], t[3];
    const int rc = pnp_wave(sh, cnt, cam, R, t);
    write_pose_row(out, lane, rc, cnt, R, t, prop0, kx, ky, ks);
}

}  // namespace

void launch_pose_tail_cands(const float* records, const int* counts, int frames, int C, const double* kp3d, const PnpCam& cam,
                            int left_number, double* poses, float* merged, int* info, hipStream_t s) {
    BP_CHECK(C >= 1 && C <= PT_MAXC, "candidate pose tail: 1 to 8 candidates per frame (BP_MAX_CANDIDATES)");
    hipLaunchKernelGGL(pose_tail_cands_kernel, dim3(frames), dim3(64), 0, s, records, counts, C, kp3d, cam, left_number, poses, merged,
                       info);
}

}  // namespace bp
