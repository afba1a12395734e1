// Pieces shared by the device pose tails (pose_tail.hip, pose_tail_cands.hip, pose_tail_inst.hip): the key-point decode,
// the scan and filters of a merged pose, the left_number pruning and the writers of the pose row.  Included inside
// `namespace bp { namespace {` after pnp_wave.inc, in a unit that has `#pragma clang fp contract(off)` in force.

__device__ __forceinline__ float sign_np(float v) { return v > 0.f ? 1.f : (v < 0.f ? -1.f : (v == 0.f ? 0.f : v)); }
__device__ __forceinline__ float max_np(float a, float b) { return (a != a) ? a : ((b != b) ? b : (a >= b ? a : b)); }

// key point `k` of one 316-float record (eval.decode_keypoints, resH 80, resW 64, inpH 320, inpW 256) -> image x, y and
// the score with pose_nms' 0 -> 1e-5 fix (pPose_nms.py:33)
__device__ __forceinline__ void decode_kp(const float* __restrict__ rec, int k, float* ox, float* oy, float* os) {
    const float* kp = rec + 16 + k * 6;
    const int idx = __float_as_int(kp[0]);
    const float maxval = kp[1];
    int xm = idx % 64;
    if (xm < 0) xm += 64;
    const int yq = (idx - xm) / 64;          // floor division, as numpy
    float x = (float)xm, y = (float)yq;
    const bool pos = maxval > 0;
    x = pos ? x : 0.f;
    y = pos ? y : 0.f;
    const bool inner = (x > 0.f) && (x < 63.f) && (y > 0.f) && (y < 79.f);
    const float sx = sign_np(kp[3] - kp[2]), sy = sign_np(kp[5] - kp[4]);
    x = x + (inner ? sx * 0.25f : 0.f);
    y = y + (inner ? sy * 0.25f : 0.f);
    const float px = x + 0.2f, py = y + 0.2f;
    // transformBoxInvert_batch (KPD/src/utils/img.py:216-239); F32(320 / 256) = 1.25f, F32(256 / 320) = 0.8f
    const float ulx = rec[8], uly = rec[9], brx = rec[10], bry = rec[11];
    const float cenx = ((brx - 1.f) - ulx) / 2.f, ceny = ((bry - 1.f) - uly) / 2.f;
    const float sizex = (brx - ulx) * 1.25f, sizey = bry - uly;
    const float lenH = max_np(sizex, sizey);
    const float lenW = lenH * 0.8f;
    const float ptx = (px * lenH) / 80.f, pty = (py * lenH) / 80.f;
    const float dx = max_np((lenW - 1.f) / 2.f - cenx, 0.f);
    const float dy = max_np((lenH - 1.f) / 2.f - ceny, 0.f);
    *ox = (ptx - dx) + ulx;
    *oy = (pty - dy) + uly;
    *os = maxval == 0.f ? 1e-5f : maxval;   // pPose_nms.py:33
}

// pruning: drop the first minimum score (np.argmin: a NaN is the minimum) until left_number remain, then compact the kept
// points in their original order into sh.P (from kp3d) / sh.U (f64 from the f32 key points).  kept[] must be all ones on
// entry (and visible to the wave); returns the number of points kept.
__device__ __forceinline__ int prune_and_compact(PnpShared& sh, const float* kx, const float* ky, const float* ks, int* kept,
                                                 const double* __restrict__ kp3d, int left_number, int lane) {
    int cnt = PT_K;
    while (cnt > left_number && cnt > 0) {
        int d = -1;
        for (int k = 0; k < PT_K; ++k) {
            if (!kept[k]) continue;
            if (d < 0) { d = k; continue; }
            const float b = ks[d], s = ks[k];
            if (b != b) continue;
            if (s != s || s < b) d = k;
        }
        wsync();
        if (lane == 0) kept[d] = 0;
        wsync();
        --cnt;
    }
    // compact the kept points in their original order: 2-D in f64 from the f32 key points, 3-D from kp3d
    if (lane < PT_K && kept[lane]) {
        int j = 0;
        for (int k = 0; k < lane; ++k) j += kept[k];
        sh.P[3 * j] = kp3d[3 * lane];
        sh.P[3 * j + 1] = kp3d[3 * lane + 1];
        sh.P[3 * j + 2] = kp3d[3 * lane + 2];
        sh.U[2 * j] = (double)kx[lane];
        sh.U[2 * j + 1] = (double)ky[lane];
    }
    wsync();
    return cnt;
}

// the end of pose_nms for one merged pose x / y / s [PT_K] (host_post.cpp, pPose_nms.py:85-110): max and sum of the scores,
// bounding box, the score and area filters; the same sequential scan on every lane.  false: the pose is dropped.
__device__ __forceinline__ bool merged_pose_scan(const float* x, const float* y, const float* s, float* ssum_out, float* smax_out) {
    float smax = -HUGE_VALF, ssum = 0.f, xmin = HUGE_VALF, xmax = -HUGE_VALF, ymin = HUGE_VALF, ymax = -HUGE_VALF;
    for (int k = 0; k < PT_K; ++k) {
        smax = fmaxs(smax, s[k]); ssum += s[k];
        xmin = fmins(xmin, x[k]); xmax = fmaxs(xmax, x[k]);
        ymin = fmins(ymin, y[k]); ymax = fmaxs(ymax, y[k]);
    }
    *ssum_out = ssum;
    *smax_out = smax;
    return !(smax < 0.3f) && !(1.5f * 1.5f * (xmax - xmin) * (ymax - ymin) < 0.f);
}
__device__ __forceinline__ float proposal_score(float ssum, float smax, float box_score) {
    return ssum / (float)PT_K + box_score + 1.25f * smax;
}

// ---- the pose row [PT_POSE] f64 (include/betapose_hip.h BP_POSE_DOUBLES): 0 status, 1 points kept, 2..10 R, 11..13 t
// (NaN unless status 0), 14 proposal score, 15 RANSAC inlier set (0 here), 16.. the 50 key points (x, y, score).
// pnp_ransac.hip's select kernel rewrites slots 0, 2..13 and 15 of a row that the prepare launch wrote through here.
__device__ __forceinline__ void write_pose_row(double* __restrict__ out, int lane, int rc, int cnt, const double* R, const double* t,
                                               float prop, const float* kx, const float* ky, const float* ks) {
    const double qnan = __builtin_nan("");
    for (int e = lane; e < PT_POSE; e += 64) {
        double v;
        if (e == 0) v = rc;
        else if (e == 1) v = cnt;
        else if (e < 11) v = rc == 0 ? R[e - 2] : qnan;
        else if (e < 14) v = rc == 0 ? t[e - 11] : qnan;
        else if (e == 14) v = prop;
        else if (e == 15) v = 0.0;
        else {
            const int k = (e - 16) / 3, c = (e - 16) % 3;
            v = c == 0 ? kx[k] : (c == 1 ? ky[k] : ks[k]);
        }
        out[e] = v;
    }
}
// a row without a pose: status 1 (no detection / no candidate) or 2 (dropped by pPose-NMS), NaN in R and t, zeros elsewhere
__device__ __forceinline__ void write_status_row(double* __restrict__ out, int lane, int status) {
    for (int e = lane; e < PT_POSE; e += 64) out[e] = e == 0 ? (double)status : ((e >= 2 && e < 14) ? __builtin_nan("") : 0.0);
}
