// The wave64 PnP shared by the device pose tails (pose_tail.hip, pose_tail_cands.hip, pose_tail_inst.hip) and the device
// RANSAC (pnp_ransac.hip): pnp_wave, which is solve_pnp_iterative of host_post.cpp with the loops over the points spread
// over the lanes.  Everything of O(1) size is pnp_math.inc, the same text the host compiles; what is here is what differs
// by nature: the LDS arrays, the lane-per-accumulator sums in the host's order and the wave-parallel Jacobi.  Included
// inside `namespace bp { namespace {` of a unit that includes pose_tail.h and has `#pragma clang fp contract(off)` in
// force; the numerical contract and the wave layout are described at the top of pose_tail.hip.

#include "pnp_math.inc"

struct PnpShared {
    double P[PT_MAXN * 3], U[PT_MAXN * 2], mn[PT_MAXN * 2], xy[PT_MAXN * 2];
    double A[144], V[144];
    double J[PT_MAXN * 2 * 6], err[PT_MAXN * 2];
    double JtJ[36], JtErr[6];
};

__device__ __forceinline__ void wsync() { __syncthreads(); }   // the workgroup is one wave
__device__ __forceinline__ float fmaxs(float a, float b) { return a < b ? b : a; }      // std::max
__device__ __forceinline__ float fmins(float a, float b) { return b < a ? b : a; }      // std::min

// ---------------------------------------------------------------- wave-parallel pieces (LDS)
// cyclic Jacobi of the symmetric n x n matrix sh.A (n <= 12), eigenvectors in the columns of sh.V, eigenvalues in w
// (registers, every lane).  Rotation order, sweep test and per-element arithmetic are the host's.
__device__ void jacobi_wave(PnpShared& sh, int n, double* w) {
    const int lane = threadIdx.x;
    for (int e = lane; e < n * n; e += 64) sh.V[e] = (e / n == e % n) ? 1.0 : 0.0;
    wsync();
    for (int sweep = 0; sweep < 100; ++sweep) {
        double off = 0.0;
        for (int i = 0; i < n; ++i)
            for (int j = i + 1; j < n; ++j) off += sh.A[i * n + j] * sh.A[i * n + j];
        if (off < 1e-300) break;
        for (int p = 0; p < n; ++p)
            for (int q = p + 1; q < n; ++q) {
                const double apq = sh.A[p * n + q];
                if (fabs(apq) < 1e-300) continue;
                double c, s;
                jacobi_rotation(sh.A[p * n + p], sh.A[q * n + q], apq, &c, &s);
                wsync();
                if (lane < n) jacobi_apply(c, s, &sh.A[lane * n + p], &sh.A[lane * n + q]);                 // columns p, q of row k
                else if (lane >= 32 && lane - 32 < n) jacobi_apply(c, s, &sh.V[(lane - 32) * n + p], &sh.V[(lane - 32) * n + q]);
                wsync();
                if (lane < n) jacobi_apply(c, s, &sh.A[p * n + lane], &sh.A[q * n + lane]);                 // rows p, q of column k
                wsync();
            }
    }
    for (int i = 0; i < n; ++i) w[i] = sh.A[i * n + i];
}

// cvProjectPoints2, zero distortion: err = proj - observed (sh.err); with_j: the 2n x 6 Jacobian (sh.J).  Lane i = point i.
__device__ void project_residuals(PnpShared& sh, int n, const PnpCam& cam, const double* prm, bool with_j) {
    const int i = threadIdx.x;
    double R[9], Jr[9];
    rodrigues_exp(prm, R);
    if (with_j) right_jacobian(prm, Jr);
    if (i < n)
        project_point(cam, R, Jr, prm, sh.P + 3 * i, sh.U + 2 * i, sh.err + 2 * i, with_j, sh.J + (2 * i) * 6, sh.J + (2 * i + 1) * 6);
    wsync();
}

// entries of the two rows a correspondence adds to a normal matrix, selected by index (no local arrays):
// homography rows {x, y, 1, 0, 0, 0, -u x, -u y, -u} / {0, 0, 0, x, y, 1, -v x, -v y, -v}
__device__ __forceinline__ double hom_r1(int a, double x, double y, double u) {
    return a < 3 ? (a == 0 ? x : (a == 1 ? y : 1.0)) : (a < 6 ? 0.0 : (a < 8 ? -u * (a == 6 ? x : y) : -u));
}
__device__ __forceinline__ double hom_r2(int a, double x, double y, double v) {
    return a < 3 ? 0.0 : (a < 6 ? (a == 3 ? x : (a == 4 ? y : 1.0)) : (a < 8 ? -v * (a == 6 ? x : y) : -v));
}
// DLT rows {X, Y, Z, 1, 0, 0, 0, 0, -x X, -x Y, -x Z, -x} / {0, 0, 0, 0, X, Y, Z, 1, -y X, -y Y, -y Z, -y}
__device__ __forceinline__ double pick3(int i, double X, double Y, double Z) { return i == 0 ? X : (i == 1 ? Y : Z); }
__device__ __forceinline__ double dlt_r1(int a, double X, double Y, double Z, double x) {
    return a < 3 ? pick3(a, X, Y, Z) : (a == 3 ? 1.0 : (a < 8 ? 0.0 : (a < 11 ? -x * pick3(a - 8, X, Y, Z) : -x)));
}
__device__ __forceinline__ double dlt_r2(int a, double X, double Y, double Z, double y) {
    return a < 4 ? 0.0 : (a < 7 ? pick3(a - 4, X, Y, Z) : (a == 7 ? 1.0 : (a < 11 ? -y * pick3(a - 8, X, Y, Z) : -y)));
}

// homography m ~ H (x, y, 1) by the normalised DLT on sh.xy -> sh.mn (host homography_dlt)
__device__ bool homography_dlt(PnpShared& sh, int n, double* H) {
    const int lane = threadIdx.x;
    double c0[2] = {0, 0}, c1[2] = {0, 0};
    for (int i = 0; i < n; ++i) {
        c0[0] += sh.xy[2 * i] / n; c0[1] += sh.xy[2 * i + 1] / n;
        c1[0] += sh.mn[2 * i] / n; c1[1] += sh.mn[2 * i + 1] / n;
    }
    double d0 = 0, d1 = 0;
    for (int i = 0; i < n; ++i) {
        d0 += hypot(sh.xy[2 * i] - c0[0], sh.xy[2 * i + 1] - c0[1]) / n;
        d1 += hypot(sh.mn[2 * i] - c1[0], sh.mn[2 * i + 1] - c1[1]) / n;
    }
    if (!(d0 > 0) || !(d1 > 0)) return false;
    const double s0 = sqrt(2.0) / d0, s1 = sqrt(2.0) / d1;
    for (int e = lane; e < 81; e += 64) {
        const int a = e / 9, b = e % 9;
        double acc = 0;
        for (int i = 0; i < n; ++i) {
            const double x = s0 * (sh.xy[2 * i] - c0[0]), y = s0 * (sh.xy[2 * i + 1] - c0[1]);
            const double u = s1 * (sh.mn[2 * i] - c1[0]), v = s1 * (sh.mn[2 * i + 1] - c1[1]);
            acc += hom_r1(a, x, y, u) * hom_r1(b, x, y, u) + hom_r2(a, x, y, v) * hom_r2(b, x, y, v);
        }
        sh.A[e] = acc;
    }
    wsync();
    double w[9];
    jacobi_wave(sh, 9, w);
    int k = 0;
    for (int i = 1; i < 9; ++i)
        if (w[i] < w[k]) k = i;
    double Hn[9];
    for (int i = 0; i < 9; ++i) Hn[i] = sh.V[i * 9 + k];
    const double T0[9] = {s0, 0, -s0 * c0[0], 0, s0, -s0 * c0[1], 0, 0, 1};
    const double T1i[9] = {1 / s1, 0, c1[0], 0, 1 / s1, c1[1], 0, 0, 1};
    double T[9];
    mul33(Hn, T0, T);
    mul33(T1i, T, H);
    return true;
}

// solve_pnp_iterative (host_post.cpp) on the n points in sh.P / sh.U; every lane returns the same status, R and t
__device__ int pnp_wave(PnpShared& sh, int n, const PnpCam& cam, double* Rout, double* tout) {
    const int lane = threadIdx.x;
    if (n < 4) return -1;
    const double fx = cam.fx, fy = cam.fy, cx = cam.cx, cy = cam.cy;
    if (lane < n) {
        sh.mn[2 * lane] = (sh.U[2 * lane] - cx) / fx;
        sh.mn[2 * lane + 1] = (sh.U[2 * lane + 1] - cy) / fy;
    }
    // ---- spread of the model
    double Mc[3] = {0, 0, 0};
    for (int i = 0; i < n; ++i)
        for (int k = 0; k < 3; ++k) Mc[k] += sh.P[3 * i + k] / n;
    if (lane < 9) {
        const int a = lane / 3, b = lane % 3;
        double acc = 0;
        for (int i = 0; i < n; ++i) acc += (sh.P[3 * i + a] - Mc[a]) * (sh.P[3 * i + b] - Mc[b]);
        sh.A[lane] = acc;
    }
    wsync();
    double MM[9], Vm[9], Wm[3];
#pragma unroll
    for (int e = 0; e < 9; ++e) MM[e] = sh.A[e];
    jacobi_small<3>(MM, Vm, Wm);
    int ord[3];
    order3_desc(Wm, ord);
    double prm[6], R[9], t[3];
    if (!(Wm[ord[0]] > 0)) return -2;
    wsync();                           // sh.A is rewritten below
    if (Wm[ord[2]] / dmax(Wm[ord[1]], 1e-300) < 1e-3) {
        // ---- planar model
        double Rt[9], Tt[3];
        plane_frame(Vm, ord, Mc, Rt, Tt);
        if (lane < n)
#pragma unroll
            for (int r = 0; r < 2; ++r)
                sh.xy[2 * lane + r] = Rt[r * 3] * sh.P[3 * lane] + Rt[r * 3 + 1] * sh.P[3 * lane + 1] +
                                      Rt[r * 3 + 2] * sh.P[3 * lane + 2] + Tt[r];
        wsync();
        double H[9];
        if (homography_dlt(sh, n, H)) {
            if (!homography_pose(H, Rt, Tt, R, t)) return -2;
        } else {
            identity33(R);
            t[0] = t[1] = t[2] = 0;
        }
    } else {
        // ---- DLT on the raw object coordinates: lane e (and e + 64, e + 128) owns LL[e]
        if (n < 6) return -1;
        for (int e = lane; e < 144; e += 64) {
            const int a = e / 12, b = e % 12;
            double acc = 0;
            for (int i = 0; i < n; ++i) {
                const double x = sh.mn[2 * i], y = sh.mn[2 * i + 1];
                const double X = sh.P[3 * i], Y = sh.P[3 * i + 1], Z = sh.P[3 * i + 2];
                acc += dlt_r1(a, X, Y, Z, x) * dlt_r1(b, X, Y, Z, x) + dlt_r2(a, X, Y, Z, y) * dlt_r2(b, X, Y, Z, y);
            }
            sh.A[e] = acc;
        }
        wsync();
        double w[12];
        jacobi_wave(sh, 12, w);
        int m = 0;
        for (int i = 1; i < 12; ++i)
            if (w[i] < w[m]) m = i;
        if (!dlt_pose(sh.V + m, R, t)) return -2;
    }
    pose_to_params(R, t, prm);

    // ---- CvLevMarq
    const int ne = 2 * n;
    double prev[6];
    int lambdaLg10 = -3, iters = 0;
    double prevErrNorm = 0;
    for (;;) {
        project_residuals(sh, n, cam, prm, true);
        if (lane < 42) {                // lane a < 6: JtErr[a]; lane 6 + a * 6 + b: JtJ[a][b]; each sums over e in order
            const int a = lane < 6 ? lane : (lane - 6) / 6, b = lane < 6 ? 0 : (lane - 6) % 6;
            double acc = 0;
            if (lane < 6)
                for (int e = 0; e < ne; ++e) acc += sh.J[e * 6 + a] * sh.err[e];
            else
                for (int e = 0; e < ne; ++e) acc += sh.J[e * 6 + a] * sh.J[e * 6 + b];
            if (lane < 6) sh.JtErr[a] = acc;
            else sh.JtJ[a * 6 + b] = acc;
        }
        wsync();
#pragma unroll
        for (int i = 0; i < 6; ++i) prev[i] = prm[i];
        if (iters == 0) prevErrNorm = norm_l2(sh.err, ne);
        double errNorm;
        do {
            lm_step(sh.JtJ, sh.JtErr, cam.lam[lambdaLg10 + 16], prev, prm);
            wsync();                     // sh.err is rewritten
            project_residuals(sh, n, cam, prm, false);
            errNorm = norm_l2(sh.err, ne);
        } while (lm_retry(errNorm, prevErrNorm, &lambdaLg10));
        lambdaLg10 = lm_relax(lambdaLg10);
        const bool stop = lm_converged(prm, prev);
        wsync();                         // sh.J / sh.err / sh.JtJ are rewritten by the next iteration
        if (++iters >= 20 || stop) break;
        prevErrNorm = errNorm;
    }
    return params_to_pose(prm, Rout, tout);
}
