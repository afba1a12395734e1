// The wave64 PnP shared by the device pose tail (pose_tail.hip) and the device RANSAC (pnp_ransac.hip): pnp_wave, the
// twin of solve_pnp_iterative of host_post.cpp in the host's operation order, with its helpers (project_residuals,
// rodrigues_exp / rodrigues_log, the cyclic Jacobi solvers).  Included inside `namespace bp { namespace {` of a unit
// that has `#pragma clang fp contract(off)` in force; the numerical contract and the wave layout are described at the
// top of pose_tail.hip.

constexpr int PT_MAXN = 64;            // points per problem (one per lane)
constexpr int PT_K = 50;               // key points per frame record
constexpr int PT_REC = 316;            // BP_RESULT_FLOATS
constexpr int PT_POSE = 166;           // BP_POSE_DOUBLES

struct PnpShared {
    double P[PT_MAXN * 3], U[PT_MAXN * 2], mn[PT_MAXN * 2], xy[PT_MAXN * 2];
    double A[144], V[144];
    double J[PT_MAXN * 2 * 6], err[PT_MAXN * 2];
    double JtJ[36], JtErr[6];
};

__device__ __forceinline__ void wsync() { __syncthreads(); }   // the workgroup is one wave
__device__ __forceinline__ double dmax(double a, double b) { return a < b ? b : a; }   // std::max
__device__ __forceinline__ float fmaxs(float a, float b) { return a < b ? b : a; }      // std::max
__device__ __forceinline__ float fmins(float a, float b) { return b < a ? b : a; }      // std::min

// ---------------------------------------------------------------- O(1) pieces, every lane redundantly (registers)
template <int N>
__device__ void jacobi_small(double* A, double* V, double* w) {
#pragma unroll
    for (int i = 0; i < N; ++i)
#pragma unroll
        for (int j = 0; j < N; ++j) V[i * N + j] = i == j ? 1.0 : 0.0;
    for (int sweep = 0; sweep < 100; ++sweep) {
        double off = 0.0;
#pragma unroll
        for (int i = 0; i < N; ++i)
#pragma unroll
            for (int j = i + 1; j < N; ++j) off += A[i * N + j] * A[i * N + j];
        if (off < 1e-300) break;
#pragma unroll
        for (int p = 0; p < N; ++p)
#pragma unroll
            for (int q = p + 1; q < N; ++q) {
                const double apq = A[p * N + q];
                if (fabs(apq) < 1e-300) continue;
                const double theta = (A[q * N + q] - A[p * N + p]) / (2.0 * apq);
                const double t = (theta >= 0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
                const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
#pragma unroll
                for (int k = 0; k < N; ++k) {
                    const double akp = A[k * N + p], akq = A[k * N + q];
                    A[k * N + p] = c * akp - s * akq;
                    A[k * N + q] = s * akp + c * akq;
                }
#pragma unroll
                for (int k = 0; k < N; ++k) {
                    const double apk = A[p * N + k], aqk = A[q * N + k];
                    A[p * N + k] = c * apk - s * aqk;
                    A[q * N + k] = s * apk + c * aqk;
                }
#pragma unroll
                for (int k = 0; k < N; ++k) {
                    const double vkp = V[k * N + p], vkq = V[k * N + q];
                    V[k * N + p] = c * vkp - s * vkq;
                    V[k * N + q] = s * vkp + c * vkq;
                }
            }
    }
#pragma unroll
    for (int i = 0; i < N; ++i) w[i] = A[i * N + i];
}

__device__ __forceinline__ double det3(const double* M) {
    return M[0] * (M[4] * M[8] - M[5] * M[7]) - M[1] * (M[3] * M[8] - M[5] * M[6]) + M[2] * (M[3] * M[7] - M[4] * M[6]);
}
__device__ __forceinline__ void mul33(const double* A, const double* B, double* C) {
    double T[9];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) T[i * 3 + j] = A[i * 3] * B[j] + A[i * 3 + 1] * B[3 + j] + A[i * 3 + 2] * B[6 + j];
#pragma unroll
    for (int i = 0; i < 9; ++i) C[i] = T[i];
}

__device__ void polar_rotation(const double* M, double* R) {
    double MtM[9], V[9], w[3];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) MtM[i * 3 + j] = M[i] * M[j] + M[3 + i] * M[3 + j] + M[6 + i] * M[6 + j];
    jacobi_small<3>(MtM, V, w);
    double S[9];
#pragma unroll
    for (int i = 0; i < 9; ++i) S[i] = 0.0;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const double s = sqrt(dmax(w[i], 1e-300));
#pragma unroll
        for (int r = 0; r < 3; ++r)
#pragma unroll
            for (int c = 0; c < 3; ++c) S[r * 3 + c] += V[r * 3 + i] * V[c * 3 + i] / s;
    }
    mul33(M, S, R);
}

__device__ void rodrigues_exp(const double* w, double* R) {
    const double th = sqrt(w[0] * w[0] + w[1] * w[1] + w[2] * w[2]);
    double a, b;
    if (th < 1e-8) { a = 1.0 - th * th / 6.0; b = 0.5 - th * th / 24.0; }
    else { a = sin(th) / th; b = (1.0 - cos(th)) / (th * th); }
    const double K[9] = {0, -w[2], w[1], w[2], 0, -w[0], -w[1], w[0], 0};
    double K2[9];
    mul33(K, K, K2);
#pragma unroll
    for (int i = 0; i < 9; ++i) R[i] = (i % 4 == 0 ? 1.0 : 0.0) + a * K[i] + b * K2[i];
}

__device__ void rodrigues_log(const double* R, double* r) {
    const double rx = R[7] - R[5], ry = R[2] - R[6], rz = R[3] - R[1];
    const double s = 0.5 * sqrt(rx * rx + ry * ry + rz * rz);
    double c = 0.5 * (R[0] + R[4] + R[8] - 1.0);
    c = c > 1.0 ? 1.0 : (c < -1.0 ? -1.0 : c);
    const double th = acos(c);
    if (s < 1e-5) {
        if (c > 0) { r[0] = r[1] = r[2] = 0.0; return; }
        double t = (R[0] + 1) * 0.5;
        r[0] = sqrt(dmax(t, 0.0));
        t = (R[4] + 1) * 0.5;
        r[1] = sqrt(dmax(t, 0.0)) * (R[1] < 0 ? -1.0 : 1.0);
        t = (R[8] + 1) * 0.5;
        r[2] = sqrt(dmax(t, 0.0)) * (R[2] < 0 ? -1.0 : 1.0);
        if (fabs(r[0]) < fabs(r[1]) && fabs(r[0]) < fabs(r[2]) && (R[5] > 0) != (r[1] * r[2] > 0)) r[2] = -r[2];
        const double nr = sqrt(r[0] * r[0] + r[1] * r[1] + r[2] * r[2]);
#pragma unroll
        for (int i = 0; i < 3; ++i) r[i] *= th / dmax(nr, 1e-300);
        return;
    }
    const double k = th / (2.0 * s);
    r[0] = rx * k; r[1] = ry * k; r[2] = rz * k;
}

// Gaussian elimination with partial pivoting on the 6x6 damped system (host solve_n); the row swap is written as
// selects so that the arrays stay in registers
__device__ bool solve6(double* A, double* b) {
#pragma unroll
    for (int c = 0; c < 6; ++c) {
        int piv = c;
        double best = fabs(A[c * 6 + c]);
#pragma unroll
        for (int r = c + 1; r < 6; ++r) {
            const double v = fabs(A[r * 6 + c]);
            if (v > best) { piv = r; best = v; }
        }
        if (best < 1e-300) return false;
#pragma unroll
        for (int r = c + 1; r < 6; ++r) {
            if (r != piv) continue;
#pragma unroll
            for (int k = 0; k < 6; ++k) { const double x = A[c * 6 + k]; A[c * 6 + k] = A[r * 6 + k]; A[r * 6 + k] = x; }
            const double x = b[c]; b[c] = b[r]; b[r] = x;
        }
#pragma unroll
        for (int r = c + 1; r < 6; ++r) {
            const double f = A[r * 6 + c] / A[c * 6 + c];
#pragma unroll
            for (int k = c; k < 6; ++k) A[r * 6 + k] -= f * A[c * 6 + k];
            b[r] -= f * b[c];
        }
    }
#pragma unroll
    for (int r = 5; r >= 0; --r) {
        double s = b[r];
#pragma unroll
        for (int k = r + 1; k < 6; ++k) s -= A[r * 6 + k] * b[k];
        b[r] = s / A[r * 6 + r];
    }
    return true;
}

__device__ double norm_l2_lds(const double* v, int n) {
    double s = 0;
    for (int i = 0; i < n; ++i) s += v[i] * v[i];
    return sqrt(s);
}

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
                const double theta = (sh.A[q * n + q] - sh.A[p * n + p]) / (2.0 * apq);
                const double t = (theta >= 0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
                const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
                wsync();
                if (lane < n) {                       // columns p, q of row k
                    const int k = lane;
                    const double akp = sh.A[k * n + p], akq = sh.A[k * n + q];
                    sh.A[k * n + p] = c * akp - s * akq;
                    sh.A[k * n + q] = s * akp + c * akq;
                } else if (lane >= 32 && lane - 32 < n) {   // eigenvector columns p, q of row k
                    const int k = lane - 32;
                    const double vkp = sh.V[k * n + p], vkq = sh.V[k * n + q];
                    sh.V[k * n + p] = c * vkp - s * vkq;
                    sh.V[k * n + q] = s * vkp + c * vkq;
                }
                wsync();
                if (lane < n) {                       // rows p, q of column k
                    const int k = lane;
                    const double apk = sh.A[p * n + k], aqk = sh.A[q * n + k];
                    sh.A[p * n + k] = c * apk - s * aqk;
                    sh.A[q * n + k] = s * apk + c * aqk;
                }
                wsync();
            }
    }
    for (int i = 0; i < n; ++i) w[i] = sh.A[i * n + i];
}

// cvProjectPoints2, zero distortion: err = proj - observed (sh.err); with_j: the 2n x 6 Jacobian (sh.J).  Lane i = point i.
__device__ void project_residuals(PnpShared& sh, int n, const PnpCam& cam, const double* prm, bool with_j) {
    const int i = threadIdx.x;
    double R[9];
    rodrigues_exp(prm, R);
    const double fx = cam.fx, fy = cam.fy, cx = cam.cx, cy = cam.cy;
    double Jr[9];
    if (with_j) {
        const double* w = prm;
        const double th = sqrt(w[0] * w[0] + w[1] * w[1] + w[2] * w[2]);
        double a, b;
        if (th < 1e-6) { a = 0.5 - th * th / 24.0; b = 1.0 / 6.0 - th * th / 120.0; }
        else { a = (1.0 - cos(th)) / (th * th); b = (th - sin(th)) / (th * th * th); }
        const double Kx[9] = {0, -w[2], w[1], w[2], 0, -w[0], -w[1], w[0], 0};
        double K2[9];
        mul33(Kx, Kx, K2);
#pragma unroll
        for (int e = 0; e < 9; ++e) Jr[e] = (e % 4 == 0 ? 1.0 : 0.0) - a * Kx[e] + b * K2[e];
    }
    if (i < n) {
        const double X[3] = {sh.P[3 * i], sh.P[3 * i + 1], sh.P[3 * i + 2]};
        const double Y0 = R[0] * X[0] + R[1] * X[1] + R[2] * X[2] + prm[3];
        const double Y1 = R[3] * X[0] + R[4] * X[1] + R[5] * X[2] + prm[4];
        const double Y2 = R[6] * X[0] + R[7] * X[1] + R[8] * X[2] + prm[5];
        const double iz = Y2 != 0.0 ? 1.0 / Y2 : 1.0;
        sh.err[2 * i] = fx * Y0 * iz + cx - sh.U[2 * i];
        sh.err[2 * i + 1] = fy * Y1 * iz + cy - sh.U[2 * i + 1];
        if (with_j) {
            const double Xx[9] = {0, -X[2], X[1], X[2], 0, -X[0], -X[1], X[0], 0};
            double T[9], D[9];
            mul33(R, Xx, T);
            mul33(T, Jr, D);
            const double du[3] = {fx * iz, 0, -fx * Y0 * iz * iz};
            const double dv[3] = {0, fy * iz, -fy * Y1 * iz * iz};
            double* Ju = sh.J + (2 * i) * 6;
            double* Jv = sh.J + (2 * i + 1) * 6;
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                Ju[c] = -(du[0] * D[c] + du[1] * D[3 + c] + du[2] * D[6 + c]);
                Jv[c] = -(dv[0] * D[c] + dv[1] * D[3 + c] + dv[2] * D[6 + c]);
                Ju[3 + c] = du[c];
                Jv[3 + c] = dv[c];
            }
        }
    }
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
    int ord[3] = {0, 1, 2};           // std::sort of three: insertion sort, descending
    for (int i = 1; i < 3; ++i) {
        const int v = ord[i];
        int j = i;
        while (j > 0 && Wm[v] > Wm[ord[j - 1]]) { ord[j] = ord[j - 1]; --j; }
        ord[j] = v;
    }
    double prm[6], R[9], t[3];
    if (!(Wm[ord[0]] > 0)) return -2;
    wsync();                           // sh.A is rewritten below
    if (Wm[ord[2]] / dmax(Wm[ord[1]], 1e-300) < 1e-3) {
        // ---- planar model
        double Rt[9];
        for (int r = 0; r < 3; ++r)
            for (int c = 0; c < 3; ++c) Rt[r * 3 + c] = Vm[c * 3 + ord[r]];
        if (Rt[6] * Rt[6] + Rt[7] * Rt[7] < 1e-10) {
#pragma unroll
            for (int e = 0; e < 9; ++e) Rt[e] = e % 4 == 0 ? 1.0 : 0.0;
        }
        if (det3(Rt) < 0)
#pragma unroll
            for (int e = 0; e < 9; ++e) Rt[e] = -Rt[e];
        double Tt[3];
#pragma unroll
        for (int r = 0; r < 3; ++r) Tt[r] = -(Rt[r * 3] * Mc[0] + Rt[r * 3 + 1] * Mc[1] + Rt[r * 3 + 2] * Mc[2]);
        if (lane < n)
#pragma unroll
            for (int r = 0; r < 2; ++r)
                sh.xy[2 * lane + r] = Rt[r * 3] * sh.P[3 * lane] + Rt[r * 3 + 1] * sh.P[3 * lane + 1] +
                                      Rt[r * 3 + 2] * sh.P[3 * lane + 2] + Tt[r];
        wsync();
        double H[9];
        if (homography_dlt(sh, n, H)) {
            double h1[3] = {H[0], H[3], H[6]}, h2[3] = {H[1], H[4], H[7]}, h3[3] = {H[2], H[5], H[8]};
            const double zc = h3[2];
            if (zc < 0)
#pragma unroll
                for (int k = 0; k < 3; ++k) { h1[k] = -h1[k]; h2[k] = -h2[k]; h3[k] = -h3[k]; }
            const double n1 = sqrt(h1[0] * h1[0] + h1[1] * h1[1] + h1[2] * h1[2]);
            const double n2 = sqrt(h2[0] * h2[0] + h2[1] * h2[1] + h2[2] * h2[2]);
            if (!(n1 > 0) || !(n2 > 0)) return -2;
#pragma unroll
            for (int k = 0; k < 3; ++k) { h1[k] /= n1; h2[k] /= n2; t[k] = h3[k] * 2.0 / (n1 + n2); }
            const double hx[3] = {h1[1] * h2[2] - h1[2] * h2[1], h1[2] * h2[0] - h1[0] * h2[2], h1[0] * h2[1] - h1[1] * h2[0]};
            double Hm[9] = {h1[0], h2[0], hx[0], h1[1], h2[1], hx[1], h1[2], h2[2], hx[2]};
            double rv[3], Hp[9];
            polar_rotation(Hm, Hp);
            rodrigues_log(Hp, rv);
            rodrigues_exp(rv, Hm);
#pragma unroll
            for (int r = 0; r < 3; ++r) t[r] += Hm[r * 3] * Tt[0] + Hm[r * 3 + 1] * Tt[1] + Hm[r * 3 + 2] * Tt[2];
            mul33(Hm, Rt, R);
        } else {
#pragma unroll
            for (int e = 0; e < 9; ++e) R[e] = e % 4 == 0 ? 1.0 : 0.0;
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
        double RR[9], tt[3];
        for (int r = 0; r < 3; ++r) {
            for (int c = 0; c < 3; ++c) RR[r * 3 + c] = sh.V[(r * 4 + c) * 12 + m];
            tt[r] = sh.V[(r * 4 + 3) * 12 + m];
        }
        if (det3(RR) < 0) {
#pragma unroll
            for (int e = 0; e < 9; ++e) RR[e] = -RR[e];
#pragma unroll
            for (int e = 0; e < 3; ++e) tt[e] = -tt[e];
        }
        double sc = 0;
#pragma unroll
        for (int e = 0; e < 9; ++e) sc += RR[e] * RR[e];
        sc = sqrt(sc);
        if (!(sc > 0)) return -2;
        polar_rotation(RR, R);
#pragma unroll
        for (int e = 0; e < 3; ++e) t[e] = tt[e] * (sqrt(3.0) / sc);
    }
    rodrigues_log(R, prm);
    prm[3] = t[0]; prm[4] = t[1]; prm[5] = t[2];

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
        if (iters == 0) prevErrNorm = norm_l2_lds(sh.err, ne);
        double errNorm;
        for (;;) {
            // step(): (JtJ with its diagonal scaled by 1 + lambda) d = JtErr, param = previous - d
            const double lambda = cam.lam[lambdaLg10 + 16];
            double A[36], d[6];
#pragma unroll
            for (int e = 0; e < 36; ++e) A[e] = sh.JtJ[e];
#pragma unroll
            for (int e = 0; e < 6; ++e) d[e] = sh.JtErr[e];
#pragma unroll
            for (int e = 0; e < 6; ++e) A[e * 6 + e] *= 1.0 + lambda;
            if (!solve6(A, d))
#pragma unroll
                for (int e = 0; e < 6; ++e) d[e] = 0.0;
#pragma unroll
            for (int e = 0; e < 6; ++e) prm[e] = prev[e] - d[e];
            wsync();                     // sh.err is rewritten
            project_residuals(sh, n, cam, prm, false);
            errNorm = norm_l2_lds(sh.err, ne);
            if (errNorm > prevErrNorm && ++lambdaLg10 <= 16) continue;
            break;
        }
        lambdaLg10 = lambdaLg10 - 1 < -16 ? -16 : lambdaLg10 - 1;
        double dn = 0;
#pragma unroll
        for (int i = 0; i < 6; ++i) dn += (prm[i] - prev[i]) * (prm[i] - prev[i]);
        double pn = 0;
#pragma unroll
        for (int i = 0; i < 6; ++i) pn += prev[i] * prev[i];
        const double rel = sqrt(dn) / dmax(sqrt(pn), 2.2250738585072014e-308);
        wsync();                         // sh.J / sh.err / sh.JtJ are rewritten by the next iteration
        if (++iters >= 20 || rel < (double)1.19209290e-07F) break;
        prevErrNorm = errNorm;
    }
    rodrigues_exp(prm, Rout);
    tout[0] = prm[3]; tout[1] = prm[4]; tout[2] = prm[5];
    for (int i = 0; i < 9; ++i)
        if (!isfinite(Rout[i])) return -2;
    for (int i = 0; i < 3; ++i)
        if (!isfinite(tout[i])) return -2;
    return 0;
}
