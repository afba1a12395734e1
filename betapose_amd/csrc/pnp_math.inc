// The PnP arithmetic of O(1) size, ONE source for the host solver (host_post.cpp solve_pnp_iterative) and the wave64 device
// solver (pnp_wave.inc pnp_wave): everything whose size does not depend on the number of points.  The project's numerical
// contract -- host and device do the same f64 operations in the same order, without FMA contraction -- holds because both
// compile this text; only who loops over the points, and where the arrays live, differs per side.
// Plain C++17, no HIP header, no std:: containers.  Included inside `namespace bp { namespace {` after <cmath> and
// pose_tail.h (PnpCam), in a unit that has `#pragma clang fp contract(off)` in force.
#if defined(__HIPCC__)
#define BP_HD __host__ __device__ inline __attribute__((always_inline))   // (__forceinline__ without needing the HIP header)
#else
#define BP_HD inline
#endif

BP_HD double dmax(double a, double b) { return a < b ? b : a; }   // std::max

BP_HD double norm_l2(const double* v, int n) {
    double s = 0;
    for (int i = 0; i < n; ++i) s += v[i] * v[i];
    return sqrt(s);
}

// ---------------------------------------------------------------- cyclic Jacobi
// the rotation that annihilates a[p][q] of a symmetric matrix, and its application to a pair of entries; shared by
// jacobi_small below, the host's n x n jacobi_eig and the device's jacobi_wave
BP_HD void jacobi_rotation(double app, double aqq, double apq, double* c, double* s) {
    const double theta = (aqq - app) / (2.0 * apq);
    const double t = (theta >= 0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
    *c = 1.0 / sqrt(t * t + 1.0);
    *s = t * *c;
}
BP_HD void jacobi_apply(double c, double s, double* xp, double* xq) {
    const double p = *xp, q = *xq;
    *xp = c * p - s * q;
    *xq = s * p + c * q;
}

// symmetric N x N matrix (row-major, destroyed) in registers; V columns = eigenvectors
template <int N>
BP_HD void jacobi_small(double* A, double* V, double* w) {
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
                double c, s;
                jacobi_rotation(A[p * N + p], A[q * N + q], apq, &c, &s);
#pragma unroll
                for (int k = 0; k < N; ++k) jacobi_apply(c, s, &A[k * N + p], &A[k * N + q]);
#pragma unroll
                for (int k = 0; k < N; ++k) jacobi_apply(c, s, &A[p * N + k], &A[q * N + k]);
#pragma unroll
                for (int k = 0; k < N; ++k) jacobi_apply(c, s, &V[k * N + p], &V[k * N + q]);
            }
    }
#pragma unroll
    for (int i = 0; i < N; ++i) w[i] = A[i * N + i];
}

// ---------------------------------------------------------------- 3x3 pieces
BP_HD double det3(const double* M) {
    return M[0] * (M[4] * M[8] - M[5] * M[7]) - M[1] * (M[3] * M[8] - M[5] * M[6]) + M[2] * (M[3] * M[7] - M[4] * M[6]);
}
BP_HD void mul33(const double* A, const double* B, double* C) {
    double T[9];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) T[i * 3 + j] = A[i * 3] * B[j] + A[i * 3 + 1] * B[3 + j] + A[i * 3 + 2] * B[6 + j];
#pragma unroll
    for (int i = 0; i < 9; ++i) C[i] = T[i];
}
BP_HD void identity33(double* R) {
#pragma unroll
    for (int e = 0; e < 9; ++e) R[e] = e % 4 == 0 ? 1.0 : 0.0;
}
BP_HD void skew33(const double* w, double* K) {
    K[0] = 0; K[1] = -w[2]; K[2] = w[1]; K[3] = w[2]; K[4] = 0; K[5] = -w[0]; K[6] = -w[1]; K[7] = w[0]; K[8] = 0;
}

// The orthogonal polar factor M (M^T M)^(-1/2) = U V^T of M's SVD, through the eigen-decomposition (V, w) of M^T M:
// polar_factor gives M V diag(1 / sqrt(w)) V^T, with the eigen-direction `neg` negated (-1: none).
BP_HD void polar_eig(const double* M, double* V, double* w) {
    double MtM[9];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) MtM[i * 3 + j] = M[i] * M[j] + M[3 + i] * M[3 + j] + M[6 + i] * M[6 + j];
    jacobi_small<3>(MtM, V, w);
}
BP_HD void polar_factor(const double* M, const double* V, const double* w, int neg, double* R) {
    double S[9];
#pragma unroll
    for (int i = 0; i < 9; ++i) S[i] = 0.0;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        double s = sqrt(dmax(w[i], 1e-300));
        if (i == neg) s = -s;
#pragma unroll
        for (int r = 0; r < 3; ++r)
#pragma unroll
            for (int c = 0; c < 3; ++c) S[r * 3 + c] += V[r * 3 + i] * V[c * 3 + i] / s;
    }
    mul33(M, S, R);
}
// (det(M) > 0 on every path that calls this, so the factor is a rotation)
BP_HD void polar_rotation(const double* M, double* R) {
    double V[9], w[3];
    polar_eig(M, V, w);
    polar_factor(M, V, w, -1, R);
}

// Rodrigues vector -> matrix (cvRodrigues2, vector input)
BP_HD void rodrigues_exp(const double* w, double* R) {
    const double th = sqrt(w[0] * w[0] + w[1] * w[1] + w[2] * w[2]);
    double a, b;
    if (th < 1e-8) { a = 1.0 - th * th / 6.0; b = 0.5 - th * th / 24.0; }
    else { a = sin(th) / th; b = (1.0 - cos(th)) / (th * th); }
    double K[9], K2[9];
    skew33(w, K);
    mul33(K, K, K2);
#pragma unroll
    for (int i = 0; i < 9; ++i) R[i] = (i % 4 == 0 ? 1.0 : 0.0) + a * K[i] + b * K2[i];
}

// rotation matrix -> Rodrigues vector (cvRodrigues2, matrix input; angle in [0, pi])
BP_HD void rodrigues_log(const double* R, double* r) {
    const double rx = R[7] - R[5], ry = R[2] - R[6], rz = R[3] - R[1];
    const double s = 0.5 * sqrt(rx * rx + ry * ry + rz * rz);
    double c = 0.5 * (R[0] + R[4] + R[8] - 1.0);
    c = c > 1.0 ? 1.0 : (c < -1.0 ? -1.0 : c);
    const double th = acos(c);
    if (s < 1e-5) {
        if (c > 0) { r[0] = r[1] = r[2] = 0.0; return; }
        // angle pi: the axis from the diagonal, signs from the off-diagonal sums
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

// (R, t) -> the minimiser's six parameters (Rodrigues vector, translation)
BP_HD void pose_to_params(const double* R, const double* t, double* prm) {
    rodrigues_log(R, prm);
    prm[3] = t[0]; prm[4] = t[1]; prm[5] = t[2];
}

// right Jacobian of SO(3) at the Rodrigues vector w: d(R X)/dr = -R [X]x Jr(r)
BP_HD void right_jacobian(const double* w, double* Jr) {
    const double th = sqrt(w[0] * w[0] + w[1] * w[1] + w[2] * w[2]);
    double a, b;
    if (th < 1e-6) { a = 0.5 - th * th / 24.0; b = 1.0 / 6.0 - th * th / 120.0; }
    else { a = (1.0 - cos(th)) / (th * th); b = (th - sin(th)) / (th * th * th); }
    double Kx[9], K2[9];
    skew33(w, Kx);
    mul33(Kx, Kx, K2);
#pragma unroll
    for (int e = 0; e < 9; ++e) Jr[e] = (e % 4 == 0 ? 1.0 : 0.0) - a * Kx[e] + b * K2[e];
}

// Gaussian elimination with partial pivoting on the 6x6 damped system, in place; the row swap is written as selects so
// that on the device the arrays stay in registers
BP_HD bool solve6(double* A, double* b) {
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

// ---------------------------------------------------------------- one point of cvProjectPoints2, zero distortion
// pixel residual e[2] = proj - observed of the point Xp seen at u under (R = exp(prm[0..2]), prm[3..5]) and, with_j, its
// two rows Ju, Jv of the Jacobian [dp/dr | dp/dt] (Jr = right_jacobian(prm))
BP_HD void project_point(const PnpCam& cam, const double* R, const double* Jr, const double* prm, const double* Xp,
                         const double* u, double* e, bool with_j, double* Ju, double* Jv) {
    const double X[3] = {Xp[0], Xp[1], Xp[2]};
    const double Y0 = R[0] * X[0] + R[1] * X[1] + R[2] * X[2] + prm[3];
    const double Y1 = R[3] * X[0] + R[4] * X[1] + R[5] * X[2] + prm[4];
    const double Y2 = R[6] * X[0] + R[7] * X[1] + R[8] * X[2] + prm[5];
    const double iz = Y2 != 0.0 ? 1.0 / Y2 : 1.0;                      // as OpenCV: z = z ? 1./z : 1
    e[0] = cam.fx * Y0 * iz + cam.cx - u[0];
    e[1] = cam.fy * Y1 * iz + cam.cy - u[1];
    if (!with_j) return;
    double Xx[9], T[9], D[9];                                          // dY/dr = -R [X]x Jr
    skew33(X, Xx);
    mul33(R, Xx, T);
    mul33(T, Jr, D);
    const double du[3] = {cam.fx * iz, 0, -cam.fx * Y0 * iz * iz};
    const double dv[3] = {0, cam.fy * iz, -cam.fy * Y1 * iz * iz};
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        Ju[c] = -(du[0] * D[c] + du[1] * D[3 + c] + du[2] * D[6 + c]);
        Jv[c] = -(dv[0] * D[c] + dv[1] * D[3 + c] + dv[2] * D[6 + c]);
        Ju[3 + c] = du[c];
        Jv[3 + c] = dv[c];
    }
}

// ---------------------------------------------------------------- initialisation: closed forms
// indices of the three eigenvalues Wm in descending order: an insertion sort.  On three elements it gives what the
// std::sort the host solver used to call gives, except possibly on exact ties (std::sort promises no order among equals).
BP_HD void order3_desc(const double* Wm, int* ord) {
    ord[0] = 0; ord[1] = 1; ord[2] = 2;
    for (int i = 1; i < 3; ++i) {
        const int v = ord[i];
        int j = i;
        while (j > 0 && Wm[v] > Wm[ord[j - 1]]) { ord[j] = ord[j - 1]; --j; }
        ord[j] = v;
    }
}

// planar model: the frame (Rt, Tt) that takes the model to z = 0 -- rows of Rt = principal directions Vm[:, ord], the plane
// normal last -- from the centroid Mc
BP_HD void plane_frame(const double* Vm, const int* ord, const double* Mc, double* Rt, double* Tt) {
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) Rt[r * 3 + c] = Vm[c * 3 + ord[r]];
    if (Rt[6] * Rt[6] + Rt[7] * Rt[7] < 1e-10) identity33(Rt);
    if (det3(Rt) < 0)
#pragma unroll
        for (int e = 0; e < 9; ++e) Rt[e] = -Rt[e];
#pragma unroll
    for (int r = 0; r < 3; ++r) Tt[r] = -(Rt[r * 3] * Mc[0] + Rt[r * 3 + 1] * Mc[1] + Rt[r * 3 + 2] * Mc[2]);
}

// planar model: homography H of the plane z = 0 to the normalised image, in the frame (Rt, Tt) -> R, t.  Columns h1, h2
// normalised, t = h3 * 2 / (|h1| + |h2|), third column h1 x h2, Rodrigues round trip to orthonormalise.  false: degenerate.
BP_HD bool homography_pose(const double* H, const double* Rt, const double* Tt, double* R, double* t) {
    double h1[3] = {H[0], H[3], H[6]}, h2[3] = {H[1], H[4], H[7]}, h3[3] = {H[2], H[5], H[8]};
    if (h3[2] < 0)                     // a homography is defined up to sign: keep the plane in front of the camera
#pragma unroll
        for (int k = 0; k < 3; ++k) { h1[k] = -h1[k]; h2[k] = -h2[k]; h3[k] = -h3[k]; }
    const double n1 = sqrt(h1[0] * h1[0] + h1[1] * h1[1] + h1[2] * h1[2]);
    const double n2 = sqrt(h2[0] * h2[0] + h2[1] * h2[1] + h2[2] * h2[2]);
    if (!(n1 > 0) || !(n2 > 0)) return false;
#pragma unroll
    for (int k = 0; k < 3; ++k) { h1[k] /= n1; h2[k] /= n2; t[k] = h3[k] * 2.0 / (n1 + n2); }
    const double hx[3] = {h1[1] * h2[2] - h1[2] * h2[1], h1[2] * h2[0] - h1[0] * h2[2], h1[0] * h2[1] - h1[1] * h2[0]};
    double Hm[9] = {h1[0], h2[0], hx[0], h1[1], h2[1], hx[1], h1[2], h2[2], hx[2]};
    double rv[3], Hp[9];
    polar_rotation(Hm, Hp);            // cvRodrigues2 orthonormalises a matrix input through its SVD
    rodrigues_log(Hp, rv);
    rodrigues_exp(rv, Hm);
#pragma unroll
    for (int r = 0; r < 3; ++r) t[r] += Hm[r * 3] * Tt[0] + Hm[r * 3 + 1] * Tt[1] + Hm[r * 3 + 2] * Tt[2];
    mul33(Hm, Rt, R);
    return true;
}

// DLT: column v (stride 12: v[12 * i], i = 0 .. 11) of the 12 x 12 eigenvector matrix, the rows of [RR | tt] -> R, t.
// Negated if det(RR) < 0; R = U V^T of RR's SVD; t = tt * |R|_F / |RR|_F.  false: degenerate.
BP_HD bool dlt_pose(const double* v, double* R, double* t) {
    double RR[9], tt[3];
    for (int r = 0; r < 3; ++r) {
        for (int c = 0; c < 3; ++c) RR[r * 3 + c] = v[(r * 4 + c) * 12];
        tt[r] = v[(r * 4 + 3) * 12];
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
    if (!(sc > 0)) return false;
    polar_rotation(RR, R);
#pragma unroll
    for (int e = 0; e < 3; ++e) t[e] = tt[e] * (sqrt(3.0) / sc);
    return true;
}

// ---------------------------------------------------------------- CvLevMarq pieces
// the damped step: (JtJ with its diagonal scaled by 1 + lambda) d = JtErr, prm = prev - d (d = 0 if the system is singular)
BP_HD void lm_step(const double* JtJ, const double* JtErr, double lambda, const double* prev, double* prm) {
    double A[36], d[6];
#pragma unroll
    for (int e = 0; e < 36; ++e) A[e] = JtJ[e];
#pragma unroll
    for (int e = 0; e < 6; ++e) d[e] = JtErr[e];
#pragma unroll
    for (int e = 0; e < 6; ++e) A[e * 6 + e] *= 1.0 + lambda;
    if (!solve6(A, d))
#pragma unroll
        for (int e = 0; e < 6; ++e) d[e] = 0.0;
#pragma unroll
    for (int e = 0; e < 6; ++e) prm[e] = prev[e] - d[e];
}
// a step that raised the error is retried with more damping, up to lambdaLg10 = 16; an accepted one relaxes it, down to -16
BP_HD bool lm_retry(double errNorm, double prevErrNorm, int* lambdaLg10) { return errNorm > prevErrNorm && ++*lambdaLg10 <= 16; }
BP_HD int lm_relax(int lambdaLg10) { return lambdaLg10 - 1 < -16 ? -16 : lambdaLg10 - 1; }
// the stop test of an accepted step: |prm - prev| / max(|prev|, DBL_MIN) < FLT_EPSILON
BP_HD bool lm_converged(const double* prm, const double* prev) {
    double dn = 0;
#pragma unroll
    for (int i = 0; i < 6; ++i) dn += (prm[i] - prev[i]) * (prm[i] - prev[i]);
    double pn = 0;
#pragma unroll
    for (int i = 0; i < 6; ++i) pn += prev[i] * prev[i];
    const double rel = sqrt(dn) / dmax(sqrt(pn), 2.2250738585072014e-308);
    return rel < (double)1.19209290e-07F;
}
// the minimiser's parameters -> R (cv2.Rodrigues), t; -2 unless every entry is finite
BP_HD int params_to_pose(const double* prm, double* Rout, double* tout) {
    rodrigues_exp(prm, Rout);
    tout[0] = prm[3]; tout[1] = prm[4]; tout[2] = prm[5];
    for (int i = 0; i < 9; ++i)
        if (!(fabs(Rout[i]) <= 1.7976931348623157e308)) return -2;       // isfinite
    for (int i = 0; i < 3; ++i)
        if (!(fabs(tout[i]) <= 1.7976931348623157e308)) return -2;
    return 0;
}
