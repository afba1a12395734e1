// The depth refinement's arithmetic of O(1) size, ONE source for the host twin (icp_host.cpp) and the device kernels
// (icp.hip): the accept / reject decision of a pixel with its normal, residual and Jacobian row, one term of the normal
// equations, and the step of a pose -- guards, the 6x6 solve, the update and the final verdict.  Host and device compile
// this text and do the same f64 operations in the same order, without FMA contraction, so every per-pixel decision and
// value has the same bits on both sides; only the order in which the pixels' terms are summed differs.
// Plain C++17, no HIP header.  Included inside `namespace bp { namespace {` after icp.h (IcpParams) and pnp_math.inc
// (solve6, rodrigues_exp, mul33), in a unit that has `#pragma clang fp contract(off)` in force.
//
// Definition (DESIGN.md §3.5, metrics.refine_poses_depth).  z_r is the render of the mesh at the current pose, z_t the test
// depth.  A pixel (x, y) takes part when its own render and its four neighbours' (x +- 1, y), (x, y +- 1) are inside the
// image and drawn and z_t != 0.  Ray d = ((x + c - cx) / fx, (y + c - cy) / fy, 1), model point q = z_r d, normal
// n = m / |m| of m = (q(x+1,y) - q(x-1,y)) x (q(x,y+1) - q(x,y-1)) turned so that n.d <= 0.  Rejected: |m| = 0,
// -(n.d) / |d| < min_cos, |z_t - z_r| > max_dist.  Residual r = (z_t - z_r) (n.d) = (s - q).n with s the observed point on
// the same ray; the twist is taken about the object's origin, q_c = q - t, J = [q_c x n, n].

constexpr double ICP_RUNNING = -1.0;    // stats[5] while a pose is still iterated; never returned
constexpr double ICP_OK = 0.0;          // every iteration was taken
constexpr double ICP_TOO_FEW = 1.0;     // fewer than min_pixels pixels took part: no step from there
constexpr double ICP_SINGULAR = 2.0;    // solve6 found no pivot
constexpr double ICP_DIVERGED = 3.0;    // |omega| > 0.5 rad or |v| > 4 max_dist: the pose before that step is kept
constexpr double ICP_REJECTED = 4.0;    // the rms residual grew: the input pose is returned bit for bit
constexpr double ICP_NO_IMAGE = 5.0;    // test index outside [0, T): pose unchanged

constexpr double ICP_MAX_OMEGA = 0.5;
constexpr double ICP_MAX_V_DISTS = 4.0;

// Pixel (x, y) with 1 <= x <= W - 2, 1 <= y <= H - 2: zc its render, zl / zr / zu / zd those of (x-1, y), (x+1, y),
// (x, y-1), (x, y+1) (0 = nothing drawn), zt its test depth (0 = missing), t the pose's translation.  Returns 1 and
// fills J[6], r for a pixel that takes part, else 0.
BP_HD int icp_pixel(const IcpParams& p, int x, int y, double zc, double zl, double zr, double zu, double zd, double zt,
                    const double* t, double* J, double* r) {
    if (!(zc > 0.0 && zl > 0.0 && zr > 0.0 && zu > 0.0 && zd > 0.0) || zt == 0.0) return 0;
    const double dx = (((double)x + p.c) - p.cx) / p.fx;
    const double dy = (((double)y + p.c) - p.cy) / p.fy;
    const double dxl = (((double)(x - 1) + p.c) - p.cx) / p.fx, dxr = (((double)(x + 1) + p.c) - p.cx) / p.fx;
    const double dyu = (((double)(y - 1) + p.c) - p.cy) / p.fy, dyd = (((double)(y + 1) + p.c) - p.cy) / p.fy;
    // a = q(x+1, y) - q(x-1, y), b = q(x, y+1) - q(x, y-1)
    const double ax = zr * dxr - zl * dxl, ay = zr * dy - zl * dy, az = zr - zl;
    const double bx = zd * dx - zu * dx, by = zd * dyd - zu * dyu, bz = zd - zu;
    double nx = ay * bz - az * by, ny = az * bx - ax * bz, nz = ax * by - ay * bx;
    const double len = sqrt((nx * nx + ny * ny) + nz * nz);
    if (!(len > 0.0)) return 0;
    nx /= len; ny /= len; nz /= len;
    double nd = (nx * dx + ny * dy) + nz;
    if (nd > 0.0) { nx = -nx; ny = -ny; nz = -nz; nd = -nd; }
    const double dl = sqrt((dx * dx + dy * dy) + 1.0);
    if (-nd / dl < p.min_cos) return 0;
    const double dz = zt - zc;
    if (fabs(dz) > p.max_dist) return 0;
    *r = dz * nd;
    const double qx = zc * dx - t[0], qy = zc * dy - t[1], qz = zc - t[2];
    J[0] = qy * nz - qz * ny;
    J[1] = qz * nx - qx * nz;
    J[2] = qx * ny - qy * nx;
    J[3] = nx; J[4] = ny; J[5] = nz;
    return 1;
}

// acc[ICP_ACC] += one pixel's term: J^T J (upper triangle, row by row), J^T r, 1, r^2
BP_HD void icp_add(double* acc, const double* J, double r) {
    int k = 0;
#pragma unroll
    for (int i = 0; i < 6; ++i)
#pragma unroll
        for (int j = i; j < 6; ++j) acc[k++] += J[i] * J[j];
#pragma unroll
    for (int i = 0; i < 6; ++i) acc[21 + i] += J[i] * r;
    acc[27] += 1.0;
    acc[28] += r * r;
}

BP_HD void icp_init(const double* pose_in, bool has_image, double* pose, double* stats) {
#pragma unroll
    for (int i = 0; i < 12; ++i) pose[i] = pose_in[i];
#pragma unroll
    for (int i = 0; i < ICP_STATS; ++i) stats[i] = 0.0;
    stats[5] = has_image ? ICP_RUNNING : ICP_NO_IMAGE;
}

// Accumulation number k (0 .. iterations) of a pose that is still running: records N and the rms residual, then either
// ends the pose (the last accumulation, or a guard) or solves A xi = b, xi = (omega, v), and sets R <- exp(omega) R,
// t <- t + v.  A pose that ends with a larger rms than it began with gets its input pose back, bit for bit; its stats then
// describe that pose.
BP_HD void icp_step(const double* acc, int k, const IcpParams& p, const double* pose_in, double* pose, double* stats) {
    const double N = acc[27];
    const double rms = N > 0.0 ? sqrt(acc[28] / N) : 0.0;
    if (k == 0) { stats[0] = N; stats[1] = rms; }
    stats[2] = N;
    stats[3] = rms;
    double status = ICP_RUNNING;
    double A[36], xi[6];
    if (k >= p.iterations) {
        status = ICP_OK;
    } else if (N < (double)p.min_pixels) {
        status = ICP_TOO_FEW;
    } else {
        int e = 0;
#pragma unroll
        for (int i = 0; i < 6; ++i)
#pragma unroll
            for (int j = i; j < 6; ++j) { A[i * 6 + j] = acc[e]; A[j * 6 + i] = acc[e]; ++e; }
#pragma unroll
        for (int i = 0; i < 6; ++i) xi[i] = acc[21 + i];
        if (!solve6(A, xi)) {
            status = ICP_SINGULAR;
        } else {
            const double w = sqrt((xi[0] * xi[0] + xi[1] * xi[1]) + xi[2] * xi[2]);
            const double v = sqrt((xi[3] * xi[3] + xi[4] * xi[4]) + xi[5] * xi[5]);
            if (!(w <= ICP_MAX_OMEGA) || !(v <= ICP_MAX_V_DISTS * p.max_dist)) status = ICP_DIVERGED;
        }
    }
    if (status == ICP_RUNNING) {
        double E[9], R[9], Rn[9];
        rodrigues_exp(xi, E);
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
            for (int j = 0; j < 3; ++j) R[i * 3 + j] = pose[i * 4 + j];
        mul33(E, R, Rn);
#pragma unroll
        for (int i = 0; i < 3; ++i) {
#pragma unroll
            for (int j = 0; j < 3; ++j) pose[i * 4 + j] = Rn[i * 3 + j];
            pose[i * 4 + 3] += xi[3 + i];
        }
        stats[4] += 1.0;
        return;
    }
    if (stats[3] > stats[1]) {
        status = ICP_REJECTED;
#pragma unroll
        for (int i = 0; i < 12; ++i) pose[i] = pose_in[i];
        stats[2] = stats[0];
        stats[3] = stats[1];
    }
    stats[5] = status;
}
