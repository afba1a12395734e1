// The colour renderer's arithmetic of O(1) size, ONE source for the host twin (raster_color_host.cpp) and the device
// kernels (raster_color.hip): the 64-bit z-test key, the shading of a winning fragment (its geometry is the textured
// resolve's too, raster_texture_math.inc), the set-up, stepping and colour of
// one edge of a 3-D bounding box and the blend of a rendered pixel over a frame.  Host and device compile this text and do
// the same f64 / integer operations in the same order, without FMA contraction, so their images agree byte for byte.
// Plain C++17, f64 and integers only.  Included right after raster_math.inc (it uses RsCam, rs_transform and the integer
// helpers; ColorLight and COLOR_MAX_IDS, the two things c_api.cpp needs too, are raster.h's), in a unit that has
// `#pragma clang fp contract(off)` in force.  DESIGN.md §3.5 has the definition in words.

// ---- the z-test key: (f32 depth bits << 32) | fragment id, minimum wins: nearest first, then the lowest pose slot, then
// the lowest face.  id = q * F + f with q the CALL's pose slot.  A pixel kept from an earlier call (accumulation) carries
// RC_KEEP as its id, above every fragment's: it gives way only to a fragment of smaller or equal depth bits, and keeps
// its colour unless one arrives.  An untouched pixel holds RC_EMPTY_KEY.
constexpr uint32_t RC_KEEP = 0xFFFFFFFFu;
constexpr unsigned long long RC_EMPTY_KEY = ~0ull;

BP_HD unsigned long long rc_key(uint32_t depth_bits, uint32_t id) { return ((unsigned long long)depth_bits << 32) | id; }

BP_HD double rc_clamp01(double w) { return w < 0.0 ? 0.0 : (w > 1.0 ? 1.0 : w); }

// (P - X) x (Q - X) . n
BP_HD double rc_sub_area(const double* P, const double* Q, const double* X, double nx, double ny, double nz) {
    const double px = P[0] - X[0], py = P[1] - X[1], pz = P[2] - X[2];
    const double qx = Q[0] - X[0], qy = Q[1] - X[1], qz = Q[2] - X[2];
    const double cx = py * qz - pz * qy;
    const double cy = pz * qx - px * qz;
    const double cz = px * qy - py * qx;
    return (cx * nx + cy * ny) + cz * nz;
}

// What the two resolves (vertex colours: rc_shade; texture: raster_texture_math.inc tx_shade) share of a fragment: the
// plane n . X = nd of the triangle with n.n = nn, the clamped perspective-correct weights of its three vertices at the
// point where the pixel's ray meets the plane, and the light weight.
struct RcFrag {
    double nx, ny, nz, nd, nn;
    double wa, wb, wc;
    double light_w;
};

// The fragment of pixel (x, y) on the triangle with camera-space vertices A, B, C IN THE FACE'S OWN ORDER:
// perspective-correct weights at the point X where the pixel's ray meets the triangle's plane (the same clamped f64
// depth rs_depth_bits rounds to f32) and the two-sided diffuse + ambient weight of the reference's fragment shader,
// light_w = min(ambient + 0.5 max(L . N, 0), 1).
BP_HD void rc_fragment(const RsCam& cam, const double* A, const double* B, const double* C, int x, int y, const ColorLight& lt,
                       RcFrag* g) {
    // the plane and the depth exactly as rs_setup / rs_depth_bits compute them
    const double e1x = B[0] - A[0], e1y = B[1] - A[1], e1z = B[2] - A[2];
    const double e2x = C[0] - A[0], e2y = C[1] - A[1], e2z = C[2] - A[2];
    const double nx = e1y * e2z - e1z * e2y;
    const double ny = e1z * e2x - e1x * e2z;
    const double nz = e1x * e2y - e1y * e2x;
    const double nd = (nx * A[0] + ny * A[1]) + nz * A[2];
    const double lo = A[2] < B[2] ? A[2] : B[2], hi = A[2] < B[2] ? B[2] : A[2];
    const double zmin = C[2] < lo ? C[2] : lo;
    const double zmax = C[2] > hi ? C[2] : hi;
    const double dx = (((double)x + cam.c) - cam.cx) / cam.fx;
    const double dy = (((double)y + cam.c) - cam.cy) / cam.fy;
    double z = nd / ((nx * dx + ny * dy) + nz);
    if (!(z >= zmin)) z = zmin;
    if (z > zmax) z = zmax;
    const double X[3] = {z * dx, z * dy, z};

    const double nn = (nx * nx + ny * ny) + nz * nz;
    double wa = 1.0 / 3.0, wb = 1.0 / 3.0, wc = 1.0 / 3.0;
    double Nx = 0.0, Ny = 0.0, Nz = 0.0;
    if (nn > 0.0) {
        const double a = rc_clamp01(rc_sub_area(B, C, X, nx, ny, nz) / nn);
        const double b = rc_clamp01(rc_sub_area(C, A, X, nx, ny, nz) / nn);
        const double c = rc_clamp01(rc_sub_area(A, B, X, nx, ny, nz) / nn);
        const double sum = (a + b) + c;
        if (sum > 0.0) {
            wa = a / sum;
            wb = b / sum;
            wc = c / sum;
        }
        const double len = sqrt(nn);
        Nx = nx / len;
        Ny = ny / len;
        Nz = nz / len;
        if ((Nx * X[0] + Ny * X[1]) + Nz * X[2] > 0.0) {     // two-sided: the normal faces the camera
            Nx = -Nx;
            Ny = -Ny;
            Nz = -Nz;
        }
    }
    const double lx = lt.x - X[0], ly = lt.y - X[1], lz = lt.z - X[2];
    const double ll = sqrt((lx * lx + ly * ly) + lz * lz);
    double diffuse = 0.0;
    if (ll > 0.0) diffuse = ((lx / ll) * Nx + (ly / ll) * Ny) + (lz / ll) * Nz;
    if (!(diffuse > 0.0)) diffuse = 0.0;
    double light_w = lt.ambient + 0.5 * diffuse;
    if (light_w > 1.0) light_w = 1.0;
    g->nx = nx; g->ny = ny; g->nz = nz; g->nd = nd; g->nn = nn;
    g->wa = wa; g->wb = wb; g->wc = wc;
    g->light_w = light_w;
}

// a channel of the image from its unlit value `base` (0 .. 255) and the light weight
BP_HD unsigned char rc_lit(double light_w, double base) {
    const double v = floor(light_w * base + 0.5);
    return (unsigned char)(v >= 255.0 ? 255 : (v > 0.0 ? (int)v : 0));
}

// Colour of that fragment from the vertex colours ca, cb, cc [3] u8: their mix by the fragment's weights, lit.
BP_HD void rc_shade(const RsCam& cam, const double* A, const double* B, const double* C, const unsigned char* ca,
                    const unsigned char* cb, const unsigned char* cc, int x, int y, const ColorLight& lt, unsigned char* out) {
    RcFrag g;
    rc_fragment(cam, A, B, C, x, y, lt, &g);
#pragma unroll
    for (int k = 0; k < 3; ++k) out[k] = rc_lit(g.light_w, (g.wa * (double)ca[k] + g.wb * (double)cb[k]) + g.wc * (double)cc[k]);
}

// ---- 3-D bounding boxes: the 12 edges of the reference's Model3D._compute_bbox between its 8 corners
// (min/max x outermost, then z, then y: corner k = (x: k & 4, z: k & 2, y: k & 1))
constexpr int RC_BOX_EDGES = 12;
constexpr double RC_LINE_RANGE = 1048576.0;     // projected segments are clipped to +-2^20 px before snapping

BP_HD void rc_box_edge(int e, int* ia, int* ib) {
    // edges (0,1) (0,2) (3,1) (3,2) (4,5) (4,6) (7,5) (7,6) (0,4) (1,5) (2,6) (3,7), one nibble per edge, edge 0 lowest
    *ia = (int)((0x321077443300ull >> (4 * e)) & 15);
    *ib = (int)((0x765465652121ull >> (4 * e)) & 15);
}

// one Liang-Barsky boundary: keeps the part of [t0, t1] where p + t d <= lim (selects, not stores through a chosen
// pointer: t0 and t1 stay in registers on the device)
BP_HD int rc_clip_le(double p, double d, double lim, double* t0, double* t1) {
    if (d == 0.0) return p <= lim;
    const double t = (lim - p) / d;
    const double a = *t0, b = *t1;
    *t1 = (d > 0.0 && t < b) ? t : b;
    *t0 = (d < 0.0 && t > a) ? t : a;
    return *t0 <= *t1;
}

struct RcEdge {
    int major_x;            // 1: the edge is stepped along x, 0: along y
    int m0, n0, m1, n1;     // snapped end points (1/256 px) as (major, minor), ordered so that m0 <= m1
    int ia, ib;             // the corners at (m0, n0) and (m1, n1)
    int p0, p1;             // major-axis pixel positions to draw, inclusive, clamped to the image
};

BP_HD long long rc_floor_div64(long long a, long long b) { return a >= 0 ? a / b : -((-a + b - 1) / b); }   // b > 0

// Edge e of the box with object-frame corners [8][3] at `pose`.  The camera-space segment is clipped against z = near by
// its parameter (dropped when wholly behind, shortened when it crosses), projected to pixel-index coordinates, clipped
// to +-2^20 px (so the snapped integers cannot overflow; an image is 2^24 pixels at most), snapped to 1/256 px.  Returns 0
// when nothing of it can be drawn.
BP_HD int rc_edge_setup(const RsCam& cam, const double* pose, const double* corners, int e, int H, int W, RcEdge* out) {
    int ia, ib;
    rc_box_edge(e, &ia, &ib);
    double A[3], B[3];
    rs_transform(pose, corners[ia * 3 + 0], corners[ia * 3 + 1], corners[ia * 3 + 2], A);
    rs_transform(pose, corners[ib * 3 + 0], corners[ib * 3 + 1], corners[ib * 3 + 2], B);
    const int a_in = A[2] >= cam.near, b_in = B[2] >= cam.near;
    if (!a_in && !b_in) return 0;                              // (a NaN depth counts as behind)
    if (!a_in) {                                               // (no pointer to A or B: they stay in registers)
        if (!(A[2] < cam.near)) return 0;                      // NaN
        const double t = (cam.near - A[2]) / (B[2] - A[2]);
        A[0] = A[0] + t * (B[0] - A[0]);
        A[1] = A[1] + t * (B[1] - A[1]);
        A[2] = cam.near;
    } else if (!b_in) {
        if (!(B[2] < cam.near)) return 0;
        const double t = (cam.near - B[2]) / (A[2] - B[2]);
        B[0] = B[0] + t * (A[0] - B[0]);
        B[1] = B[1] + t * (A[1] - B[1]);
        B[2] = cam.near;
    }
    double ua = (cam.fx * (A[0] / A[2]) + cam.cx) - cam.c, va = (cam.fy * (A[1] / A[2]) + cam.cy) - cam.c;
    double ub = (cam.fx * (B[0] / B[2]) + cam.cx) - cam.c, vb = (cam.fy * (B[1] / B[2]) + cam.cy) - cam.c;
    if (!(fabs(ua) <= 1e300) || !(fabs(va) <= 1e300) || !(fabs(ub) <= 1e300) || !(fabs(vb) <= 1e300)) return 0;
    const double du = ub - ua, dv = vb - va;
    double t0 = 0.0, t1 = 1.0;
    if (!rc_clip_le(ua, du, RC_LINE_RANGE, &t0, &t1) || !rc_clip_le(-ua, -du, RC_LINE_RANGE, &t0, &t1) ||
        !rc_clip_le(va, dv, RC_LINE_RANGE, &t0, &t1) || !rc_clip_le(-va, -dv, RC_LINE_RANGE, &t0, &t1))
        return 0;
    if (t1 < 1.0) { ub = ua + t1 * du; vb = va + t1 * dv; }
    if (t0 > 0.0) { ua = ua + t0 * du; va = va + t0 * dv; }
    if (!(fabs(ua) <= 2.0 * RC_LINE_RANGE) || !(fabs(va) <= 2.0 * RC_LINE_RANGE) || !(fabs(ub) <= 2.0 * RC_LINE_RANGE) ||
        !(fabs(vb) <= 2.0 * RC_LINE_RANGE))
        return 0;
    const int xa = (int)rint(ua * (double)RS_SUB), ya = (int)rint(va * (double)RS_SUB);
    const int xb = (int)rint(ub * (double)RS_SUB), yb = (int)rint(vb * (double)RS_SUB);
    const int adx = xb >= xa ? xb - xa : xa - xb, ady = yb >= ya ? yb - ya : ya - yb;
    out->major_x = adx >= ady;
    int ma = out->major_x ? xa : ya, na = out->major_x ? ya : xa;
    int mb = out->major_x ? xb : yb, nb = out->major_x ? yb : xb;
    if (ma <= mb) { out->m0 = ma; out->n0 = na; out->m1 = mb; out->n1 = nb; out->ia = ia; out->ib = ib; }
    else          { out->m0 = mb; out->n0 = nb; out->m1 = ma; out->n1 = na; out->ia = ib; out->ib = ia; }
    // the pixels whose centre 256 p lies in [m0, m1], clamped to the image BEFORE any loop
    out->p0 = rs_imax(0, rs_ceil_div(out->m0, RS_SUB));
    out->p1 = rs_imin((out->major_x ? W : H) - 1, rs_floor_div(out->m1, RS_SUB));
    return out->p1 >= out->p0;
}

// minor-axis pixel of the edge at major-axis pixel p (p0 <= p <= p1), rounded to nearest, halves up; the caller tests it
// against the image
BP_HD long long rc_edge_minor(const RcEdge& g, int p) {
    const long long dm = (long long)g.m1 - g.m0;
    if (dm == 0) return rc_floor_div64((long long)g.n0 + RS_SUB / 2, RS_SUB);
    const long long a = (long long)p * RS_SUB - g.m0;                                  // 0 .. dm
    const long long num = (long long)g.n0 * dm + ((long long)g.n1 - g.n0) * a;          // minor coordinate * dm, |.| < 2^59
    return rc_floor_div64(2 * num + RS_SUB * dm, 2 * RS_SUB * dm);
}

// colour of that pixel: the two corner colours mixed linearly by the position along the snapped edge, integers, rounded
// to nearest
BP_HD void rc_edge_color(const RcEdge& g, int p, const unsigned char* corner_colors, unsigned char* out) {
    const long long dm = (long long)g.m1 - g.m0;
    const long long a = (long long)p * RS_SUB - g.m0;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const long long c0 = corner_colors[g.ia * 3 + k], c1 = corner_colors[g.ib * 3 + k];
        out[k] = (unsigned char)(dm == 0 ? c0 : (c0 * (dm - a) + c1 * a + dm / 2) / dm);
    }
}

// ---- compositing: a rendered pixel over a frame pixel, alpha in 0 .. 256
BP_HD unsigned char rc_blend(int alpha, unsigned char color, unsigned char frame) {
    return (unsigned char)((alpha * (int)color + (256 - alpha) * (int)frame + 128) >> 8);
}
