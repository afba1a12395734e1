// The depth rasteriser's arithmetic of O(1) size, ONE source for the host renderer (raster_host.cpp render_depth_host) and
// the device kernels (raster.hip): the camera transform of a vertex, its projection and snapping, the set-up of a
// triangle, the coverage test of a pixel and the depth at a covered pixel.  Host and device compile this text and do the
// same f64 / integer operations in the same order, without FMA contraction, so their images agree bit for bit; who loops
// over a pose's triangles and their pixels is raster_walk.inc, one source too.
// Plain C++17, no HIP header.  Included inside `namespace bp { namespace {` after <cmath>, <cstdint> and raster.h (the
// camera, RsCam, is raster.h's: the launchers take it), in a unit that has `#pragma clang fp contract(off)` in force.
//
// Conventions (DESIGN.md §3.5): the centre of pixel (x, y) lies at image coordinates (x + c, y + c), c = pixel_center.
// Projected vertices are snapped to 1/256 px in PIXEL-INDEX coordinates (u - c, v - c), so that the centre of pixel x is
// the integer 256 x.  Coverage is decided by int64 edge functions of the snapped vertices with the top-left fill rule,
// both windings.  Depth is NOT interpolated from the snapped vertices: it is the f64 intersection of the pixel's ray with
// the triangle's camera-space plane, clamped to the triangle's depth range, rounded to f32.
#ifndef BP_HD
#if defined(__HIPCC__)
#define BP_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define BP_HD inline
#endif
#endif

constexpr int RS_SUB = 256;                     // sub-pixel steps per pixel
constexpr double RS_MAX_UV = 16384.0;           // |u|, |v| beyond 2^14 px: the triangle is skipped (and counted)
constexpr int RS_INVALID = INT32_MIN;           // snapped x of a vertex that fails the near / range test
constexpr uint32_t RS_EMPTY = 0x7f800000u;      // +inf: the z-buffer's cleared value
constexpr int RS_COOP_AREA = 256;               // bounding boxes above this many pixels are rasterised by the whole wave

// vertex of the posed mesh in the camera frame: X = R x + t, pose = [R|t] row-major 3x4
BP_HD void rs_transform(const double* pose, double x, double y, double z, double* X) {
    X[0] = ((pose[0] * x + pose[1] * y) + pose[2] * z) + pose[3];
    X[1] = ((pose[4] * x + pose[5] * y) + pose[6] * z) + pose[7];
    X[2] = ((pose[8] * x + pose[9] * y) + pose[10] * z) + pose[11];
}

// projection, snapped to 1/256 px in pixel-index coordinates; (RS_INVALID, 0) for a vertex nearer than `near`, out of
// the +-2^14 px range or not finite
BP_HD void rs_project(const RsCam& cam, const double* X, int* sx, int* sy) {
    *sx = RS_INVALID;
    *sy = 0;
    if (!(X[2] >= cam.near)) return;
    const double u = cam.fx * (X[0] / X[2]) + cam.cx;
    const double v = cam.fy * (X[1] / X[2]) + cam.cy;
    if (!(fabs(u) <= RS_MAX_UV) || !(fabs(v) <= RS_MAX_UV)) return;
    *sx = (int)rint((u - cam.c) * (double)RS_SUB);
    *sy = (int)rint((v - cam.c) * (double)RS_SUB);
}

// everything a pixel needs of one triangle
struct RsTri {
    int x0, y0, x1, y1, x2, y2;     // snapped vertices, ordered so that the doubled area is positive
    int bx0, by0, bx1, by1;         // pixel bounding box clamped to the image, inclusive; empty when bx1 < bx0 or by1 < by0
    double nx, ny, nz, nd;          // camera-space plane n . X = nd
    double zmin, zmax;              // depth range of the three vertices
};

BP_HD int rs_imin(int a, int b) { return a < b ? a : b; }
BP_HD int rs_imax(int a, int b) { return a < b ? b : a; }
BP_HD int rs_floor_div(int a, int b) { return a >= 0 ? a / b : -((-a + b - 1) / b); }   // b > 0
BP_HD int rs_ceil_div(int a, int b) { return a >= 0 ? (a + b - 1) / b : -(-a / b); }    // b > 0

// Set-up from three camera-space vertices A, B, C and their snapped projections (all valid).  Returns 0 when the snapped
// area is zero or the clamped bounding box holds no pixel centre: nothing to draw.
BP_HD int rs_setup(const double* A, const double* B, const double* C, int ax, int ay, int bx, int by, int cx, int cy,
                   int H, int W, RsTri* t) {
    const long long area = (long long)(bx - ax) * (cy - ay) - (long long)(by - ay) * (cx - ax);
    if (area == 0) return 0;
    t->x0 = ax; t->y0 = ay;
    if (area > 0) { t->x1 = bx; t->y1 = by; t->x2 = cx; t->y2 = cy; }
    else          { t->x1 = cx; t->y1 = cy; t->x2 = bx; t->y2 = by; }
    // pixels whose centre 256 x lies in [min, max] of the snapped vertices, clamped to the image BEFORE any loop
    const int xmin = rs_imin(ax, rs_imin(bx, cx)), xmax = rs_imax(ax, rs_imax(bx, cx));
    const int ymin = rs_imin(ay, rs_imin(by, cy)), ymax = rs_imax(ay, rs_imax(by, cy));
    t->bx0 = rs_imax(0, rs_ceil_div(xmin, RS_SUB));
    t->bx1 = rs_imin(W - 1, rs_floor_div(xmax, RS_SUB));
    t->by0 = rs_imax(0, rs_ceil_div(ymin, RS_SUB));
    t->by1 = rs_imin(H - 1, rs_floor_div(ymax, RS_SUB));
    if (t->bx1 < t->bx0 || t->by1 < t->by0) return 0;
    // plane through the camera-space vertices, n = (B - A) x (C - A)
    const double e1x = B[0] - A[0], e1y = B[1] - A[1], e1z = B[2] - A[2];
    const double e2x = C[0] - A[0], e2y = C[1] - A[1], e2z = C[2] - A[2];
    t->nx = e1y * e2z - e1z * e2y;
    t->ny = e1z * e2x - e1x * e2z;
    t->nz = e1x * e2y - e1y * e2x;
    t->nd = (t->nx * A[0] + t->ny * A[1]) + t->nz * A[2];
    const double lo = A[2] < B[2] ? A[2] : B[2], hi = A[2] < B[2] ? B[2] : A[2];
    t->zmin = C[2] < lo ? C[2] : lo;
    t->zmax = C[2] > hi ? C[2] : hi;
    return 1;
}

// edge function of the directed edge a -> b at p (all in 1/256 px), with the top-left rule folded in: > 0 means inside
// or on an edge that owns its pixels.  With the doubled area positive in image coordinates (y down) the interior lies
// where every edge function is positive; an edge going up (dy < 0) is a left edge, a horizontal edge going right
// (dy == 0, dx > 0) is a top edge.
BP_HD long long rs_edge(int ax, int ay, int bx, int by, int px, int py) {
    const long long dx = (long long)bx - ax, dy = (long long)by - ay;
    const long long e = dx * ((long long)py - ay) - dy * ((long long)px - ax);
    const int owns = dy < 0 || (dy == 0 && dx > 0);
    return e + owns;
}

BP_HD int rs_covers(const RsTri& t, int x, int y) {
    const int px = x * RS_SUB, py = y * RS_SUB;
    return rs_edge(t.x0, t.y0, t.x1, t.y1, px, py) > 0 && rs_edge(t.x1, t.y1, t.x2, t.y2, px, py) > 0 &&
           rs_edge(t.x2, t.y2, t.x0, t.y0, px, py) > 0;
}

// depth of the triangle's plane along the ray of pixel (x, y), clamped to the triangle's range, as f32 bits; positive
// floats order as unsigned integers, so the z-buffer is a min over these
BP_HD uint32_t rs_depth_bits(const RsCam& cam, const RsTri& t, int x, int y) {
    const double dx = (((double)x + cam.c) - cam.cx) / cam.fx;
    const double dy = (((double)y + cam.c) - cam.cy) / cam.fy;
    double z = t.nd / ((t.nx * dx + t.ny * dy) + t.nz);
    if (!(z >= t.zmin)) z = t.zmin;     // (also what a NaN or a ray parallel to the plane becomes)
    if (z > t.zmax) z = t.zmax;
    const float f = (float)z;
    uint32_t bits;
    __builtin_memcpy(&bits, &f, 4);
    return bits;
}
