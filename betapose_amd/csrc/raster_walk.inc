// The walk over a posed mesh's triangles and the pixels of their bounding boxes, ONE source for the depth and the colour
// rasteriser on both sides: raster_host.cpp and raster_color_host.cpp call rs_walk_host, raster_tri_kernel (raster.hip)
// and color_visibility_kernel (raster_color.hip) call rs_walk.  What differs between depth and colour is the SINK, what
// becomes of a covered pixel: sink(at, bits, face) with at = y * W + x, bits the f32 depth bits there and face the index of
// the triangle that covers it.  A sink keeps a minimum (of the bits, or of rc_key(bits, id of the face)), which does not
// depend on the order of its operands, so host and device images are equal bit for bit whoever walks.
// Included right after raster_math.inc, under the same conditions; plain C++17 with no HIP header unless the unit asks
// for the device walk with RS_WALK_DEVICE.

// One triangle from its vertex indices, with the posed mesh's camera-space X [n][3] and snapped S [n][2]: 1 = *t is set
// up, 0 = nothing to draw, -1 = skipped (an index outside [0, n), or a vertex that failed the near / range test), which
// the caller counts.
BP_HD int rs_triangle(int ia, int ib, int ic, int n, const double* X, const int* S, int H, int W, RsTri* t) {
    if ((unsigned)ia >= (unsigned)n || (unsigned)ib >= (unsigned)n || (unsigned)ic >= (unsigned)n) return -1;
    // (on the device both halves of a snapped vertex are fetched before the test and the nine coordinates before the
    // set-up's early returns: each group is one round trip to memory)
    const int ax = S[(size_t)ia * 2], ay = S[(size_t)ia * 2 + 1];
    const int bx = S[(size_t)ib * 2], by = S[(size_t)ib * 2 + 1];
    const int cx = S[(size_t)ic * 2], cy = S[(size_t)ic * 2 + 1];
    if (ax == RS_INVALID || bx == RS_INVALID || cx == RS_INVALID) return -1;
    double A[3], B[3], C[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        A[k] = X[(size_t)ia * 3 + k];
        B[k] = X[(size_t)ib * 3 + k];
        C[k] = X[(size_t)ic * 3 + k];
    }
    return rs_setup(A, B, C, ax, ay, bx, by, cx, cy, H, W, t);
}

template <class Sink>
BP_HD void rs_pixel(const RsCam& cam, const RsTri& t, int x, int y, int W, int face, const Sink& sink) {
    if (rs_covers(t, x, y)) sink((size_t)y * W + x, rs_depth_bits(cam, t, x, y), face);
}

// Host: one pose.  Transforms and projects the n vertices into the caller's X [n][3] and S [n][2], draws the F triangles
// (indices checked by the caller) and returns how many were skipped.
template <class Sink>
inline int rs_walk_host(const RsCam& cam, const double* pose, const double* vertices, int n, const int* faces, int F, int H,
                        int W, double* X, int* S, const Sink& sink) {
    for (int i = 0; i < n; ++i) {
        rs_transform(pose, vertices[i * 3 + 0], vertices[i * 3 + 1], vertices[i * 3 + 2], &X[(size_t)i * 3]);
        rs_project(cam, &X[(size_t)i * 3], &S[(size_t)i * 2], &S[(size_t)i * 2 + 1]);
    }
    int skip = 0;
    for (int f = 0; f < F; ++f) {
        RsTri t;
        const int have = rs_triangle(faces[f * 3 + 0], faces[f * 3 + 1], faces[f * 3 + 2], n, X, S, H, W, &t);
        skip += have < 0;
        if (have <= 0) continue;
        for (int y = t.by0; y <= t.by1; ++y)
            for (int x = t.bx0; x <= t.bx1; ++x) rs_pixel(cam, t, x, y, W, f, sink);
    }
    return skip;
}

#ifdef RS_WALK_DEVICE      // defined by a unit that has the HIP runtime header: the kernels' side
__device__ __forceinline__ RsTri rs_broadcast(const RsTri& t, int src) {
    RsTri u;
    u.x0 = __shfl(t.x0, src, 64); u.y0 = __shfl(t.y0, src, 64);
    u.x1 = __shfl(t.x1, src, 64); u.y1 = __shfl(t.y1, src, 64);
    u.x2 = __shfl(t.x2, src, 64); u.y2 = __shfl(t.y2, src, 64);
    u.bx0 = __shfl(t.bx0, src, 64); u.by0 = __shfl(t.by0, src, 64);
    u.bx1 = __shfl(t.bx1, src, 64); u.by1 = __shfl(t.by1, src, 64);
    u.nx = __shfl(t.nx, src, 64); u.ny = __shfl(t.ny, src, 64);
    u.nz = __shfl(t.nz, src, 64); u.nd = __shfl(t.nd, src, 64);
    u.zmin = __shfl(t.zmin, src, 64); u.zmax = __shfl(t.zmax, src, 64);
    return u;
}

// The lane's triangle f and its vertex indices (-1 each where f >= F): fetched once by the kernel, above its loop over
// the poses of a grid column, so that a pose costs no second fetch
struct RsFace {
    int f, a, b, c;
};
__device__ __forceinline__ RsFace rs_face(const int* __restrict__ faces, int F, int f) {
    RsFace r{f, -1, -1, -1};
    if (f < F) {
        r.a = faces[(size_t)f * 3 + 0];
        r.b = faces[(size_t)f * 3 + 1];
        r.c = faces[(size_t)f * 3 + 2];
    }
    return r;
}

// Device: triangle `face` of one pose (X, S: the pose's rows of the vertex workspace), one lane per triangle; every lane of the
// block calls it, whether or not f < F, since the ballots see whole waves.  A lane walks a small clamped box alone.  A
// triangle whose box holds more than RS_COOP_AREA pixels (a close-up box: 12 triangles over the whole frame) is left for
// the wave: the big lanes are collected with __ballot, each one's set-up is broadcast and the box's pixels are strided
// over the 64 lanes, the sink told the SOURCE lane's face.  No worklist, no second launch.  Every pixel loop runs over a
// box that rs_setup has clamped to the image, so every index a sink gets is in range by construction.  ADDS the wave's
// skipped triangles to *skipped.
template <class Sink>
__device__ __forceinline__ void rs_walk(const RsCam& cam, const RsFace& face, int F, int n, const double* __restrict__ X,
                                        const int* __restrict__ S, int H, int W, int* __restrict__ skipped,
                                        const Sink& sink) {
    const int lane = threadIdx.x & 63, f = face.f;
    RsTri t = {};
    int have = 0;
    if (f < F) have = rs_triangle(face.a, face.b, face.c, n, X, S, H, W, &t);
    const unsigned long long sk = __ballot(have < 0);
    if (lane == 0 && sk) atomicAdd(skipped, (int)__popcll(sk));

    int big = 0;
    if (have > 0) {
        const int w = t.bx1 - t.bx0 + 1, h = t.by1 - t.by0 + 1;   // w * h <= H * W <= 2^24
        if (w * h > RS_COOP_AREA) {
            big = 1;
        } else {
            for (int y = t.by0; y <= t.by1; ++y)
                for (int x = t.bx0; x <= t.bx1; ++x) rs_pixel(cam, t, x, y, W, f, sink);
        }
    }
    // the wave takes its big triangles one after the other, 64 pixels of the box at a time
    unsigned long long todo = __ballot(big);
    while (todo) {
        const int src = __ffsll((long long)todo) - 1;
        todo &= todo - 1;
        const RsTri u = rs_broadcast(t, src);
        const int w = u.bx1 - u.bx0 + 1, cnt = w * (u.by1 - u.by0 + 1);
        for (int k = lane; k < cnt; k += 64) rs_pixel(cam, u, u.bx0 + k % w, u.by0 + k / w, W, f - lane + src, sink);
    }
}
#endif
