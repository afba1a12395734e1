// The key-point annotator's arithmetic of O(1) size, ONE source for the host twins (annotate_host.cpp) and the device
// kernels (annotate.hip): the label and the visibility flags of one (pose, key point), the visibility of one rendered
// pixel, the splat of one vertex, the heat-map centre of one part and one value of a target map.  Host and device compile
// this text and do the same f64 / f32 / integer operations in the same order, without FMA contraction, so their outputs
// agree bit for bit; only who loops over what differs per side.
// Plain C++17, no HIP header.  Included inside `namespace bp { namespace {` after <cmath> and <cstdint>, in a unit that
// has `#pragma clang fp contract(off)` in force.
//
// Conventions (DESIGN.md §3.8): the centre of pixel (x, y) lies at image coordinates (x + c, y + c), c = pixel_center,
// as in the rasteriser, so the pixel a projection (u, v) falls in is (floor(u - c + 0.5), floor(v - c + 0.5)).  Boxes
// are (xmin, xmax, ymin, ymax), inclusive, the reference's get_bbox_from_mask order.
#ifndef BP_HD
#if defined(__HIPCC__)
#define BP_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define BP_HD inline
#endif
#endif

constexpr unsigned AN_FRONT = 1u;           // Z >= near
constexpr unsigned AN_IN_IMAGE = 2u;        // the projection falls in a pixel of the image
constexpr unsigned AN_SELF_VISIBLE = 4u;    // the object's own render does not lie in front of the point
constexpr unsigned AN_SCENE_VISIBLE = 8u;   // the scene's depth does not lie more than delta in front of the point
constexpr unsigned AN_SCENE_KNOWN = 16u;    // the scene's depth is present at the point's pixel

constexpr int AN_BOX_INTS = 5;              // accumulator of one box: xmin, xmax, ymin, ymax, count
constexpr int AN_BOX_EMPTY_MIN = INT32_MAX; // (an empty box keeps these; its count stays 0)
constexpr int AN_BOX_EMPTY_MAX = -1;

struct AnCam {
    double fx, skew, cx, fy, cy;
    double c;       // pixel_center
    double near;
};

BP_HD AnCam an_cam(const double* K, double pixel_center, double near) {
    return AnCam{K[0], K[1], K[2], K[4], K[5], pixel_center, near};
}

// X = R m + t, pose = [R|t] row-major 3x4 (raster_math.inc rs_transform's order)
BP_HD void an_transform(const double* pose, const double* m, double* X) {
    X[0] = ((pose[0] * m[0] + pose[1] * m[1]) + pose[2] * m[2]) + pose[3];
    X[1] = ((pose[4] * m[0] + pose[5] * m[1]) + pose[6] * m[2]) + pose[7];
    X[2] = ((pose[8] * m[0] + pose[9] * m[1]) + pose[10] * m[2]) + pose[11];
}

// the reference's project_kp order (multiply, divide, add) plus the skew term
BP_HD void an_project(const AnCam& cam, const double* X, double* u, double* v) {
    *u = (cam.fx * X[0] + cam.skew * X[1]) / X[2] + cam.cx;
    *v = (cam.fy * X[1]) / X[2] + cam.cy;
}

// One (pose, key point).  model_depth: the render of this pose [H][W] or null; scene: the scene depth image of this pose
// [H][W] or null.  Every index is formed only after the pixel has been tested against the image.
BP_HD unsigned an_keypoint(const AnCam& cam, const double* pose, const double* m, int H, int W, const float* model_depth,
                           const float* scene, double self_tol, double delta, double* xy, double* z) {
    double X[3], u, v;
    an_transform(pose, m, X);
    *z = X[2];
    if (!(X[2] >= cam.near)) {
        xy[0] = -1.0;
        xy[1] = -1.0;
        return 0u;
    }
    an_project(cam, X, &u, &v);
    xy[0] = u;
    xy[1] = v;
    unsigned flags = AN_FRONT;
    const double fx = floor((u - cam.c) + 0.5), fy = floor((v - cam.c) + 0.5);
    if (!(fx >= 0.0 && fx < (double)W && fy >= 0.0 && fy < (double)H)) return flags;   // (NaN lands here too)
    flags |= AN_IN_IMAGE;
    const size_t idx = (size_t)(int)fy * W + (int)fx;
    int self = 1, seen = 1;
    if (model_depth) {
        const float D = model_depth[idx];
        if (D > 0.0f && (double)D < X[2] - self_tol) self = 0;      // an uncovered pixel occludes nothing
    }
    if (scene) {
        const float S = scene[idx];
        if (S > 0.0f) flags |= AN_SCENE_KNOWN;
        seen = S == 0.0f || X[2] - (double)S <= delta;
    }
    if (self) flags |= AN_SELF_VISIBLE;
    if (seen) flags |= AN_SCENE_VISIBLE;
    return flags;
}

// metrics.vsd_masks's visib_gt of one covered pixel (D > 0): distances along the pixel's ray, S = 0 is missing
BP_HD int an_pixel_visible(const AnCam& cam, int x, int y, float D, float S, double delta) {
    const double a = (((double)x + cam.c) - cam.cx) / cam.fx;
    const double b = (((double)y + cam.c) - cam.cy) / cam.fy;
    const double r = sqrt((a * a + b * b) + 1.0);
    const double dg = (double)D * r, dt = (double)S * r;
    return dg > 0.0 && ((dg - dt <= delta) || dt == 0.0);
}

// the reference's project_all of one vertex: the pixel (int(x), int(y)), truncated toward zero, counts iff
// 0 < int(x) < W and 0 < int(y) < H -- that is 1 <= x < W and 1 <= y < H, tested before the conversion
BP_HD int an_splat(const AnCam& cam, const double* pose, const double* m, int H, int W, int* ix, int* iy) {
    double X[3], u, v;
    an_transform(pose, m, X);
    an_project(cam, X, &u, &v);
    if (!(u >= 1.0 && u < (double)W && v >= 1.0 && v < (double)H)) return 0;
    *ix = (int)u;
    *iy = (int)v;
    return 1;
}

// generateSampleBox's test of one part against its window and transformBox's centre, in the reference's float32
// arithmetic; round() of the widened value is Python's round-half-to-even.  Returns 0 (centre -1, -1) for a part that is
// not drawn.
BP_HD int an_target_centre(double px, double py, float ulx, float uly, float brx, float bry, int inpH, int inpW, int resH,
                           int* cx, int* cy) {
    *cx = -1;
    *cy = -1;
    if (!(px > 0.0 && px > (double)ulx && py > (double)uly && px < (double)brx && py < (double)bry)) return 0;
    const float c0 = ((brx - 1.0f) - ulx) / 2.0f;
    const float c1 = ((bry - 1.0f) - uly) / 2.0f;
    const float wide = ((brx - ulx) * (float)inpH) / (float)inpW;
    const float tall = bry - uly;
    const float lenH = tall > wide ? tall : wide;
    const float lenW = (lenH * (float)inpW) / (float)inpH;
    float p0 = (float)px - ulx;
    float p1 = (float)py - uly;
    const float m0 = (lenW - 1.0f) / 2.0f - c0;
    const float m1 = (lenH - 1.0f) / 2.0f - c1;
    p0 = p0 + (m0 > 0.0f ? m0 : 0.0f);
    p1 = p1 + (m1 > 0.0f ? m1 : 0.0f);
    const float q0 = (p0 * (float)resH) / lenH;
    const float q1 = (p1 * (float)resH) / lenH;
    *cx = (int)rint((double)q0);
    *cy = (int)rint((double)q1);
    return 1;
}

// drawGaussian's clipped copy of g [size][size] about centre (cx, cy), at map pixel (x, y); an undrawn part (cx < 0)
// and every pixel outside the patch are 0
BP_HD float an_target_value(const float* g, int size, int cx, int cy, int x, int y) {
    if (cx < 0) return 0.0f;
    const int half = size / 2;
    const long long gx = (long long)x - ((long long)cx - half), gy = (long long)y - ((long long)cy - half);
    if (gx < 0 || gx >= size || gy < 0 || gy >= size) return 0.0f;
    return g[gy * size + gx];
}
