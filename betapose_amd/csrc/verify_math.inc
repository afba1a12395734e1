// Pose verification by gradient agreement, ONE source for the host twin (verify_host.cpp) and the kernels (verify.hip):
// the arithmetic of one pixel (DESIGN.md 3.18; the reference's verify_6D_poses, utils/utils.py:558-610).
//   gray    (4899 R + 9617 G + 1868 B + 8192) >> 14 of a uint8 pixel
//   Sobel   ksize 5, separable: d = [-1, -2, 0, 2, 1], s = [1, 4, 6, 4, 1]; gx = s along y then d along x, gy = d along
//           y then s along x (correlation), border reflect-101.  |g| <= 255 * 3 * 16 = 12240, gx^2 + gy^2 fits an int32
//   mask    a pixel is kept iff m2 = gx^2 + gy^2 >= min_sq, in integers
//   unit    mag = sqrtf((float)m2) + 0.001f, n = (float)g / mag -- square root and quotient correctly rounded to f32,
//           spelled through f64 (exact for both: 53 >= 2 * 24 + 2), so no compiler flag can make the two sides differ
//   term    q = lrintf(|rnx snx + rny sny| * 2^24), two products, one sum, no contraction; the sum of the q is an integer
// Everything up to the unit vectors is integer and the sum is integer, so host and device agree byte for byte and the
// result does not depend on the order of the pixels.
// Plain C++17, no HIP header.  Included inside `namespace bp { namespace {` after <cmath> and <cstdint>, in a unit that
// has `#pragma clang fp contract(off)` in force.
#ifndef BP_HD
#if defined(__HIPCC__)
#define BP_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define BP_HD inline
#endif
#endif

constexpr int VF_HALO = 2;                     // pixels a 5-tap stencil reaches on each side

BP_HD int vf_gray(int r, int g, int b) { return (4899 * r + 9617 * g + 1868 * b + 8192) >> 14; }

// reflect-101 of an index i in [-n + 1, 2 n - 2]: -1 -> 1, -2 -> 2, n -> n - 2, n + 1 -> n - 3
BP_HD int vf_reflect(int i, int n) { return i < 0 ? -i : (i >= n ? 2 * n - 2 - i : i); }

// the vertical pass of one column: five grays, top to bottom
BP_HD void vf_column(int g0, int g1, int g2, int g3, int g4, int& vs, int& vd) {
    vs = g0 + 4 * g1 + 6 * g2 + 4 * g3 + g4;
    vd = -g0 - 2 * g1 + 2 * g3 + g4;
}

// the horizontal pass over five columns' vertical sums, left to right
BP_HD void vf_row(const int* vs, const int* vd, int& gx, int& gy) {
    gx = -vs[0] - 2 * vs[1] + 2 * vs[3] + vs[4];
    gy = vd[0] + 4 * vd[1] + 6 * vd[2] + 4 * vd[3] + vd[4];
}

struct VfUnit {
    float nx, ny, mag;                         // a masked pixel: all three 0
};

// the unit gradient of a pixel; false (and zeros) where it is masked
BP_HD bool vf_unit(int gx, int gy, int min_sq, VfUnit& u) {
    const int m2 = gx * gx + gy * gy;
    if (m2 < min_sq) {
        u.nx = u.ny = u.mag = 0.0f;
        return false;
    }
    const float mag = (float)sqrt((double)(float)m2) + 0.001f;
    u.nx = (float)((double)gx / (double)mag);
    u.ny = (float)((double)gy / (double)mag);
    u.mag = mag;
    return true;
}

// one pixel's term of the sum, in units of 2^-24.  Unit vectors give t <= 1 + a few ulp; a scene gradient that is none
// (NaN, or longer than 2) counts 0, so that the conversion is defined on both sides.
BP_HD uint32_t vf_term(float rnx, float rny, float snx, float sny) {
    const float a = rnx * snx;
    const float b = rny * sny;
    const float t = fabsf(a + b);
    if (!(t <= 2.0f)) return 0u;
    return (uint32_t)lrintf(t * 16777216.0f);
}

BP_HD double vf_score(uint64_t sum, int count) { return (double)sum / 16777216.0 / (double)(count + 1); }

// the row of a pose whose frame index lies outside [0, T): score NaN, sum 0, count -1
BP_HD double vf_no_score() { return __builtin_nan(""); }
