// The key-point designator's arithmetic of O(1) size, ONE source for the host twins (designate_host.cpp) and the device
// kernels (designate.hip): the squared distance of two points, the exponential of the Gaussian weights, one weight, the
// extremum tests of one DoG value and the ordering of (value, index) pairs.  Host and device compile this text and do
// the same f64 / integer operations in the same order, without FMA contraction, so their outputs agree bit for bit;
// only who loops over what differs per side.
// Plain C++17, no HIP header.  Included inside `namespace bp { namespace {` after <cmath> and <cstdint>, in a unit that
// has `#pragma clang fp contract(off)` in force.  Definitions: DESIGN.md §3.9.
#ifndef BP_HD
#if defined(__HIPCC__)
#define BP_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define BP_HD inline
#endif
#endif

constexpr int DS_MAX_SCALES = DESIGNATE_MAX_SCALES;     // (designate.h)
constexpr double DS_THIN_CAP = 100.0;                   // Model3D.refine's hard-wired start of the running minimum

// sigma^2 and the cut-off 9 sigma^2 of every scale of an octave; the scales ascend (checked by the C entry points)
struct DsScales {
    int ns;
    double s2[DS_MAX_SCALES];
    double r9[DS_MAX_SCALES];
};

BP_HD DsScales ds_scales(const double* scales, int ns) {
    DsScales s;
    s.ns = ns;
    for (int i = 0; i < DS_MAX_SCALES; ++i) {
        const double sg = i < ns ? scales[i] : 0.0;
        s.s2[i] = sg * sg;
        s.r9[i] = 9.0 * s.s2[i];
    }
    return s;
}

BP_HD double ds_d2(double px, double py, double pz, double qx, double qy, double qz) {
    const double dx = px - qx, dy = py - qy, dz = pz - qz;
    return (dx * dx + dy * dy) + dz * dz;
}

// the distance the thinning compares: the correctly rounded square root of ds_d2 (numpy's sqrt of the summed squares)
BP_HD double ds_dist(const double* p, const double* q) { return sqrt(ds_d2(p[0], p[1], p[2], q[0], q[1], q[2])); }

// exp(x) for x in [-4.5, 0] (any x in [-700, 0.3] in fact) from + - * and a bit-built power of two: x = k ln2 + r with
// |r| <= 0.35 (ln2 split into a 32-bit head, so k * head is exact, and a tail), the degree-13 Taylor polynomial of
// exp(r) by Horner's rule (truncation below 2^-57, thirteen rounded steps below 3e-15 relative), times 2^k.  Neither
// libm's nor ocml's exp: the two differ, and the host's and the device's weights must not.
BP_HD double ds_exp(double x) {
    const int k = (int)(x * 1.44269504088896338700e+00 - 0.5);      // truncation of a value <= -0.5: round to nearest
    const double kd = (double)k;
    const double r = (x - kd * 6.93147180369123816490e-01) - kd * 1.90821492927058770002e-10;
    double p = 1.0 / 6227020800.0;
    p = p * r + 1.0 / 479001600.0;
    p = p * r + 1.0 / 39916800.0;
    p = p * r + 1.0 / 3628800.0;
    p = p * r + 1.0 / 362880.0;
    p = p * r + 1.0 / 40320.0;
    p = p * r + 1.0 / 5040.0;
    p = p * r + 1.0 / 720.0;
    p = p * r + 1.0 / 120.0;
    p = p * r + 1.0 / 24.0;
    p = p * r + 1.0 / 6.0;
    p = p * r + 0.5;
    p = p * r + 1.0;
    p = p * r + 1.0;
    const uint64_t bits = (uint64_t)(1023 + k) << 52;               // 2^k, k in [-1010, 0]
    double scale;
    __builtin_memcpy(&scale, &bits, sizeof scale);
    return p * scale;
}

// the weight of a pair at squared distance d2 <= 9 sigma^2 under the scale with sigma^2 = s2
BP_HD double ds_weight(double d2, double s2) { return ds_exp((-0.5 * d2) / s2); }

// what a point's own three DoG values allow: -1 a minimum, +1 a maximum, 0 neither
BP_HD int ds_own_sign(double v, double below, double above, double min_contrast) {
    if (!(fabs(v) >= min_contrast)) return 0;
    if (v < below && v < above) return -1;
    if (v > below && v > above) return 1;
    return 0;
}

// a neighbour's three DoG values (scales j-1, j, j+1) do not contradict the extremum of the given sign
BP_HD bool ds_nbr_ok(int sign, double v, double a, double b, double c) {
    return sign < 0 ? (v <= a && v <= b && v <= c) : (v >= a && v >= b && v >= c);
}

// (d, i) orders before (e, j): the smaller value, then the lower index
BP_HD bool ds_less(double d, int i, double e, int j) { return d < e || (d == e && i < j); }
// (d, i) is the better maximum: the larger value, then the lower index
BP_HD bool ds_more(double d, int i, double e, int j) { return d > e || (d == e && i < j); }
