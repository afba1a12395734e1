// Host twins of the key-point designator (include/betapose_hip.h bp_voxel_grid_host, bp_sift_octave_host,
// bp_farthest_points_host, bp_thin_points_host): plain loops around the arithmetic of designate_math.inc, the text
// designate.hip compiles too.  Every floating-point sum runs in ascending index order here and there, and every choice
// among equals goes to the lower index, so these results and the kernels' are equal bit for bit.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <limits>
#include <utility>
#include <vector>

#include "designate.h"

#pragma clang fp contract(off)

namespace bp {

namespace {
#include "designate_math.inc"

static_assert(DESIGNATE_MAX_K >= 25, "the reference's neighbourhood is 25 points");
}  // namespace

void voxel_grid_host(const double* points, int n, double leaf, double* out, int* n_out) {
    double lo[3], hi[3];
    for (int a = 0; a < 3; ++a) lo[a] = hi[a] = std::floor(points[a] / leaf);
    for (int i = 1; i < n; ++i)
        for (int a = 0; a < 3; ++a) {
            const double c = std::floor(points[(size_t)i * 3 + a] / leaf);
            lo[a] = std::min(lo[a], c);
            hi[a] = std::max(hi[a], c);
        }
    const double dx = hi[0] - lo[0] + 1.0, dy = hi[1] - lo[1] + 1.0, dz = hi[2] - lo[2] + 1.0;
    if (!(dx * dy * dz <= (double)INT32_MAX)) {     // PCL's "leaf size is too small": the cloud passes through
        std::copy(points, points + (size_t)n * 3, out);
        *n_out = n;
        return;
    }
    const int64_t Dx = (int64_t)dx, Dxy = Dx * (int64_t)dy;
    std::vector<std::pair<int64_t, int>> keyed(n);
    for (int i = 0; i < n; ++i) {
        const double* p = points + (size_t)i * 3;
        const int64_t ci = (int64_t)(std::floor(p[0] / leaf) - lo[0]), cj = (int64_t)(std::floor(p[1] / leaf) - lo[1]),
                      ck = (int64_t)(std::floor(p[2] / leaf) - lo[2]);
        keyed[i] = {ci + cj * Dx + ck * Dxy, i};
    }
    std::sort(keyed.begin(), keyed.end());          // by key, then by input index
    int m = 0;
    for (int i = 0; i < n;) {
        double sx = 0.0, sy = 0.0, sz = 0.0;
        int j = i;
        for (; j < n && keyed[j].first == keyed[i].first; ++j) {
            const double* p = points + (size_t)keyed[j].second * 3;
            sx += p[0];
            sy += p[1];
            sz += p[2];
        }
        const double cnt = (double)(j - i);
        out[(size_t)m * 3] = sx / cnt;
        out[(size_t)m * 3 + 1] = sy / cnt;
        out[(size_t)m * 3 + 2] = sz / cnt;
        ++m;
        i = j;
    }
    *n_out = m;
}

void sift_octave_host(const double* points, int n, int field, const double* scales, int ns, int k, double min_contrast,
                      double* dog, signed char* flags) {
    const DsScales sc = ds_scales(scales, ns);
    const int kk = k < n ? k : n, nd = ns - 1, nf = ns - 3;
    std::vector<double> nbr_d((size_t)n * kk);
    std::vector<int> nbr_i((size_t)n * kk);
    for (int p = 0; p < n; ++p) {
        const double* P = points + (size_t)p * 3;
        double num[DS_MAX_SCALES] = {0}, den[DS_MAX_SCALES] = {0};
        double* ld = nbr_d.data() + (size_t)p * kk;
        int* li = nbr_i.data() + (size_t)p * kk;
        int cnt = 0;
        for (int q = 0; q < n; ++q) {
            const double* Q = points + (size_t)q * 3;
            const double d2 = ds_d2(P[0], P[1], P[2], Q[0], Q[1], Q[2]);
            for (int i = ns - 1; i >= 0 && d2 <= sc.r9[i]; --i) {
                const double w = ds_weight(d2, sc.s2[i]);
                num[i] += Q[field] * w;
                den[i] += w;
            }
            if (cnt < kk || d2 < ld[kk - 1]) {      // (an equal d2 at a higher index orders after)
                int at = cnt < kk ? cnt++ : kk - 1;
                for (; at > 0 && ld[at - 1] > d2; --at) {
                    ld[at] = ld[at - 1];
                    li[at] = li[at - 1];
                }
                ld[at] = d2;
                li[at] = q;
            }
        }
        double g_prev = num[0] / den[0];
        for (int j = 0; j < nd; ++j) {
            const double g = num[j + 1] / den[j + 1];
            dog[(size_t)p * nd + j] = g - g_prev;
            g_prev = g;
        }
    }
    for (int p = 0; p < n; ++p) {
        const double* row = dog + (size_t)p * nd;
        const int* li = nbr_i.data() + (size_t)p * kk;
        for (int j = 1; j <= ns - 3; ++j) {
            const double v = row[j];
            int sign = ds_own_sign(v, row[j - 1], row[j + 1], min_contrast);
            for (int t = 0; t < kk && sign; ++t) {
                const double* r = dog + (size_t)li[t] * nd + (j - 1);
                if (!ds_nbr_ok(sign, v, r[0], r[1], r[2])) sign = 0;
            }
            flags[(size_t)p * nf + (j - 1)] = (signed char)sign;
        }
    }
}

void farthest_points_host(const double* points, int n, int K, int start, int* idx, double* d2) {
    double sx = 0.0, sy = 0.0, sz = 0.0;
    for (int i = 0; i < n; ++i) {
        sx += points[(size_t)i * 3];
        sy += points[(size_t)i * 3 + 1];
        sz += points[(size_t)i * 3 + 2];
    }
    const double cx = sx / (double)n, cy = sy / (double)n, cz = sz / (double)n;
    auto from_centre = [&](int i) {
        const double* p = points + (size_t)i * 3;
        return ds_d2(p[0], p[1], p[2], cx, cy, cz);
    };
    if (start < 0) {
        start = 0;
        double best = from_centre(0);
        for (int i = 1; i < n; ++i) {
            const double d = from_centre(i);
            if (ds_more(d, i, best, start)) {
                best = d;
                start = i;
            }
        }
    }
    idx[0] = start;
    d2[0] = from_centre(start);
    std::vector<double> mind(n, std::numeric_limits<double>::infinity());
    for (int r = 1; r < K; ++r) {
        const double* L = points + (size_t)idx[r - 1] * 3;
        int bi = 0;
        double bd = -1.0;
        for (int i = 0; i < n; ++i) {
            const double* p = points + (size_t)i * 3;
            const double d = ds_d2(p[0], p[1], p[2], L[0], L[1], L[2]);
            if (d < mind[i]) mind[i] = d;
            if (ds_more(mind[i], i, bd, bi)) {
                bd = mind[i];
                bi = i;
            }
        }
        idx[r] = bi;
        d2[r] = bd;
    }
}

void thin_points_host(const double* points, int n, int keep, unsigned char* alive, int* state) {
    const double inf = std::numeric_limits<double>::infinity();
    std::vector<double> nn_d(n);
    std::vector<int> nn_j(n);
    auto nearest = [&](int i) {     // over the living j != i: the smallest (distance, j)
        const double* p = points + (size_t)i * 3;
        double bd = inf;
        int bj = n;
        for (int j = 0; j < n; ++j) {
            if (j == i || !alive[j]) continue;
            const double* q = points + (size_t)j * 3;
            const double d = ds_dist(p, q);
            if (ds_less(d, j, bd, bj)) {
                bd = d;
                bj = j;
            }
        }
        nn_d[i] = bd;
        nn_j[i] = bj;
    };
    for (int i = 0; i < n; ++i) alive[i] = 1;
    for (int i = 0; i < n; ++i) nearest(i);
    const int rounds = n > keep ? n - keep : 0;
    int done = 0, last = -1;
    for (; done < rounds; ++done) {
        double bd = inf;
        int bi = n;
        for (int i = 0; i < n; ++i)
            if (alive[i] && ds_less(nn_d[i], i, bd, bi)) {
                bd = nn_d[i];
                bi = i;
            }
        if (!(bd < DS_THIN_CAP)) break;     // from here on the reference deletes the carried position again and again
        alive[bi] = 0;
        last = bi;
        for (int i = 0; i < n; ++i)
            if (alive[i] && nn_j[i] == bi) nearest(i);
    }
    int pos = 0;
    for (int i = 0; i < last; ++i) pos += alive[i];
    state[0] = done;
    state[1] = pos;
}

}  // namespace bp
