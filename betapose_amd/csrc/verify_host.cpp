// Host twin of the verification kernels (include/betapose_hip.h bp_image_gradients_host, bp_gradient_scores_host):
// plain loops over images, rows and pixels around verify_math.inc, the text verify.hip compiles too.  Equal to the
// kernels byte for byte.  No HIP header: the file also builds with a plain C++ compiler.
#include <cmath>
#include <cstdint>
#include <vector>

#include "verify.h"

#pragma clang fp contract(off)

namespace bp {

namespace {
#include "verify_math.inc"

// gx, gy of every pixel of one image, from its gray (reflect-101 at the border)
void sobel_image(const uint8_t* img, int H, int W, int red, std::vector<int>& gray, std::vector<int>& vs, std::vector<int>& vd,
                 std::vector<int>& gx, std::vector<int>& gy) {
    const size_t HW = (size_t)H * W;
    gray.resize(HW), vs.resize(HW), vd.resize(HW), gx.resize(HW), gy.resize(HW);
    for (size_t p = 0; p < HW; ++p) gray[p] = vf_gray(img[3 * p + red], img[3 * p + 1], img[3 * p + 2 - red]);
    for (int y = 0; y < H; ++y) {
        const int* r[5];
        for (int k = 0; k < 5; ++k) r[k] = gray.data() + (size_t)vf_reflect(y - VF_HALO + k, H) * W;
        for (int x = 0; x < W; ++x) vf_column(r[0][x], r[1][x], r[2][x], r[3][x], r[4][x], vs[(size_t)y * W + x], vd[(size_t)y * W + x]);
    }
    for (int y = 0; y < H; ++y)
        for (int x = 0; x < W; ++x) {
            int cs[5], cd[5];
            for (int k = 0; k < 5; ++k) {
                const size_t q = (size_t)y * W + vf_reflect(x - VF_HALO + k, W);
                cs[k] = vs[q];
                cd[k] = vd[q];
            }
            vf_row(cs, cd, gx[(size_t)y * W + x], gy[(size_t)y * W + x]);
        }
}
}  // namespace

void image_gradients_host(const uint8_t* images, int I, int H, int W, int red_channel, int min_sq, float* grad, float* mag) {
    const size_t HW = (size_t)H * W;
    std::vector<int> gray, vs, vd, gx, gy;
    for (int i = 0; i < I; ++i) {
        sobel_image(images + (size_t)i * HW * 3, H, W, red_channel, gray, vs, vd, gx, gy);
        float* g = grad + (size_t)i * HW * 2;
        for (size_t p = 0; p < HW; ++p) {
            VfUnit u;
            vf_unit(gx[p], gy[p], min_sq, u);
            g[2 * p] = u.nx;
            g[2 * p + 1] = u.ny;
            if (mag) mag[(size_t)i * HW + p] = u.mag;
        }
    }
}

void gradient_scores_host(const uint8_t* renders, const float* scene_grad, const int* frame_index, int P, int T, int H, int W,
                          int red_channel, int render_min_sq, uint64_t* sum, int* count, double* score) {
    const size_t HW = (size_t)H * W;
    std::vector<int> gray, vs, vd, gx, gy;
    for (int p = 0; p < P; ++p) {
        const int fi = frame_index[p];
        if (fi < 0 || fi >= T) {
            sum[p] = 0, count[p] = -1, score[p] = vf_no_score();
            continue;
        }
        sobel_image(renders + (size_t)p * HW * 3, H, W, red_channel, gray, vs, vd, gx, gy);
        const float* sg = scene_grad + (size_t)fi * HW * 2;
        uint64_t s = 0;
        int c = 0;
        for (size_t q = 0; q < HW; ++q) {
            VfUnit u;
            if (!vf_unit(gx[q], gy[q], render_min_sq, u)) continue;
            ++c;
            s += vf_term(u.nx, u.ny, sg[2 * q], sg[2 * q + 1]);
        }
        sum[p] = s, count[p] = c, score[p] = vf_score(s, c);
    }
}

}  // namespace bp
