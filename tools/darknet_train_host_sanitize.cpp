// A stand-alone run of the training iteration's host twins (csrc/darknet_train_host.cpp) for the host sanitizers: each
// GEMM role on shapes with partial tiles, stride 2 on an odd size and more than one reduction slice, batch norm forward
// and backward with and without normalisation, and the update, on buffers of exactly the documented sizes so that a
// stray index is caught.
//   clang++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I betapose_amd/csrc \
//       tools/darknet_train_host_sanitize.cpp betapose_amd/csrc/darknet_train_host.cpp -o /tmp/dt_san && /tmp/dt_san
#include <cstdio>
#include <vector>

#include "darknet_train.h"

static std::vector<float> fill(size_t n, unsigned seed) {
    std::vector<float> v(n);
    for (size_t i = 0; i < n; ++i) v[i] = (float)((int)(((i + seed) * 2654435761u) >> 20) % 2001 - 1000) / 1000.0f;
    return v;
}

int main() {
    double sum = 0.0;
    // the last two: c512_k1024 and k2049 of tests/darknet_train_common.py (16 block rows with chains of 4608 and 9216
    // terms; a second reduction slice of one value)
    const int shapes[6][7] = {{3, 3, 9, 11, 18, 3, 1}, {1, 5, 13, 13, 7, 3, 2}, {2, 9, 7, 6, 4, 1, 2}, {3, 3, 27, 27, 5, 3, 1},
                              {2, 512, 2, 2, 1024, 3, 1}, {3, 4, 1, 683, 5, 1, 1}};
    for (const auto& s : shapes) {
        const int N = s[0], C = s[1], H = s[2], W = s[3], K = s[4], size = s[5], stride = s[6], pad = size / 2;
        const int OH = (H + 2 * pad - size) / stride + 1, OW = (W + 2 * pad - size) / stride + 1;
        std::vector<float> x = fill((size_t)N * C * H * W, 1), w = fill((size_t)K * C * size * size, 2);
        std::vector<float> y((size_t)N * K * OH * OW), scratch(bp::train_conv_scratch(N, C, H, W, K, size, stride));
        bp::train_conv_host(0, x.data(), w.data(), y.data(), N, C, H, W, K, size, stride, nullptr);
        std::vector<float> wu = fill(w.size(), 3), dx = fill(x.size(), 4);
        bp::train_conv_host(1, x.data(), wu.data(), y.data(), N, C, H, W, K, size, stride, scratch.data());
        bp::train_conv_host(2, dx.data(), w.data(), y.data(), N, C, H, W, K, size, stride, nullptr);
        for (float v : y) sum += v;
        for (float v : wu) sum += v;
        for (float v : dx) sum += v;
    }
    for (int bn = 0; bn < 2; ++bn) {
        const int N = 3, C = 7, S = 169;
        const size_t n = (size_t)N * C * S;
        std::vector<float> x = fill(n, 5), scales = fill(C, 6), biases = fill(C, 7), rm = fill(C, 8), rv(C, 1.0f), mean(C), var(C);
        std::vector<float> xn(n), out(n), delta = fill(n, 9), bu(C, 0.0f), su(C, 0.0f), stat(2 * C);
        bp::train_bn_forward_host(x.data(), N, C, S, scales.data(), biases.data(), rm.data(), rv.data(), mean.data(), var.data(),
                                  xn.data(), out.data(), bn, 1, 1);
        bp::train_bn_forward_host(x.data(), N, C, S, scales.data(), biases.data(), rm.data(), rv.data(), nullptr, nullptr, nullptr,
                                  out.data(), bn, 0, 0);
        bp::train_bn_backward_host(out.data(), delta.data(), x.data(), xn.data(), mean.data(), var.data(), scales.data(), N, C, S,
                                   bu.data(), su.data(), stat.data(), bn, 1);
        for (float v : delta) sum += v;
    }
    std::vector<float> p0 = fill(1, 10), u0 = fill(1, 11), p1 = fill(4099, 12), u1 = fill(4099, 13);
    const bp::TrainTensor table[2] = {{p0.data(), u0.data(), 1, 0}, {p1.data(), u1.data(), 4099, 1}};
    bp::train_update_host(table, 2, 0.001f, -0.002f, 0.9f);
    for (float v : p1) sum += v;
    std::printf("sum %.6f\n", sum);
    return 0;
}
