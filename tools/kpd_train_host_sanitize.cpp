// A stand-alone run of the key-point detector's training host twins (csrc/kpd_train_host.cpp, and the GEMM core of
// csrc/darknet_train_host.cpp at size 7 and as a Linear) for the host sanitizers: batch norm forward and backward with and
// without normalisation, the block tail with and without the gate, the SE pool, the sigmoid, the max-pool and RMSprop, at
// S a multiple of 4 (units of four values) and not, on buffers of exactly the documented sizes so that a stray index of
// the lane and unit functions -- the text the kernels compile too -- is caught.
//   clang++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I betapose_amd/csrc \
//       tools/kpd_train_host_sanitize.cpp betapose_amd/csrc/kpd_train_host.cpp betapose_amd/csrc/darknet_train_host.cpp \
//       -o /tmp/kt_san && /tmp/kt_san
#include <cstdio>
#include <vector>

#include "kpd_train.h"

static std::vector<float> fill(size_t n, unsigned seed) {
    std::vector<float> v(n);
    for (size_t i = 0; i < n; ++i) v[i] = (float)((int)(((i + seed) * 2654435761u) >> 20) % 2001 - 1000) / 1000.0f;
    return v;
}

int main() {
    double sum = 0.0;
    const int convs[3][7] = {{2, 3, 9, 11, 5, 7, 2}, {1, 3, 14, 10, 4, 7, 2}, {3, 8, 1, 1, 8, 1, 1}};
    for (const auto& s : convs) {
        const int N = s[0], C = s[1], H = s[2], W = s[3], K = s[4], size = s[5], stride = s[6], pad = size / 2;
        const int OH = (H + 2 * pad - size) / stride + 1, OW = (W + 2 * pad - size) / stride + 1;
        std::vector<float> x = fill((size_t)N * C * H * W, 1), w = fill((size_t)K * C * size * size, 2);
        std::vector<float> y((size_t)N * K * OH * OW), scratch(bp::train_conv_scratch(N, C, H, W, K, size, stride));
        bp::train_conv_host(0, x.data(), w.data(), y.data(), N, C, H, W, K, size, stride, nullptr);
        std::vector<float> wu = fill(w.size(), 3), dx = fill(x.size(), 4);
        bp::train_conv_host(1, x.data(), wu.data(), y.data(), N, C, H, W, K, size, stride, scratch.data());
        bp::train_conv_host(2, dx.data(), w.data(), y.data(), N, C, H, W, K, size, stride, nullptr);
        for (float v : wu) sum += v;
        for (float v : dx) sum += v;
    }
    const int shapes[5][3] = {{1, 2, 2}, {3, 5, 7}, {4, 2, 260}, {257, 2, 4}, {3, 4, 343}};
    for (const auto& s : shapes)
        for (int bn = 0; bn < 2; ++bn) {
            const int N = s[0], C = s[1], S = s[2];
            const size_t n = (size_t)N * C * S;
            std::vector<float> x = fill(n, 5), w = fill(C, 6), b = fill(C, 7), rm = fill(C, 8), rv(C, 1.0f), mean(C), invstd(C);
            std::vector<float> out(n), d = fill(n, 9), gw(C, 0.0f), gb(C, 0.0f);
            bp::kpd_train_bn_forward_host(x.data(), N, C, S, w.data(), b.data(), rm.data(), rv.data(), mean.data(), invstd.data(), out.data(),
                                          bn, 1, 1);
            bp::kpd_train_bn_backward_host(out.data(), d.data(), x.data(), mean.data(), invstd.data(), w.data(), N, C, S, gw.data(), gb.data(),
                                           bn, 1);
            bp::kpd_train_bn_forward_host(x.data(), N, C, S, w.data(), b.data(), rm.data(), rv.data(), nullptr, nullptr, out.data(), bn, 0, 0);
            for (float v : d) sum += v;
            std::vector<float> sc = fill((size_t)N * C, 10), res = fill(n, 11), dres = fill(n, 12), dy(n), ds((size_t)N * C), pool((size_t)N * C);
            for (int gate = 0; gate < 2; ++gate) {
                bp::kpd_train_tail_forward_host(x.data(), gate ? sc.data() : nullptr, res.data(), out.data(), N, C, S);
                bp::kpd_train_tail_backward_host(out.data(), d.data(), x.data(), gate ? sc.data() : nullptr, dres.data(), dy.data(),
                                                 gate ? ds.data() : nullptr, N, C, S);
            }
            bp::kpd_train_pool_forward_host(x.data(), N * C, S, pool.data());
            bp::kpd_train_pool_backward_host(pool.data(), dy.data(), N * C, S);
            bp::kpd_train_sigmoid_forward_host(pool.data(), sc.data(), (long long)N * C);
            bp::kpd_train_sigmoid_backward_host(sc.data(), ds.data(), (long long)N * C);
            for (float v : dy) sum += v;
            for (float v : ds) sum += v;
        }
    const int maps[4][3] = {{3, 18, 14}, {2, 5, 5}, {2, 1, 9}, {1, 4, 1}};
    for (const auto& m : maps) {
        const int P = m[0], H = m[1], W = m[2], OH = (H - 1) / 2 + 1, OW = (W - 1) / 2 + 1;
        std::vector<float> x = fill((size_t)P * H * W, 13), out((size_t)P * OH * OW), dout = fill(out.size(), 14), dx(x.size());
        std::vector<int> arg(out.size());
        bp::kpd_train_maxpool_forward_host(x.data(), P, H, W, out.data(), arg.data());
        bp::kpd_train_maxpool_backward_host(dout.data(), arg.data(), P, H, W, dx.data());
        for (float v : dx) sum += v;
    }
    for (int mom = 0; mom < 2; ++mom) {
        std::vector<float> p0 = fill(1, 15), g0 = fill(1, 16), v0(1, 0.0f), b0(1, 0.0f), p1 = fill(1025, 17), g1 = fill(1025, 18), v1(1025, 0.25f),
                           b1(1025, 0.0f);
        const bp::KpdTrainTensor table[2] = {{p0.data(), g0.data(), v0.data(), mom ? b0.data() : nullptr, 1},
                                             {p1.data(), g1.data(), v1.data(), mom ? b1.data() : nullptr, 1025}};
        bp::kpd_train_rmsprop_host(table, 2, {1e-3f, 0.99f, 0.01f, 1e-8f, mom ? 1e-4f : 0.0f, mom ? 0.9f : 0.0f});
        for (float v : p1) sum += v;
    }
    std::printf("sum %.6f\n", sum);
    return 0;
}
