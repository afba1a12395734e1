// One key-point-detector training iteration outside its convolutions: the declarations shared by
// kpd_train_host.cpp, kpd_train.hip and c_api_kpd_train.cpp, so a signature that drifts fails to compile.  Needs no HIP
// header.  The convolutions and Linears are darknet_train.h's train_conv_host / launch_train_conv.
#pragma once
#include <cstddef>
#include <cstdint>

#include "darknet_train.h"

namespace bp {

// One row of the RMSprop table, on the side that runs it: parameter, gradient, square_avg, momentum buffer (read and
// written only with momentum > 0) and the element count
struct KpdTrainTensor {
    float* p;
    float* g;
    float* v;
    float* b;
    long long count;
};
struct KpdTrainOpt {
    float lr, alpha, one_minus_alpha, eps, wd, momentum;
};

// ---- kpd_train_host.cpp: the host twins, all pointers host.
// x [N][C][S] the raw convolution.  bn and train: mean, invstd [C] are written and the running pair updated; bn and
// !train: the running pair normalises; !bn: out = relu?(x + b)
void kpd_train_bn_forward_host(const float* x, int N, int C, int S, const float* w, const float* b, float* running_mean,
                               float* running_var, float* mean, float* invstd, float* out, int bn, int relu, int train);
// d [N][C][S], the gradient of out, becomes the gradient of x; grad_w, grad_b [C] are added to
void kpd_train_bn_backward_host(const float* out, float* d, const float* x, const float* mean, const float* invstd, const float* w,
                                int N, int C, int S, float* grad_w, float* grad_b, int bn, int relu);
// out = relu(y * s[n][c] + res); s may be null
void kpd_train_tail_forward_host(const float* y, const float* s, const float* res, float* out, int N, int C, int S);
// m = dout * (out > 0): dres += m, dy = m * s, ds [N][C] = sum_S m * y (s, ds may be null together)
void kpd_train_tail_backward_host(const float* out, const float* dout, const float* y, const float* s, float* dres, float* dy,
                                  float* ds, int N, int C, int S);
void kpd_train_pool_forward_host(const float* y, int rows, int S, float* pool);
void kpd_train_pool_backward_host(const float* dpool, float* dy, int rows, int S);
void kpd_train_sigmoid_forward_host(const float* x, float* s, long long n);
void kpd_train_sigmoid_backward_host(const float* s, float* g, long long n);
// x [planes][H][W] -> out, arg [planes][OH][OW] (arg: iy * W + ix of the window's first maximum)
void kpd_train_maxpool_forward_host(const float* x, int planes, int H, int W, float* out, int* arg);
void kpd_train_maxpool_backward_host(const float* dout, const int* arg, int planes, int H, int W, float* dx);
void kpd_train_rmsprop_host(const KpdTrainTensor* table, int tensors, KpdTrainOpt o);
int kpd_train_update_chunk();

// ---- kpd_train.hip: the same on device pointers (the table too), enqueued on s
void launch_kpd_train_bn_forward(const float* x, int N, int C, int S, const float* w, const float* b, float* running_mean,
                                 float* running_var, float* mean, float* invstd, float* out, int bn, int relu, int train,
                                 hipStream_t s);
void launch_kpd_train_bn_backward(const float* out, float* d, const float* x, const float* mean, const float* invstd, const float* w,
                                  int N, int C, int S, float* grad_w, float* grad_b, int bn, int relu, hipStream_t s);
void launch_kpd_train_tail_forward(const float* y, const float* sc, const float* res, float* out, int N, int C, int S, hipStream_t s);
void launch_kpd_train_tail_backward(const float* out, const float* dout, const float* y, const float* sc, float* dres, float* dy,
                                    float* ds, int N, int C, int S, hipStream_t s);
void launch_kpd_train_pool_forward(const float* y, int rows, int S, float* pool, hipStream_t s);
void launch_kpd_train_pool_backward(const float* dpool, float* dy, int rows, int S, hipStream_t s);
void launch_kpd_train_sigmoid_forward(const float* x, float* sg, long long n, hipStream_t s);
void launch_kpd_train_sigmoid_backward(const float* sg, float* g, long long n, hipStream_t s);
void launch_kpd_train_maxpool_forward(const float* x, int planes, int H, int W, float* out, int* arg, hipStream_t s);
void launch_kpd_train_maxpool_backward(const float* dout, const int* arg, int planes, int H, int W, float* dx, hipStream_t s);
// blocks: the sum over the table of ceil(count / kpd_train_update_chunk())
void launch_kpd_train_rmsprop(const KpdTrainTensor* table, int tensors, int blocks, KpdTrainOpt o, hipStream_t s);

}  // namespace bp
