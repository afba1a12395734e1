// One Darknet training iteration: the declarations shared by darknet_train_host.cpp, darknet_train.hip
// and c_api_train.cpp, so a signature that drifts fails to compile.  Needs no HIP header (darknet_train_host.cpp is plain
// C++): the stream type is declared as hip_runtime_api.h declares it.
#pragma once
#include <cstddef>
#include <cstdint>

typedef struct ihipStream_t* hipStream_t;

namespace bp {

// floats of scratch the filter gradient needs: one partial sum per reduction slice and filter element
size_t train_conv_scratch(int N, int C, int H, int W, int K, int size, int stride);

// One row of the update's table, on the side that runs it: the parameter, its update buffer, the element count and the
// kind (1: filters, which take the decay step; 0: biases and scales)
struct TrainTensor {
    float* p;
    float* u;
    long long count;
    long long kind;
};

// ---- darknet_train_host.cpp: the host twins, all pointers host.
// role 0: y [N][K][OH][OW] = conv(x [N][C][H][W], w [K][C][size][size]); role 1: w (the filter updates) += delta (y) x
// im2col(x), through scratch; role 2: x (the input's delta) += w^T delta (y)
void train_conv_host(int role, float* x, float* w, float* y, int N, int C, int H, int W, int K, int size, int stride,
                     float* scratch);
// x [N][C][S] the raw convolution.  bn: mean, var [C] are written (train) and the rolling pair updated, or the rolling
// pair is used (!train); x_norm (train only) and out are written.  !bn: out = act(x + bias)
void train_bn_forward_host(const float* x, int N, int C, int S, const float* scales, const float* biases, float* rolling_mean,
                           float* rolling_var, float* mean, float* var, float* x_norm, float* out, int bn, int leaky, int train);
// delta [N][C][S] becomes the delta of the raw convolution; bias_updates, scale_updates [C] are added to; stat [2][C]
// (mean_delta, variance_delta) is scratch
void train_bn_backward_host(const float* out, float* delta, const float* x, const float* x_norm, const float* mean,
                            const float* var, const float* scales, int N, int C, int S, float* bias_updates,
                            float* scale_updates, float* stat, int bn, int leaky);
void train_update_host(const TrainTensor* table, int tensors, float rate_over_batch, float decay_term, float momentum);

// ---- darknet_train.hip: the same on device pointers (the table too), enqueued on s
void launch_train_conv(int role, float* x, float* w, float* y, int N, int C, int H, int W, int K, int size, int stride,
                       float* scratch, hipStream_t s);
void launch_train_bn_forward(const float* x, int N, int C, int S, const float* scales, const float* biases, float* rolling_mean,
                             float* rolling_var, float* mean, float* var, float* x_norm, float* out, int bn, int leaky, int train,
                             hipStream_t s);
void launch_train_bn_backward(const float* out, float* delta, const float* x, const float* x_norm, const float* mean,
                              const float* var, const float* scales, int N, int C, int S, float* bias_updates,
                              float* scale_updates, float* stat, int bn, int leaky, hipStream_t s);
// blocks: the sum over the table of ceil(count / train_update_chunk()); each block finds its tensor in the table
void launch_train_update(const TrainTensor* table, int tensors, int blocks, float rate_over_batch, float decay_term,
                         float momentum, hipStream_t s);
int train_update_chunk();

}  // namespace bp
