// extern "C" boundary, the training iteration: bp_train_conv, bp_train_bn_forward, bp_train_bn_backward,
// bp_train_update and their _host twins -- see include/betapose_hip.h.  Every function checks its arguments and makes one
// bp:: call: the host twin (darknet_train_host.cpp) or the launch (darknet_train.hip).  What a host / device pair checks
// alike is stated once, in the check functions.
#include <vector>

#include "c_api_util.h"
#include "darknet_train.h"

static void train_check_conv(int role, const void* x, const void* w, const void* y, int N, int C, int H, int W, int K, int size,
                             int stride, const void* scratch) {
    bp_check_train_conv(role, x, w, y, N, C, H, W, K, size, stride, scratch, false);
}

static void train_check_bn(int N, int C, int S, int bn, int train) {
    BP_CHECK(N > 0 && C > 0 && S > 0, "N, C and S must be positive");
    BP_CHECK((long long)N * C * S < (1ll << 31), "a tensor of 2^31 elements or more");
    BP_CHECK(!(bn && train) || (long long)N * S > 1, "batch * spatial must exceed 1: the variance divides by batch * spatial - 1");
}

// the rows of a host copy of the table; the number of blocks they need
static long long train_check_table(const bp::TrainTensor* t, int tensors) {
    long long blocks = 0;
    for (int i = 0; i < tensors; ++i) {
        BP_CHECK(t[i].p && t[i].u && t[i].count > 0 && t[i].count < (1ll << 40) && (t[i].kind == 0 || t[i].kind == 1),
                 "a table row needs two pointers, a positive count and kind 0 or 1");
        blocks += (t[i].count + bp::train_update_chunk() - 1) / bp::train_update_chunk();
    }
    return blocks;
}

extern "C" {

size_t bp_train_conv_scratch(int N, int C, int H, int W, int K, int size, int stride) {
    if (N <= 0 || C <= 0 || H <= 0 || W <= 0 || K <= 0 || !bp_train_conv_size_ok(size, false) || (stride != 1 && stride != 2)) return 0;
    return bp::train_conv_scratch(N, C, H, W, K, size, stride);
}

int bp_train_update_chunk(void) { return bp::train_update_chunk(); }

int bp_train_conv_host(int role, float* x, float* w, float* y, int N, int C, int H, int W, int K, int size, int stride,
                       float* scratch) {
    BP_TRY
    train_check_conv(role, x, w, y, N, C, H, W, K, size, stride, scratch);
    bp::train_conv_host(role, x, w, y, N, C, H, W, K, size, stride, scratch);
    return 0;
    BP_CATCH
}

int bp_train_conv(int role, float* d_x, float* d_w, float* d_y, int N, int C, int H, int W, int K, int size, int stride,
                  float* d_scratch, void* stream) {
    BP_TRY
    train_check_conv(role, d_x, d_w, d_y, N, C, H, W, K, size, stride, d_scratch);
    bp::launch_train_conv(role, d_x, d_w, d_y, N, C, H, W, K, size, stride, d_scratch, (hipStream_t)stream);
    return 0;
    BP_CATCH
}

int bp_train_bn_forward_host(const float* x, int N, int C, int S, const float* scales, const float* biases, float* rolling_mean,
                             float* rolling_var, float* mean, float* var, float* x_norm, float* out, int bn, int leaky,
                             int train) {
    BP_TRY
    BP_CHECK(x && biases && out && x != out, "null argument, or x and out are the same tensor");
    BP_CHECK(!bn || (scales && rolling_mean && rolling_var && (!train || (mean && var && x_norm))), "null batch-norm argument");
    train_check_bn(N, C, S, bn, train);
    bp::train_bn_forward_host(x, N, C, S, scales, biases, rolling_mean, rolling_var, mean, var, x_norm, out, bn, leaky, train);
    return 0;
    BP_CATCH
}

int bp_train_bn_forward(const float* d_x, int N, int C, int S, const float* d_scales, const float* d_biases,
                        float* d_rolling_mean, float* d_rolling_var, float* d_mean, float* d_var, float* d_x_norm, float* d_out,
                        int bn, int leaky, int train, void* stream) {
    BP_TRY
    BP_CHECK(d_x && d_biases && d_out && d_x != d_out, "null argument, or x and out are the same tensor");
    BP_CHECK(!bn || (d_scales && d_rolling_mean && d_rolling_var && (!train || (d_mean && d_var && d_x_norm))),
             "null batch-norm argument");
    train_check_bn(N, C, S, bn, train);
    bp::launch_train_bn_forward(d_x, N, C, S, d_scales, d_biases, d_rolling_mean, d_rolling_var, d_mean, d_var, d_x_norm, d_out, bn,
                                leaky, train, (hipStream_t)stream);
    return 0;
    BP_CATCH
}

int bp_train_bn_backward_host(const float* out, float* delta, const float* x, const float* x_norm, const float* mean,
                              const float* var, const float* scales, int N, int C, int S, float* bias_updates,
                              float* scale_updates, float* stat, int bn, int leaky) {
    BP_TRY
    BP_CHECK(out && delta && bias_updates, "null argument");
    BP_CHECK(!bn || (x && x_norm && mean && var && scales && scale_updates && stat), "null batch-norm argument");
    train_check_bn(N, C, S, bn, 1);
    bp::train_bn_backward_host(out, delta, x, x_norm, mean, var, scales, N, C, S, bias_updates, scale_updates, stat, bn, leaky);
    return 0;
    BP_CATCH
}

int bp_train_bn_backward(const float* d_out, float* d_delta, const float* d_x, const float* d_x_norm, const float* d_mean,
                         const float* d_var, const float* d_scales, int N, int C, int S, float* d_bias_updates,
                         float* d_scale_updates, float* d_stat, int bn, int leaky, void* stream) {
    BP_TRY
    BP_CHECK(d_out && d_delta && d_bias_updates, "null argument");
    BP_CHECK(!bn || (d_x && d_x_norm && d_mean && d_var && d_scales && d_scale_updates && d_stat), "null batch-norm argument");
    train_check_bn(N, C, S, bn, 1);
    bp::launch_train_bn_backward(d_out, d_delta, d_x, d_x_norm, d_mean, d_var, d_scales, N, C, S, d_bias_updates, d_scale_updates,
                                 d_stat, bn, leaky, (hipStream_t)stream);
    return 0;
    BP_CATCH
}

int bp_train_update_host(const void* table, int tensors, float rate_over_batch, float decay_term, float momentum) {
    BP_TRY
    BP_CHECK(table && tensors > 0, "null or empty table");
    train_check_table((const bp::TrainTensor*)table, tensors);
    bp::train_update_host((const bp::TrainTensor*)table, tensors, rate_over_batch, decay_term, momentum);
    return 0;
    BP_CATCH
}

int bp_train_update(const void* d_table, int tensors, int blocks, float rate_over_batch, float decay_term, float momentum,
                    void* stream) {
    BP_TRY
    // the table stays on the device (a training step reads nothing back but its cost): its rows are the caller's to get
    // right, as any pointer is; a block past the rows' chunks does nothing
    BP_CHECK(d_table && tensors > 0 && tensors <= 65536 && blocks > 0, "null or empty table, or no blocks");
    bp::launch_train_update((const bp::TrainTensor*)d_table, tensors, blocks, rate_over_batch, decay_term, momentum,
                            (hipStream_t)stream);
    return 0;
    BP_CATCH
}

}  // extern "C"
