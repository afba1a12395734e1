// extern "C" boundary, the key-point detector's training iteration: bp_kpd_train_* and their _host twins
// -- see include/betapose_hip.h.  Every function checks its arguments and makes one bp:: call: the host twin
// (kpd_train_host.cpp, darknet_train_host.cpp) or the launch (kpd_train.hip, darknet_train.hip).  What a host / device
// pair checks alike is stated once, in the check functions; dev adds the 16-byte alignment the device's vector accesses
// need where S is a multiple of 4.
#include <cstdint>
#include <initializer_list>

#include "c_api_util.h"
#include "kpd_train.h"

static void kt_check_conv(int role, const void* x, const void* w, const void* y, int N, int C, int H, int W, int K, int size,
                          int stride, const void* scratch) {
    bp_check_train_conv(role, x, w, y, N, C, H, W, K, size, stride, scratch, true);
}

static bool kt_aligned(const void* p) { return ((uintptr_t)p & 15) == 0; }

static void kt_check_ncs(long long N, long long C, long long S) {
    BP_CHECK(N > 0 && C > 0 && S > 0, "N, C and S must be positive");
    // (a lane's unit index steps by the block's 256 lanes past the end before its loop stops: an int must hold that too)
    BP_CHECK(N * C * S < (1ll << 31) - 1024, "a tensor of 2^31 - 1024 elements or more");
}

static void kt_check_vec(int S, std::initializer_list<const void*> tensors) {
    if (S % 4) return;
    for (const void* p : tensors) BP_CHECK(kt_aligned(p), "a tensor with S a multiple of 4 must be 16-byte aligned on the device");
}

static void kt_check_bn_forward(const float* x, int N, int C, int S, const float* w, const float* b, float* rm, float* rv, float* mean,
                                float* invstd, float* out, int bn, int train) {
    BP_CHECK(x && b && out && x != out, "null argument, or x and out are the same tensor");
    BP_CHECK(!bn || (w && rm && rv && (!train || (mean && invstd))), "null batch-norm argument");
    kt_check_ncs(N, C, S);
    BP_CHECK(!(bn && train) || (long long)N * S > 1, "batch norm in training needs more than one value per channel");
}

static void kt_check_bn_backward(const float* out, float* d, const float* x, const float* mean, const float* invstd, const float* w,
                                 int N, int C, int S, float* gw, float* gb, int bn, int relu) {
    BP_CHECK(d && gb && (!relu || out), "null argument");
    BP_CHECK(!bn || (x && mean && invstd && w && gw), "null batch-norm argument");
    kt_check_ncs(N, C, S);
}

static void kt_check_pool_shape(int planes, int H, int W) {
    BP_CHECK(planes > 0 && H > 0 && W > 0, "planes, H and W must be positive");
    BP_CHECK((long long)planes * H * W < (1ll << 31), "a tensor of 2^31 elements or more");
}

static bp::KpdTrainOpt kt_opt(double lr, double alpha, double eps, double wd, double momentum) {
    BP_CHECK(lr >= 0 && alpha >= 0 && eps >= 0 && wd >= 0 && momentum >= 0, "negative hyper-parameter");
    return {(float)lr, (float)alpha, (float)(1.0 - alpha), (float)eps, (float)wd, (float)momentum};
}

extern "C" {

size_t bp_kpd_train_conv_scratch(int N, int C, int H, int W, int K, int size, int stride) {
    if (N <= 0 || C <= 0 || H <= 0 || W <= 0 || K <= 0 || !bp_train_conv_size_ok(size, true) || (stride != 1 && stride != 2)) return 0;
    return bp::train_conv_scratch(N, C, H, W, K, size, stride);
}

int bp_kpd_train_update_chunk(void) { return bp::kpd_train_update_chunk(); }

int bp_kpd_train_conv_host(int role, float* x, float* w, float* y, int N, int C, int H, int W, int K, int size, int stride,
                           float* scratch) {
    BP_TRY
    kt_check_conv(role, x, w, y, N, C, H, W, K, size, stride, scratch);
    bp::train_conv_host(role, x, w, y, N, C, H, W, K, size, stride, scratch);
    return 0;
    BP_CATCH
}

int bp_kpd_train_conv(int role, float* d_x, float* d_w, float* d_y, int N, int C, int H, int W, int K, int size, int stride,
                      float* d_scratch, void* stream) {
    BP_TRY
    kt_check_conv(role, d_x, d_w, d_y, N, C, H, W, K, size, stride, d_scratch);
    bp::launch_train_conv(role, d_x, d_w, d_y, N, C, H, W, K, size, stride, d_scratch, (hipStream_t)stream);
    return 0;
    BP_CATCH
}

int bp_kpd_train_bn_forward_host(const float* x, int N, int C, int S, const float* w, const float* b, float* running_mean,
                                 float* running_var, float* mean, float* invstd, float* out, int bn, int relu, int train) {
    BP_TRY
    kt_check_bn_forward(x, N, C, S, w, b, running_mean, running_var, mean, invstd, out, bn, train);
    bp::kpd_train_bn_forward_host(x, N, C, S, w, b, running_mean, running_var, mean, invstd, out, bn, relu, train);
    return 0;
    BP_CATCH
}

int bp_kpd_train_bn_forward(const float* d_x, int N, int C, int S, const float* d_w, const float* d_b, float* d_running_mean,
                            float* d_running_var, float* d_mean, float* d_invstd, float* d_out, int bn, int relu, int train,
                            void* stream) {
    BP_TRY
    kt_check_bn_forward(d_x, N, C, S, d_w, d_b, d_running_mean, d_running_var, d_mean, d_invstd, d_out, bn, train);
    kt_check_vec(S, {d_x, d_out});
    bp::launch_kpd_train_bn_forward(d_x, N, C, S, d_w, d_b, d_running_mean, d_running_var, d_mean, d_invstd, d_out, bn, relu, train,
                                    (hipStream_t)stream);
    return 0;
    BP_CATCH
}

int bp_kpd_train_bn_backward_host(const float* out, float* d, const float* x, const float* mean, const float* invstd, const float* w,
                                  int N, int C, int S, float* grad_w, float* grad_b, int bn, int relu) {
    BP_TRY
    kt_check_bn_backward(out, d, x, mean, invstd, w, N, C, S, grad_w, grad_b, bn, relu);
    bp::kpd_train_bn_backward_host(out, d, x, mean, invstd, w, N, C, S, grad_w, grad_b, bn, relu);
    return 0;
    BP_CATCH
}

int bp_kpd_train_bn_backward(const float* d_out, float* d_d, const float* d_x, const float* d_mean, const float* d_invstd,
                             const float* d_w, int N, int C, int S, float* d_grad_w, float* d_grad_b, int bn, int relu,
                             void* stream) {
    BP_TRY
    kt_check_bn_backward(d_out, d_d, d_x, d_mean, d_invstd, d_w, N, C, S, d_grad_w, d_grad_b, bn, relu);
    kt_check_vec(S, {d_out, d_d, d_x});
    bp::launch_kpd_train_bn_backward(d_out, d_d, d_x, d_mean, d_invstd, d_w, N, C, S, d_grad_w, d_grad_b, bn, relu,
                                     (hipStream_t)stream);
    return 0;
    BP_CATCH
}

int bp_kpd_train_tail_forward_host(const float* y, const float* s, const float* res, float* out, int N, int C, int S) {
    BP_TRY
    BP_CHECK(y && res && out, "null argument");
    kt_check_ncs(N, C, S);
    bp::kpd_train_tail_forward_host(y, s, res, out, N, C, S);
    return 0;
    BP_CATCH
}

int bp_kpd_train_tail_forward(const float* d_y, const float* d_s, const float* d_res, float* d_out, int N, int C, int S,
                              void* stream) {
    BP_TRY
    BP_CHECK(d_y && d_res && d_out, "null argument");
    kt_check_ncs(N, C, S);
    kt_check_vec(S, {d_y, d_res, d_out});
    bp::launch_kpd_train_tail_forward(d_y, d_s, d_res, d_out, N, C, S, (hipStream_t)stream);
    return 0;
    BP_CATCH
}

int bp_kpd_train_tail_backward_host(const float* out, const float* dout, const float* y, const float* s, float* dres, float* dy,
                                    float* ds, int N, int C, int S) {
    BP_TRY
    BP_CHECK(out && dout && dres && dy && dy != dout && dy != out && dy != y && dres != dout, "null or aliased argument");
    BP_CHECK(!s || (y && ds), "the gate's gradient needs y and ds");
    kt_check_ncs(N, C, S);
    bp::kpd_train_tail_backward_host(out, dout, y, s, dres, dy, ds, N, C, S);
    return 0;
    BP_CATCH
}

int bp_kpd_train_tail_backward(const float* d_out, const float* d_dout, const float* d_y, const float* d_s, float* d_dres,
                               float* d_dy, float* d_ds, int N, int C, int S, void* stream) {
    BP_TRY
    BP_CHECK(d_out && d_dout && d_dres && d_dy && d_dy != d_dout && d_dy != d_out && d_dy != d_y && d_dres != d_dout,
             "null or aliased argument");
    BP_CHECK(!d_s || (d_y && d_ds), "the gate's gradient needs y and ds");
    kt_check_ncs(N, C, S);
    kt_check_vec(S, {d_out, d_dout, d_y, d_dres, d_dy});
    bp::launch_kpd_train_tail_backward(d_out, d_dout, d_y, d_s, d_dres, d_dy, d_ds, N, C, S, (hipStream_t)stream);
    return 0;
    BP_CATCH
}

int bp_kpd_train_pool_forward_host(const float* y, int rows, int S, float* pool) {
    BP_TRY
    BP_CHECK(y && pool, "null argument");
    kt_check_ncs(rows, 1, S);
    bp::kpd_train_pool_forward_host(y, rows, S, pool);
    return 0;
    BP_CATCH
}

int bp_kpd_train_pool_forward(const float* d_y, int rows, int S, float* d_pool, void* stream) {
    BP_TRY
    BP_CHECK(d_y && d_pool, "null argument");
    kt_check_ncs(rows, 1, S);
    kt_check_vec(S, {d_y});
    bp::launch_kpd_train_pool_forward(d_y, rows, S, d_pool, (hipStream_t)stream);
    return 0;
    BP_CATCH
}

int bp_kpd_train_pool_backward_host(const float* dpool, float* dy, int rows, int S) {
    BP_TRY
    BP_CHECK(dpool && dy, "null argument");
    kt_check_ncs(rows, 1, S);
    bp::kpd_train_pool_backward_host(dpool, dy, rows, S);
    return 0;
    BP_CATCH
}

int bp_kpd_train_pool_backward(const float* d_dpool, float* d_dy, int rows, int S, void* stream) {
    BP_TRY
    BP_CHECK(d_dpool && d_dy, "null argument");
    kt_check_ncs(rows, 1, S);
    kt_check_vec(S, {d_dy});
    bp::launch_kpd_train_pool_backward(d_dpool, d_dy, rows, S, (hipStream_t)stream);
    return 0;
    BP_CATCH
}

int bp_kpd_train_sigmoid_forward_host(const float* x, float* s, long long n) {
    BP_TRY
    BP_CHECK(x && s && n > 0 && n < (1ll << 31), "null argument, or a count outside (0, 2^31)");
    bp::kpd_train_sigmoid_forward_host(x, s, n);
    return 0;
    BP_CATCH
}

int bp_kpd_train_sigmoid_forward(const float* d_x, float* d_s, long long n, void* stream) {
    BP_TRY
    BP_CHECK(d_x && d_s && n > 0 && n < (1ll << 31), "null argument, or a count outside (0, 2^31)");
    bp::launch_kpd_train_sigmoid_forward(d_x, d_s, n, (hipStream_t)stream);
    return 0;
    BP_CATCH
}

int bp_kpd_train_sigmoid_backward_host(const float* s, float* g, long long n) {
    BP_TRY
    BP_CHECK(s && g && n > 0 && n < (1ll << 31), "null argument, or a count outside (0, 2^31)");
    bp::kpd_train_sigmoid_backward_host(s, g, n);
    return 0;
    BP_CATCH
}

int bp_kpd_train_sigmoid_backward(const float* d_s, float* d_g, long long n, void* stream) {
    BP_TRY
    BP_CHECK(d_s && d_g && n > 0 && n < (1ll << 31), "null argument, or a count outside (0, 2^31)");
    bp::launch_kpd_train_sigmoid_backward(d_s, d_g, n, (hipStream_t)stream);
    return 0;
    BP_CATCH
}

int bp_kpd_train_maxpool_forward_host(const float* x, int planes, int H, int W, float* out, int* arg) {
    BP_TRY
    BP_CHECK(x && out && arg, "null argument");
    kt_check_pool_shape(planes, H, W);
    bp::kpd_train_maxpool_forward_host(x, planes, H, W, out, arg);
    return 0;
    BP_CATCH
}

int bp_kpd_train_maxpool_forward(const float* d_x, int planes, int H, int W, float* d_out, int* d_arg, void* stream) {
    BP_TRY
    BP_CHECK(d_x && d_out && d_arg, "null argument");
    kt_check_pool_shape(planes, H, W);
    bp::launch_kpd_train_maxpool_forward(d_x, planes, H, W, d_out, d_arg, (hipStream_t)stream);
    return 0;
    BP_CATCH
}

int bp_kpd_train_maxpool_backward_host(const float* dout, const int* arg, int planes, int H, int W, float* dx) {
    BP_TRY
    BP_CHECK(dout && arg && dx, "null argument");
    kt_check_pool_shape(planes, H, W);
    bp::kpd_train_maxpool_backward_host(dout, arg, planes, H, W, dx);
    return 0;
    BP_CATCH
}

int bp_kpd_train_maxpool_backward(const float* d_dout, const int* d_arg, int planes, int H, int W, float* d_dx, void* stream) {
    BP_TRY
    BP_CHECK(d_dout && d_arg && d_dx, "null argument");
    kt_check_pool_shape(planes, H, W);
    bp::launch_kpd_train_maxpool_backward(d_dout, d_arg, planes, H, W, d_dx, (hipStream_t)stream);
    return 0;
    BP_CATCH
}

int bp_kpd_train_rmsprop_host(const void* table, int tensors, double lr, double alpha, double eps, double weight_decay,
                              double momentum) {
    BP_TRY
    BP_CHECK(table && tensors > 0, "null or empty table");
    const bp::KpdTrainTensor* t = (const bp::KpdTrainTensor*)table;
    for (int i = 0; i < tensors; ++i)
        BP_CHECK(t[i].p && t[i].g && t[i].v && (momentum <= 0 || t[i].b) && t[i].count > 0 && t[i].count < (1ll << 40),
                 "a table row needs its pointers and a positive count");
    bp::kpd_train_rmsprop_host(t, tensors, kt_opt(lr, alpha, eps, weight_decay, momentum));
    return 0;
    BP_CATCH
}

int bp_kpd_train_rmsprop(const void* d_table, int tensors, int blocks, double lr, double alpha, double eps, double weight_decay,
                         double momentum, void* stream) {
    BP_TRY
    // the table stays on the device: its rows are the caller's to get right, as any pointer is; a block past the rows'
    // chunks does nothing
    BP_CHECK(d_table && tensors > 0 && tensors <= 65536 && blocks > 0, "null or empty table, or no blocks");
    bp::launch_kpd_train_rmsprop((const bp::KpdTrainTensor*)d_table, tensors, blocks, kt_opt(lr, alpha, eps, weight_decay, momentum),
                                 (hipStream_t)stream);
    return 0;
    BP_CATCH
}

}  // extern "C"
