// KPD training samples: the declarations shared by kpd_sample_host.cpp, kpd_sample.hip, eval_device.cpp and
// c_api_eval.cpp, so a signature that drifts fails to compile.  Needs no HIP header (kpd_sample_host.cpp is plain C++):
// the stream type is declared as hip_runtime_api.h declares it.
#pragma once
#include <cstddef>
#include <cstdint>

typedef struct ihipStream_t* hipStream_t;

namespace bp {

// ---- kpd_sample_host.cpp: the host twins, all pointers host.  gains [B][3], blank [B], perm [C], set_mask and grad may
// be null.  frames [N][H][W][3] uint8, frame_index [B] (an index outside [0, N) gives a zero sample), inp [B][3][inpH][inpW].
void kpd_inputs_host(const unsigned char* frames, int N, int H, int W, const int* frame_index, const float* ul, const float* br,
                     const float* gains, const unsigned char* blank, int B, int inpH, int inpW, float* inp);
// x, y [B][C][H][W] (distinct), flip [B], cs [B][2] = (cos, sin) of each sample's angle, perm [C] the channel a flipped
// sample reads for each output channel
void kpd_augment_host(const float* x, int B, int C, int H, int W, const unsigned char* flip, const double* cs, const int* perm,
                      float* y);
// out, labels, set_mask, grad [B][K][H][W]; partial [B * K] is scratch; loss [1], acc [K + 1], preds, gt [B][K][2],
// dists [K][B]
void heatmap_loss_acc_host(const float* out, const float* labels, const float* set_mask, int B, int K, int H, int W,
                           double* partial, double* loss, float* acc, int* preds, int* gt, float* dists, float* grad);

// ---- kpd_sample.hip: the same on device pointers, enqueued on s
void launch_kpd_inputs(const unsigned char* frames, int N, int H, int W, const int* frame_index, const float* ul,
                       const float* br, const float* gains, const unsigned char* blank, int B, int inpH, int inpW, float* inp,
                       hipStream_t s);
void launch_kpd_augment(const float* x, int B, int C, int H, int W, const unsigned char* flip, const double* cs, const int* perm,
                        float* y, hipStream_t s);
void launch_heatmap_loss_acc(const float* out, const float* labels, const float* set_mask, int B, int K, int H, int W,
                             double* partial, double* loss, float* acc, int* preds, int* gt, float* dists, float* grad,
                             hipStream_t s);

// ---- eval_device.cpp: the device drivers (arguments checked by the caller); they only enqueue
#pragma GCC visibility push(hidden)     // the library's own: not in its dynamic symbol table
void kpd_inputs(const unsigned char* frames, int N, int H, int W, const int* frame_index, const float* ul, const float* br,
                const float* gains, const unsigned char* blank, int B, int inpH, int inpW, float* inp, hipStream_t s);
void kpd_augment(const float* x, int B, int C, int H, int W, const unsigned char* flip, const double* cs, const int* perm,
                 float* y, hipStream_t s);
void heatmap_loss_acc(const float* out, const float* labels, const float* set_mask, int B, int K, int H, int W, double* partial,
                      double* loss, float* acc, int* preds, int* gt, float* dists, float* grad, hipStream_t s);
#pragma GCC visibility pop

}  // namespace bp
