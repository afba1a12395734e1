// Pose verification by gradient agreement (include/betapose_hip.h bp_image_gradients, bp_gradient_scores; DESIGN.md
// 3.18): unit Sobel gradients of uint8 images and the score of renders against a scene's gradients.  verify_host.cpp is
// the host twin and needs no HIP header; verify.hip holds the kernels.  The two give the same bytes.
#pragma once
#include <cstdint>
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#endif

namespace bp {

// images [I][H][W][3] uint8 -> grad [I][H][W][2] (nx, ny) and, unless NULL, mag [I][H][W]; H, W >= 3
void image_gradients_host(const uint8_t* images, int I, int H, int W, int red_channel, int min_sq, float* grad, float* mag);
// renders [P][H][W][3] against scene_grad [T][H][W][2]: sum [P] (units of 2^-24), count [P] (kept render pixels),
// score [P] = sum / 2^24 / (count + 1); a frame index outside [0, T): sum 0, count -1, score NaN
void gradient_scores_host(const uint8_t* renders, const float* scene_grad, const int* frame_index, int P, int T, int H, int W,
                          int red_channel, int render_min_sq, uint64_t* sum, int* count, double* score);

#if defined(__HIPCC__)
void launch_image_gradients(const uint8_t* d_images, int I, int H, int W, int red_channel, int min_sq, float* d_grad,
                            float* d_mag, hipStream_t s);
void launch_gradient_scores(const uint8_t* d_renders, const float* d_scene_grad, const int* d_frame_index, int P, int T, int H,
                            int W, int red_channel, int render_min_sq, unsigned long long* d_sum, int* d_count, double* d_score,
                            hipStream_t s);
#endif

}  // namespace bp
