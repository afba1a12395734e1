// Key-point annotator: the declarations shared by annotate_host.cpp, annotate.hip, eval_device.cpp and c_api_eval.cpp, so
// a signature that drifts fails to compile.  Needs no HIP header (annotate_host.cpp is plain C++): the stream type is
// declared as hip_runtime_api.h declares it.
#pragma once
#include <cstddef>
#include <cstdint>

typedef struct ihipStream_t* hipStream_t;

namespace bp {

constexpr int ANNOT_BOX_INTS = 5;      // accumulator ints per box: xmin, xmax, ymin, ymax, count (annotate_math.inc)

// ---- annotate_host.cpp: the host twins, all pointers host.  model_depth [P][H][W], scene_depth [T][H][W] and
// scene_index [P] may be null (scene_depth and scene_index together); a scene index outside [0, T) has been refused by
// the caller.
void annotate_keypoints_host(const double* poses, int P, const double* kp, int Kp, const double* K, int H, int W,
                             double pixel_center, double near, const float* model_depth, const float* scene_depth,
                             const int* scene_index, double self_tol, double delta, double* xy, double* z,
                             unsigned char* flags);
void mask_boxes_host(const float* depth, int P, int H, int W, const double* K, double pixel_center, const float* scene_depth,
                     const int* scene_index, double delta, int* boxes, int* counts);
void vertex_boxes_host(const double* poses, int P, const double* vertices, int n, const double* K, int H, int W, int* boxes);
void kpd_targets_host(const double* parts, const float* ul, const float* br, int B, int Kp, int inpH, int inpW, int resH,
                      int resW, const float* g, int size, float* out, int* centres, float* set_mask);

// ---- annotate.hip: the same on device pointers, enqueued on s
void launch_annotate_keypoints(const double* poses, int P, const double* kp, int Kp, const double* K, int H, int W,
                               double pixel_center, double near, const float* model_depth, const float* scene_depth,
                               const int* scene_index, double self_tol, double delta, double* xy, double* z,
                               unsigned char* flags, hipStream_t s);
// acc [P][2][ANNOT_BOX_INTS] is scratch that the launch initialises itself; boxes [P][2][4], counts [P][2]
void launch_mask_boxes(const float* depth, int P, int H, int W, const double* K, double pixel_center, const float* scene_depth,
                       const int* scene_index, double delta, int* acc, int* boxes, int* counts, hipStream_t s);
// acc [P][ANNOT_BOX_INTS] likewise; boxes [P][4]
void launch_vertex_boxes(const double* poses, int P, const double* vertices, int n, const double* K, int H, int W, int* acc,
                         int* boxes, hipStream_t s);
void launch_kpd_targets(const double* parts, const float* ul, const float* br, int B, int Kp, int inpH, int inpW, int resH,
                        int resW, const float* g, int size, float* out, int* centres, float* set_mask, hipStream_t s);

// ---- eval_device.cpp: the device drivers (arguments checked by the caller, the scene indices among them): the host
// twins' arguments on device pointers (K stays host) plus the stream.  The two box drivers bring their accumulators and
// return when their work is done; the other two only enqueue.
#pragma GCC visibility push(hidden)     // the library's own: not in its dynamic symbol table
void annotate_keypoints(const double* poses, int P, const double* kp, int Kp, const double* K, int H, int W, double pixel_center,
                        double near, const float* model_depth, const float* scene_depth, const int* scene_index,
                        double self_tol, double delta, double* xy, double* z, unsigned char* flags, hipStream_t s);
void mask_boxes(const float* depth, int P, int H, int W, const double* K, double pixel_center, const float* scene_depth,
                const int* scene_index, double delta, int* boxes, int* counts, hipStream_t s);
void vertex_boxes(const double* poses, int P, const double* vertices, int n, const double* K, int H, int W, int* boxes,
                  hipStream_t s);
void kpd_targets(const double* parts, const float* ul, const float* br, int B, int Kp, int inpH, int inpW, int resH, int resW,
                 const float* g, int size, float* out, int* centres, float* set_mask, hipStream_t s);
#pragma GCC visibility pop

}  // namespace bp
