// Detector training batches and the yolo-layer loss: the declarations shared by yolo_train_host.cpp, yolo_train.hip,
// eval_device.cpp and c_api_eval.cpp, so a signature that drifts fails to compile.  Needs no HIP header
// (yolo_train_host.cpp is plain C++): the stream type is declared as hip_runtime_api.h declares it.
#pragma once
#include <cstddef>
#include <cstdint>

typedef struct ihipStream_t* hipStream_t;

namespace bp {

// doubles of scratch bp_yolo_loss needs in `partial`: the any-obj block sums, the per-image sums of the truth walk and
// the block sums of the cost, in this order (yolo_train_host.cpp)
size_t yolo_loss_partials(int B, int n, int classes, int h, int w);

// ---- yolo_train_host.cpp: the host twins, all pointers host.  frames [N][H][W][3] uint8, frame_index [B] (an index
// outside [0, N) gives a zero sample), crop [B][4] = (pleft, ptop, swidth, sheight), flip [B], hsv [B][3] or null,
// out [B][3][net_h][net_w]
void yolo_inputs_host(const unsigned char* frames, int N, int H, int W, const int* frame_index, const int* crop,
                      const unsigned char* flip, const float* hsv, int B, int net_h, int net_w, float* out);
// labels [M][5] = (id, x, y, w, h), first [B + 1] (non-decreasing, within [0, M]: checked by the caller on the host,
// clamped by the kernel), swap [M], geom [B][4] = (dx, dy, sx, sy), flip [B], order [M] scratch,
// truth [B][max_boxes][5], kept [B]
void yolo_truth_host(const float* labels, int M, const int* first, const int* swap, const float* geom, const unsigned char* flip,
                     int B, int classes, int max_boxes, int net_w, int net_h, int small_object, int* order, float* truth,
                     int* kept);
// x, act (may be null), delta [B][n * (5 + classes)][h][w]; anchors [total][2]; mask [n] (values in [0, total): checked
// by the caller); truth [B][max_boxes][5]; cost [1]; stats [7] = sums of IoU, class, obj, any-obj, recall .5, recall .75
// and the count; partial [yolo_loss_partials()]
void yolo_loss_host(const float* x, int B, int n, int classes, int h, int w, int net_w, int net_h, const float* anchors, int total,
                    const int* mask, const float* truth, int max_boxes, float ignore_thresh, float truth_thresh, float* act,
                    float* delta, double* cost, double* stats, double* partial);

// ---- yolo_train.hip: the same on device pointers, enqueued on s
void launch_yolo_inputs(const unsigned char* frames, int N, int H, int W, const int* frame_index, const int* crop,
                        const unsigned char* flip, const float* hsv, int B, int net_h, int net_w, float* out, hipStream_t s);
void launch_yolo_truth(const float* labels, int M, const int* first, const int* swap, const float* geom, const unsigned char* flip,
                       int B, int classes, int max_boxes, int net_w, int net_h, int small_object, int* order, float* truth,
                       int* kept, hipStream_t s);
void launch_yolo_loss(const float* x, int B, int n, int classes, int h, int w, int net_w, int net_h, const float* anchors,
                      int total, const int* mask, const float* truth, int max_boxes, float ignore_thresh, float truth_thresh,
                      float* act, float* delta, double* cost, double* stats, double* partial, hipStream_t s);

// ---- eval_device.cpp: the device drivers (arguments checked by the caller); they only enqueue
#pragma GCC visibility push(hidden)     // the library's own: not in its dynamic symbol table
void yolo_inputs(const unsigned char* frames, int N, int H, int W, const int* frame_index, const int* crop,
                 const unsigned char* flip, const float* hsv, int B, int net_h, int net_w, float* out, hipStream_t s);
void yolo_truth(const float* labels, int M, const int* first, const int* swap, const float* geom, const unsigned char* flip, int B,
                int classes, int max_boxes, int net_w, int net_h, int small_object, int* order, float* truth, int* kept,
                hipStream_t s);
void yolo_loss(const float* x, int B, int n, int classes, int h, int w, int net_w, int net_h, const float* anchors, int total,
               const int* mask, const float* truth, int max_boxes, float ignore_thresh, float truth_thresh, float* act,
               float* delta, double* cost, double* stats, double* partial, hipStream_t s);
#pragma GCC visibility pop

}  // namespace bp
