// Detector validation (Darknet's `detector map`): the declarations shared by yolo_map_host.cpp, yolo_map.hip,
// eval_device.cpp and c_api_eval.cpp, so a signature that drifts fails to compile.  Needs no HIP header
// (yolo_map_host.cpp is plain C++): the stream type is declared as hip_runtime_api.h declares it.
#pragma once
#include <cstddef>
#include <cstdint>

typedef struct ihipStream_t* hipStream_t;

namespace bp {

int yolo_map_max_dets();                                            // the device's cap on max_dets
int yolo_map_max_heads();
size_t yolo_detections_scratch(int B, int max_dets, int classes);   // bytes: the candidate rows before they are ordered
size_t map_reduce_scratch(int D, int truths);                       // bytes: the rank keys and the first claimant per truth

// ---- yolo_map_host.cpp: the host twins, all pointers host.  heads [nheads][4] = (first row, anchors, gh, gw), checked
// by the caller; pred [B][rows][5 + classes]; dets [B][max_dets][6 + classes]; count [B]
void yolo_detections_host(const float* pred, int B, int rows, const int* heads, int nheads, int net_w, int net_h, int classes,
                          float thresh, float nms, int max_dets, float* dets, int* count);
// labels [M][5], first [B + 1] (checked by the caller); rec [B][rec_stride][6], rec_count [B], truth_classes_count
// [classes] (added to), img_stats [B][3] = (tp, fp, iou_sum)
void map_match_host(const float* dets, const int* count, int B, int max_dets, int classes, const float* labels, int M,
                    const int* first, float iou_thresh, float thresh_calc, int truth_base, int image_base, int rec_stride,
                    float* rec, int* rec_count, int* truth_classes_count, double* img_stats);
// rec [D][6]; img_stats [N][3]; ap [classes]; stats [8]; pr null or [classes][D][2] = (precision, recall) per rank
void map_reduce_host(const float* rec, int D, const int* truth_classes_count, int classes, int truths, const double* img_stats,
                     int N, double* ap, double* stats, double* pr);

// ---- yolo_map.hip: the same on device pointers (heads stays a host array), enqueued on s
void launch_yolo_detections(const float* pred, int B, int rows, const int* heads, int nheads, int net_w, int net_h, int classes,
                            float thresh, float nms, int max_dets, float* dets, int* count, void* scratch, hipStream_t s);
void launch_map_match(const float* dets, const int* count, int B, int max_dets, int classes, const float* labels, int M,
                      const int* first, float iou_thresh, float thresh_calc, int truth_base, int image_base, int rec_stride,
                      float* rec, int* rec_count, int* truth_classes_count, double* img_stats, int* claim, hipStream_t s);
void launch_map_reduce(const float* rec, int D, const int* truth_classes_count, int classes, int truths, const double* img_stats,
                       int N, double* ap, double* stats, double* pr, void* scratch, hipStream_t s);

// ---- eval_device.cpp: the device drivers (arguments checked by the caller); they only enqueue
#pragma GCC visibility push(hidden)     // the library's own: not in its dynamic symbol table
void yolo_detections(const float* pred, int B, int rows, const int* heads, int nheads, int net_w, int net_h, int classes,
                     float thresh, float nms, int max_dets, float* dets, int* count, void* scratch, hipStream_t s);
void map_match(const float* dets, const int* count, int B, int max_dets, int classes, const float* labels, int M, const int* first,
               float iou_thresh, float thresh_calc, int truth_base, int image_base, int rec_stride, float* rec, int* rec_count,
               int* truth_classes_count, double* img_stats, int* claim, hipStream_t s);
void map_reduce(const float* rec, int D, const int* truth_classes_count, int classes, int truths, const double* img_stats, int N,
                double* ap, double* stats, double* pr, void* scratch, hipStream_t s);
#pragma GCC visibility pop

}  // namespace bp
