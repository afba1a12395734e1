// A stand-alone run of the detector-training host twins (csrc/yolo_train_host.cpp) for the host sanitizers: one case of
// each of the three functions, on buffers of exactly the documented sizes so that a stray index is caught.
//   clang++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I betapose_amd/csrc \
//       tools/yolo_train_host_sanitize.cpp betapose_amd/csrc/yolo_train_host.cpp -o /tmp/yt_san && /tmp/yt_san
#include <cstdio>
#include <vector>

#include "yolo_train.h"

int main() {
    // inputs: two 37 x 70 frames, a crop past every edge, flipped and distorted, an odd output width, a zero sample
    const int N = 2, H = 37, W = 70, B = 3, net_h = 13, net_w = 10;
    std::vector<unsigned char> frames((size_t)N * H * W * 3);
    for (size_t i = 0; i < frames.size(); ++i) frames[i] = (unsigned char)((i * 2654435761u) >> 24);
    const int idx[B] = {0, 1, 5};
    const int crop[B * 4] = {-9, -6, 90, 50, 5, 4, 50, 29, 30, 5, 2, 2};
    const unsigned char flip[B] = {1, 0, 1};
    const float hsv[B * 3] = {-0.12f, 0.77f, 1.27f, 0.07f, 1.31f, 0.81f, 0.3f, 1.5f, 1.5f};
    std::vector<float> out((size_t)B * 3 * net_h * net_w);
    bp::yolo_inputs_host(frames.data(), N, H, W, idx, crop, flip, hsv, B, net_h, net_w, out.data());
    bp::yolo_inputs_host(frames.data(), N, H, W, idx, crop, flip, nullptr, B, net_h, net_w, out.data());
    double sum = 0.0;
    for (float v : out) sum += v;

    // truth rows: 95 labels in one sample (cut to 90), an empty sample, one with a marker line and a foreign class
    const int M = 99, max_boxes = 90;
    std::vector<float> labels((size_t)M * 5);
    std::vector<int> swap(M), order(M);
    for (int i = 0; i < M; ++i) {
        float* L = &labels[(size_t)i * 5];
        L[0] = (float)(i % 2), L[1] = 0.1f + 0.008f * i, L[2] = 0.9f - 0.008f * i, L[3] = i % 9 ? 0.2f : 0.0005f, L[4] = 0.1f;
        swap[i] = i < 95 ? (i * 7) % 95 : (i - 95 + 1) % 4;
    }
    labels[96 * 5 + 1] = labels[96 * 5 + 2] = 0.0f;
    labels[97 * 5] = 7.0f;
    const int first[4] = {0, 95, 95, 99};
    const float geom[12] = {0.03f, -0.03f, 1.05f, 0.95f, 0, 0, 1, 1, -0.07f, 0.07f, 0.97f, 1.1f};
    const unsigned char tflip[3] = {1, 0, 0};
    std::vector<float> truth((size_t)3 * max_boxes * 5);
    int kept[3];
    bp::yolo_truth_host(labels.data(), M, first, swap.data(), geom, tflip, 3, 2, max_boxes, 416, 416, 1, order.data(), truth.data(), kept);

    // loss: a 5 x 7 grid, 3 anchors, 2 classes, the truths above (a full row of 90 in image 0, none in image 1)
    const int n = 3, classes = 2, h = 7, w = 5, total = 9;
    const float anchors[18] = {10, 13, 16, 30, 33, 23, 30, 61, 62, 45, 59, 119, 116, 90, 156, 198, 373, 326};
    const int mask[3] = {3, 4, 5};
    const size_t elems = (size_t)3 * n * (5 + classes) * h * w;
    std::vector<float> x(elems), act(elems), delta(elems);
    for (size_t i = 0; i < elems; ++i) x[i] = (float)((int)((i * 40503u) % 600) - 300) / 100.0f;
    std::vector<double> partial(bp::yolo_loss_partials(3, n, classes, h, w));
    double cost, stats[7];
    bp::yolo_loss_host(x.data(), 3, n, classes, h, w, 416, 416, anchors, total, mask, truth.data(), max_boxes, 0.5f, 0.9f, act.data(),
                       delta.data(), &cost, stats, partial.data());
    bp::yolo_loss_host(x.data(), 3, n, classes, h, w, 416, 416, anchors, total, mask, truth.data(), max_boxes, 0.7f, 1.0f, nullptr,
                       delta.data(), &cost, stats, partial.data());
    std::printf("inputs sum %.6f, kept %d %d %d, cost %.6f, count %.0f\n", sum, kept[0], kept[1], kept[2], cost, stats[6]);
    return 0;
}
