// A stand-alone run of the detector-validation host twins (csrc/yolo_map_host.cpp) for the host sanitizers: the three
// calls in a chain, on buffers of exactly the documented sizes so that a stray index is caught; an image over max_dets,
// an image without labels, a label with an id outside the classes, D = 0.
//   clang++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I betapose_amd/csrc \
//       tools/yolo_map_host_sanitize.cpp betapose_amd/csrc/yolo_map_host.cpp -o /tmp/ym_san && /tmp/ym_san
#include <cstdio>
#include <vector>

#include "yolo_map.h"

int main() {
    const int B = 3, classes = 3, attrs = 5 + classes, S = 6 + classes, net = 64, max_dets = 40;
    const int heads[2 * 4] = {0, 3, 2, 3, 18, 2, 4, 4};        // 3 anchors on a 2 x 3 grid, 2 on a 4 x 4 grid
    const int rows = 18 + 32;
    std::vector<float> pred((size_t)B * rows * attrs);
    unsigned s = 12345u;
    auto rnd = [&]() { s = s * 1664525u + 1013904223u; return (float)(s >> 8) / 16777216.0f; };
    for (int b = 0; b < B; ++b)
        for (int r = 0; r < rows; ++r) {
            float* p = pred.data() + ((size_t)b * rows + r) * attrs;
            p[0] = 10.0f + 44.0f * rnd(), p[1] = 10.0f + 44.0f * rnd(), p[2] = 8.0f + 30.0f * rnd(), p[3] = 8.0f + 30.0f * rnd();
            p[4] = b == 1 ? (r % 3 ? 0.001f : rnd()) : rnd();   // image 1 keeps 17 candidates, images 0 and 2 overflow 40
            for (int k = 0; k < classes; ++k) p[5 + k] = rnd();
        }
    std::vector<float> dets((size_t)B * max_dets * S);
    std::vector<int> count(B);
    bp::yolo_detections_host(pred.data(), B, rows, heads, 2, net, net, classes, 0.005f, 0.45f, max_dets, dets.data(), count.data());
    std::vector<float> all((size_t)B * rows * S);
    std::vector<int> count_all(B);
    bp::yolo_detections_host(pred.data(), B, rows, heads, 2, net, net, classes, 0.005f, 0.45f, rows, all.data(), count_all.data());
    bp::yolo_detections_host(pred.data(), B, rows, heads, 2, net, net, classes, 0.005f, 0.0f, rows, all.data(), count_all.data());

    const int M = 5;
    const float labels[M * 5] = {0, 0.5f, 0.5f, 0.3f, 0.3f, 2, 0.3f, 0.4f, 0.4f, 0.2f, 7, 0.5f, 0.5f, 0.1f, 0.1f,
                                 1, 0.6f, 0.6f, 0.4f, 0.4f, -1, 0.2f, 0.2f, 0.1f, 0.1f};
    const int first[B + 1] = {0, 3, 3, 5};
    for (int stride : {rows * classes, 7}) {                    // the second cuts the record lists
        std::vector<float> rec((size_t)B * stride * 6);
        std::vector<int> rec_count(B), tcc(classes, 0);
        std::vector<double> st((size_t)B * 3);
        bp::map_match_host(all.data(), count_all.data(), B, rows, classes, labels, M, first, 0.5f, 0.25f, 11, 4, stride, rec.data(),
                           rec_count.data(), tcc.data(), st.data());
        std::vector<float> flat;
        for (int b = 0; b < B; ++b) {
            const int n = rec_count[b] < stride ? rec_count[b] : stride;
            flat.insert(flat.end(), rec.begin() + (size_t)b * stride * 6, rec.begin() + ((size_t)b * stride + n) * 6);
        }
        const int D = (int)(flat.size() / 6);
        std::vector<double> ap(classes), stats(8), pr((size_t)classes * D * 2);
        bp::map_reduce_host(flat.data(), D, tcc.data(), classes, 11 + M, st.data(), B, ap.data(), stats.data(), pr.data());
        bp::map_reduce_host(nullptr, 0, tcc.data(), classes, 11 + M, st.data(), B, ap.data(), stats.data(), nullptr);
        std::printf("stride %d: D %d, counts %d %d %d, mAP %.6f\n", stride, D, count[0], count[1], count[2], stats[0]);
    }
    return 0;
}
