/* Runs the reference's forward_yolo_layer (CPU, train = 1) on one head read from a file; the project's own driver for
 * tools/make_golden_yolo_train.py, compiled there against the reference's headers (-I) and oracle/_ref/libdarknet_ref.so.
 *
 *   yolo_layer_ref_driver <in> <out>
 *   in:  int32 B, n, total, classes, h, w, net_w, net_h, max_boxes; float32 ignore_thresh, truth_thresh; int32 mask[n];
 *        float32 anchors[2 total], truth[B max_boxes 5], x[B n (5 + classes) h w]
 *   out: float32 delta[...], output[...], cost
 * The layer's own log line goes to stdout. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "network.h"
#include "yolo_layer.h"

static void get(void* p, size_t size, size_t n, FILE* f) {
    if (fread(p, size, n, f) != n) {
        fprintf(stderr, "short input\n");
        exit(2);
    }
}

int main(int argc, char** argv) {
    if (argc != 3) return 2;
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 2;
    int hd[9];
    float th[2];
    get(hd, sizeof(int), 9, f);
    get(th, sizeof(float), 2, f);
    const int B = hd[0], n = hd[1], total = hd[2], classes = hd[3], h = hd[4], w = hd[5], max_boxes = hd[8];
    int* mask = calloc(n, sizeof(int));
    float* anchors = calloc(2 * total, sizeof(float));
    float* truth = calloc((size_t)B * max_boxes * 5, sizeof(float));
    const size_t count = (size_t)B * n * (5 + classes) * h * w;
    float* x = calloc(count, sizeof(float));
    get(mask, sizeof(int), n, f);
    get(anchors, sizeof(float), 2 * total, f);
    get(truth, sizeof(float), (size_t)B * max_boxes * 5, f);
    get(x, sizeof(float), count, f);
    fclose(f);

    layer l = make_yolo_layer(B, w, h, n, total, mask, classes, max_boxes);
    memcpy(l.biases, anchors, 2 * total * sizeof(float));
    l.ignore_thresh = th[0];
    l.truth_thresh = th[1];
    network_state state = {0};
    state.train = 1;
    state.truth = truth;
    state.input = x;
    state.net.w = hd[6];
    state.net.h = hd[7];
    state.index = 0;
    forward_yolo_layer(l, state);
    fflush(stdout);

    f = fopen(argv[2], "wb");
    if (!f) return 2;
    fwrite(l.delta, sizeof(float), count, f);
    fwrite(l.output, sizeof(float), count, f);
    fwrite(l.cost, sizeof(float), 1, f);
    fclose(f);
    return 0;
}
