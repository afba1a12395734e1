/* Runs the reference's detection list and its `detector map` for tools/make_golden_yolo_map.py; the project's own driver,
 * compiled there against the reference's headers (-I) and oracle/_ref/libdarknet_ref.so.
 *
 *   yolo_map_ref_driver boxes <in> <out>
 *     in:  int32 nheads, classes, total, net_w, net_h; float32 thresh, nms; float32 anchors[2 total]; per head int32 n, gh,
 *          gw, mask[n], float32 output[n (5 + classes) gh gw] (l.output: activated, Darknet's layout)
 *     out: int32 nboxes; per box float32 x, y, w, h, objectness, prob[classes]
 *          = get_network_boxes(net, 1, 1, thresh, 0, 0, 0, &n, 0) then, if nms, do_nms_sort(dets, n, classes, nms)
 *   yolo_map_ref_driver map <data> <cfg> <weights> <thresh_calc_avg_iou>
 *     validate_detector_map itself; its report goes to stdout
 *   yolo_map_ref_driver rows <list> <cfg> <weights> <out>
 *     per image of the list, as validate_detector_map prepares it (load_image_color, resize_image, network_predict):
 *     out gets, per [yolo] layer in order, int32 n, gh, gw and float32 l.output[n (5 + classes) gh gw]                  */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "network.h"
#include "parser.h"
#include "yolo_layer.h"
#include "box.h"
#include "image.h"
#include "data.h"
#include "utils.h"

void validate_detector_map(char* datacfg, char* cfgfile, char* weightfile, float thresh_calc_avg_iou);

static void get(void* p, size_t size, size_t n, FILE* f) {
    if (n && fread(p, size, n, f) != n) {
        fprintf(stderr, "short input\n");
        exit(2);
    }
}

static int boxes(const char* in, const char* out) {
    FILE* f = fopen(in, "rb");
    if (!f) return 2;
    int hd[5];
    float th[2];
    get(hd, sizeof(int), 5, f);
    get(th, sizeof(float), 2, f);
    const int nheads = hd[0], classes = hd[1], total = hd[2];
    float* anchors = calloc(2 * total, sizeof(float));
    get(anchors, sizeof(float), 2 * total, f);
    network net = make_network(nheads);
    net.w = hd[3];
    net.h = hd[4];
    for (int i = 0; i < nheads; ++i) {
        int g[3];
        get(g, sizeof(int), 3, f);
        int* mask = calloc(g[0], sizeof(int));
        get(mask, sizeof(int), g[0], f);
        layer l = make_yolo_layer(1, g[2], g[1], g[0], total, mask, classes, 90);
        memcpy(l.biases, anchors, 2 * total * sizeof(float));
        get(l.output, sizeof(float), (size_t)g[0] * (5 + classes) * g[1] * g[2], f);
        net.layers[i] = l;
    }
    fclose(f);
    int n = 0;
    detection* dets = get_network_boxes(&net, 1, 1, th[0], 0, 0, 0, &n, 0);
    if (th[1]) do_nms_sort(dets, n, classes, th[1]);
    f = fopen(out, "wb");
    if (!f) return 2;
    fwrite(&n, sizeof(int), 1, f);
    for (int i = 0; i < n; ++i) {
        fwrite(&dets[i].bbox, sizeof(float), 4, f);
        fwrite(&dets[i].objectness, sizeof(float), 1, f);
        fwrite(dets[i].prob, sizeof(float), classes, f);
    }
    fclose(f);
    return 0;
}

static int rows(char* list, char* cfg, char* weights, const char* out) {
    network net = parse_network_cfg_custom(cfg, 1);
    load_weights(&net, weights);
    fuse_conv_batchnorm(net);
    FILE* names = fopen(list, "r");
    FILE* f = fopen(out, "wb");
    if (!names || !f) return 2;
    char path[4096];
    while (fgets(path, sizeof path, names)) {
        path[strcspn(path, "\r\n")] = 0;
        if (!path[0]) continue;
        image im = load_image_color(path, 0, 0);
        image r = resize_image(im, net.w, net.h);
        network_predict(net, r.data);
        for (int i = 0; i < net.n; ++i) {
            layer l = net.layers[i];
            if (l.type != YOLO) continue;
            int g[3] = {l.n, l.h, l.w};
            fwrite(g, sizeof(int), 3, f);
            fwrite(l.output, sizeof(float), (size_t)l.n * (5 + l.classes) * l.h * l.w, f);
        }
        free_image(im);
        free_image(r);
    }
    fclose(f);
    fclose(names);
    return 0;
}

int main(int argc, char** argv) {
    if (argc == 4 && !strcmp(argv[1], "boxes")) return boxes(argv[2], argv[3]);
    if (argc == 6 && !strcmp(argv[1], "map")) {
        validate_detector_map(argv[2], argv[3], argv[4], (float)atof(argv[5]));
        fflush(stdout);
        return 0;
    }
    if (argc == 6 && !strcmp(argv[1], "rows")) return rows(argv[2], argv[3], argv[4], argv[5]);
    return 2;
}
