/* Runs the reference's CPU training step on a tiny network; the project's own driver for
 * tools/make_golden_darknet_train.py, compiled there against the reference's headers (-I) and
 * oracle/_ref/libdarknet_ref.so.
 *
 *   darknet_train_ref_driver train <cfg> <weights in> <batches> <calls> <detail> <dump> <weights out>
 *       batches: per call float32 x[batch 3 h w], truth[batch 90 5]; a file with one batch serves every call.
 *       detail 0: each call is train_network_datum.  detail 1: the same statements with a dump between the backward
 *       pass and update_network (forward_network, backward_network, get_network_cost, update_network as
 *       train_network_datum strings them), so the update buffers can be recorded before the update.
 *       dump, per call: float32 cost, rate (get_current_rate after the call's images are counted);
 *         detail 1 only: per convolution output, then with batch_normalize x, mean, variance, then weight_updates,
 *         bias_updates and (batch_normalize) scale_updates; per yolo layer delta;
 *         always, after the call: per convolution biases, (scales, rolling_mean, rolling_variance), weights, bias_updates,
 *         (scale_updates), weight_updates.
 *       weights out: save_weights after the last call.
 *   darknet_train_ref_driver rates <cfg> <out> <batch_num>...      float32 get_current_rate at each batch number */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "network.h"
#include "parser.h"

static void put(FILE* f, const float* p, size_t n) {
    if (fwrite(p, sizeof(float), n, f) != n) exit(3);
}

int main(int argc, char** argv) {
    if (argc >= 4 && !strcmp(argv[1], "rates")) {
        network net = parse_network_cfg(argv[2]);
        FILE* f = fopen(argv[3], "wb");
        if (!f) return 2;
        int i;
        for (i = 4; i < argc; ++i) {
            *net.seen = atoi(argv[i]) * net.batch * net.subdivisions;
            float r = get_current_rate(net);
            put(f, &r, 1);
        }
        fclose(f);
        return 0;
    }
    if (argc != 9 || strcmp(argv[1], "train")) return 2;
    network net = parse_network_cfg(argv[2]);
    load_weights(&net, argv[3]);
    const int calls = atoi(argv[5]), detail = atoi(argv[6]);
    const size_t nx = (size_t)net.batch * net.c * net.h * net.w, ny = (size_t)net.batch * 90 * 5;
    float* x = calloc(nx, sizeof(float));
    float* y = calloc(ny, sizeof(float));
    FILE* in = fopen(argv[4], "rb");
    FILE* out = fopen(argv[7], "wb");
    if (!in || !out) return 2;
    int call, i;
    for (call = 0; call < calls; ++call) {
        float* nxt = calloc(nx + ny, sizeof(float));
        if (fread(nxt, sizeof(float), nx + ny, in) == nx + ny) {
            memcpy(x, nxt, nx * sizeof(float));
            memcpy(y, nxt + nx, ny * sizeof(float));
        } else if (call == 0) {
            return 2;
        }
        free(nxt);
        float cost;
        if (!detail) {
            cost = train_network_datum(net, x, y);
        } else {
            network_state state;
            memset(&state, 0, sizeof(state));
            *net.seen += net.batch;
            state.index = 0;
            state.net = net;
            state.input = x;
            state.delta = 0;
            state.truth = y;
            state.train = 1;
            forward_network(net, state);
            backward_network(net, state);
            cost = get_network_cost(net);
        }
        float rate = get_current_rate(net);
        put(out, &cost, 1);
        put(out, &rate, 1);
        if (detail) {
            for (i = 0; i < net.n; ++i) {
                layer l = net.layers[i];
                if (l.type == CONVOLUTIONAL) {
                    put(out, l.output, (size_t)l.outputs * l.batch);
                    if (l.batch_normalize) {
                        put(out, l.x, (size_t)l.outputs * l.batch);
                        put(out, l.mean, l.n);
                        put(out, l.variance, l.n);
                    }
                    put(out, l.weight_updates, (size_t)l.n * l.c * l.size * l.size);
                    put(out, l.bias_updates, l.n);
                    if (l.batch_normalize) put(out, l.scale_updates, l.n);
                } else if (l.type == YOLO) {
                    put(out, l.delta, (size_t)l.outputs * l.batch);
                }
            }
            if (((*net.seen) / net.batch) % net.subdivisions == 0) update_network(net);
        }
        for (i = 0; i < net.n; ++i) {
            layer l = net.layers[i];
            if (l.type != CONVOLUTIONAL) continue;
            put(out, l.biases, l.n);
            if (l.batch_normalize) {
                put(out, l.scales, l.n);
                put(out, l.rolling_mean, l.n);
                put(out, l.rolling_variance, l.n);
            }
            put(out, l.weights, (size_t)l.n * l.c * l.size * l.size);
            put(out, l.bias_updates, l.n);
            if (l.batch_normalize) put(out, l.scale_updates, l.n);
            put(out, l.weight_updates, (size_t)l.n * l.c * l.size * l.size);
        }
    }
    fclose(in);
    fclose(out);
    save_weights(net, argv[8]);
    return 0;
}
