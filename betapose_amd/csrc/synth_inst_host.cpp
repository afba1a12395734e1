// Host twin of the instance kernels (include/betapose_hip.h bp_synth_instances_host): plain loops over images, pixels
// and objects around synth_inst_math.inc, the text synth_inst.hip compiles too.  Equal to the kernels byte for byte.
#include <cstdint>

#include "synth.h"

namespace bp {

namespace {
#include "synth_inst_math.inc"
}  // namespace

void synth_instances_host(const float* alone, int J, int I, int H, int W, const unsigned char* present, unsigned char* ids,
                          float* depth, int* stats) {
    const size_t HW = (size_t)H * W;
    for (int i = 0; i < I; ++i) {
        unsigned char* m = ids + (size_t)i * HW;
        float* z = depth + (size_t)i * HW;
        for (size_t p = 0; p < HW; ++p) {
            float best = 0.0f;
            int id = 0;
            for (int j = 0; j < J; ++j)
                if (present[(size_t)i * J + j]) si_pick(alone[((size_t)j * I + i) * HW + p], j, best, id);
            m[p] = (unsigned char)id;
            z[p] = best;
        }
        for (int j = 0; j < J; ++j) {
            const float* a = alone + ((size_t)j * I + i) * HW;
            SiBox full = si_box_empty(), vis = si_box_empty();
            for (int y = 0; y < H; ++y)
                for (int x = 0; x < W; ++x) si_stats_add(full, vis, a[(size_t)y * W + x], m[(size_t)y * W + x], j, x, y);
            int* s = stats + ((size_t)i * J + j) * SY_INST_STATS;
            s[SI_PX_ALL] = full.count;
            s[SI_PX_VISIB] = vis.count;
            const SiBox* b[2] = {&full, &vis};
            for (int k = 0; k < 2; ++k) {
                int* o = s + (k ? SI_BOX_VISIB : SI_BOX_FULL);
                o[0] = b[k]->xmin;
                o[1] = b[k]->xmax;
                o[2] = b[k]->ymin;
                o[3] = b[k]->ymax;
                si_box_finish(o, b[k]->count);
            }
        }
    }
}

}  // namespace bp
