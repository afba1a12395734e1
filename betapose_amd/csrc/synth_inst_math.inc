// Instance ownership of a multi-object scene, ONE source for the host twin (synth_inst_host.cpp) and the kernels
// (synth_inst.hip): who owns a pixel, and the counts and boxes of an object's full and visible masks (DESIGN.md 3.16).
// One float comparison per (pixel, object) and integer minimum / maximum / sum: nothing depends on who computes a pixel
// or in which order the pixels are met, so host and device agree byte for byte by construction.
// Plain C++17, no HIP header.  Included inside `namespace bp { namespace {` after <cstdint> and synth.h.
#ifndef BP_HD
#if defined(__HIPCC__)
#define BP_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define BP_HD inline
#endif
#endif

constexpr int SI_EMPTY_MIN = 0x7fffffff;     // a box nothing was added to
constexpr int SI_EMPTY_MAX = -1;
// a row of `stats`: px_all, px_visib, the full box and the visible box, each (xmin, xmax, ymin, ymax)
constexpr int SI_PX_ALL = 0, SI_PX_VISIB = 1, SI_BOX_FULL = 2, SI_BOX_VISIB = 6;
static_assert(SI_BOX_VISIB + 4 == SY_INST_STATS, "synth.h and synth_inst_math.inc disagree");

// Object j's depth d at a pixel against the winner so far (id = 1 + its index, 0: none yet).  The objects are offered in
// ASCENDING j and `<=` lets the later one take a tie: equal positive floats have equal bits, so this is the rule of
// render_color(into=...), whose later call wins a fragment of exactly the same depth.  A NaN is not > 0: never drawn.
BP_HD void si_pick(float d, int j, float& best, int& id) {
    if (d > 0.0f && (id == 0 || d <= best)) {
        best = d;
        id = j + 1;
    }
}

struct SiBox {
    int xmin, xmax, ymin, ymax, count;
};

BP_HD SiBox si_box_empty() { return SiBox{SI_EMPTY_MIN, SI_EMPTY_MAX, SI_EMPTY_MIN, SI_EMPTY_MAX, 0}; }

BP_HD void si_box_add(SiBox& b, int x, int y) {
    b.xmin = x < b.xmin ? x : b.xmin;
    b.xmax = x > b.xmax ? x : b.xmax;
    b.ymin = y < b.ymin ? y : b.ymin;
    b.ymax = y > b.ymax ? y : b.ymax;
    ++b.count;
}

// the pixel (x, y) of object j (stats id j + 1): d its depth alone, owner the scene's id there
BP_HD void si_stats_add(SiBox& full, SiBox& vis, float d, int owner, int j, int x, int y) {
    if (!(d > 0.0f)) return;
    si_box_add(full, x, y);
    if (owner == j + 1) si_box_add(vis, x, y);
}

// a box of the accumulated row as it is returned: -1 four times when its count is 0
BP_HD void si_box_finish(int* box, int count) {
    if (count > 0) return;
    box[0] = box[1] = box[2] = box[3] = -1;
}
