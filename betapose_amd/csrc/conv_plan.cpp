// The convolution planner: which kernel runs a layer and with how many K slices -- the measured tables, the heuristics for the shapes no
// table has, the policy a caller may set -- and the launch layouts that follow from the choice (K cut, hybrid tail, XCD-home, filter
// prefetch).  Host only: nothing here touches the device; the per-kernel conv_*_eligible predicates live beside their kernels.
#include "conv_plan.h"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "engine.h"

namespace bp {

// One row of every table: a layer shape at one batch size -> the kernel and the K slices it runs fastest with.
struct PlanRow { int M, CoutPad, nchunks, tile, splits; };

static bool env_set(const char* name) { return std::getenv(name) != nullptr; }
static int env_int(const char* name, int dflt) { const char* v = std::getenv(name); return v ? std::atoi(v) : dflt; }
// filter prefetch (ConvParams::pf_*): one extra block per (N-tile, K-slice) pair of the next launch pulls at most this much
static const int kPrefetchCap = env_int("BP_PF_CAP_KB", 128) * 1024;
static std::vector<PlanRow> read_plan_file(const char* path) {
    std::vector<PlanRow> v;
    if (FILE* f = path ? std::fopen(path, "r") : nullptr) {
        PlanRow e;
        while (std::fscanf(f, "%d %d %d %d %d", &e.M, &e.CoutPad, &e.nchunks, &e.tile, &e.splits) == 5) v.push_back(e);
        std::fclose(f);
    }
    return v;
}

// The planner's switches (A/B runs, tests, sweeps), read once per process, at the first plan.  BP_HYBRID and BP_XCD_FAULT are not
// here on purpose: they are read per call, outside anything cached (conv_hybrid_plan, Net::prepare_conv).
struct PlanSwitches {
    const bool no_s1 = env_set("BP_NO_S1");          // the batched fp16 1x1 layers stay on the plane tiles (no conv_s1.hip)
    const bool no_p3 = env_set("BP_NO_P3");          // the batched fp16 3x3 / stride-1 layers stay on the halo plane tile (no conv_p3.hip)
    const int p3_k1 = env_int("BP_P3_K1", 1);        // conv_p3.hip's 1x1 form: 0 off, 1 the layers with K >= 512, 2 every eligible 1x1 layer
    const bool no_halo = env_set("BP_NO_HALO");      // bf16x3 without conv_halo.hip: the round-3 plan, filters-direct kernel everywhere
    const bool no_stem7 = env_set("BP_NO_STEM7");    // the 7x7 RGB stem of the fp16 modes on the fp32 MFMA kernel
#ifdef BP_EXPERIMENTAL
    const bool legacy = env_set("BP_LEGACY");        // the fp32-activation kernels in every mode (A/B runs of the whole pipeline)
    const bool b3_pl64bd = env_set("BP_B3_PL64BD");  // bf16x3 on planes with the filters-direct plane tile (conv_pl.hip BDIR)
#else
    static constexpr bool legacy = false, b3_pl64bd = false;
#endif
    // "M CoutPad nchunks tile splits" lines that take precedence over the built-in tables, so that a tuning sweep can be tried in the
    // whole pipeline without a rebuild (tools only)
    const std::vector<PlanRow> plan_file = read_plan_file(std::getenv("BP_PLAN_FILE"));
};
static const PlanSwitches& sw() { static const PlanSwitches s; return s; }

// Split-K slice counts measured on MI355X for every batch-1 conv shape of the two networks, one kernel at a time
// (tools/tune_conv.py, 64x64 tile): {M, CoutPad, K-chunks, the fp32 tile, slices}.  Other shapes use the fill rule in plan_conv.
static const PlanRow kSplitTable[] = {
    {    80,   512,   64, TILE_64x64,  6},
    {    80,   512,  144, TILE_64x64, 12},
    {    80,  2048,   16, TILE_64x64,  3},
    {    80,  2048,   32, TILE_64x64,  3},
    {   169,    64,   32, TILE_64x64, 10},
    {   169,   256,   16, TILE_64x64,  5},
    {   169,   512,   32, TILE_64x64,  5},
    {   169,  1024,  144, TILE_64x64,  5},
    {   320,   256,   32, TILE_64x64,  5},
    {   320,   256,   72, TILE_64x64,  8},
    {   320,   512,   32, TILE_64x64,  5},
    {   320,  1024,    8, TILE_64x64,  1},
    {   320,  1024,   16, TILE_64x64,  3},
    {   320,  1024,  144, TILE_64x64,  6},
    {   676,    64,   16, TILE_64x64,  4},
    {   676,   128,    8, TILE_64x64,  3},
    {   676,   256,   16, TILE_64x64,  3},
    {   676,   256,   24, TILE_64x64,  5},
    {   676,   512,   72, TILE_64x64,  5},
    {  1280,   128,   16, TILE_64x64,  3},
    {  1280,   128,   36, TILE_64x64,  5},
    {  1280,   256,   16, TILE_64x64,  3},
    {  1280,   512,    4, TILE_64x64,  1},
    {  1280,   512,    8, TILE_64x64,  1},
    {  1280,   512,   72, TILE_64x64,  3},
    {  2704,    64,    8, TILE_64x64,  1},
    {  2704,   128,    8, TILE_64x64,  1},
    {  2704,   128,   12, TILE_64x64,  2},
    {  2704,   256,   36, TILE_64x64,  4},
    {  5120,    64,    2, TILE_64x64,  1},
    {  5120,    64,    8, TILE_64x64,  1},
    {  5120,    64,   18, TILE_64x64,  3},
    {  5120,    64,   36, TILE_64x64,  3},
    {  5120,   128,    8, TILE_64x64,  1},
    {  5120,   256,    2, TILE_64x64,  1},
    { 10816,    64,    4, TILE_64x64,  1},
    { 10816,   128,   18, TILE_64x64,  3},
    { 43264,    64,    2, TILE_64x64,  1},
    { 43264,    64,    9, TILE_64x64,  1},
};

// 16-bit precision modes: {M, CoutPad, K-chunks} -> {tile, slices}, measured one kernel at a time over both kernel
// families (tools/tune_conv.py [--f16 | --kg], profiles/r02_tune_{b3,f16,b3_kernels}.txt: at batch 1 the 64x64-block
// kernels of conv_igemm.hip win every shape of the two networks, in the bf16x3 mode its filters-direct variant; the
// slice counts are those the whole pipeline runs fastest with, which are higher than a kernel timed alone prefers);
// other shapes use the heuristic in choose_h16.
// COVERAGE: the rows below are the conv shapes of the two networks at BATCH 1 (M = OH x OW of one 416x416 frame / one 320x256 crop);
// the conv_pl tables further down also carry batch 28 (BASELINE configs[2]).  Any other batch size or input resolution takes the
// heuristics in choose_h16 / choose_pl, which are measured at batch 2, 4 and 28 only (tools/batch_check.sh, profiles/r04_batched.txt).
static const PlanRow kPlanB3[] = {
    // (round 4, TILE_BD_K2 rows: the filters-direct tile with two K groups inside an eight-wave block and about half the K slices
    // between blocks -- alone it is no faster than the four-wave tile on any shape (tools/bench_bdk2.py, profiles/r04_bdk2_kernels.txt),
    // in the pipeline the plan with these rows is +2-2.8 % on three boxes (tools/plans/bdk2*.txt, profiles/r04_ab_bdk2.txt): fewer
    // blocks and slabs for the same work)
    // round 4, conv_halo.hip: the 3x3 / stride-1 layers on the tap-resident halo tile -- rows apply where conv_halo_eligible()
    // holds (a stride-2 layer of the same {M, CoutPad, K-chunks} falls through to its filters-direct row below).  Slice counts from
    // A/B runs of the whole pipeline, four frames in flight (profiles/r04_halo_ab.txt)
    // (first the 64x128 tile with 8 / 6 / 4 / 3 / 2 slices: +4-5 %; then the 64x64 tile with two K groups inside the block and half the
    // slices -- none at 52x52: a further +1.2-2 %, tools/plans/k2*.txt)
    {   169,  1024,  144, TILE_HALO64K2,  4},
    {   320,  1024,  144, TILE_HALO64K2,  4},
    {   676,   512,   72, TILE_HALO64K2,  2},
    {  1280,   512,   72, TILE_HALO64K2,  2},
    {  2704,   256,   36, TILE_HALO64K2,  1},
    {    80,   512,   64, TILE_BD_K2,  4},
    {    80,   512,  144, TILE_BD_K2,  6},
    {    80,  2048,   16, TILE_BD_K2,  2},
    {    80,  2048,   32, TILE_BD_K2,  2},
    {   169,    64,   32, TILE_BD_K2,  6},
    {   169,   256,   16, TILE_BD_K2,  3},
    {   169,   512,   32, TILE_BD_K2,  6},
    {   169,  1024,  144, TILE_64x64_BD,  5},
    {   320,   256,   32, TILE_BD_K2,  6},
    {   320,   256,   72, TILE_BD_K2,  6},
    {   320,   512,   32, TILE_BD_K2,  3},
    {   320,  1024,    8, TILE_BD_K2,  1},
    {   320,  1024,   16, TILE_BD_K2,  2},
    {   320,  1024,  144, TILE_64x64_BD,  6},
    {   676,    64,   16, TILE_BD_K2,  3},
    {   676,   128,    8, TILE_BD_K2,  1},
    {   676,   256,   16, TILE_BD_K2,  3},
    {   676,   256,   24, TILE_BD_K2,  3},
    {   676,   512,   72, TILE_64x64_BD,  5},
    {  1280,   128,   16, TILE_BD_K2,  3},
    {  1280,   128,   36, TILE_BD_K2,  3},
    {  1280,   256,   16, TILE_BD_K2,  2},
    {  1280,   512,    4, TILE_64x64_BD,  1},
    {  1280,   512,    8, TILE_BD_K2,  1},
    {  1280,   512,   72, TILE_64x64_BD,  3},
    {  2704,    64,    8, TILE_BD_K2,  1},
    {  2704,   128,    8, TILE_BD_K2,  1},
    {  2704,   128,   12, TILE_BD_K2,  1},
    {  2704,   256,   36, TILE_64x64_BD,  2},   // in the pipeline: 2 slices 933, 3: 929, 4: 921, 5+: 910 frames/s (tools/tune_splits_insitu.py)
    {  5120,    64,    2, TILE_64x64_BD,  1},
    {  5120,    64,    8, TILE_BD_K2,  1},
    {  5120,    64,   18, TILE_BD_K2,  2},
    {  5120,    64,   36, TILE_BD_K2,  2},
    {  5120,   128,    8, TILE_BD_K2,  1},
    {  5120,   256,    2, TILE_64x64_BD,  1},
    { 10816,    64,    4, TILE_BD_K2,  1},
    { 10816,   128,   18, TILE_BD_K2,  1},
    { 43264,    64,    2, TILE_64x64_BD,  1},
    { 43264,    64,    9, TILE_64x64_BD,  1},
};
// The lone-frame latency mode (Net::set_prefetch) keeps the four-wave filters-direct tile on the rows the table above gives to TILE_BD_K2:
// its XCD-local hand-off and filter prefetch blocks exist for that tile (conv_home_layout, conv_prefetch_of), and one frame at a time
// they are worth more than the K groups (2.46 against 2.56 ms per frame).  Slice counts: the round-3 table.
static const PlanRow kPlanB3Lone[] = {
    {    80,   512,   64, TILE_64x64_BD,  6},
    {    80,   512,  144, TILE_64x64_BD, 10},
    {    80,  2048,   16, TILE_64x64_BD,  3},
    {    80,  2048,   32, TILE_64x64_BD,  3},
    {   169,    64,   32, TILE_64x64_BD, 10},
    {   169,   256,   16, TILE_64x64_BD,  5},
    {   169,   512,   32, TILE_64x64_BD,  5},
    {   320,   256,   32, TILE_64x64_BD,  5},
    {   320,   256,   72, TILE_64x64_BD,  8},
    {   320,   512,   32, TILE_64x64_BD,  5},
    {   320,  1024,    8, TILE_64x64_BD,  1},
    {   320,  1024,   16, TILE_64x64_BD,  3},
    {   676,    64,   16, TILE_64x64_BD,  5},
    {   676,   128,    8, TILE_64x64_BD,  1},
    {   676,   256,   16, TILE_64x64_BD,  3},
    {   676,   256,   24, TILE_64x64_BD,  5},
    {  1280,   128,   16, TILE_64x64_BD,  3},
    {  1280,   128,   36, TILE_64x64_BD,  5},
    {  1280,   256,   16, TILE_64x64_BD,  3},
    {  1280,   512,    8, TILE_64x64_BD,  1},
    {  2704,    64,    8, TILE_64x64_BD,  1},
    {  2704,   128,    8, TILE_64x64_BD,  1},
    {  2704,   128,   12, TILE_64x64_BD,  1},
    {  5120,    64,    8, TILE_64x64_BD,  1},
    {  5120,    64,   18, TILE_64x64_BD,  3},
    {  5120,    64,   36, TILE_64x64_BD,  3},
    {  5120,   128,    8, TILE_64x64_BD,  1},
    { 10816,    64,    4, TILE_64x64_BD,  1},
    { 10816,   128,   18, TILE_64x64_BD,  2},
};
#ifdef BP_EXPERIMENTAL
// (fp16, batch 1: the filters-direct variant wins 40 of 47 shapes alone by 4.5 % in the sum, profiles/r02_tune_f16.txt, and
// LOSES in the pipeline -- 1 329 against 1 381 frames/s, A/B on one box -- so the batch-1 rows stay on the staged kernel)
static const PlanRow kPlanF16[] = {
    {    80,   512,   64, 0,  5},
    {    80,   512,  144, 0,  6},
    {    80,  2048,   16, 0,  1},
    {    80,  2048,   32, 0,  3},
    {   169,    64,   32, 0,  4},
    {   169,   256,   16, 0,  1},
    {   169,   512,   32, 0,  3},
    {   169,  1024,  144, 0,  5},
    {   320,   256,   32, 0,  3},
    {   320,   256,   72, 0,  5},
    {   320,   512,   32, 0,  3},
    {   320,  1024,    8, 0,  1},
    {   320,  1024,   16, 0,  1},
    {   320,  1024,  144, 0,  5},
    {   676,    64,   16, 0,  1},
    {   676,   128,    8, 0,  1},
    {   676,   256,   16, 0,  1},
    {   676,   256,   24, 0,  1},
    {   676,   512,   72, 0,  5},
    {  1280,   128,   16, 0,  1},
    {  1280,   128,   36, 0,  3},
    {  1280,   256,   16, 0,  1},
    {  1280,   512,    4, 0,  1},
    {  1280,   512,    8, 0,  1},
    {  1280,   512,   72, 0,  3},
    {  2704,    64,    8, 0,  1},
    {  2704,   128,    8, 0,  1},
    {  2704,   128,   12, 0,  1},
    {  2704,   256,   36, 0,  1},
    {  5120,    64,    2, 0,  1},
    {  5120,    64,    8, 0,  1},
    {  5120,    64,   18, 0,  1},
    {  5120,    64,   36, 0,  3},
    {  5120,   128,    8, 0,  1},
    {  5120,   256,    2, 0,  1},
    { 10816,    64,    4, 0,  1},
    { 10816,   128,   18, 0,  1},
    { 43264,    64,    2, 0,  1},
    { 43264,    64,    9, 0,  1},
    // batch 28 (BASELINE configs[2]; profiles/r02_tune_f16_batch28.txt, with the 128x64 block and the filters-direct kernel among the candidates)
    {  2240,   512,   64, 1,  1},
    {  2240,   512,  144, 1,  1},
    {  2240,  2048,   16, 0,  1},
    {  2240,  2048,   32, 0,  1},
    {  4732,    64,   32, 12,  1},
    {  4732,   256,   16, 1,  1},
    {  4732,   512,   32, 12,  1},
    {  4732,  1024,  144, 1,  1},
    {  8960,   256,   32, 6,  1},
    {  8960,   256,   72, 6,  1},
    {  8960,   512,   32, 0,  1},
    {  8960,  1024,    8, 0,  1},
    {  8960,  1024,   16, 0,  1},
    {  8960,  1024,  144, 1,  1},
    { 18928,    64,   16, 0,  1},
    { 18928,   128,    8, 6,  1},
    { 18928,   256,   16, 0,  1},
    { 18928,   256,   24, 0,  1},
    { 18928,   512,   72, 6,  1},
    { 35840,   128,   16, 0,  1},
    { 35840,   128,   36, 0,  1},
    { 35840,   256,   16, 6,  1},
    { 35840,   512,    4, 0,  1},
    { 35840,   512,    8, 0,  1},
    { 35840,   512,   72, 6,  1},
    { 75712,    64,    8, 0,  1},
    { 75712,   128,    8, 0,  1},
    { 75712,   128,   12, 6,  1},
    { 75712,   256,   36, 6,  1},
    {143360,    64,    2, 0,  1},
    {143360,    64,    8, 0,  1},
    {143360,    64,   18, 12,  1},
    {143360,    64,   36, 12,  1},
    {143360,   128,    8, 6,  1},
    {143360,   256,    2, 0,  1},
    {302848,    64,    4, 0,  1},
    {302848,   128,   18, 6,  1},
    {1211392,    64,    2, 12,  1},
    {1211392,    64,    9, 1,  1},
};
#endif   // BP_EXPERIMENTAL

// conv_pl.hip, bf16x3 mode, batch 1: {M, CoutPad, K-chunks} -> {tile, slices}, every conv shape of the two networks timed alone with the
// epilogue the networks run (residual + operand planes; tools/tune_conv.py --pl, profiles/r03_tune_pl_b3.txt)
static const PlanRow kPlanPL3[] = {
    {    80,   512,   64, TILE_PL64,  6},
    {    80,   512,  144, TILE_PL64, 10},
    {    80,  2048,   16, TILE_PL64,  3},
    {    80,  2048,   32, TILE_PL64,  3},
    {   169,    64,   32, TILE_PL64, 10},
    {   169,   256,   16, TILE_PL64,  4},
    {   169,   512,   32, TILE_PL64,  4},
    {   169,  1024,  144, TILE_PL64,  5},
    {   320,   256,   32, TILE_PL64,  4},
    {   320,   256,   72, TILE_PL64,  5},
    {   320,   512,   32, TILE_PL64,  3},
    {   320,  1024,    8, TILE_PL64,  1},
    {   320,  1024,   16, TILE_PL64,  1},
    {   320,  1024,  144, TILE_PL64,  3},
    {   676,    64,   16, TILE_PL64,  5},
    {   676,   128,    8, TILE_PL64,  1},
    {   676,   256,   16, TILE_PL64,  3},
    {   676,   256,   24, TILE_PL64,  3},
    {   676,   512,   72, TILE_PL64,  2},
    {  1280,   128,   16, TILE_PL64,  3},
    {  1280,   128,   36, TILE_PL64,  4},
    {  1280,   256,   16, TILE_PL64,  1},
    {  1280,   512,    4, TILE_PL64,  1},
    {  1280,   512,    8, TILE_PL64,  1},
    {  1280,   512,   72, TILE_PL64,  3},
    {  2704,    64,    8, TILE_PL64,  1},
    {  2704,   128,    8, TILE_PL64,  1},
    {  2704,   128,   12, TILE_PL64,  1},
    {  2704,   256,   36, TILE_PL64,  1},
    {  5120,    64,    2, TILE_PL64,  1},
    {  5120,    64,    8, TILE_PL64,  1},
    {  5120,    64,   18, TILE_PL64,  1},
    {  5120,    64,   36, TILE_PL64,  2},
    {  5120,   128,    8, TILE_PL64,  1},
    {  5120,   256,    2, TILE_PL64,  1},
    { 10816,    64,    4, TILE_PL64,  1},
    { 10816,   128,   18, TILE_PL64,  1},
    { 43264,    64,    2, TILE_PL64,  1},
    { 43264,    64,    9, TILE_PL64,  1},
};
// ... fp16 mode (tools/tune_conv.py --pl --f16, profiles/r03_tune_pl_f16.txt)
static const PlanRow kPlanPL1[] = {
    {    80,   512,   64, TILE_PL64,  4},
    {    80,   512,  144, TILE_PL64,  6},
    {    80,  2048,   16, TILE_PL64,  1},
    {    80,  2048,   32, TILE_PL64,  1},
    {   169,    64,   32, TILE_PL64,  4},
    {   169,   256,   16, TILE_PL64,  3},
    {   169,   512,   32, TILE_PL64,  4},
    {   169,  1024,  144, TILE_PL64,  4},
    {   320,   256,   32, TILE_PL64,  4},
    {   320,   256,   72, TILE_PL64,  4},
    {   320,   512,   32, TILE_PL64,  3},
    {   320,  1024,    8, TILE_PL64,  1},
    {   320,  1024,   16, TILE_PL64,  1},
    {   320,  1024,  144, TILE_PL64,  3},
    {   676,    64,   16, TILE_PL64,  1},
    {   676,   128,    8, TILE_PL64,  1},
    {   676,   256,   16, TILE_PL64,  1},
    {   676,   256,   24, TILE_PL64,  1},
    {   676,   512,   72, TILE_PL64,  2},
    {  1280,   128,   16, TILE_PL64,  1},
    {  1280,   128,   36, TILE_PL64,  3},
    {  1280,   256,   16, TILE_PL64,  1},
    {  1280,   512,    4, TILE_PL64,  1},
    {  1280,   512,    8, TILE_PL64,  1},
    {  1280,   512,   72, TILE_PL64,  3},
    {  2704,    64,    8, TILE_PL64,  1},
    {  2704,   128,    8, TILE_PL64,  1},
    {  2704,   128,   12, TILE_PL64,  1},
    {  2704,   256,   36, TILE_PL64,  1},
    {  5120,    64,    2, TILE_PL64,  1},
    {  5120,    64,    8, TILE_PL64,  1},
    {  5120,    64,   18, TILE_PL64,  1},
    {  5120,    64,   36, TILE_PL64,  1},
    {  5120,   128,    8, TILE_PL64,  1},
    {  5120,   256,    2, TILE_PL64,  1},
    { 10816,    64,    4, TILE_PL64,  1},
    { 10816,   128,   18, TILE_PL64,  1},
    { 43264,    64,    2, TILE_PL64,  1},
    { 43264,    64,    9, TILE_PL64,  1},
    // batch 28 (BASELINE configs[2]; tools/tune_conv.py --pl --f16 --big --batch 28, profiles/r03_tune_pl_f16_batch28.txt)
    // round 4: the 3x3 / stride-1 layers on the halo form of the 128x128 tile (TILE_PLH128; tools/bench_plh.py, profiles/r04_plh_kernels.txt:
    // 7-10 % faster alone than the best all-DMA tile, +1.7-2.6 % on configs[2]).  A row is taken only by layers the tile can run
    // (choose_pl checks conv_plh_eligible): the stride-2 layers that share a row's key fall through to the row below it
    {   4732,  1024,  144, TILE_PLH128,  1},
    {   8960,  1024,  144, TILE_PLH128,  1},   // DUC1 / DUC2 (round 5: their PixelShuffle stores take the staged epilogue in conv_pl.hip too)
    {  35840,   512,   72, TILE_PLH128,  1},
    {   8960,   256,   72, TILE_PLH128,  1},
    {  18928,   512,   72, TILE_PLH128,  1},
    {  35840,   128,   36, TILE_PLH128,  1},
    {  75712,   256,   36, TILE_PLH128,  1},
    { 302848,   128,   18, TILE_PLH128,  1},   // the 104x104 layers (round 5: 384 halo rows)
    {   2240,   512,   64, TILE_PL64,  1},
    {   2240,   512,  144, TILE_PL64,  1},
    {   2240,  2048,   16, TILE_PL64,  1},
    {   2240,  2048,   32, TILE_PL128,  1},
    {   4732,    64,   32, TILE_PL64,  1},
    {   4732,   256,   16, TILE_PL128x64,  1},
    {   4732,   512,   32, TILE_PL64,  1},
    {   4732,  1024,  144, TILE_PL128,  1},
    {   8960,   256,   32, TILE_PL64,  1},
    {   8960,   256,   72, TILE_PL64,  1},
    {   8960,   512,   32, TILE_PL64,  1},
    {   8960,  1024,    8, TILE_PL64,  1},
    {   8960,  1024,   16, TILE_PL64,  1},
    {   8960,  1024,  144, TILE_PL256x128,  1},
    {  18928,    64,   16, TILE_PL64,  1},
    {  18928,   128,    8, TILE_PL64,  1},
    {  18928,   256,   16, TILE_PL64,  1},
    {  18928,   256,   24, TILE_PL64,  1},
    {  18928,   512,   72, TILE_PL256x128,  1},
    {  35840,   128,   16, TILE_PL64,  1},
    {  35840,   128,   36, TILE_PL64,  1},
    {  35840,   256,   16, TILE_PL64,  1},
    {  35840,   512,    4, TILE_PL64,  1},
    {  35840,   512,    8, TILE_PL64,  1},
    {  35840,   512,   72, TILE_PL256x128,  1},
    {  75712,    64,    8, TILE_PL64,  1},
    {  75712,   128,    8, TILE_PL64,  1},
    {  75712,   128,   12, TILE_PL256x128,  1},
    {  75712,   256,   36, TILE_PL128,  1},
    { 143360,    64,    2, TILE_PL64,  1},
    { 143360,    64,    8, TILE_PL64,  1},
    { 143360,    64,   18, TILE_PL64,  1},
    { 143360,    64,   36, TILE_PL64,  1},
    { 143360,   128,    8, TILE_PL64,  1},
    { 143360,   256,    2, TILE_PL64,  1},
    { 302848,    64,    4, TILE_PL64,  1},
    { 302848,   128,   18, TILE_PL256x128,  1},
    {1211392,    64,    2, TILE_PL64,  1},
    {1211392,    64,    9, TILE_PL64,  1},
};

// The one lookup of every table: the first row of this shape whose tile can run the layer.
template <class Table, class CanRun>
static const PlanRow* find_row(const Table& table, int M, int CoutPad, int nchunks, CanRun can_run) {
    for (const PlanRow& e : table)
        if (e.M == M && e.CoutPad == CoutPad && e.nchunks == nchunks && can_run(e)) return &e;
    return nullptr;
}
static bool any_row(const PlanRow&) { return true; }

static long long grid_tiles(long long M, int CoutPad, int tile) {
    const int bm = conv_tile_bm(tile), bn = conv_tile_bn(tile);
    return ((M + bm - 1) / bm) * ((CoutPad + bn - 1) / bn);
}
// the fill rule: K slices until the grid has `target` blocks, with at least min_chunks chunks per slice
static int fill_splits(long long blocks, int nchunks, int target, int min_chunks, int max_splits) {
    int s = 1;
    while (blocks * s < target && nchunks / (s + 1) >= min_chunks && s < max_splits) ++s;
    return s;
}

// conv_pl.hip (operand planes + LDS-DMA): which block tile, how many K slices
static ConvLaunch choose_pl(const ConvParams& c, long long M, int mode, int sk_max) {
    auto plh_fits = [&](const PlanRow& e) { return !conv_tile_is_plh(e.tile) || conv_plh_eligible(c); };     // (a 3x3 row also matches stride-2 / 1x1 layers of the same K)
    // (a plan-file row naming the streaming 1x1 kernel for a layer it cannot run is ignored, not a failed launch)
    const PlanRow* e = find_row(sw().plan_file, (int)M, c.CoutPad, c.nchunks, [&](const PlanRow& r) {
        return conv_tile_is_pl(r.tile) && plh_fits(r) && (r.tile != TILE_S1 || (r.splits == 1 && conv_s1_eligible(c, M))) &&
               (r.tile != TILE_P3 || (r.splits == 1 && conv_p3_eligible(c, M)));
    });
    if (!e) e = mode == PREC_F16 ? find_row(kPlanPL1, (int)M, c.CoutPad, c.nchunks, plh_fits) : find_row(kPlanPL3, (int)M, c.CoutPad, c.nchunks, plh_fits);
    if (e) return {e->tile, e->splits};
    // other shapes (batched runs): the 128x128 block once its grid covers the chip (half the operand bytes per FLOP of the
    // 64x64 block: profiles/r03_bench_pl_batch28.txt), else the 64x64 block with enough K slices to fill it
    // (short K loops -- the 1x1 layers of the bottlenecks -- stay on the 64x64 block even then: a 128x128 block runs one per
    // CU and its prologue / epilogue are not covered by a neighbour's K loop; profiles/r03_tune_pl_f16_batch28.txt)
    const long long tiles128 = ((M + 127) / 128) * ((c.CoutPad + 127) / 128);
    int t = (c.CoutPad >= 128 && tiles128 >= 192 && c.nchunks >= 32) ? TILE_PL128 : TILE_PL64;
    if (t == TILE_PL128 && mode == PREC_F16 && conv_plh_eligible(c)) t = TILE_PLH128;     // 3x3 / stride 1: the halo form beats the all-DMA tile wherever both run
    int s = 1;
    if (t == TILE_PL64) s = fill_splits(grid_tiles(M, c.CoutPad, t), c.nchunks, 256, mode == PREC_F16 ? 8 : 4, sk_max);
    return {t, s};
}

static ConvLaunch choose_h16(const ConvParams& c, long long M, int mode, int sk_max, bool lone) {
    // layers with operand planes (the fp16 mode; bf16x3 under BP_B3_PLANES) run on conv_pl.hip
    if (conv_pl_eligible(c) && !sw().legacy) {
        ConvLaunch k = choose_pl(c, M, mode, sk_max);
        if (k.tile == TILE_PL64 && mode == PREC_BF16X3 && c.wbd && sw().b3_pl64bd) k.tile = TILE_PL64BD;
        return k;
    }
    if (mode == PREC_BF16X3)
        if (const PlanRow* e = find_row(sw().plan_file, (int)M, c.CoutPad, c.nchunks, [&](const PlanRow& r) {
                return !conv_tile_is_pl(r.tile) && (!conv_tile_is_halo(r.tile) || conv_halo_eligible(c, r.tile)); }))
            return {e->tile, e->splits};
    const bool halo_on = !sw().no_halo && mode == PREC_BF16X3;
    auto halo_fits = [&](const PlanRow& r) { return !conv_tile_is_halo(r.tile) || (halo_on && conv_halo_eligible(c, r.tile)); };
#ifdef BP_EXPERIMENTAL
    const PlanRow* e = mode == PREC_F16 ? find_row(kPlanF16, (int)M, c.CoutPad, c.nchunks, halo_fits) : find_row(kPlanB3, (int)M, c.CoutPad, c.nchunks, halo_fits);
#else
    const PlanRow* e = find_row(kPlanB3, (int)M, c.CoutPad, c.nchunks, halo_fits);
#endif
    if (e) {
        if (lone && e->tile == TILE_BD_K2)
            if (const PlanRow* l = find_row(kPlanB3Lone, e->M, e->CoutPad, e->nchunks, any_row)) e = l;
        return {e->tile, e->splits};
    }
    int t = TILE_64x64_BD;   // bf16x3: the filters-direct 64x64 kernel at every batch size (profiles/r02_tune_b3_batch28.txt)
    // ... except the 3x3 / stride-1 layers of batched runs once one slice of halo tiles fills the chip: the 64x128 halo tile is
    // 1.2-1.5x the filters-direct kernel there (batch 28: 52x52 128 -> 256 217.6 against 319.0 us, 40x32 256 -> 512 378.8 against
    // 545.1 us; tools/bench_halo.py --batch 28, profiles/r04_halo_kernels.txt)
    constexpr int halo_min_tiles = 64;   // (64: batch 2 x 4 streams 1 118 -> 1 209, 4 x 3 1 274 -> 1 384, 28 x 2 1 509 -> 1 754 frames/s; 256 and 16 lose 4-8 % of that at batch 2 / 4)
    if (halo_on && c.in16 == nullptr) {
        const int ht = conv_halo_eligible(c, TILE_HALO128) ? TILE_HALO128 : (conv_halo_eligible(c, TILE_HALO64K2) ? TILE_HALO64K2 : -1);
        if (ht >= 0 && ((M + 63) / 64) * (c.CoutPad / conv_tile_bn(ht)) >= halo_min_tiles) return {ht, 1};
    }
#ifdef BP_EXPERIMENTAL
    const long long tiles128 = ((M + 127) / 128) * ((c.CoutPad + 127) / 128);
    if (!(mode == PREC_BF16X3 && c.w16s)) t = (c.CoutPad >= 128 && tiles128 >= 128) ? TILE_W64_2x2 : TILE_64x64;
#endif
    const int target = t == TILE_W64_2x2 ? 256 : (mode == PREC_F16 ? 128 : 512);
    return {t, fill_splits(grid_tiles(M, c.CoutPad, t), c.nchunks, target, mode == PREC_F16 ? 8 : 4, sk_max)};
}

// a forced kernel id (bp_*_set_policy, tests and sweeps) applies to the layers it can run and is ignored for the others:
// the fp32-MFMA tiles run any layer (they read the fp32 activations), the operand-plane tiles the layers with planes
static bool tile_runs(int tile, const ConvParams& c, long long M = 0) {
    // a layer planned on the operand planes (in16 + wpl) may have NO fp32 input: plan_planes() dropped the fp32 store of producers
    // whose readers all take the planes.  The kernels that read fp32 activations are therefore never forced onto such a layer
    // (round-3 advisor finding: a forced tile 0 / 1 in the fp16 mode read tensors nobody stored)
    const bool on_planes = c.in16 != nullptr && c.wpl != nullptr;
    if (tile == TILE_64x64 || tile == TILE_128x64) return !on_planes;
    if (tile == TILE_S1) return conv_s1_eligible(c, M);
    if (tile == TILE_P3) return conv_p3_eligible(c, M);
    if (conv_tile_is_pl(tile)) return c.mfma_mode != PREC_F32 && conv_pl_eligible(c) && (!conv_tile_is_plh(tile) || conv_plh_eligible(c));
    if (tile == TILE_64x64_BD || tile == TILE_BD_K2) return c.mfma_mode == PREC_BF16X3 && conv_h16_eligible(c) && c.w16s != nullptr && !on_planes;
    if (conv_tile_is_halo(tile)) return c.mfma_mode == PREC_BF16X3 && c.in16 == nullptr && conv_halo_eligible(c, tile);
#ifdef BP_EXPERIMENTAL
    if (tile >= 0 && tile <= TILE_LAST) return c.mfma_mode != PREC_F32 && conv_h16_eligible(c);
#endif
    return false;
}

ConvLaunch plan_conv(const Op& op, int batch, const PlanPolicy& pol) {
    const ConvParams& c = op.conv;
    const int mode = c.mfma_mode, force_tile = pol.force_tile;
    const long long M = (long long)batch * c.OH * c.OW;
    const bool default_policy = pol.sk_target == 512 && pol.sk_min_chunks == 4 && pol.sk_max == 8;   // (else: an explicit policy -- tests, sweeps)
    int t = TILE_64x64, s = 1;   // fp32 MFMA kernel: 128x64 measured slower on every layer of both networks (tools/bench_conv.py)
    if (mode != PREC_F32) {
        const ConvLaunch k = choose_h16(c, M, mode, pol.sk_max, pol.lone);
        t = k.tile; s = k.splits;
        if (t == TILE_S1 && op.pool_out) t = TILE_PL64;     // (a plan-file row: the SE pool rides in the 64-row epilogue of the plane tile only)
        const bool one_f16_launch = mode == PREC_F16 && s == 1 && !op.pool_out;
        // round 5: the 1x1 layers of the batched fp16 runs (one K slice on a conv_pl tile, no SE pool in the epilogue) on the persistent
        // streaming kernel (conv_s1.hip)
        if (!sw().no_s1 && one_f16_launch && conv_tile_is_pl(t) && conv_s1_eligible(c, M)) t = TILE_S1;
        // round 6: the 3x3 / stride-1 layers of the batched fp16 runs that were planned on the halo plane tile, on the persistent kernel
        // (conv_p3.hip)
        if (!sw().no_p3 && one_f16_launch && t == TILE_PLH128 && conv_p3_eligible(c, M)) t = TILE_P3;
        // ... and its 1x1 form (128-channel groups as the "halo", four chunks as the "taps") for the 1x1 layers with K >= 512, whether they were
        // planned on the plane tile or on the streaming kernel (28 frames, f16r, one launch at a time, profiles/r06_bench_p1.txt: 20x16 1 024 -> 256
        // 15.1 / 16.4 -> 12.3 us, 13x13 1 024 -> 512 15.0 / 16.4 -> 12.5, 26x26 512 -> 256 17.2 / 16.5 -> 13.4, 40x32 512 -> 128 17.7 / 16.8 -> 15.5;
        // at K = 256 the streaming kernel keeps its layers: 256 -> 1 024 16.3 against 17.9, 52x52 256 -> 128 15.7 against 16.4)
        if (!sw().no_p3 && sw().p3_k1 && one_f16_launch && c.ksize == 1 && conv_tile_is_pl(t) && conv_p3_eligible(c, M) &&
            (sw().p3_k1 == 2 || c.Cin >= 512)) t = TILE_P3;
        if (force_tile >= 0 && !((force_tile == TILE_S1 || force_tile == TILE_P3) && op.pool_out) && tile_runs(force_tile, c, M)) t = force_tile;
        if (!default_policy) s = fill_splits(grid_tiles(M, c.CoutPad, t), c.nchunks, pol.sk_target, pol.sk_min_chunks, pol.sk_max);
    } else if ((force_tile < 0 || force_tile == TILE_STEM3) && conv_stem3_eligible(c)) {
        t = TILE_STEM3;       // the RGB 3x3 / stride-1 stem: direct convolution (conv_igemm.hip stem3x3_kernel) unless a tile is forced, no K slices
    } else if (!sw().no_stem7 && force_tile < 0 && c.net_prec == PREC_F16 && conv_stem7_eligible(c)) {
        // the 7x7 / stride-2 RGB stem when the ENGINE is in an fp16 mode (the layer itself is not 16-bit eligible: 3 input channels): fp16
        // MFMA over im2col rows in LDS, no K slices
        t = TILE_STEM7;
    } else {
        if ((force_tile == TILE_64x64 || force_tile == TILE_128x64) && tile_runs(force_tile, c)) t = force_tile;
        s = fill_splits(grid_tiles(M, c.CoutPad, t), c.nchunks, pol.sk_target, pol.sk_min_chunks, pol.sk_max);     // (CoutPad is a multiple of 64)
        if (t == TILE_64x64 && default_policy)   // default policy: measured table
            if (const PlanRow* e = find_row(kSplitTable, (int)M, c.CoutPad, c.nchunks, any_row)) s = e->splits;
    }
    return conv_launch_of(c, t, s);
}

void conv_split_plan(const ConvParams& p, int tile, int want, int* splits, int* cps) {
    const int unit = ((conv_tile_is_halo(tile) || conv_tile_is_plh(tile)) && p.nchunks % 9 == 0 && p.nchunks >= 9) ? 9 : 1;          // chunks that stay together (a layer the halo tiles cannot run is refused by the launcher)
    const int units = p.nchunks / unit;
    int s = want < 1 ? 1 : (want > units ? units : want);
    const int per = (units + s - 1) / s;
    s = (units + per - 1) / per;
    *splits = s; *cps = per * unit;
}

ConvLaunch conv_launch_of(const ConvParams& p, int tile, int want) {
    ConvLaunch l{tile, 1, 0};
    if (want <= 0) want = fill_splits(conv_tiles(p, tile), p.nchunks, 512, 4, 64);
    if (tile == TILE_S1 || tile == TILE_P3) want = 1;     // (a persistent grid: no K slices)
    conv_split_plan(p, tile, want, &l.splits, &l.cps);
    return l;
}

// Hybrid grid of a one-slice conv_pl launch (ConvParams::hy_*): when the launch is ONE block per CU plus a few more (256 < tiles
// <= 422 on 256 CUs), 256 tiles run whole and the rest are cut along K so that they spread over every CU instead of doubling
// up on a few.  Measured at batch 28, fp16 (profiles/r03_hybrid_grid.txt): 296 tiles of 256x128 72.2 -> 65.9 us, 280 tiles
// 124.8 -> 106.1 us, 296 tiles of 128x128 72.5 -> 67.5 us; with several blocks per CU in flight the dispatcher balances the
// tail by itself and the cut only adds its reduction (1 184 tiles of 128x128: 79.8 -> 98.8 us), so longer grids stay whole.
// In the PIPELINE it loses -- fp16 batch 28 x 3 streams 3 940-4 010 against 4 060-4 140 frames/s, the other runs unchanged: with
// other streams' blocks on the CUs there is no "one block per CU" to complete -- so it is OFF unless BP_HYBRID=1 (A/B runs, tests).
bool conv_hybrid_plan(const ConvParams& p, int tile, size_t partial_floats, HybridTail* h) {
    // (read per call on purpose: tests/test_gpu_conv.py::test_conv_pl_hybrid_grid toggles it inside one process; the lookup only runs
    // for one-slice conv_pl launches in eager mode and at graph capture, never in a graph replay)
    const bool off = std::getenv("BP_HYBRID") == nullptr;
    if (off || !conv_tile_is_pl(tile) || p.splits != 1 || p.xcd_home || p.nchunks < 16) return false;
    if (!(tile == TILE_PL64 || tile == TILE_PL128 || tile == TILE_PL128x64 || tile == TILE_PL256x128)) return false;
    const int T = conv_tiles(p, tile), unit = 256;
    const int rem = T - unit;
    if (rem <= 0 || rem * 100 > unit * 65) return false;
    int s = std::min(std::min(unit / rem, 8), p.nchunks / 8);
    if (s < 2) return false;
    const int cps = (p.nchunks + s - 1) / s;
    s = (p.nchunks + cps - 1) / cps;
    if (conv_slab_floats(tile, s, rem) > partial_floats) return false;
    h->full = unit; h->splits = s; h->cps = cps; h->tiles = rem; h->slab_floats = conv_slab_floats(tile, s, rem);
    return true;
}

bool conv_home_layout(int tile, int splits) {
    return splits > 1 && splits <= 64 && xcc_base() >= 0 && (tile == TILE_64x64_BD || (conv_tile_is_pl(tile) && !conv_tile_is_plh(tile)));
}

bool conv_pool_in_epilogue_ok(const ConvParams& c, int batch, int tile) {
    if (conv_tile_bm(tile) != 64 || conv_tile_bn(tile) != 64) return false;
    if (c.store_mode != ST_NHWC || c.res || c.res_scale || c.act != ACT_LINEAR || (c.out_ld & 3) || (c.Cout & 3)) return false;
    return batch == 1 || (c.OH * c.OW) % 64 == 0;
}

// p's launch carries the prefetch blocks for `next` (launched as nl), when next's work blocks of residue x read the N-tiles
// n == x (mod min(N-tiles, 8)) -- the xcd_home layout, or the plain one-slice grid of the 64x64 filters-direct kernel -- from a filter
// image that is contiguous per (N-tile, K-slice) pair
void conv_prefetch_of(ConvParams& p, const ConvParams& next, const ConvLaunch& nl) {
    p.pf_ptr = nullptr;
    const int nt = nl.tile, ns = nl.splits;
    const bool plbd = nt == TILE_PL64BD && next.mfma_mode == PREC_BF16X3 && next.wbd && conv_home_layout(nt, ns);
    const bool pl = plbd || (next.mfma_mode != PREC_F32 && (nt == TILE_PL64) && next.wpl && conv_home_layout(nt, ns));
    const bool bd = nt == TILE_64x64_BD && next.mfma_mode == PREC_BF16X3 && next.w16s && (ns == 1 || conv_home_layout(nt, ns));
    const int ntn = (next.CoutPad + 63) / 64;
    if (!(pl || bd) || (ntn & (ntn - 1)) != 0 || xcc_base() < 0) return;
    const int np = next.mfma_mode == PREC_F16 ? 1 : 3;
    p.pf_ptr = plbd ? (const void*)next.wbd : pl ? (const void*)next.wpl : (const void*)next.w16s;
    p.pf_ntn = ntn; p.pf_splits = ns; p.pf_cps = nl.cps; p.pf_nchunks = next.nchunks;
    p.pf_chunk_bytes = np * 4096;                  // 64 filter rows x 32 k x 2 B per plane
    p.pf_tile_stride = next.nchunks * p.pf_chunk_bytes;
    p.pf_cap = kPrefetchCap;
}

}  // namespace bp
