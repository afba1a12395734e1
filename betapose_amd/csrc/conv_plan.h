// The convolution planner (conv_plan.cpp): which kernel runs a layer, with how many K slices, and the launch layouts that follow.
#pragma once
#include "bp_common.h"

namespace bp {

struct Op;   // engine.h

struct ConvLaunch { int tile = TILE_64x64, splits = 1, cps = 0; };   // kernel id, K slices, chunks per slice

// what a caller may set (bp_*_set_policy, set_prefetch): a forced kernel id (-1: none), the split-K fill rule -- slices until the grid has
// sk_target blocks, at least sk_min_chunks chunks per slice, at most sk_max slices; {512, 4, 8} is the default policy, which reads the
// measured tables -- and the lone-frame latency mode
struct PlanPolicy { int force_tile = -1, sk_target = 512, sk_min_chunks = 4, sk_max = 8; bool lone = false; };

// the launch of convolution `op` at `batch` frames under `pol`, from the layer's shape and its ConvParams as set_precision left them
ConvLaunch plan_conv(const Op& op, int batch, const PlanPolicy& pol);
// the launch of `tile` with `want` K slices (<= 0: nobody planned it -- the default fill rule, up to the workspace's 64 slices): a
// persistent grid takes no slices, every other tile cuts K its own way (conv_split_plan)
ConvLaunch conv_launch_of(const ConvParams& p, int tile, int want);
// split-K slabs of a launch: one bm x bn tile of fp32 sums per (slice, tile)
inline size_t conv_slab_floats(int tile, int slices, int tiles) { return (size_t)slices * tiles * conv_tile_bm(tile) * conv_tile_bn(tile); }

// hybrid grid of a one-slice conv_pl launch (ConvParams::hy_*): `full` tiles run whole, the `tiles` after them in `splits` slices of `cps`
// chunks, which takes slab_floats of workspace and one arrival counter per tail tile
struct HybridTail { int full = 0, splits = 0, cps = 0, tiles = 0; size_t slab_floats = 0; };
bool conv_hybrid_plan(const ConvParams& p, int tile, size_t partial_floats, HybridTail* h);
bool conv_home_layout(int tile, int splits);   // the launch keeps all K slices of a tile on one XCD
// the SE average pool can ride in this launch's epilogue (ConvParams::pool_out): a 64x64 tile with the staged vector epilogue of a linear,
// residual-free NHWC layer, whose 64-row slabs never span two images of the batch
bool conv_pool_in_epilogue_ok(const ConvParams& c, int batch, int tile);
// p's launch carries the prefetch blocks for the filters of `next`, which runs as `nl`
void conv_prefetch_of(ConvParams& p, const ConvParams& next, const ConvLaunch& nl);

}  // namespace bp
