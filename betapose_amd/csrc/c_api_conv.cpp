// extern "C" boundary, the single-layer convolution harness of the tests and bench tools (bp_conv2d*) and the
// experimental library's per-XCD launch prototype (bp_mega_*) -- see include/betapose_hip.h.
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "c_api_util.h"

extern "C" {

int bp_conv2d(const float* d_in, int N, int H, int W, int Cin, const float* h_w, const float* h_bias, int Cout, int k,
              int stride, int pad, int act, int store_mode, const float* d_res, int res_after_act, int tile, int splits,
              float* d_out, int iters, float* ms_per_iter, void* stream) {
    return bp_conv2d_planes(d_in, N, H, W, Cin, h_w, h_bias, Cout, k, stride, pad, act, store_mode, d_res, res_after_act, tile,
                            splits, d_out, nullptr, iters, ms_per_iter, stream);
}

int bp_conv2d_planes(const float* d_in, int N, int H, int W, int Cin, const float* h_w, const float* h_bias, int Cout, int k,
                     int stride, int pad, int act, int store_mode, const float* d_res, int res_after_act, int tile, int splits,
                     float* d_out, unsigned short* d_out_planes, int iters, float* ms_per_iter, void* stream) {
    return bp_conv2d_se(d_in, N, H, W, Cin, h_w, h_bias, Cout, k, stride, pad, act, store_mode, d_res, res_after_act, tile, splits,
                        d_out, d_out_planes, nullptr, nullptr, iters, ms_per_iter, stream);
}

int bp_conv2d_se(const float* d_in, int N, int H, int W, int Cin, const float* h_w, const float* h_bias, int Cout, int k,
                 int stride, int pad, int act, int store_mode, const float* d_res, int res_after_act, int tile, int splits,
                 float* d_out, unsigned short* d_out_planes, const float* d_res_scale, float* d_pool_out, int iters,
                 float* ms_per_iter, void* stream) {
    BP_TRY
    BP_CHECK(d_in && h_w && d_out, "null argument");
    BP_CHECK(!d_res_scale || d_res, "a residual scale needs a residual");
    hipStream_t s = (hipStream_t)stream;
    struct OneConv : bp::Net {
        OneConv() : Net(1) {}
        using Net::add_conv;
        using Net::finalize;
        using Net::ops_;
        using Net::partial_;
        using Net::partial_floats_;
        using Net::arena_;
    } net;
    const int OH = (H + 2 * pad - k) / stride + 1, OW = (W + 2 * pad - k) / stride + 1;
    bp::Tensor in; in.p = const_cast<float*>(d_in); in.H = H; in.W = W; in.C = Cin; in.ld = Cin;
    bp::Tensor out; out.p = d_out; out.H = OH; out.W = OW; out.C = Cout;
    out.ld = store_mode == bp::ST_PIXSHUF ? Cout / 4 : Cout;
    bp::Tensor res; res.p = const_cast<float*>(d_res); res.ld = Cout; res.C = Cout; res.H = OH; res.W = OW;
    bp::ConvWeights cw; cw.w = h_w; cw.bias = h_bias;
    net.add_conv("conv", in, out, cw, Cout, k, stride, pad, act, store_mode, d_res ? &res : nullptr, d_res_scale,
                 res_after_act, 1e-5f, OH, OW);
    int t = tile;
    int prec = bp::PREC_F32;
    if (t >= 256) {   // + 256: fp16-MFMA operands, + 512: bf16x3 split operands
        prec = t >= 512 ? bp::PREC_BF16X3 : bp::PREC_F16;
        t -= t >= 512 ? 512 : 256;
        BP_CHECK(Cin % 32 == 0, "layer is not eligible for the 16-bit MFMA paths (needs Cin % 32 == 0)");
        net.set_precision(prec);
        net.ops_[0].conv.mfma_mode = prec;
#ifndef BP_EXPERIMENTAL
        BP_CHECK(bp::conv_tile_is_pl(t) || ((t == bp::TILE_64x64_BD || t == bp::TILE_BD_K2 || bp::conv_tile_is_halo(t)) && prec == bp::PREC_BF16X3),
                 "this kernel id exists only in the experimental library (python -m betapose_amd.build --experimental, BP_LIB)");
#endif
    } else {
        if (t < 0 && bp::conv_stem3_eligible(net.ops_[0].conv)) t = bp::TILE_STEM3;      // as the engine plans it
        BP_CHECK(t <= bp::TILE_128x64 || (t == bp::TILE_STEM3 && bp::conv_stem3_eligible(net.ops_[0].conv)) || (t == bp::TILE_STEM7 && bp::conv_stem7_eligible(net.ops_[0].conv)),
                 "this tile needs a 16-bit precision mode (tile + 256 / + 512), or the layer is not a 3x3 / stride-1 / 4-channel-packed stem");
    }
    bp::ConvParams p = net.ops_[0].conv;
    p.N = N; p.M = N * OH * OW;
    if (t < 0) t = bp::TILE_64x64;
    // the SE average pool in this launch's epilogue (ConvParams::pool_out): under the engine's own precondition, or not at all
    if (d_pool_out) {
        BP_CHECK(bp::conv_pool_in_epilogue_ok(p, N, t), "the average pool cannot ride in this launch's epilogue (needs a 64x64 tile, a linear "
                 "residual-free NHWC layer, Cout % 4 == 0, and one image or OH * OW % 64 == 0)");
        p.pool_out = d_pool_out;
    }
    const int np = prec == bp::PREC_F16 ? 1 : 3;
    if (bp::conv_tile_is_pl(t)) {
        // the caller's activations are fp32: their operand planes are made here, as the layer's producer would have
        const long long in_elems = (long long)N * H * W * Cin;
        BP_CHECK(Cin % 32 == 0 && k * k <= 32, "layer is not eligible for the operand-plane kernels (needs Cin % 32 == 0, k*k <= 32)");
        unsigned short* d_in16 = (unsigned short*)net.arena_.alloc_bytes((size_t)np * in_elems * 2);
        bp::launch_f32_to_planes(d_in, Cin, (long long)N * H * W, Cin, d_in16, in_elems, np, s);
        p.in16 = d_in16; p.in16_plane = in_elems;
        auto& packed = np == 1 ? net.weight_store()->wpl1 : net.weight_store()->wpl3;
        auto it = packed.find(p.w);
        if (it == packed.end()) {
            unsigned short* d = (unsigned short*)net.weight_store()->arena.alloc_bytes((size_t)np * p.CoutPad * p.Kpad * 2);
            bp::launch_pack_wpl(p.w, d, p.CoutPad, p.Kpad, p.Cin, p.ksize, np, s);
            it = packed.emplace(p.w, d).first;
        }
        p.wpl = it->second;
        if (t == bp::TILE_PL64BD) {   // the filters-direct plane tile reads stage-packed fragments in the plane kernels' K order
            auto& staged = net.weight_store()->wbd3;
            auto ib = staged.find(p.w);
            if (ib == staged.end()) {
                unsigned short* d = (unsigned short*)net.weight_store()->arena.alloc_bytes((size_t)3 * p.CoutPad * p.Kpad * 2);
                bp::launch_f32_to_bf16x3_staged(p.w, d, p.CoutPad, p.Kpad, s, p.Cin);
                ib = staged.emplace(p.w, d).first;
            }
            p.wbd = ib->second;
        }
    }
    if (const char* e = std::getenv("BP_PL_ABL")) p.abl = std::atoi(e);   // (read by experimental builds only)
    if (d_out_planes) {   // the epilogue's operand planes of the output (any kernel): [np][the output tensor's elements]
        BP_CHECK(prec != bp::PREC_F32, "output planes need a 16-bit precision mode");
        long long out_elems = (long long)N * OH * OW * Cout;
        if (store_mode == bp::ST_UP2) out_elems *= 4;
        p.out16 = d_out_planes; p.out16_plane = out_elems; p.out_np = np;
    }
    // BP_CONV_F16R=1 (bench tools, tests/test_gpu_conv.py; read per call): the launch as the engine's 'f16r' plan makes it -- the skip
    // connection read from an fp16 plane of the residual tensor (ConvParams::res16) and, when output planes are asked for, the fp32 store
    // dropped (ConvParams::skip_f32)
    if (prec == bp::PREC_F16 && std::getenv("BP_CONV_F16R")) {
        if (p.res) {
            const long long n_res = (long long)N * OH * OW;
            unsigned short* r16 = (unsigned short*)net.arena_.alloc_bytes((size_t)n_res * p.res_ld * 2);
            if (Cout % 4 == 0) bp::launch_f32_to_planes(p.res, p.res_ld, n_res, Cout, r16, n_res * p.res_ld, 1, s);
            else {
                // Cout % 4 != 0 (the element-wise epilogue's layers): the converter moves four channels at a time, and the caller's residual is
                // dense (ld == Cout) -- the tensor as one run of quads, its last 1-3 elements rounded on the host (RNE, as the device does)
                const long long total = n_res * p.res_ld, quads = total / 4;
                if (quads > 0) bp::launch_f32_to_planes(p.res, 4, quads, 4, r16, total, 1, s);
                const int nt = (int)(total - 4 * quads);
                if (nt > 0) {
                    float tail32[3];
                    unsigned short tail16[3];
                    BP_HIP(hipStreamSynchronize(s));      // (the caller's residual is ordered on `s`; the copies below run on the null stream and are
                                                          // safe only because hipMemcpy returns when the copy is done -- before the launch on `s` is enqueued)
                    BP_HIP(hipMemcpy(tail32, p.res + 4 * quads, nt * sizeof(float), hipMemcpyDeviceToHost));
                    for (int i = 0; i < nt; ++i) { const _Float16 h = (_Float16)tail32[i]; std::memcpy(&tail16[i], &h, 2); }
                    BP_HIP(hipMemcpy(r16 + 4 * quads, tail16, nt * 2, hipMemcpyHostToDevice));
                }
            }
            p.res16 = r16;
        }
        if (p.out16) p.skip_f32 = 1;
    }
    // the launch set-up is the engine's (conv_plan.h): K cut, hybrid grid when the last round is badly filled, XCD-home layout
    const bp::ConvLaunch l = bp::conv_launch_of(p, t, splits);
    const int sp = l.splits, per = l.cps;
    p.splits = sp; p.chunks_per_split = per;
    if (sp > 1) {
        const int tiles = bp::conv_tiles(p, t);
        p.partial = net.arena_.alloc(bp::conv_slab_floats(t, sp, tiles));
        p.tickets = (int*)net.arena_.alloc_bytes((size_t)(2 + 64) * tiles * sizeof(int));
        BP_HIP(hipMemset(p.tickets, 0, (size_t)(2 + 64) * tiles * sizeof(int)));
    }
    bp::HybridTail h;
    if (sp == 1 && !p.pool_out && !std::getenv("BP_CONV_SELF_PREFETCH") && bp::conv_hybrid_plan(p, t, bp::conv_slab_floats(t, 8, 256), &h)) {   // (<= 8 slices of <= 256 tail tiles)
        p.partial = net.arena_.alloc(h.slab_floats);
        p.tickets = (int*)net.arena_.alloc_bytes((size_t)h.tiles * sizeof(int));
        BP_HIP(hipMemset(p.tickets, 0, (size_t)h.tiles * sizeof(int)));
        p.hy_full = h.full; p.hy_splits = h.splits; p.hy_cps = h.cps;
    }
    if (bp::conv_home_layout(t, sp)) {   // all K slices of a tile on one XCD, hand-off through that XCD's L2
        const int tiles = bp::conv_tiles(p, t);
        p.xcd_home = 1;
        p.tickets_local = p.tickets + tiles;
        p.xcc_of = p.tickets + 2 * tiles;
    }
    if (std::getenv("BP_CONV_SELF_PREFETCH")) bp::conv_prefetch_of(p, p, l);   // (tests: the launch carries prefetch blocks, for its own filters)
    bp::launch_conv(p, t, s);
    BP_HIP(hipStreamSynchronize(s));
    if (const char* e = std::getenv("BP_CONV_STAMPS")) {   // debug: per-block s_memtime marks of one extra launch
        const int nb = bp::conv_tiles(p, t) * p.splits;
        unsigned long long* d = (unsigned long long*)net.arena_.alloc_bytes((size_t)nb * 8 * 8);
        BP_HIP(hipMemset(d, 0, (size_t)nb * 64));
        bp::ConvParams q = p; q.stamps = d;
        bp::launch_conv(q, t, s);
        BP_HIP(hipStreamSynchronize(s));
        std::vector<unsigned long long> h((size_t)nb * 8);
        BP_HIP(hipMemcpy(h.data(), d, h.size() * 8, hipMemcpyDeviceToHost));
        unsigned long long t0 = ~0ull;
        for (int b = 0; b < nb; ++b)
            if (h[(size_t)b * 8]) t0 = std::min(t0, h[(size_t)b * 8]);
        double acc[8] = {0, 0, 0, 0, 0, 0, 0, 0}, last = 0;
        int cnt[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        for (int b = 0; b < nb; ++b)
            for (int k = 0; k < 8; ++k) {
                const unsigned long long v = h[(size_t)b * 8 + k];
                if (!v) continue;
                acc[k] += (double)(v - h[(size_t)b * 8]); ++cnt[k];      // relative to the block's own entry
                last = std::max(last, (double)(v - t0));
            }
        auto mean = [&](int k) { return cnt[k] ? acc[k] / cnt[k] : 0.0; };
        if (std::getenv("BP_W64_ABLATE") && (std::atoi(std::getenv("BP_W64_ABLATE")) & 64)) {
            double sum[4] = {0, 0, 0, 0};
            for (int b = 0; b < nb; ++b) for (int k = 0; k < 4; ++k) sum[k] += (double)h[(size_t)b * 8 + 4 + k];
            const double stages = 2.0 * p.chunks_per_split * nb;
            std::fprintf(stderr, "[stage timing] cycles per stage: issue slots 0..UPW %.0f | slots ..SYNC %.0f | wait+barrier %.0f | SYNC..end %.0f\n",
                         sum[0] / stages, sum[1] / stages, sum[2] / stages, sum[3] / stages);
        }
        std::fprintf(stderr, "[stamps] blocks=%d  mean 10-ns ticks (s_memrealtime, 100 MHz) since the block's entry: index math done %.0f | chunk 0 in LDS %.0f | "
                     "K loop done %.0f | in-block sums (conv_kg) or cycles parked at the stage waits (conv_pl) %.0f | slab parked + ticket %.0f (%d blocks) | slices combined %.0f (%d) | stores done %.0f (%d) | "
                     "last mark of the grid %.0f after the first entry\n", nb, mean(1), mean(2), mean(3), mean(7), mean(5), cnt[5], mean(6),
                     cnt[6], mean(4), cnt[4], last);
    }
    if (iters > 0 && ms_per_iter) {
        hipEvent_t e0, e1;
        BP_HIP(hipEventCreate(&e0));
        BP_HIP(hipEventCreate(&e1));
        BP_HIP(hipEventRecord(e0, s));
        for (int i = 0; i < iters; ++i) bp::launch_conv(p, t, s);
        BP_HIP(hipEventRecord(e1, s));
        BP_HIP(hipEventSynchronize(e1));
        float ms = 0;
        BP_HIP(hipEventElapsedTime(&ms, e0, e1));
        *ms_per_iter = ms / iters;
        (void)hipEventDestroy(e0);
        (void)hipEventDestroy(e1);
    }
    return 0;
    BP_CATCH
}

// ------------------------------------------------------------------ the SE blocks' and the DUC layers' auxiliary kernels, one launch each (tests)
int bp_avgpool(const float* d_in, int in_ld, int N, int HW, int C, float* d_out, int* parts, void* stream) {
    BP_TRY
    BP_CHECK(N >= 1 && HW >= 1 && C >= 1 && in_ld >= C, "bad argument");
    if (parts) *parts = bp::avgpool_parts(HW);
    if (!d_out) return 0;          // (the slice count alone: the caller sizes d_out [N][parts][C] with it)
    BP_CHECK(d_in, "null argument");
    bp::launch_avgpool(d_in, in_ld, d_out, N, HW, C, (hipStream_t)stream);
    BP_HIP(hipGetLastError());
    BP_HIP(hipStreamSynchronize((hipStream_t)stream));
    return 0;
    BP_CATCH
}

int bp_fc(const float* d_in, const float* h_w, const float* h_bias, int N, int Cin, int Cout, int act, int in_parts, float in_scale,
          float* d_out, void* stream) {
    BP_TRY
    BP_CHECK(d_in && h_w && d_out && N >= 1 && Cin >= 4 && Cout >= 1 && in_parts >= 1, "bad argument");
    BP_CHECK(act == 0 || act == 2 || act == 3, "fc: act 0 linear / 2 relu / 3 sigmoid");
    hipStream_t s = (hipStream_t)stream;
    struct DevBuf {
        float* p = nullptr;
        ~DevBuf() { if (p) (void)hipFree(p); }
    } w, b;
    BP_HIP(hipMalloc((void**)&w.p, (size_t)Cout * Cin * sizeof(float)));
    BP_HIP(hipMalloc((void**)&b.p, (size_t)Cout * sizeof(float)));
    BP_HIP(hipMemcpy(w.p, h_w, (size_t)Cout * Cin * sizeof(float), hipMemcpyHostToDevice));
    if (h_bias) BP_HIP(hipMemcpy(b.p, h_bias, (size_t)Cout * sizeof(float), hipMemcpyHostToDevice));
    else BP_HIP(hipMemset(b.p, 0, (size_t)Cout * sizeof(float)));
    bp::launch_fc(d_in, w.p, b.p, d_out, N, Cin, Cout, act, in_parts, in_scale, s);
    BP_HIP(hipGetLastError());
    BP_HIP(hipStreamSynchronize(s));
    return 0;
    BP_CATCH
}

int bp_maxpool3s2p1(const float* d_in, int N, int H, int W, int C, float* d_out, unsigned short* d_out_planes, int np, void* stream) {
    BP_TRY
    BP_CHECK(d_in && d_out && N >= 1 && H >= 1 && W >= 1 && C >= 4, "bad argument");
    BP_CHECK(d_out_planes ? (np == 1 || np == 3) : np == 0, "output planes: np 1 (fp16) or 3 (bf16x3) with a plane buffer, 0 without");
    const int OH = (H - 1) / 2 + 1, OW = (W - 1) / 2 + 1;      // as the engine sizes the layer
    bp::launch_maxpool3s2p1(d_in, d_out, N, H, W, C, OH, OW, (hipStream_t)stream, d_out_planes, (long long)N * OH * OW * C, np);
    BP_HIP(hipGetLastError());
    BP_HIP(hipStreamSynchronize((hipStream_t)stream));
    return 0;
    BP_CATCH
}

int bp_pixel_shuffle2(const float* d_in, int N, int H, int W, int C, float* d_out, unsigned short* d_out_planes, int np, void* stream) {
    BP_TRY
    BP_CHECK(d_in && d_out && N >= 1 && H >= 1 && W >= 1 && C >= 4 && C % 4 == 0, "bad argument");
    BP_CHECK(d_out_planes ? (np == 1 || np == 3) : np == 0, "output planes: np 1 (fp16) or 3 (bf16x3) with a plane buffer, 0 without");
    bp::launch_pixel_shuffle2(d_in, d_out, N, H, W, C, (hipStream_t)stream, d_out_planes, (long long)N * H * W * C, np);
    BP_HIP(hipGetLastError());
    BP_HIP(hipStreamSynchronize((hipStream_t)stream));
    return 0;
    BP_CATCH
}

// ------------------------------------------------------------------ xcd mode (mega.inc): prototype entry point, experimental library only
#ifdef BP_EXPERIMENTAL
// The convolution launch lists of up to eight detector engines (clones: own activations, shared filters), one per XCD, in ONE
// persistent launch; `iters` launches timed with events.  The engines' inputs must already be in place (a forward pass of the
// ordinary path leaves them there); afterwards every engine's activations hold what its own launches would have produced.
int bp_mega_yolo_convs_stamped(bp_yolo** ys, int n, int blocks_per_xcd, int iters, float* ms_per_launch, unsigned* err_word,
                               float* op_us, int* op_info, int cap, void* stream);
int bp_mega_yolo_convs(bp_yolo** ys, int n, int blocks_per_xcd, int iters, float* ms_per_launch, unsigned* err_word, void* stream) {
    return bp_mega_yolo_convs_stamped(ys, n, blocks_per_xcd, iters, ms_per_launch, err_word, nullptr, nullptr, 0, stream);
}
// ... with per-op marks of XCD 0's launch list: op_us[i] = duration of op i incl. its barrier, op_info[3 i] = {type, items, K slices}
int bp_mega_yolo_convs_stamped(bp_yolo** ys, int n, int blocks_per_xcd, int iters, float* ms_per_launch, unsigned* err_word,
                               float* op_us, int* op_info, int cap, void* stream) {
    BP_TRY
    BP_CHECK(ys && n >= 1 && n <= 8 && blocks_per_xcd >= 1 && blocks_per_xcd <= 256 && iters >= 1, "bad argument");
    hipStream_t s = (hipStream_t)stream;
    BP_HIP(hipSetDevice(ys[0]->device));
    bp::MegaArgs a{};
    std::vector<void*> dev;
    size_t lds = 0;
    for (int k = 0; k < n; ++k) {
        std::vector<bp::MegaOp> ops;
        ys[k]->net->emit_conv_ops(1, ops);
        if (const char* e = std::getenv("BP_MEGA_EXP")) {          // prototype experiments: 1 = barriers only (no work items), 2 = without the RGB stem
            const int m = std::atoi(e);
            for (bp::MegaOp& o : ops) {
                if (m == 1) o.items = 0;
                if (m == 2 && o.type == bp::MO_STEM3) o.items = 0;
            }
        }
        for (const bp::MegaOp& o : ops) lds = std::max(lds, bp::mega_lds_bytes(o));
        void* d = nullptr;
        BP_HIP(hipMalloc(&d, ops.size() * sizeof(bp::MegaOp)));
        dev.push_back(d);
        BP_HIP(hipMemcpy(d, ops.data(), ops.size() * sizeof(bp::MegaOp), hipMemcpyHostToDevice));
        a.prog[k] = (const bp::MegaOp*)d;
        a.n_ops[k] = (int)ops.size();
    }
    unsigned* sync = nullptr;
    BP_HIP(hipMalloc((void**)&sync, 129 * sizeof(unsigned)));
    dev.push_back(sync);
    a.sync = sync;
    a.nb = blocks_per_xcd;
    unsigned long long* d_st = nullptr;
    if (op_us) {
        BP_HIP(hipMalloc((void**)&d_st, 8 * 512 * sizeof(unsigned long long)));
        BP_HIP(hipMemset(d_st, 0, 8 * 512 * sizeof(unsigned long long)));
        dev.push_back(d_st);
        a.stamps = d_st;
    }
    hipEvent_t e0, e1;
    BP_HIP(hipEventCreate(&e0));
    BP_HIP(hipEventCreate(&e1));
    bp::launch_mega(a, lds, s);                 // warm
    BP_HIP(hipStreamSynchronize(s));
    BP_HIP(hipEventRecord(e0, s));
    for (int i = 0; i < iters; ++i) bp::launch_mega(a, lds, s);
    BP_HIP(hipEventRecord(e1, s));
    BP_HIP(hipEventSynchronize(e1));
    float ms = 0;
    BP_HIP(hipEventElapsedTime(&ms, e0, e1));
    if (ms_per_launch) *ms_per_launch = ms / iters;
    unsigned err = 0;
    BP_HIP(hipMemcpy(&err, sync + 128, sizeof(unsigned), hipMemcpyDeviceToHost));
    if (err_word) *err_word = err;
    if (op_us) {
        std::vector<unsigned long long> h(512);
        BP_HIP(hipMemcpy(h.data(), d_st, 512 * sizeof(unsigned long long), hipMemcpyDeviceToHost));
        std::vector<bp::MegaOp> ops;
        ys[0]->net->emit_conv_ops(1, ops);
        for (int i = 0; i < (int)ops.size() && i < cap; ++i) {
            op_us[i] = (float)((double)(h[i + 1] - h[i]) / 100.0);         // 100 MHz reference clock
            if (op_info) { op_info[3 * i] = ops[i].type; op_info[3 * i + 1] = ops[i].items; op_info[3 * i + 2] = ops[i].conv.splits; }
        }
    }
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    for (void* d : dev) (void)hipFree(d);
    return 0;
    BP_CATCH
}
#endif

}  // extern "C"
