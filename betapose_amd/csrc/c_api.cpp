// extern "C" boundary of libbetapose_hip.so -- see include/betapose_hip.h.  This unit: version, devices, streams, the
// engines, the stand-alone stage ops and the per-frame device chains.  The other subsystems' entry points are
// c_api_conv.cpp (the single-layer convolution harness), c_api_pose.cpp (pose solvers), c_api_eval.cpp (evaluation tools)
// and c_api_io.cpp (frame input).
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <sstream>
#include <vector>

#include "c_api_util.h"
#include "frame_chain.h"

// bp_last_error()'s text: the one such string of the library (c_api_util.h)
static thread_local std::string g_err;
void bp::set_last_error(const char* text) { g_err = text; }

// The per-frame device chains.  What they share -- the frame's graph, the latency mode's re-run, the resize stage and the
// pose solver -- is frame_chain.h; `engines` lists the detector, then the key-point engine(s).
struct bp_pipeline {
    bp_yolo* y;
    bp_kpd* k;
    int H, W, batch;
    float conf;
    int num_classes;
    bp::Arena arena;
    bp::ResizeStage resize;
    float* results = nullptr;    // [batch][316] = sel[8] | pts[8] | kp[50][6], each written by its producer
    float* hm = nullptr;
    float* fixed_box = nullptr;  // [batch][4] or null
    bool use_fixed = false;
    bp::EngineList engines;
    bp::FrameGraph graph;
    int latency_faults = 0;          // frames re-run because the latency mode's placement check failed (bp_pipeline_latency_faults)
    bp::PoseSolver pose;             // bp_pipeline_set_pose_solver / _ransac: rows [batch][166]
    double* own_poses = nullptr;
};

// One shared multi-class detector pass per frame feeding K objects' pose chains (bp_scene_*): slot k = class_ids[k], its
// key-point engine (engines[1 + k]), result row k and (opt-in) its pose tail.
struct bp_scene_slot {
    bp_kpd* k = nullptr;
    bp::PoseSolver pose;
};
struct bp_scene {
    bp_yolo* y;
    std::vector<bp_scene_slot> slots;
    std::vector<int> class_ids;
    int H, W;
    float conf;
    int num_classes;
    bp::Arena arena;
    bp::ResizeStage resize;
    float* results = nullptr;    // [K][316], row k = slot k's record
    double* own_poses = nullptr; // [K][166], rows of the slots whose solver was set without a buffer
    bp::EngineList engines;
    bp::FrameGraph graph;
    int latency_faults = 0;
};

// Candidate boxes per frame (bp_cands_*): one frame, up to C NMS survivors of the detector through ONE key-point pass at
// batch C; rows [C][316], their number in counts[0]; (opt-in) the candidate pose tail over them.
struct bp_cands {
    bp_yolo* y;
    bp_kpd* k;
    int C, H, W;
    float conf, nms_conf;
    int num_classes, class_id;
    bp::Arena arena;
    bp::ResizeStage resize;
    float* results = nullptr;    // [C][316]
    int* counts = nullptr;       // [1]
    bp::EngineList engines;
    bp::FrameGraph graph;
    int latency_faults = 0;
    bp::PoseSolver pose;         // the candidate tail: row [166]; its RANSAC part stays unused
    double* own_pose = nullptr;
    float* merged = nullptr;     // [C][152]
    int* info = nullptr;         // [4]
    bool inst_on = false;
    double* inst = nullptr;      // [C][166]: a pose per merged candidate (opt-in)
    double* own_inst = nullptr;
};

static std::string read_text(const char* path) {
    std::ifstream f(path);
    if (!f) throw bp::Error(std::string("cannot open ") + path);
    std::stringstream ss;
    ss << f.rdbuf();
    return ss.str();
}

// Built-in default of newly created engines: bf16x3 = fp32-accurate convolution on the bf16 matrix pipe (exact 3-way
// operand split, passes the whole parity suite at the fp32 bars).  BP_PRECISION=f32|bf16x3|f16|f16r overrides
// it (bp_*_set_precision still wins).
static int default_precision() {
    const char* e = std::getenv("BP_PRECISION");
    if (!e || !*e) return bp::PREC_BF16X3;
    const std::string v(e);
    if (v == "f32") return bp::PREC_F32;
    if (v == "f16") return bp::PREC_F16;
    if (v == "f16r") return bp::PREC_F16_RES;
    if (v == "bf16x3") return bp::PREC_BF16X3;
    throw bp::Error("BP_PRECISION must be f32, bf16x3, f16 or f16r, not '" + v + "'");
}

// ------------------------------------------------------------------ what bp_yolo_* and bp_kpd_* do alike
// One body per operation over either handle type E; the exports forward to it.  with_net runs f(net) and turns an exception
// into -1 and bp_last_error(); a null handle is answered here, before any device call: -1 and "null argument".
template <class E, class F> static int with_net(const E* e, F f) {
    BP_TRY
    if (!e) throw bp::Error("null argument");
    return f(*e->net);
    BP_CATCH
}

// A new handle around the net `make` builds on `device`: a creator's net takes the default precision, a clone the
// precision and fusion flag of `like`.
template <class E, class Make> static void adopt(E** out, int device, const bp::Net* like, Make make) {
    BP_HIP(hipSetDevice(device));
    std::unique_ptr<E> e(new E);
    e->device = device;
    e->net.reset(make());
    const int prec = like ? like->precision_id() : default_precision();
    if (prec != bp::PREC_F32) e->net->set_precision(prec);
    if (like) e->net->set_fusion(like->fusion());
    *out = e.release();
}

template <class E> static int engine_clone(const E* e, E** out) {
    return with_net(e, [&](const bp::Net& src) {
        BP_CHECK(out, "null argument");
        adopt(out, e->device, &src, [&] { return e->net->clone(); });
        return 0;
    });
}
template <class E> static int engine_tap_count(const E* e) {
    return with_net(e, [](const bp::Net& n) { return n.tap_count(); });
}
template <class E> static int engine_tap_info(const E* e, int i, char* name, int cap, int* C, int* H, int* W) {
    return with_net(e, [&](const bp::Net& n) {
        if (!C || !H || !W) throw bp::Error("null argument");
        if (i < 0 || i >= n.tap_count()) throw bp::Error("tap index");
        if (name && cap > 0) std::snprintf(name, cap, "%s", n.tap_name(i));
        n.tap_shape(i, C, H, W);
        return 0;
    });
}
template <class E> static int engine_tap_copy(E* e, int i, int batch, float* d_out, void* stream) {
    return with_net(e, [&](bp::Net& n) {
        BP_CHECK(d_out, "null argument");
        n.tap_copy(i, batch, d_out, (hipStream_t)stream);
        return 0;
    });
}
template <class E> static int engine_set_policy(E* e, int t, int mc, int ms, int ft) {
    return with_net(e, [&](bp::Net& n) {
        BP_CHECK(t >= 1 && mc >= 1 && ms >= 1 && ft >= -1 && ft <= bp::TILE_LAST, "policy values out of range");
        n.set_splitk_policy(t, mc);
        n.set_max_splits(ms);
        n.set_force_tile(ft);
        return 0;
    });
}
template <class E> static int engine_set_precision(E* e, int prec) {
    return with_net(e, [&](bp::Net& n) {
        BP_HIP(hipSetDevice(e->device));
        n.set_precision(prec);
        return 0;
    });
}
template <class E> static int engine_op_stats(const E* e, double* flops, double* bytes, int cap) {
    return with_net(e, [&](const bp::Net& n) {
        const auto& ops = n.ops();
        for (int i = 0; i < (int)ops.size() && i < cap; ++i) {
            if (flops) flops[i] = ops[i].flops;
            if (bytes) bytes[i] = ops[i].bytes;
        }
        return (int)ops.size();
    });
}
template <class E> static int engine_profile(E* e, int batch, int iters, float* ms, int* info, int cap, void* stream) {
    return with_net(e, [&](bp::Net& n) { return n.profile(batch, iters, ms, info, cap, (hipStream_t)stream); });
}
template <class E> static int engine_set_prefetch(E* e, int on) {
    return with_net(e, [&](bp::Net& n) { n.set_prefetch(on != 0); return 0; });
}
// conv -> conv fusion of residual / bottleneck blocks (conv_fused.hip): on by default
template <class E> static int engine_set_fusion(E* e, int on) {
    return with_net(e, [&](bp::Net& n) { n.set_fusion(on != 0); return 0; });
}
// *launches = fused groups that run as ONE launch at `batch`
template <class E> static int engine_fused_launches(E* e, int batch, int* launches) {
    return with_net(e, [&](bp::Net& n) {
        BP_CHECK(launches && batch >= 1 && batch <= n.max_batch(), "arguments");
        BP_HIP(hipSetDevice(e->device));
        *launches = n.fused_launches(batch);
        return 0;
    });
}
template <class E> static int engine_xcd_errors(E* e, int* count, void* stream) {
    return with_net(e, [&](bp::Net& n) {
        BP_CHECK(count, "null argument");
        BP_HIP(hipSetDevice(e->device));
        *count = n.take_xcd_errors((hipStream_t)stream);
        return 0;
    });
}
template <class E> static int engine_set_stamps(E* e, unsigned long long* d_buf, int slots) {
    return with_net(e, [&](bp::Net& n) { n.set_stamps(d_buf, slots); return 0; });
}
template <class E> static int engine_op_name(const E* e, int i, char* out, int cap) {
    return with_net(e, [&](const bp::Net& net) {
        if (i < 0 || i >= (int)net.ops().size() || !out || cap <= 0) return -1;
        const bp::Op& op = net.ops()[i];
        if (op.type == bp::OP_CONV)   // "<name> k<ksize> <OH>x<OW> <Cin>-><Cout> s<stride>"
            std::snprintf(out, (size_t)cap, "%s k%d %dx%d %d->%d s%d", net.op_name(i), op.conv.ksize, op.conv.OH, op.conv.OW,
                          op.conv.Cin, op.conv.Cout, op.conv.stride);
        else
            std::snprintf(out, (size_t)cap, "%s", net.op_name(i));
        return op.type == bp::OP_CONV ? 1 : 0;
    });
}
template <class E> static size_t engine_device_bytes(const E* e) { return e ? e->net->device_bytes() : 0; }

extern "C" {

const char* bp_last_error(void) { return g_err.c_str(); }
int bp_version(void) { return 100; }

int bp_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}
int bp_device_name(int device, char* out, int cap) {
    BP_TRY
    hipDeviceProp_t p;
    BP_HIP(hipGetDeviceProperties(&p, device));
    std::snprintf(out, cap, "%s (%s)", p.name, p.gcnArchName);
    return 0;
    BP_CATCH
}

// ------------------------------------------------------------------ streams bound to a CU subset
int bp_stream_create_masked(const uint32_t* cu_mask, int words, void** out) {
    BP_TRY
    BP_CHECK(cu_mask && words > 0 && out, "null argument");
    hipStream_t s = nullptr;
    BP_HIP(hipExtStreamCreateWithCUMask(&s, (uint32_t)words, cu_mask));
    *out = (void*)s;
    return 0;
    BP_CATCH
}

int bp_stream_destroy(void* stream) {
    BP_TRY
    BP_HIP(hipStreamDestroy((hipStream_t)stream));
    return 0;
    BP_CATCH
}

int bp_probe_placement(int blocks, int* h_xcc, int* h_hw_id, void* stream) {
    BP_TRY
    BP_CHECK(blocks > 0 && h_xcc, "bad argument");
    int* d = nullptr;
    BP_HIP(hipMalloc(&d, (size_t)blocks * 2 * sizeof(int)));
    bp::launch_probe_placement(d, blocks, (hipStream_t)stream);
    std::vector<int> h((size_t)blocks * 2);
    hipError_t e = hipMemcpyAsync(h.data(), d, h.size() * sizeof(int), hipMemcpyDeviceToHost, (hipStream_t)stream);
    if (e == hipSuccess) e = hipStreamSynchronize((hipStream_t)stream);
    (void)hipFree(d);
    BP_HIP(e);
    for (int i = 0; i < blocks; ++i) {
        h_xcc[i] = h[2 * i];
        if (h_hw_id) h_hw_id[i] = h[2 * i + 1];
    }
    return 0;
    BP_CATCH
}

// ------------------------------------------------------------------ detector
int bp_yolo_create_from_memory(const char* cfg_text, const float* stream, size_t n_floats, int reso, int max_batch,
                               int device, bp_yolo** out) {
    BP_TRY
    BP_CHECK(cfg_text && stream && out, "null argument");
    adopt(out, device, nullptr, [&] { return new bp::YoloNet(cfg_text, stream, n_floats, reso, max_batch); });
    return 0;
    BP_CATCH
}

static std::vector<float> read_weights_file(const char* weights_path) {
    std::ifstream f(weights_path, std::ios::binary);
    if (!f) throw bp::Error(std::string("cannot open ") + weights_path);
    f.seekg(0, std::ios::end);
    const size_t bytes = (size_t)f.tellg();
    f.seekg(0);
    BP_CHECK(bytes >= 16, "truncated .weights header");
    int32_t hdr[3];
    f.read(reinterpret_cast<char*>(hdr), 12);
    // parser.c:1161-1174: major*10+minor >= 2 -> 64-bit "seen", else 32-bit
    const size_t off = (hdr[0] * 10 + hdr[1] >= 2) ? 20 : 16;
    BP_CHECK(bytes >= off && (bytes - off) % 4 == 0, "malformed .weights payload");
    std::vector<float> stream((bytes - off) / 4);
    f.seekg(off);
    f.read(reinterpret_cast<char*>(stream.data()), bytes - off);
    return stream;
}

int bp_yolo_create(const char* cfg_path, const char* weights_path, int reso, int max_batch, int device, bp_yolo** out) {
    BP_TRY
    BP_CHECK(cfg_path && weights_path && out, "null argument");
    const std::string cfg = read_text(cfg_path);
    const std::vector<float> stream = read_weights_file(weights_path);
    return bp_yolo_create_from_memory(cfg.c_str(), stream.data(), stream.size(), reso, max_batch, device, out);
    BP_CATCH
}

int bp_yolo_create_darknet(const char* cfg_path, const char* weights_path, int reso, int max_batch, int device,
                           bp_yolo** out) {
    BP_TRY
    BP_CHECK(cfg_path && weights_path && out, "null argument");
    const std::string cfg = read_text(cfg_path);
    const std::vector<float> stream = read_weights_file(weights_path);
    adopt(out, device, nullptr,
          [&] { return new bp::YoloNet(cfg, stream.data(), stream.size(), reso, max_batch, nullptr, /*darknet_bn=*/true); });
    return 0;
    BP_CATCH
}

int bp_yolo_clone(const bp_yolo* y, bp_yolo** out) { return engine_clone(y, out); }
void bp_yolo_destroy(bp_yolo* y) { delete y; }
int bp_yolo_rows(const bp_yolo* y) { return y ? y->net->rows() : -1; }
int bp_yolo_attrs(const bp_yolo* y) { return y ? y->net->attrs() : -1; }

int bp_yolo_forward(bp_yolo* y, const float* d_img, int batch, float* d_pred, void* stream) {
    BP_TRY
    BP_CHECK(y && d_img && d_pred, "null argument");
    y->net->forward(d_img, false, batch, d_pred, 0.f, 0, nullptr, (hipStream_t)stream);
    return 0;
    BP_CATCH
}
int bp_yolo_forward_select(bp_yolo* y, const float* d_img, int batch, float conf, int num_classes, float* d_pred,
                           float* d_sel, void* stream) {
    BP_TRY
    BP_CHECK(y && d_img && d_sel, "null argument");
    y->net->forward(d_img, false, batch, d_pred, conf, num_classes, d_sel, (hipStream_t)stream);
    return 0;
    BP_CATCH
}

int bp_yolo_forward_select_classes(bp_yolo* y, const float* d_img, int batch, float conf, int num_classes, const int* class_ids,
                                   int K, float* d_pred, float* d_sel, void* stream) {
    BP_TRY
    BP_CHECK(K >= 1 && K <= BP_MAX_SCENE_CLASSES, "class list: 1 to 16 class ids (BP_MAX_SCENE_CLASSES)");
    BP_CHECK(y && d_img && class_ids && d_sel, "null argument");
    y->net->forward_classes(d_img, false, batch, d_pred, conf, num_classes, class_ids, K, d_sel, (hipStream_t)stream);
    return 0;
    BP_CATCH
}

int bp_yolo_select(const float* d_pred, int batch, int rows, int attrs, float conf, int num_classes, float* d_sel,
                   void* stream) {
    BP_TRY
    BP_CHECK(d_pred && d_sel && batch >= 1 && rows >= 1 && attrs >= 6, "bad argument");
    bp::launch_yolo_select(bp::YoloRowSource::tensor(d_pred, rows, attrs), batch, conf, num_classes, d_sel, (hipStream_t)stream);
    BP_HIP(hipGetLastError());
    return 0;
    BP_CATCH
}

int bp_yolo_select_nms(const float* d_pred, int batch, int rows, int attrs, float conf, int num_classes, int class_id,
                       float nms_conf, int max_candidates, float* d_sel, int* d_counts, void* stream) {
    BP_TRY
    BP_CHECK(d_pred && d_sel && d_counts && batch >= 1 && rows >= 1 && attrs >= 6, "bad argument");
    bp::launch_yolo_select_nms(bp::YoloRowSource::tensor(d_pred, rows, attrs), batch, conf, num_classes, class_id, nms_conf, max_candidates,
                               d_sel, d_counts, (hipStream_t)stream, max_candidates * BP_SEL_FLOATS, BP_SEL_FLOATS);
    BP_HIP(hipGetLastError());
    return 0;
    BP_CATCH
}

int bp_yolo_forward_select_nms(bp_yolo* y, const float* d_img, int batch, float conf, int num_classes, int class_id,
                               float nms_conf, int max_candidates, float* d_pred, float* d_sel, int* d_counts, void* stream) {
    BP_TRY
    BP_CHECK(y && d_img && d_sel && d_counts, "null argument");
    y->net->forward_nms(d_img, false, batch, d_pred, conf, num_classes, class_id, nms_conf, max_candidates, d_sel, d_counts,
                        (hipStream_t)stream);
    return 0;
    BP_CATCH
}

int bp_yolo_tap_count(const bp_yolo* y) { return engine_tap_count(y); }
int bp_yolo_tap_info(const bp_yolo* y, int i, char* name, int cap, int* C, int* H, int* W) {
    return engine_tap_info(y, i, name, cap, C, H, W);
}
int bp_yolo_tap_copy(bp_yolo* y, int i, int batch, float* d_out, void* stream) {
    return engine_tap_copy(y, i, batch, d_out, stream);
}

// ------------------------------------------------------------------ key-point detector
int bp_kpd_create(const float* stream, size_t n_floats, int n_classes, int max_batch, int device, bp_kpd** out) {
    BP_TRY
    BP_CHECK(stream && out, "null argument");
    adopt(out, device, nullptr, [&] { return new bp::KpdNet(stream, n_floats, n_classes, max_batch); });
    return 0;
    BP_CATCH
}
int bp_kpd_clone(const bp_kpd* k, bp_kpd** out) { return engine_clone(k, out); }
void bp_kpd_destroy(bp_kpd* k) { delete k; }
int bp_kpd_forward(bp_kpd* k, const float* d_inps, int batch, float* d_hm, void* stream) {
    BP_TRY
    BP_CHECK(k && d_inps && d_hm, "null argument");
    k->net->forward(d_inps, false, batch, d_hm, nullptr, (hipStream_t)stream);
    return 0;
    BP_CATCH
}
int bp_kpd_forward_argmax(bp_kpd* k, const float* d_inps, int batch, float* d_hm, float* d_kp, void* stream) {
    BP_TRY
    BP_CHECK(k && d_inps && d_kp, "null argument");
    k->net->forward(d_inps, false, batch, d_hm, d_kp, (hipStream_t)stream);
    return 0;
    BP_CATCH
}
int bp_kpd_launch_count(bp_kpd* k, int batch) {
    BP_TRY
    BP_CHECK(k, "null argument");
    BP_CHECK(batch >= 1 && batch <= k->net->max_batch(), "batch out of range");
    BP_HIP(hipSetDevice(k->device));
    // record one forward + arg-max pass at this batch into a throw-away graph (nothing executes) and count its nodes
    hipStream_t cs = nullptr;
    BP_HIP(hipStreamCreateWithFlags(&cs, hipStreamNonBlocking));
    hipGraph_t g = nullptr;
    size_t n = 0;
    hipError_t e = hipStreamBeginCapture(cs, hipStreamCaptureModeThreadLocal);
    if (e == hipSuccess) {
        float* kp = k->net->input_nhwc();   // never written: the launches are only recorded
        try {
            k->net->forward(k->net->input_nhwc(), true, batch, nullptr, kp, cs);
        } catch (...) {
            (void)hipStreamEndCapture(cs, &g);
            if (g) (void)hipGraphDestroy(g);
            (void)hipStreamDestroy(cs);
            throw;
        }
        e = hipStreamEndCapture(cs, &g);
    }
    if (e == hipSuccess) e = hipGraphGetNodes(g, nullptr, &n);
    if (g) (void)hipGraphDestroy(g);
    (void)hipStreamDestroy(cs);
    BP_HIP(e);
    return (int)n;
    BP_CATCH
}
int bp_kpd_tap_count(const bp_kpd* k) { return engine_tap_count(k); }
int bp_kpd_tap_info(const bp_kpd* k, int i, char* name, int cap, int* C, int* H, int* W) {
    return engine_tap_info(k, i, name, cap, C, H, W);
}
int bp_kpd_tap_copy(bp_kpd* k, int i, int batch, float* d_out, void* stream) {
    return engine_tap_copy(k, i, batch, d_out, stream);
}

int bp_yolo_set_policy(bp_yolo* y, int t, int mc, int ms, int ft) { return engine_set_policy(y, t, mc, ms, ft); }
int bp_kpd_set_policy(bp_kpd* k, int t, int mc, int ms, int ft) { return engine_set_policy(k, t, mc, ms, ft); }
int bp_yolo_set_precision(bp_yolo* y, int prec) { return engine_set_precision(y, prec); }
int bp_kpd_set_precision(bp_kpd* k, int prec) { return engine_set_precision(k, prec); }
int bp_yolo_op_stats(const bp_yolo* y, double* flops, double* bytes, int cap) { return engine_op_stats(y, flops, bytes, cap); }
int bp_kpd_op_stats(const bp_kpd* k, double* flops, double* bytes, int cap) { return engine_op_stats(k, flops, bytes, cap); }
int bp_yolo_profile(bp_yolo* y, int batch, int iters, float* ms, int* info, int cap, void* stream) {
    return engine_profile(y, batch, iters, ms, info, cap, stream);
}
int bp_kpd_profile(bp_kpd* k, int batch, int iters, float* ms, int* info, int cap, void* stream) {
    return engine_profile(k, batch, iters, ms, info, cap, stream);
}
int bp_yolo_set_prefetch(bp_yolo* y, int on) { return engine_set_prefetch(y, on); }
int bp_kpd_set_prefetch(bp_kpd* k, int on) { return engine_set_prefetch(k, on); }
int bp_yolo_set_fusion(bp_yolo* y, int on) { return engine_set_fusion(y, on); }
int bp_kpd_set_fusion(bp_kpd* k, int on) { return engine_set_fusion(k, on); }
int bp_yolo_fused_launches(bp_yolo* y, int batch, int* launches) { return engine_fused_launches(y, batch, launches); }
int bp_kpd_fused_launches(bp_kpd* k, int batch, int* launches) { return engine_fused_launches(k, batch, launches); }
int bp_yolo_xcd_errors(bp_yolo* y, int* count, void* stream) { return engine_xcd_errors(y, count, stream); }
int bp_kpd_xcd_errors(bp_kpd* k, int* count, void* stream) { return engine_xcd_errors(k, count, stream); }
int bp_yolo_set_stamps(bp_yolo* y, unsigned long long* d_buf, int slots) { return engine_set_stamps(y, d_buf, slots); }
int bp_kpd_set_stamps(bp_kpd* k, unsigned long long* d_buf, int slots) { return engine_set_stamps(k, d_buf, slots); }
int bp_yolo_op_name(const bp_yolo* y, int i, char* out, int cap) { return engine_op_name(y, i, out, cap); }
int bp_kpd_op_name(const bp_kpd* k, int i, char* out, int cap) { return engine_op_name(k, i, out, cap); }
size_t bp_yolo_device_bytes(const bp_yolo* y) { return engine_device_bytes(y); }
size_t bp_kpd_device_bytes(const bp_kpd* k) { return engine_device_bytes(k); }
int bp_calibrate_ticks(long long ticks, float* ms, void* stream) {
    BP_TRY
    BP_CHECK(ms && ticks > 0, "arguments");
    hipStream_t s = (hipStream_t)stream;
    hipEvent_t e0, e1;
    BP_HIP(hipEventCreate(&e0));
    BP_HIP(hipEventCreate(&e1));
    bp::launch_spin_ticks(1000, s);            // warm
    BP_HIP(hipEventRecord(e0, s));
    bp::launch_spin_ticks(ticks, s);
    BP_HIP(hipEventRecord(e1, s));
    BP_HIP(hipEventSynchronize(e1));
    BP_HIP(hipEventElapsedTime(ms, e0, e1));
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    return 0;
    BP_CATCH
}

// ------------------------------------------------------------------ stand-alone stages
int bp_crop(const uint8_t* d_frames, int batch, int H, int W, const float* d_sel, int reso, const float* d_boxes,
            float* d_out_nchw, float* d_out_nhwc, float* d_pts, int oh, int ow, void* stream) {
    BP_TRY
    BP_CHECK(d_frames && (d_sel || d_boxes) && (d_out_nchw || d_out_nhwc), "null argument");
    bp::launch_crop(d_frames, batch, H, W, d_sel, reso, d_boxes, d_out_nhwc, d_out_nchw, d_pts, oh, ow, (hipStream_t)stream);
    BP_HIP(hipGetLastError());
    return 0;
    BP_CATCH
}

int bp_crop_candidates(const uint8_t* d_frames, int frames, int C, int H, int W, const float* d_sel, int reso, const float* d_boxes,
                       float* d_out_nchw, float* d_out_nhwc, float* d_pts, int oh, int ow, void* stream) {
    BP_TRY
    BP_CHECK(d_frames && (d_sel || d_boxes) && (d_out_nchw || d_out_nhwc), "null argument");
    BP_CHECK(frames >= 1 && C >= 1, "bp_crop_candidates: frames and crops per frame must be >= 1");
    bp::launch_crop(d_frames, frames * C, H, W, d_sel, reso, d_boxes, d_out_nhwc, d_out_nchw, d_pts, oh, ow, (hipStream_t)stream, 8, 8, C);
    BP_HIP(hipGetLastError());
    return 0;
    BP_CATCH
}

int bp_resize_bicubic(const uint8_t* d_in, int batch, int H, int W, int oh, int ow, int swap_rb, uint8_t* d_out_u8,
                      float* d_out_nhwc, void* stream) {
    BP_TRY
    BP_CHECK(d_in && (d_out_u8 || d_out_nhwc), "null argument");
    hipStream_t s = (hipStream_t)stream;
    const bp::ResizePlan ph = bp::make_bicubic_plan(W, ow), pv = bp::make_bicubic_plan(H, oh);
    bp::Arena a;
    int* hb = (int*)a.alloc_bytes(ph.bounds.size() * 4);
    int* hk = (int*)a.alloc_bytes(ph.coeffs.size() * 4);
    int* vb = (int*)a.alloc_bytes(pv.bounds.size() * 4);
    int* vk = (int*)a.alloc_bytes(pv.coeffs.size() * 4);
    uint8_t* tmp = (uint8_t*)a.alloc_bytes((size_t)batch * H * ow * 3);
    BP_HIP(hipMemcpyAsync(hb, ph.bounds.data(), ph.bounds.size() * 4, hipMemcpyHostToDevice, s));
    BP_HIP(hipMemcpyAsync(hk, ph.coeffs.data(), ph.coeffs.size() * 4, hipMemcpyHostToDevice, s));
    BP_HIP(hipMemcpyAsync(vb, pv.bounds.data(), pv.bounds.size() * 4, hipMemcpyHostToDevice, s));
    BP_HIP(hipMemcpyAsync(vk, pv.coeffs.data(), pv.coeffs.size() * 4, hipMemcpyHostToDevice, s));
    bp::ResizeTables t{hb, hk, ph.ksize, vb, vk, pv.ksize};
    bp::launch_resize_bicubic(d_in, batch, H, W, tmp, d_out_nhwc, d_out_u8, oh, ow, t, swap_rb, s);
    BP_HIP(hipGetLastError());
    BP_HIP(hipStreamSynchronize(s));   // tables live in a local arena
    return 0;
    BP_CATCH
}

int bp_heatmap_argmax(const float* d_hm, int batch, int C, int H, int W, float* d_kp, void* stream) {
    BP_TRY
    BP_CHECK(d_hm && d_kp && batch > 0 && C > 0 && H > 0 && W > 0, "bad argument");
    bp::launch_heatmap_argmax(d_hm, batch, C, H, W, d_kp, (hipStream_t)stream);
    BP_HIP(hipGetLastError());
    return 0;
    BP_CATCH
}

// ------------------------------------------------------------------ fused per-frame pipeline
static void pipeline_enqueue(bp_pipeline* p, hipStream_t s) {
    bp::YoloNet& yn = *p->y->net;
    bp::KpdNet& kn = *p->k->net;
    const int reso = yn.reso();
    // a1: Pillow-exact bicubic stretch to reso x reso, BGR -> RGB, /255, straight into the detector's NHWC input
#ifdef BP_EXPERIMENTAL   // timing experiment only (WRONG results): BP_ABLATE_RESIZE=1 leaves both resize launches out of
    // the frame (the detector sees whatever its input buffer holds) -- the upper bound of what fusing them into the stem could buy (round-4 verdict item 6; tools/ab_resize.sh)
    static const bool no_resize = std::getenv("BP_ABLATE_RESIZE") != nullptr;
    if (!no_resize) p->resize.enqueue(p->batch, p->H, p->W, yn.input_nhwc(), reso, s);
#else
    p->resize.enqueue(p->batch, p->H, p->W, yn.input_nhwc(), reso, s);
#endif
    // a3-a5: detector + decode + arg-max objectness
    // every stage writes its part of the frame's result row directly (sel[8] | pts[8] | kp[50][6]): no gather launch
    const int R = BP_RESULT_FLOATS;
    yn.forward(yn.input_nhwc(), true, p->batch, nullptr, p->conf, p->num_classes, p->results, s, R);
    // a6-a7: box rescale + crop window + bilinear crop into the KPD's NHWC input
    bp::launch_crop(p->resize.frames, p->batch, p->H, p->W, p->use_fixed ? nullptr : p->results, reso,
                    p->use_fixed ? p->fixed_box : nullptr, kn.input_nhwc(), nullptr, p->results + 8, kn.in_h(), kn.in_w(), s, R, R);
    // a8-a9: KPD + heat-map arg-max
    kn.forward(kn.input_nhwc(), true, p->batch, p->hm, p->results + 16, s, R);
    // a10 (opt-in): decode, pPose-NMS, pruning and PnP on the records just written (pose_tail.hip)
    p->pose.enqueue(p->results, p->batch, s);
    BP_HIP(hipGetLastError());
}

int bp_pipeline_create(bp_yolo* y, bp_kpd* k, int frame_h, int frame_w, int batch, float conf, int num_classes,
                       uint8_t* d_frames, float* d_results, float* d_hm, bp_pipeline** out) {
    BP_TRY
    BP_CHECK(y && k && out, "null argument");
    BP_CHECK(batch >= 1 && batch <= y->net->max_batch() && batch <= k->net->max_batch(), "pipeline batch > engine max_batch");
    BP_CHECK(k->net->out_c() == 50, "pipeline expects 50 key points");
    BP_HIP(hipSetDevice(y->device));
    std::unique_ptr<bp_pipeline> p(new bp_pipeline);
    p->y = y; p->k = k; p->H = frame_h; p->W = frame_w; p->batch = batch; p->conf = conf; p->num_classes = num_classes;
    p->engines = {{y->net.get()}, {k->net.get()}};
    p->resize.init(p->arena, d_frames, batch, frame_h, frame_w, y->net->reso());
    p->results = d_results ? d_results : p->arena.alloc((size_t)batch * BP_RESULT_FLOATS);
    p->hm = d_hm ? d_hm : p->arena.alloc((size_t)batch * 50 * k->net->out_h() * k->net->out_w());
    p->fixed_box = p->arena.alloc((size_t)batch * 4);
    BP_HIP(hipMemset(p->results, 0, (size_t)batch * BP_RESULT_FLOATS * sizeof(float)));
    *out = p.release();
    return 0;
    BP_CATCH
}
void bp_pipeline_destroy(bp_pipeline* p) { delete p; }
uint8_t* bp_pipeline_frames(bp_pipeline* p) { return p ? p->resize.frames : nullptr; }
float* bp_pipeline_results(bp_pipeline* p) { return p ? p->results : nullptr; }
float* bp_pipeline_heatmaps(bp_pipeline* p) { return p ? p->hm : nullptr; }
int bp_pipeline_kernel_count(bp_pipeline* p) { return p ? p->graph.nodes() : -1; }

int bp_pipeline_set_fixed_box(bp_pipeline* p, const float* box) {
    BP_TRY
    p->graph.drop();
    p->use_fixed = box != nullptr;
    if (box) {
        std::vector<float> h((size_t)p->batch * 4);
        for (int b = 0; b < p->batch; ++b) std::memcpy(&h[b * 4], box, 4 * sizeof(float));
        BP_HIP(hipMemcpy(p->fixed_box, h.data(), h.size() * sizeof(float), hipMemcpyHostToDevice));
    }
    return 0;
    BP_CATCH
}

int bp_pipeline_set_pose_solver(bp_pipeline* p, const double* kp3d, int n_kp, const double* K, int left_number,
                                double* d_poses) {
    BP_TRY
    BP_CHECK(p, "null argument");
    p->graph.drop();
    if (!kp3d) {
        p->pose.off();
        return 0;
    }
    const int dev = p->y->device;
    p->pose.set(p->arena, dev, kp3d, n_kp, K, left_number,
                d_poses ? d_poses : bp::own_pose_rows(p->arena, dev, p->own_poses, p->batch));
    return 0;
    BP_CATCH
}
double* bp_pipeline_poses(bp_pipeline* p) { return p ? p->pose.poses : nullptr; }

int bp_pipeline_set_pose_ransac(bp_pipeline* p, double reproj_err, int max_trials, double confidence) {
    BP_TRY
    BP_CHECK(p, "null argument");
    p->graph.drop();
    BP_CHECK(max_trials == 0 || p->pose.on, "bp_pipeline_set_pose_ransac: set a pose solver first (bp_pipeline_set_pose_solver)");
    p->pose.set_ransac(p->arena, p->y->device, p->batch, reproj_err, max_trials, confidence);
    return 0;
    BP_CATCH
}

int bp_pipeline_prepare(bp_pipeline* p) {
    BP_TRY
    BP_CHECK(p, "null argument");
    p->graph.capture(p->engines, [p](hipStream_t s) { pipeline_enqueue(p, s); });
    return 0;
    BP_CATCH
}

int bp_pipeline_run(bp_pipeline* p, int use_graph, void* stream) {
    BP_TRY
    BP_CHECK(p, "null argument");
    hipStream_t s = (hipStream_t)stream;
    auto launch = [&] { p->graph.launch(use_graph, s, p->engines, [p](hipStream_t q) { pipeline_enqueue(p, q); }); };
    launch();
    bp::latency_rerun(p->engines, p->y->device, s, p->latency_faults, launch);   // (lone-frame latency mode only)
    return 0;
    BP_CATCH
}
int bp_pipeline_latency_faults(const bp_pipeline* p) { return p ? p->latency_faults : -1; }

// ------------------------------------------------------------------ scene: one detector pass, K objects' pose chains
// Everything on ONE stream in sequence (no parallel branches in the captured graph): resize once, the shared detector with
// the per-class select writing sel[8] of all K rows, then per slot crop -> KPD -> arg-max -> (opt-in) pose tail -- the
// launches pipeline_enqueue makes for that object, reading row k's own select record.
static void scene_enqueue(bp_scene* p, hipStream_t s) {
    bp::YoloNet& yn = *p->y->net;
    const int reso = yn.reso(), R = BP_RESULT_FLOATS, K = (int)p->slots.size();
    p->resize.enqueue(1, p->H, p->W, yn.input_nhwc(), reso, s);
    yn.forward_classes(yn.input_nhwc(), true, 1, nullptr, p->conf, p->num_classes, p->class_ids.data(), K, p->results, s, K * R, R);
    for (int k = 0; k < K; ++k) {
        bp_scene_slot& sl = p->slots[k];
        bp::KpdNet& kn = *sl.k->net;
        float* row = p->results + (size_t)k * R;
        bp::launch_crop(p->resize.frames, 1, p->H, p->W, row, reso, nullptr, kn.input_nhwc(), nullptr, row + 8, kn.in_h(), kn.in_w(), s, R, R);
        kn.forward(kn.input_nhwc(), true, 1, nullptr, row + 16, s, R);
        sl.pose.enqueue(row, 1, s);
    }
    BP_HIP(hipGetLastError());
}

int bp_scene_create(bp_yolo* y, bp_kpd* const* kpds, const int* class_ids, int K, int frame_h, int frame_w, float conf,
                    int num_classes, uint8_t* d_frames, float* d_results, bp_scene** out) {
    BP_TRY
    BP_CHECK(K >= 1 && K <= BP_MAX_SCENE_CLASSES, "class list: 1 to 16 class ids (BP_MAX_SCENE_CLASSES)");
    BP_CHECK(y && kpds && class_ids && out, "null argument");
    BP_CHECK(frame_h >= 1 && frame_w >= 1, "frame size");
    (void)bp::make_class_list(class_ids, K, num_classes, y->net->attrs());
    std::unique_ptr<bp_scene> p(new bp_scene);
    p->y = y; p->H = frame_h; p->W = frame_w; p->conf = conf; p->num_classes = num_classes;
    p->class_ids.assign(class_ids, class_ids + K);
    p->slots.resize(K);
    p->engines = {{y->net.get()}};
    for (int k = 0; k < K; ++k) {
        BP_CHECK(kpds[k], "null key-point engine");
        BP_CHECK(kpds[k]->net->out_c() == 50, "scene expects 50 key points");
        BP_CHECK(kpds[k]->device == y->device, "scene: every engine on the detector's device");
        for (int j = 0; j < k; ++j) BP_CHECK(kpds[j] != kpds[k], "scene: one key-point engine per object (its activations are the slot's)");
        p->slots[k].k = kpds[k];
        p->engines.push_back({kpds[k]->net.get()});
    }
    BP_HIP(hipSetDevice(y->device));
    p->resize.init(p->arena, d_frames, 1, frame_h, frame_w, y->net->reso());
    p->results = d_results ? d_results : p->arena.alloc((size_t)K * BP_RESULT_FLOATS);
    BP_HIP(hipMemset(p->results, 0, (size_t)K * BP_RESULT_FLOATS * sizeof(float)));
    *out = p.release();
    return 0;
    BP_CATCH
}
void bp_scene_destroy(bp_scene* s) { delete s; }
float* bp_scene_results(bp_scene* s) { return s ? s->results : nullptr; }
double* bp_scene_poses(bp_scene* s) { return s ? s->own_poses : nullptr; }
int bp_scene_kernel_count(bp_scene* s) { return s ? s->graph.nodes() : -1; }

int bp_scene_set_pose_solver(bp_scene* p, int k, const double* kp3d, int n_kp, const double* K, int left_number, double* d_poses_row) {
    BP_TRY
    BP_CHECK(p, "null argument");
    BP_CHECK(k >= 0 && k < (int)p->slots.size(), "scene: slot out of range");
    bp::PoseSolver& pose = p->slots[k].pose;
    p->graph.drop();
    if (!kp3d) {
        pose.off();
        return 0;
    }
    const int dev = p->y->device;
    pose.set(p->arena, dev, kp3d, n_kp, K, left_number,
             d_poses_row ? d_poses_row : bp::own_pose_rows(p->arena, dev, p->own_poses, p->slots.size()) + (size_t)k * BP_POSE_DOUBLES);
    return 0;
    BP_CATCH
}

int bp_scene_set_pose_ransac(bp_scene* p, int k, double reproj_err, int max_trials, double confidence) {
    BP_TRY
    BP_CHECK(p, "null argument");
    BP_CHECK(k >= 0 && k < (int)p->slots.size(), "scene: slot out of range");
    bp::PoseSolver& pose = p->slots[k].pose;
    p->graph.drop();
    BP_CHECK(max_trials == 0 || pose.on, "bp_scene_set_pose_ransac: set the slot's pose solver first (bp_scene_set_pose_solver)");
    pose.set_ransac(p->arena, p->y->device, 1, reproj_err, max_trials, confidence);
    return 0;
    BP_CATCH
}

int bp_scene_prepare(bp_scene* p) {
    BP_TRY
    BP_CHECK(p, "null argument");
    p->graph.capture(p->engines, [p](hipStream_t s) { scene_enqueue(p, s); });
    return 0;
    BP_CATCH
}

int bp_scene_run(bp_scene* p, int use_graph, void* stream) {
    BP_TRY
    BP_CHECK(p, "null argument");
    hipStream_t s = (hipStream_t)stream;
    auto launch = [&] { p->graph.launch(use_graph, s, p->engines, [p](hipStream_t q) { scene_enqueue(p, q); }); };
    launch();
    bp::latency_rerun(p->engines, p->y->device, s, p->latency_faults, launch);
    return 0;
    BP_CATCH
}

// ------------------------------------------------------------------ candidates: NMS survivors of one frame, one key-point pass at batch C
// One stream, one hipGraph: resize -> detector -> select with box NMS (C records + count) -> one crop launch over the C
// boxes -> key-point net at batch C -> arg-max -> (opt-in) the candidate pose tail.  The graph always runs at batch C:
// a slot without a box crops as a frame without a detection does, and the tail reads the count.
static void cands_enqueue(bp_cands* p, hipStream_t s) {
    bp::YoloNet& yn = *p->y->net;
    bp::KpdNet& kn = *p->k->net;
    const int reso = yn.reso(), R = BP_RESULT_FLOATS, C = p->C;
    const bp::PoseSolver& ps = p->pose;
    p->resize.enqueue(1, p->H, p->W, yn.input_nhwc(), reso, s);
    yn.forward_nms(yn.input_nhwc(), true, 1, nullptr, p->conf, p->num_classes, p->class_id, p->nms_conf, C, p->results, p->counts, s,
                   C * R, R);
    bp::launch_crop(p->resize.frames, C, p->H, p->W, p->results, reso, nullptr, kn.input_nhwc(), nullptr, p->results + 8, kn.in_h(), kn.in_w(),
                    s, R, R, C);
    kn.forward(kn.input_nhwc(), true, C, nullptr, p->results + 16, s, R);
    if (ps.on)
        bp::launch_pose_tail_cands(p->results, p->counts, 1, C, ps.kp3d, ps.cam, ps.left_number, ps.poses, p->merged, p->info, s);
    if (ps.on && p->inst_on)
        bp::launch_pose_instances(p->merged, p->info, ps.poses, 1, C, ps.kp3d, ps.cam, ps.left_number, p->inst, s);
    BP_HIP(hipGetLastError());
}

int bp_cands_create(bp_yolo* y, bp_kpd* k, int max_candidates, int frame_h, int frame_w, float conf, int num_classes, int class_id,
                    float nms_conf, uint8_t* d_frame, float* d_results, bp_cands** out) {
    BP_TRY
    BP_CHECK(y && k && out, "null argument");
    const int C = max_candidates;
    BP_CHECK(C >= 1 && C <= BP_MAX_CANDIDATES, "bp_cands_create: 1 to 8 candidates (BP_MAX_CANDIDATES)");
    BP_CHECK(C <= k->net->max_batch(), "bp_cands_create: the key-point engine's max_batch is below the candidate count");
    BP_CHECK(k->net->out_c() == 50, "candidate pipeline expects 50 key points");
    BP_CHECK(k->device == y->device, "candidate pipeline: both engines on one device");
    BP_CHECK(frame_h >= 1 && frame_w >= 1, "frame size");
    const int ncls = num_classes < y->net->attrs() - 5 ? num_classes : y->net->attrs() - 5;
    BP_CHECK(class_id >= 0 && class_id < ncls, "bp_cands_create: class id is not below the detector's class count");
    BP_HIP(hipSetDevice(y->device));
    std::unique_ptr<bp_cands> p(new bp_cands);
    p->y = y; p->k = k; p->C = C; p->H = frame_h; p->W = frame_w; p->conf = conf; p->nms_conf = nms_conf;
    p->num_classes = num_classes; p->class_id = class_id;
    p->engines = {{y->net.get()}, {k->net.get()}};
    p->resize.init(p->arena, d_frame, 1, frame_h, frame_w, y->net->reso());
    p->results = d_results ? d_results : p->arena.alloc((size_t)C * BP_RESULT_FLOATS);
    p->counts = (int*)p->arena.alloc_bytes(sizeof(int));
    BP_HIP(hipMemset(p->results, 0, (size_t)C * BP_RESULT_FLOATS * sizeof(float)));
    BP_HIP(hipMemset(p->counts, 0, sizeof(int)));
    *out = p.release();
    return 0;
    BP_CATCH
}
void bp_cands_destroy(bp_cands* s) { delete s; }
float* bp_cands_results(bp_cands* s) { return s ? s->results : nullptr; }
int* bp_cands_counts(bp_cands* s) { return s ? s->counts : nullptr; }
double* bp_cands_pose(bp_cands* s) { return s ? s->pose.poses : nullptr; }
float* bp_cands_merged(bp_cands* s) { return s ? s->merged : nullptr; }
int* bp_cands_info(bp_cands* s) { return s ? s->info : nullptr; }
double* bp_cands_instance_poses(bp_cands* s) { return s && s->inst_on ? s->inst : nullptr; }
int bp_cands_kernel_count(bp_cands* s) { return s ? s->graph.nodes() : -1; }

int bp_cands_set_pose_solver(bp_cands* p, const double* kp3d, int n_kp, const double* K, int left_number, double* d_pose) {
    BP_TRY
    BP_CHECK(p, "null argument");
    p->graph.drop();
    if (!kp3d) {
        p->pose.off();
        p->inst_on = false;          // the instance poses read the tail's outputs
        return 0;
    }
    const int dev = p->y->device;
    if (!p->info) {   // the tail's other outputs, before the tail can be on
        BP_HIP(hipSetDevice(dev));
        p->merged = p->arena.alloc((size_t)p->C * 152);
        BP_HIP(hipMemset(p->merged, 0, (size_t)p->C * 152 * sizeof(float)));
        int* info = (int*)p->arena.alloc_bytes(4 * sizeof(int));
        BP_HIP(hipMemset(info, 0, 4 * sizeof(int)));
        p->info = info;
    }
    p->pose.set(p->arena, dev, kp3d, n_kp, K, left_number, d_pose ? d_pose : bp::own_pose_rows(p->arena, dev, p->own_pose, 1));
    return 0;
    BP_CATCH
}

int bp_cands_set_instance_poses(bp_cands* p, int on, double* d_inst_poses) {
    BP_TRY
    BP_CHECK(p, "null argument");
    BP_CHECK(p->pose.on, "bp_cands_set_instance_poses: set a pose solver first (bp_cands_set_pose_solver)");
    p->graph.drop();
    if (!on) {
        p->inst_on = false;
        return 0;
    }
    p->inst = d_inst_poses ? d_inst_poses : bp::own_pose_rows(p->arena, p->y->device, p->own_inst, p->C);
    p->inst_on = true;
    return 0;
    BP_CATCH
}

int bp_cands_prepare(bp_cands* p) {
    BP_TRY
    BP_CHECK(p, "null argument");
    p->graph.capture(p->engines, [p](hipStream_t s) { cands_enqueue(p, s); });
    return 0;
    BP_CATCH
}

int bp_cands_run(bp_cands* p, int use_graph, void* stream) {
    BP_TRY
    BP_CHECK(p, "null argument");
    hipStream_t s = (hipStream_t)stream;
    auto launch = [&] { p->graph.launch(use_graph, s, p->engines, [p](hipStream_t q) { cands_enqueue(p, q); }); };
    launch();
    bp::latency_rerun(p->engines, p->y->device, s, p->latency_faults, launch);
    return 0;
    BP_CATCH
}

int bp_upload(void* d_dst, const void* h_src, size_t bytes, void* stream) {
    BP_TRY
    BP_CHECK(d_dst && h_src, "null argument");
    BP_HIP(hipMemcpyAsync(d_dst, h_src, bytes, hipMemcpyHostToDevice, (hipStream_t)stream));
    return 0;
    BP_CATCH
}

}  // extern "C"
