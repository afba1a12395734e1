// extern "C" boundary of libbetapose_hip.so -- see include/betapose_hip.h.
#include "../../include/betapose_hip.h"

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <memory>
#include <sstream>
#include <vector>

#include "annotate.h"
#include "engine.h"
#include "frame_chain.h"
#include "frame_io.h"
#include "icp.h"
#include "pose_tail.h"
#include "raster.h"

static thread_local std::string g_err;

#define BP_TRY try {
#define BP_CATCH                                   \
    }                                              \
    catch (const std::exception& e) {              \
        g_err = e.what();                          \
        return -1;                                 \
    }                                              \
    catch (...) {                                  \
        g_err = "unknown error";                   \
        return -1;                                 \
    }

struct bp_yolo {
    std::unique_ptr<bp::YoloNet> net;
    int device;
};
struct bp_kpd {
    std::unique_ptr<bp::KpdNet> net;
    int device;
};

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
    bp::launch_yolo_select(d_pred, batch, rows, attrs, conf, num_classes, d_sel, (hipStream_t)stream);
    BP_HIP(hipGetLastError());
    return 0;
    BP_CATCH
}

int bp_yolo_select_nms(const float* d_pred, int batch, int rows, int attrs, float conf, int num_classes, int class_id,
                       float nms_conf, int max_candidates, float* d_sel, int* d_counts, void* stream) {
    BP_TRY
    BP_CHECK(d_pred && d_sel && d_counts && batch >= 1 && rows >= 1 && attrs >= 6, "bad argument");
    bp::launch_yolo_select_nms(d_pred, batch, rows, attrs, conf, num_classes, class_id, nms_conf, max_candidates, d_sel, d_counts,
                               (hipStream_t)stream, max_candidates * BP_SEL_FLOATS, BP_SEL_FLOATS);
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

int bp_pose_errors(const double* d_model, int n, const double* d_gt, const double* d_est, int P, const double* K, int want,
                   double* d_out, void* stream) {
    BP_TRY
    BP_CHECK(d_model && d_gt && d_est && d_out, "null argument");
    BP_CHECK(n > 0 && P > 0, "n and P must be positive");
    BP_CHECK(want >= 1 && want <= 7, "want must be a non-empty mask of 1 (ADD), 2 (ADD-S), 4 (2-D)");
    BP_CHECK(K || !(want & 4), "K is required for the 2-D projection error");
    hipStream_t s = (hipStream_t)stream;
    bp::Arena a;
    double* partial = (double*)a.alloc_bytes((size_t)P * bp::pose_error_blocks(n) * 3 * sizeof(double));
    bp::launch_pose_errors(d_model, n, d_gt, d_est, P, K, want, partial, d_out, s);
    BP_HIP(hipGetLastError());
    BP_HIP(hipStreamSynchronize(s));   // partials live in a local arena
    return 0;
    BP_CATCH
}

int bp_pose_errors_sym(const double* d_model, int n, const double* d_gt, const double* d_est, int P, const double* d_sym,
                       int S, const double* K, int want, double* d_out, void* stream) {
    BP_TRY
    BP_CHECK(d_model && d_gt && d_est && d_sym && d_out, "null argument");
    BP_CHECK(n > 0 && P > 0 && S > 0, "n, P and S must be positive");
    BP_CHECK(want >= 1 && want <= 3, "want must be a non-empty mask of 1 (MSSD), 2 (MSPD)");
    BP_CHECK(K || !(want & 2), "K is required for the projection distance (MSPD)");
    hipStream_t s = (hipStream_t)stream;
    bp::Arena a;
    double* scratch = (double*)a.alloc_bytes(bp::pose_errors_sym_scratch_bytes(n, P, S));
    bp::launch_pose_errors_sym(d_model, n, d_gt, d_est, P, d_sym, S, K, want, scratch, d_out, s);
    BP_HIP(hipGetLastError());
    BP_HIP(hipStreamSynchronize(s));   // the per-symmetry maxima live in a local arena
    return 0;
    BP_CATCH
}

// what the three rasteriser calls check alike
static void raster_check_sizes(int n, int F, int P, int H, int W, double near_z) {
    BP_CHECK(n > 0 && F > 0 && P > 0 && H > 0 && W > 0, "n, F, P, H and W must be positive");
    BP_CHECK((long long)H * W <= (1ll << 24), "H * W must not exceed 2^24");
    BP_CHECK(near_z > 0.0, "near must be positive");
}
constexpr size_t RASTER_WS_BYTES = (size_t)256 << 20;      // what the chunked calls keep their workspaces under

int bp_render_depth_host(const double* poses, int P, const double* vertices, int n, const int* faces, int F, const double* K,
                         int H, int W, double pixel_center, double near_z, float* depth, int* skipped) {
    BP_TRY
    BP_CHECK(poses && vertices && faces && K && depth && skipped, "null argument");
    raster_check_sizes(n, F, P, H, W, near_z);
    BP_CHECK(bp::render_depth_host(poses, P, vertices, n, faces, F, K, H, W, pixel_center, near_z, depth, skipped) == 0,
             "a face index lies outside [0, n)");
    return 0;
    BP_CATCH
}

int bp_render_depth(const double* d_model, int n, const int* d_faces, int F, const double* d_poses, int P, const double* K,
                    int H, int W, double pixel_center, double near_z, float* d_depth, int* d_skipped, void* stream) {
    BP_TRY
    BP_CHECK(d_model && d_faces && d_poses && K && d_depth && d_skipped, "null argument");
    raster_check_sizes(n, F, P, H, W, near_z);
    hipStream_t s = (hipStream_t)stream;
    const size_t HW = (size_t)H * W;
    size_t chunk = RASTER_WS_BYTES / bp::raster_vertex_bytes(n, 1);
    chunk = std::max<size_t>(1, std::min<size_t>(chunk, (size_t)P));
    bp::Arena a;
    void* ws = a.alloc_bytes(bp::raster_vertex_bytes(n, (int)chunk));
    BP_HIP(hipMemsetD32Async((hipDeviceptr_t)d_depth, 0x7f800000, (size_t)P * HW, s));   // +inf
    BP_HIP(hipMemsetAsync(d_skipped, 0, (size_t)P * sizeof(int), s));
    for (size_t p0 = 0; p0 < (size_t)P; p0 += chunk) {
        const int c = (int)std::min(chunk, (size_t)P - p0);
        bp::launch_raster(d_model, n, d_faces, F, d_poses + p0 * 12, c, nullptr, 0, K, H, W, pixel_center, near_z, ws,
                          (uint32_t*)d_depth + p0 * HW, d_skipped + p0, s);
    }
    bp::launch_raster_finish((uint32_t*)d_depth, (size_t)P * HW, s);
    BP_HIP(hipGetLastError());
    BP_HIP(hipStreamSynchronize(s));   // the vertex workspace lives in a local arena
    return 0;
    BP_CATCH
}

// what the colour renderer's calls check of image_index (host, may be NULL): pose p -> image p needs I == P, otherwise
// non-decreasing values in [0, I), which lets a call split its work into pose ranges without splitting an image
static void raster_check_image_index(const int* image_index, int P, int I) {
    BP_CHECK(I > 0, "I must be positive");
    if (!image_index) {
        BP_CHECK(I == P, "without image_index the call needs I == P");
        return;
    }
    for (int p = 0; p < P; ++p) {
        BP_CHECK(image_index[p] >= 0 && image_index[p] < I, "image_index must lie in [0, I)");
        BP_CHECK(p == 0 || image_index[p] >= image_index[p - 1], "image_index must be non-decreasing");
    }
}

// poses [*p0, return) of the call go to images [i0, i1); *p0 on entry: the first pose not yet consumed
static int raster_pose_range(const int* image_index, int P, int i1, int p0) {
    if (!image_index) return std::min(P, i1);
    int p = p0;
    while (p < P && image_index[p] < i1) ++p;
    return p;
}

int bp_render_color_host(const double* poses, int P, const double* vertices, int n, const int* faces, int F,
                         const unsigned char* colors, const int* image_index, int I, const double* K, int H, int W,
                         double pixel_center, double near_z, double ambient, const double* light, int accumulate,
                         unsigned char* color, float* depth, int* skipped) {
    BP_TRY
    BP_CHECK(poses && vertices && faces && colors && K && light && color && depth && skipped, "null argument");
    raster_check_sizes(n, F, P, H, W, near_z);
    raster_check_image_index(image_index, P, I);
    BP_CHECK((unsigned long long)P * (unsigned long long)F <= bp::COLOR_MAX_IDS, "P * F must not exceed 2^32 - 2");
    BP_CHECK(bp::render_color_host(poses, P, vertices, n, faces, F, colors, image_index, I, K, H, W, pixel_center, near_z, ambient,
                                   light, accumulate, color, depth, skipped) == 0,
             "a face index lies outside [0, n)");   // (its scan comes before it touches anything)
    return 0;
    BP_CATCH
}

int bp_render_color(const double* d_model, int n, const int* d_faces, int F, const unsigned char* d_colors,
                    const double* d_poses, int P, const int* image_index, int I, const double* K, int H, int W,
                    double pixel_center, double near_z, double ambient, const double* light, int accumulate,
                    unsigned char* d_color, float* d_depth, int* d_skipped, void* stream) {
    BP_TRY
    BP_CHECK(d_model && d_faces && d_colors && d_poses && K && light && d_color && d_depth && d_skipped, "null argument");
    raster_check_sizes(n, F, P, H, W, near_z);
    raster_check_image_index(image_index, P, I);
    BP_CHECK((unsigned long long)P * (unsigned long long)F <= bp::COLOR_MAX_IDS, "P * F must not exceed 2^32 - 2");
    hipStream_t s = (hipStream_t)stream;
    const size_t HW = (size_t)H * W;
    // images in flight: 8 bytes of key per pixel; poses in flight: their vertex workspace; each under RASTER_WS_BYTES
    const size_t ichunk = std::max<size_t>(1, std::min<size_t>(RASTER_WS_BYTES / (HW * 8), (size_t)I));
    const size_t pchunk = std::max<size_t>(1, std::min<size_t>(RASTER_WS_BYTES / bp::raster_vertex_bytes(n, 1), (size_t)P));
    bp::Arena a;
    unsigned long long* keys = (unsigned long long*)a.alloc_bytes(ichunk * HW * 8);
    void* ws = a.alloc_bytes(bp::raster_vertex_bytes(n, (int)pchunk));
    int* d_index = nullptr;
    if (image_index) {
        d_index = (int*)a.alloc_bytes((size_t)P * sizeof(int));
        BP_HIP(hipMemcpyAsync(d_index, image_index, (size_t)P * sizeof(int), hipMemcpyHostToDevice, s));
    }
    BP_HIP(hipMemsetAsync(d_skipped, 0, (size_t)P * sizeof(int), s));
    const bp::ColorLight lt{ambient, light[0], light[1], light[2]};
    int p0 = 0;
    for (size_t i0 = 0; i0 < (size_t)I; i0 += ichunk) {
        const int m = (int)std::min(ichunk, (size_t)I - i0);
        const int p1 = raster_pose_range(image_index, P, (int)i0 + m, p0);
        bp::launch_color_clear(keys, d_depth + i0 * HW, accumulate, (size_t)m * HW, s);
        for (int q0 = p0; q0 < p1; q0 += (int)pchunk) {
            const int c = std::min((int)pchunk, p1 - q0);
            bp::launch_raster_transform(d_model, n, d_poses + (size_t)q0 * 12, c, K, pixel_center, near_z, ws, s);
            bp::launch_color_visibility(d_faces, F, n, ws, q0, c, d_index, (int)i0, K, H, W, pixel_center, near_z, keys,
                                        d_skipped, s);
        }
        bp::launch_color_resolve(keys, m, d_model, d_faces, F, d_colors, d_poses, K, H, W, pixel_center, near_z, lt,
                                 d_color + i0 * HW * 3, d_depth + i0 * HW, s);
        p0 = p1;
    }
    BP_HIP(hipGetLastError());
    BP_HIP(hipStreamSynchronize(s));   // the keys and the vertex workspace live in a local arena
    return 0;
    BP_CATCH
}

static void raster_check_boxes(int P, int I, int H, int W, double near_z) {
    BP_CHECK(P > 0 && I > 0 && H > 0 && W > 0, "P, I, H and W must be positive");
    BP_CHECK((long long)H * W <= (1ll << 24), "H * W must not exceed 2^24");
    BP_CHECK(P <= (1 << 24), "P must not exceed 2^24");
    BP_CHECK(near_z > 0.0, "near must be positive");
}

int bp_draw_boxes_host(const double* poses, int P, const double* corners, const unsigned char* corner_colors,
                       const int* image_index, int I, const double* K, int H, int W, double pixel_center, double near_z,
                       unsigned char* color) {
    BP_TRY
    BP_CHECK(poses && corners && corner_colors && K && color, "null argument");
    raster_check_boxes(P, I, H, W, near_z);
    raster_check_image_index(image_index, P, I);
    bp::draw_boxes_host(poses, P, corners, corner_colors, image_index, I, K, H, W, pixel_center, near_z, color);
    return 0;
    BP_CATCH
}

int bp_draw_boxes(const double* d_poses, int P, const double* d_corners, const unsigned char* d_corner_colors,
                  const int* image_index, int I, const double* K, int H, int W, double pixel_center, double near_z,
                  unsigned char* d_color, void* stream) {
    BP_TRY
    BP_CHECK(d_poses && d_corners && d_corner_colors && K && d_color, "null argument");
    raster_check_boxes(P, I, H, W, near_z);
    raster_check_image_index(image_index, P, I);
    hipStream_t s = (hipStream_t)stream;
    const size_t HW = (size_t)H * W;
    const size_t ichunk = std::max<size_t>(1, std::min<size_t>(RASTER_WS_BYTES / (HW * 4), (size_t)I));
    bp::Arena a;
    uint32_t* ids = (uint32_t*)a.alloc_bytes(ichunk * HW * 4);
    int* d_index = nullptr;
    if (image_index) {
        d_index = (int*)a.alloc_bytes((size_t)P * sizeof(int));
        BP_HIP(hipMemcpyAsync(d_index, image_index, (size_t)P * sizeof(int), hipMemcpyHostToDevice, s));
    }
    int p0 = 0;
    for (size_t i0 = 0; i0 < (size_t)I; i0 += ichunk) {
        const int m = (int)std::min(ichunk, (size_t)I - i0);
        const int p1 = raster_pose_range(image_index, P, (int)i0 + m, p0);
        if (p1 > p0)
            bp::launch_draw_boxes(d_poses, p0, p1 - p0, d_corners, d_corner_colors, d_index, (int)i0, m, K, H, W, pixel_center,
                                  near_z, ids, d_color + i0 * HW * 3, s);
        p0 = p1;
    }
    BP_HIP(hipGetLastError());
    BP_HIP(hipStreamSynchronize(s));   // the id planes live in a local arena
    return 0;
    BP_CATCH
}

int bp_overlay_host(const unsigned char* frames, const unsigned char* color, const float* depth, int I, int H, int W, int alpha,
                    unsigned char* out) {
    BP_TRY
    BP_CHECK(frames && color && depth && out, "null argument");
    BP_CHECK(I > 0 && H > 0 && W > 0, "I, H and W must be positive");
    BP_CHECK((long long)H * W <= (1ll << 24), "H * W must not exceed 2^24");
    BP_CHECK(alpha >= 0 && alpha <= 256, "alpha must lie in 0 .. 256");
    bp::overlay_host(frames, color, depth, I, H, W, alpha, out);
    return 0;
    BP_CATCH
}

int bp_overlay(const unsigned char* d_frames, const unsigned char* d_color, const float* d_depth, int I, int H, int W, int alpha,
               unsigned char* d_out, void* stream) {
    BP_TRY
    BP_CHECK(d_frames && d_color && d_depth && d_out, "null argument");
    BP_CHECK(I > 0 && H > 0 && W > 0, "I, H and W must be positive");
    BP_CHECK((long long)H * W <= (1ll << 24), "H * W must not exceed 2^24");
    BP_CHECK(alpha >= 0 && alpha <= 256, "alpha must lie in 0 .. 256");
    hipStream_t s = (hipStream_t)stream;
    bp::launch_overlay(d_frames, d_color, d_depth, (size_t)I * H * W, alpha, d_out, s);
    BP_HIP(hipGetLastError());
    return 0;
    BP_CATCH
}

int bp_vsd_errors(const double* d_model, int n, const int* d_faces, int F, const double* d_gt, const double* d_est, int P,
                  const double* K, const uint16_t* d_depth_test, int T, int H, int W, double depth_scale,
                  const int* d_test_index, double delta, const double* taus, int n_tau, double diameter, double pixel_center,
                  double near_z, int chunk, double* d_err, int* d_counts, void* stream) {
    BP_TRY
    BP_CHECK(d_model && d_faces && d_gt && d_est && K && d_depth_test && d_test_index && taus && d_err && d_counts,
             "null argument");
    raster_check_sizes(n, F, P, H, W, near_z);
    BP_CHECK(T > 0, "T must be positive");
    BP_CHECK(n_tau >= 1 && n_tau <= bp::VSD_MAX_TAUS, "n_tau must lie in 1 .. 16");
    BP_CHECK(diameter > 0.0 && depth_scale > 0.0 && chunk >= 0, "diameter and depth_scale must be positive, chunk >= 0");
    hipStream_t s = (hipStream_t)stream;
    const size_t HW = (size_t)H * W;
    size_t c = (size_t)chunk;
    if (c == 0)   // both workspaces (2 c z-buffers, 2 c posed meshes) under RASTER_WS_BYTES
        c = std::min(RASTER_WS_BYTES / (2 * HW * sizeof(float)), RASTER_WS_BYTES / bp::raster_vertex_bytes(n, 2));
    c = std::max<size_t>(1, std::min<size_t>(c, (size_t)P));
    bp::VsdTaus tv{};
    for (int k = 0; k < n_tau; ++k) tv.tau[k] = taus[k];
    bp::Arena a;
    uint32_t* zbuf = (uint32_t*)a.alloc_bytes(2 * c * HW * sizeof(uint32_t));
    void* ws = a.alloc_bytes(bp::raster_vertex_bytes(n, (int)(2 * c)));
    int* skipped = (int*)a.alloc_bytes(2 * c * sizeof(int));
    int* acc = (int*)a.alloc_bytes((size_t)P * bp::VSD_ACC * sizeof(int));
    BP_HIP(hipMemsetAsync(acc, 0, (size_t)P * bp::VSD_ACC * sizeof(int), s));
    BP_HIP(hipMemsetAsync(skipped, 0, 2 * c * sizeof(int), s));
    for (size_t p0 = 0; p0 < (size_t)P; p0 += c) {
        const int m = (int)std::min(c, (size_t)P - p0);
        BP_HIP(hipMemsetD32Async((hipDeviceptr_t)zbuf, 0x7f800000, 2 * (size_t)m * HW, s));   // +inf
        bp::launch_raster(d_model, n, d_faces, F, d_gt + p0 * 12, m, d_est + p0 * 12, m, K, H, W, pixel_center, near_z, ws, zbuf,
                          skipped, s);
        bp::launch_vsd_reduce(zbuf, m, d_depth_test, T, d_test_index + p0, H, W, K, pixel_center, depth_scale, delta, tv, n_tau,
                              diameter, acc + p0 * bp::VSD_ACC, s);
    }
    bp::launch_vsd_finish(acc, d_test_index, T, P, n_tau, d_err, d_counts, s);
    BP_HIP(hipGetLastError());
    BP_HIP(hipStreamSynchronize(s));   // the renders live in a local arena
    return 0;
    BP_CATCH
}

// ---- the key-point annotator (annotate.hip / annotate_host.cpp)
static void annot_check_image(int P, int H, int W) {
    BP_CHECK(P > 0 && H > 0 && W > 0, "P, H and W must be positive");
    BP_CHECK((long long)H * W <= (1ll << 24), "H * W must not exceed 2^24");
}
// scene depth and scene index come together; every index (host copy) must name one of the T images
static void annot_check_scene(const void* scene_depth, const void* scene_index, const int* host_index, int P, int T) {
    BP_CHECK((scene_depth != nullptr) == (scene_index != nullptr), "scene_depth and scene_index are given together");
    if (!scene_depth) return;
    BP_CHECK(T > 0, "T must be positive");
    for (int p = 0; p < P; ++p) BP_CHECK(host_index[p] >= 0 && host_index[p] < T, "a scene index lies outside [0, T)");
}
// the device calls read the index back to check it before any kernel uses it
static void annot_check_scene_device(const float* d_scene_depth, const int* d_scene_index, int P, int T, hipStream_t s) {
    std::vector<int> idx;
    if (d_scene_depth && d_scene_index) {
        idx.resize(P);
        BP_HIP(hipMemcpyAsync(idx.data(), d_scene_index, (size_t)P * sizeof(int), hipMemcpyDeviceToHost, s));
        BP_HIP(hipStreamSynchronize(s));
    }
    annot_check_scene(d_scene_depth, d_scene_index, idx.data(), P, T);
}

int bp_annotate_keypoints_host(const double* poses, int P, const double* kp, int Kp, const double* K, int H, int W,
                               double pixel_center, double near_z, const float* model_depth, const float* scene_depth, int T,
                               const int* scene_index, double self_tol, double delta, double* xy, double* z,
                               unsigned char* flags) {
    BP_TRY
    BP_CHECK(poses && kp && K && xy && z && flags, "null argument");
    annot_check_image(P, H, W);
    BP_CHECK(Kp > 0 && (long long)P * Kp < (1ll << 31), "Kp must be positive and P * Kp below 2^31");
    BP_CHECK(near_z > 0.0, "near must be positive");
    annot_check_scene(scene_depth, scene_index, scene_index, P, T);
    bp::annotate_keypoints_host(poses, P, kp, Kp, K, H, W, pixel_center, near_z, model_depth, scene_depth, scene_index, self_tol,
                                delta, xy, z, flags);
    return 0;
    BP_CATCH
}

int bp_annotate_keypoints(const double* d_poses, int P, const double* d_kp, int Kp, const double* K, int H, int W,
                          double pixel_center, double near_z, const float* d_model_depth, const float* d_scene_depth, int T,
                          const int* d_scene_index, double self_tol, double delta, double* d_xy, double* d_z,
                          unsigned char* d_flags, void* stream) {
    BP_TRY
    BP_CHECK(d_poses && d_kp && K && d_xy && d_z && d_flags, "null argument");
    annot_check_image(P, H, W);
    BP_CHECK(Kp > 0 && (long long)P * Kp < (1ll << 31), "Kp must be positive and P * Kp below 2^31");
    BP_CHECK(near_z > 0.0, "near must be positive");
    hipStream_t s = (hipStream_t)stream;
    annot_check_scene_device(d_scene_depth, d_scene_index, P, T, s);
    bp::launch_annotate_keypoints(d_poses, P, d_kp, Kp, K, H, W, pixel_center, near_z, d_model_depth, d_scene_depth,
                                  d_scene_index, self_tol, delta, d_xy, d_z, d_flags, s);
    BP_HIP(hipGetLastError());
    return 0;
    BP_CATCH
}

int bp_mask_boxes_host(const float* depth, int P, int H, int W, const double* K, double pixel_center, const float* scene_depth,
                       int T, const int* scene_index, double delta, int* boxes, int* counts) {
    BP_TRY
    BP_CHECK(depth && K && boxes && counts, "null argument");
    annot_check_image(P, H, W);
    annot_check_scene(scene_depth, scene_index, scene_index, P, T);
    bp::mask_boxes_host(depth, P, H, W, K, pixel_center, scene_depth, scene_index, delta, boxes, counts);
    return 0;
    BP_CATCH
}

int bp_mask_boxes(const float* d_depth, int P, int H, int W, const double* K, double pixel_center, const float* d_scene_depth,
                  int T, const int* d_scene_index, double delta, int* d_boxes, int* d_counts, void* stream) {
    BP_TRY
    BP_CHECK(d_depth && K && d_boxes && d_counts, "null argument");
    annot_check_image(P, H, W);
    BP_CHECK(P < (1 << 28), "P must be below 2^28");
    hipStream_t s = (hipStream_t)stream;
    annot_check_scene_device(d_scene_depth, d_scene_index, P, T, s);
    bp::Arena a;
    int* acc = (int*)a.alloc_bytes((size_t)P * 2 * bp::ANNOT_BOX_INTS * sizeof(int));
    bp::launch_mask_boxes(d_depth, P, H, W, K, pixel_center, d_scene_depth, d_scene_index, delta, acc, d_boxes, d_counts, s);
    BP_HIP(hipGetLastError());
    BP_HIP(hipStreamSynchronize(s));   // the accumulators live in a local arena
    return 0;
    BP_CATCH
}

int bp_vertex_boxes_host(const double* poses, int P, const double* vertices, int n, const double* K, int H, int W, int* boxes) {
    BP_TRY
    BP_CHECK(poses && vertices && K && boxes, "null argument");
    annot_check_image(P, H, W);
    BP_CHECK(n > 0, "n must be positive");
    bp::vertex_boxes_host(poses, P, vertices, n, K, H, W, boxes);
    return 0;
    BP_CATCH
}

int bp_vertex_boxes(const double* d_poses, int P, const double* d_vertices, int n, const double* K, int H, int W, int* d_boxes,
                    void* stream) {
    BP_TRY
    BP_CHECK(d_poses && d_vertices && K && d_boxes, "null argument");
    annot_check_image(P, H, W);
    BP_CHECK(n > 0 && P < (1 << 28), "n must be positive and P below 2^28");
    hipStream_t s = (hipStream_t)stream;
    bp::Arena a;
    int* acc = (int*)a.alloc_bytes((size_t)P * bp::ANNOT_BOX_INTS * sizeof(int));
    bp::launch_vertex_boxes(d_poses, P, d_vertices, n, K, H, W, acc, d_boxes, s);
    BP_HIP(hipGetLastError());
    BP_HIP(hipStreamSynchronize(s));   // the accumulators live in a local arena
    return 0;
    BP_CATCH
}

static void annot_check_targets(int B, int Kp, int inpH, int inpW, int resH, int resW, int size) {
    BP_CHECK(B > 0 && Kp > 0 && inpH > 0 && inpW > 0 && resH > 0 && resW > 0, "B, Kp and the resolutions must be positive");
    BP_CHECK(size >= 1 && size % 2 == 1 && size <= 1025, "the Gaussian table needs an odd size of at most 1025");
    // (the kernel indexes rows in groups of four floats: the width counts rounded up to a multiple of 4)
    BP_CHECK((long long)B * Kp * resH * ((resW + 3) / 4 * 4) < (1ll << 31), "the target tensor must hold fewer than 2^31 values");
}

int bp_kpd_targets_host(const double* parts, const float* ul, const float* br, int B, int Kp, int inpH, int inpW, int resH,
                        int resW, const float* g, int size, float* out, int* centres, float* set_mask) {
    BP_TRY
    BP_CHECK(parts && ul && br && g && out && centres, "null argument");
    annot_check_targets(B, Kp, inpH, inpW, resH, resW, size);
    bp::kpd_targets_host(parts, ul, br, B, Kp, inpH, inpW, resH, resW, g, size, out, centres, set_mask);
    return 0;
    BP_CATCH
}

int bp_kpd_targets(const double* d_parts, const float* d_ul, const float* d_br, int B, int Kp, int inpH, int inpW, int resH,
                   int resW, const float* d_g, int size, float* d_out, int* d_centres, float* d_set_mask, void* stream) {
    BP_TRY
    BP_CHECK(d_parts && d_ul && d_br && d_g && d_out && d_centres, "null argument");
    annot_check_targets(B, Kp, inpH, inpW, resH, resW, size);
    bp::launch_kpd_targets(d_parts, d_ul, d_br, B, Kp, inpH, inpW, resH, resW, d_g, size, d_out, d_centres, d_set_mask,
                           (hipStream_t)stream);
    BP_HIP(hipGetLastError());
    return 0;
    BP_CATCH
}

// what the four refinement calls check alike, and the parameter block they hand on
static bp::IcpParams icp_params(const double* K, int T, double depth_scale, int iterations, double max_dist, double min_cos,
                                int min_pixels, double pixel_center) {
    BP_CHECK(T > 0, "T must be positive");
    BP_CHECK(depth_scale > 0.0 && max_dist > 0.0, "depth_scale and max_dist must be positive");
    BP_CHECK(min_cos >= 0.0 && min_cos <= 1.0, "min_cos must lie in [0, 1]");
    BP_CHECK(iterations >= 0 && iterations <= 1000 && min_pixels >= 0, "iterations must lie in 0 .. 1000, min_pixels >= 0");
    return bp::IcpParams{K[0], K[4], K[2], K[5], pixel_center, depth_scale, max_dist, min_cos, min_pixels, iterations};
}

// poses per chunk of the device calls: the z-buffers and the posed meshes of a chunk each stay under RASTER_WS_BYTES
static size_t icp_chunk(int chunk, int n, int P, size_t HW) {
    size_t c = (size_t)chunk;
    if (c == 0) c = std::min(RASTER_WS_BYTES / (HW * sizeof(float)), RASTER_WS_BYTES / bp::raster_vertex_bytes(n, 1));
    return std::max<size_t>(1, std::min<size_t>(c, (size_t)P));
}

int bp_icp_normal_equations_host(const double* poses, int P, const double* vertices, int n, const int* faces, int F,
                                 const double* K, const uint16_t* depth_test, int T, int H, int W, double depth_scale,
                                 const int* test_index, double max_dist, double min_cos, double pixel_center, double near_z,
                                 double* out) {
    BP_TRY
    BP_CHECK(poses && vertices && faces && K && depth_test && test_index && out, "null argument");
    raster_check_sizes(n, F, P, H, W, near_z);
    const bp::IcpParams prm = icp_params(K, T, depth_scale, 0, max_dist, min_cos, 0, pixel_center);
    BP_CHECK(bp::icp_normal_equations_host(poses, P, vertices, n, faces, F, K, depth_test, T, test_index, H, W, prm, near_z,
                                           out) == 0,
             "a face index lies outside [0, n)");
    return 0;
    BP_CATCH
}

int bp_refine_depth_host(const double* poses, int P, const double* vertices, int n, const int* faces, int F, const double* K,
                         const uint16_t* depth_test, int T, int H, int W, double depth_scale, const int* test_index,
                         int iterations, double max_dist, double min_cos, int min_pixels, double pixel_center, double near_z,
                         double* poses_out, double* stats) {
    BP_TRY
    BP_CHECK(poses && vertices && faces && K && depth_test && test_index && poses_out && stats, "null argument");
    raster_check_sizes(n, F, P, H, W, near_z);
    const bp::IcpParams prm = icp_params(K, T, depth_scale, iterations, max_dist, min_cos, min_pixels, pixel_center);
    BP_CHECK(bp::refine_depth_host(poses, P, vertices, n, faces, F, K, depth_test, T, test_index, H, W, prm, near_z, poses_out,
                                   stats) == 0,
             "a face index lies outside [0, n)");
    return 0;
    BP_CATCH
}

int bp_icp_normal_equations(const double* d_model, int n, const int* d_faces, int F, const double* d_poses, int P,
                            const double* K, const uint16_t* d_depth_test, int T, int H, int W, double depth_scale,
                            const int* d_test_index, double max_dist, double min_cos, double pixel_center, double near_z,
                            int chunk, double* d_out, void* stream) {
    BP_TRY
    BP_CHECK(d_model && d_faces && d_poses && K && d_depth_test && d_test_index && d_out, "null argument");
    raster_check_sizes(n, F, P, H, W, near_z);
    BP_CHECK(chunk >= 0, "chunk must not be negative");
    const bp::IcpParams prm = icp_params(K, T, depth_scale, 0, max_dist, min_cos, 0, pixel_center);
    hipStream_t s = (hipStream_t)stream;
    const size_t HW = (size_t)H * W, c = icp_chunk(chunk, n, P, HW);
    const int slices = bp::icp_slices(H, W);
    bp::Arena a;
    uint32_t* zbuf = (uint32_t*)a.alloc_bytes(c * HW * sizeof(uint32_t));
    void* ws = a.alloc_bytes(bp::raster_vertex_bytes(n, (int)c));
    int* skipped = (int*)a.alloc_bytes(c * sizeof(int));
    double* partial = (double*)a.alloc_bytes(c * slices * bp::ICP_ACC * sizeof(double));
    BP_HIP(hipMemsetAsync(skipped, 0, c * sizeof(int), s));
    for (size_t p0 = 0; p0 < (size_t)P; p0 += c) {
        const int m = (int)std::min(c, (size_t)P - p0);
        BP_HIP(hipMemsetD32Async((hipDeviceptr_t)zbuf, 0x7f800000, (size_t)m * HW, s));   // +inf
        bp::launch_raster(d_model, n, d_faces, F, d_poses + p0 * 12, m, nullptr, 0, K, H, W, pixel_center, near_z, ws, zbuf,
                          skipped, s);
        bp::launch_icp_accumulate(zbuf, d_poses + p0 * 12, m, d_depth_test, T, d_test_index + p0, H, W, prm, nullptr, partial, s);
        bp::launch_icp_sum(partial, d_test_index + p0, T, m, slices, d_out + p0 * bp::ICP_ACC, s);
    }
    BP_HIP(hipGetLastError());
    BP_HIP(hipStreamSynchronize(s));   // the renders and partial sums live in a local arena
    return 0;
    BP_CATCH
}

int bp_refine_depth(const double* d_model, int n, const int* d_faces, int F, const double* d_poses, int P, const double* K,
                    const uint16_t* d_depth_test, int T, int H, int W, double depth_scale, const int* d_test_index,
                    int iterations, double max_dist, double min_cos, int min_pixels, double pixel_center, double near_z,
                    int chunk, double* d_poses_out, double* d_stats, void* stream) {
    BP_TRY
    BP_CHECK(d_model && d_faces && d_poses && K && d_depth_test && d_test_index && d_poses_out && d_stats, "null argument");
    BP_CHECK(d_poses_out != d_poses, "d_poses_out must not be d_poses: a rejected pose gets its input back");
    raster_check_sizes(n, F, P, H, W, near_z);
    BP_CHECK(chunk >= 0, "chunk must not be negative");
    const bp::IcpParams prm = icp_params(K, T, depth_scale, iterations, max_dist, min_cos, min_pixels, pixel_center);
    hipStream_t s = (hipStream_t)stream;
    const size_t HW = (size_t)H * W, c = icp_chunk(chunk, n, P, HW);
    const int slices = bp::icp_slices(H, W);
    bp::Arena a;
    uint32_t* zbuf = (uint32_t*)a.alloc_bytes(c * HW * sizeof(uint32_t));
    void* ws = a.alloc_bytes(bp::raster_vertex_bytes(n, (int)c));
    int* skipped = (int*)a.alloc_bytes(c * sizeof(int));
    double* partial = (double*)a.alloc_bytes(c * slices * bp::ICP_ACC * sizeof(double));
    BP_HIP(hipMemsetAsync(skipped, 0, c * sizeof(int), s));
    bp::launch_icp_init(d_poses, d_test_index, T, P, d_poses_out, d_stats, s);
    for (size_t p0 = 0; p0 < (size_t)P; p0 += c) {
        const int m = (int)std::min(c, (size_t)P - p0);
        double* pose = d_poses_out + p0 * 12;
        double* stats = d_stats + p0 * bp::ICP_STATS;
        // the whole loop is enqueued: no host round trip between the iterations
        for (int k = 0; k <= iterations; ++k) {
            BP_HIP(hipMemsetD32Async((hipDeviceptr_t)zbuf, 0x7f800000, (size_t)m * HW, s));   // +inf
            bp::launch_raster(d_model, n, d_faces, F, pose, m, nullptr, 0, K, H, W, pixel_center, near_z, ws, zbuf, skipped, s);
            bp::launch_icp_accumulate(zbuf, pose, m, d_depth_test, T, d_test_index + p0, H, W, prm, stats, partial, s);
            bp::launch_icp_step(partial, m, slices, k, prm, d_poses + p0 * 12, pose, stats, s);
        }
    }
    BP_HIP(hipGetLastError());
    BP_HIP(hipStreamSynchronize(s));   // the renders and partial sums live in a local arena
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

int bp_conv2d(const float* d_in, int N, int H, int W, int Cin, const float* h_w, const float* h_bias, int Cout, int k,
              int stride, int pad, int act, int store_mode, const float* d_res, int res_after_act, int tile, int splits,
              float* d_out, int iters, float* ms_per_iter, void* stream) {
    return bp_conv2d_planes(d_in, N, H, W, Cin, h_w, h_bias, Cout, k, stride, pad, act, store_mode, d_res, res_after_act, tile,
                            splits, d_out, nullptr, iters, ms_per_iter, stream);
}

int bp_conv2d_planes(const float* d_in, int N, int H, int W, int Cin, const float* h_w, const float* h_bias, int Cout, int k,
                     int stride, int pad, int act, int store_mode, const float* d_res, int res_after_act, int tile, int splits,
                     float* d_out, unsigned short* d_out_planes, int iters, float* ms_per_iter, void* stream) {
    BP_TRY
    BP_CHECK(d_in && h_w && d_out, "null argument");
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
    net.add_conv("conv", in, out, cw, Cout, k, stride, pad, act, store_mode, d_res ? &res : nullptr, nullptr,
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
    if (sp == 1 && !std::getenv("BP_CONV_SELF_PREFETCH") && bp::conv_hybrid_plan(p, t, bp::conv_slab_floats(t, 8, 256), &h)) {   // (<= 8 slices of <= 256 tail tiles)
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

int bp_pose_from_records(const float* d_records, int batch, const double* d_kp3d, int n_kp, const double* K,
                         int left_number, double* d_poses, void* stream) {
    BP_TRY
    BP_CHECK(d_records && d_kp3d && K && d_poses, "null argument");
    BP_CHECK(batch >= 0, "batch must be >= 0");
    bp::check_pose_points(n_kp, left_number);
    if (batch == 0) return 0;
    bp::launch_pose_tail(d_records, batch, d_kp3d, bp::make_pnp_cam(K), left_number, d_poses, (hipStream_t)stream);
    BP_HIP(hipGetLastError());
    return 0;
    BP_CATCH
}

int bp_pose_from_candidate_records(const float* d_records, const int* d_counts, int frames, int C, const double* d_kp3d, int n_kp,
                                   const double* K, int left_number, double* d_poses, float* d_merged, int* d_info, void* stream) {
    BP_TRY
    BP_CHECK(d_records && d_counts && d_kp3d && K && d_poses && d_merged && d_info, "null argument");
    BP_CHECK(frames >= 0, "frames must be >= 0");
    BP_CHECK(C >= 1 && C <= BP_MAX_CANDIDATES, "1 to 8 candidates per frame (BP_MAX_CANDIDATES)");
    bp::check_pose_points(n_kp, left_number);
    if (frames == 0) return 0;
    bp::launch_pose_tail_cands(d_records, d_counts, frames, C, d_kp3d, bp::make_pnp_cam(K), left_number, d_poses, d_merged, d_info,
                               (hipStream_t)stream);
    BP_HIP(hipGetLastError());
    return 0;
    BP_CATCH
}

int bp_pose_instances_from_merged(const float* d_merged, const int* d_info, const double* d_poses, int frames, int C,
                                  const double* d_kp3d, int n_kp, const double* K, int left_number, double* d_inst_poses,
                                  void* stream) {
    BP_TRY
    BP_CHECK(C >= 1 && C <= BP_MAX_CANDIDATES, "1 to 8 candidates per frame (BP_MAX_CANDIDATES)");
    BP_CHECK(d_merged && d_info && d_poses && d_kp3d && K && d_inst_poses, "null argument");
    BP_CHECK(frames >= 0 && frames <= 65535, "frames must be in [0, 65535]");
    bp::check_pose_points(n_kp, left_number);
    if (frames == 0) return 0;
    bp::launch_pose_instances(d_merged, d_info, d_poses, frames, C, d_kp3d, bp::make_pnp_cam(K), left_number, d_inst_poses,
                              (hipStream_t)stream);
    BP_HIP(hipGetLastError());
    return 0;
    BP_CATCH
}

int bp_solve_pnp_batch(const double* d_pts3d, int shared_3d, const double* d_pts2d, int n, int P, const double* K,
                       double* d_Rt, int* d_status, void* stream) {
    BP_TRY
    BP_CHECK(d_pts3d && d_pts2d && K && d_Rt && d_status, "null argument");
    BP_CHECK(n >= 0 && n <= BP_PNP_MAX_POINTS, "bp_solve_pnp_batch: n must be in [0, 64] points per problem");
    BP_CHECK(P >= 0, "P must be >= 0");
    if (P == 0) return 0;
    bp::launch_solve_pnp_batch(d_pts3d, shared_3d, d_pts2d, n, P, bp::make_pnp_cam(K), d_Rt, d_status, (hipStream_t)stream);
    BP_HIP(hipGetLastError());
    return 0;
    BP_CATCH
}

int bp_pnp_ransac_samples(int n, int max_trials, int* idx) {
    BP_TRY
    BP_CHECK(idx, "null argument");
    BP_CHECK(n >= 6 && max_trials >= 1, "bp_pnp_ransac_samples: needs n >= 6 points and max_trials >= 1");
    bp::pnp_ransac_samples(n, max_trials, idx);
    return 0;
    BP_CATCH
}

int bp_pnp_ransac_trials_needed(int n, double confidence, int* need) {
    BP_TRY
    BP_CHECK(need, "null argument");
    BP_CHECK(n >= 1 && confidence > 0 && confidence < 1, "bp_pnp_ransac_trials_needed: needs n >= 1 and a confidence in (0, 1)");
    bp::pnp_ransac_trials_needed(n, confidence, need);
    return 0;
    BP_CATCH
}

size_t bp_pnp_ransac_workspace_bytes(int P, int max_trials) {
    return P > 0 && max_trials > 0 ? bp::pnp_ransac_workspace_bytes(P, max_trials) : 0;
}

int bp_solve_pnp_ransac_batch(const double* d_pts3d, int shared_3d, const double* d_pts2d, int n, int P, const double* K,
                              double reproj_err, int max_trials, double confidence, double* d_Rt, int* d_status,
                              unsigned char* d_inliers, void* d_workspace, size_t workspace_bytes, void* stream) {
    BP_TRY
    BP_CHECK(d_pts3d && d_pts2d && K && d_Rt && d_status, "null argument");
    BP_CHECK(n >= 0 && n <= BP_PNP_MAX_POINTS, "bp_solve_pnp_ransac_batch: n must be in [0, 64] points per problem");
    BP_CHECK(P >= 0, "P must be >= 0");
    bp::check_ransac_params(reproj_err, max_trials, confidence);
    if (P == 0) return 0;
    BP_CHECK(d_workspace && workspace_bytes >= bp::pnp_ransac_workspace_bytes(P, max_trials),
             "bp_solve_pnp_ransac_batch: workspace smaller than bp_pnp_ransac_workspace_bytes(P, max_trials)");
    BP_CHECK(((uintptr_t)d_workspace & 7) == 0, "bp_solve_pnp_ransac_batch: workspace must be 8-byte aligned");
    std::vector<int> samples, need;
    bp::ransac_tables(n, max_trials, confidence, samples, need);
    bp::launch_pnp_ransac(d_pts3d, shared_3d ? 0 : (size_t)n * 3, d_pts2d, (size_t)n * 2, nullptr, n, P, bp::make_pnp_cam(K), reproj_err,
                          max_trials, samples.data(), need.data(), d_workspace, d_Rt, d_status, d_inliers, nullptr,
                          (hipStream_t)stream);
    BP_HIP(hipGetLastError());
    return 0;
    BP_CATCH
}

int bp_pipeline_set_pose_ransac(bp_pipeline* p, double reproj_err, int max_trials, double confidence) {
    BP_TRY
    BP_CHECK(p, "null argument");
    p->graph.drop();
    BP_CHECK(max_trials == 0 || p->pose.on, "bp_pipeline_set_pose_ransac: set a pose solver first (bp_pipeline_set_pose_solver)");
    p->pose.set_ransac(p->arena, p->y->device, p->batch, reproj_err, max_trials, confidence);
    return 0;
    BP_CATCH
}

size_t bp_pose_ransac_workspace_bytes(int batch, int max_trials) {
    return batch > 0 && max_trials > 0 ? bp::pose_ransac_ws_bytes(batch, max_trials) : 0;
}

int bp_pose_from_records_ransac(const float* d_records, int batch, const double* d_kp3d, int n_kp, const double* K,
                                int left_number, double reproj_err, int max_trials, double confidence, double* d_poses,
                                void* d_workspace, size_t workspace_bytes, void* stream) {
    BP_TRY
    BP_CHECK(d_records && d_kp3d && K && d_poses, "null argument");
    BP_CHECK(batch >= 0, "batch must be >= 0");
    bp::check_pose_points(n_kp, left_number);
    bp::check_ransac_params(reproj_err, max_trials, confidence);
    if (batch == 0) return 0;
    BP_CHECK(d_workspace && workspace_bytes >= bp::pose_ransac_ws_bytes(batch, max_trials),
             "bp_pose_from_records_ransac: workspace smaller than bp_pose_ransac_workspace_bytes(batch, max_trials)");
    BP_CHECK(((uintptr_t)d_workspace & 7) == 0, "bp_pose_from_records_ransac: workspace must be 8-byte aligned");
    std::vector<int> samples, need;
    bp::ransac_tables(bp::pose_points(left_number), max_trials, confidence, samples, need);
    bp::pose_tail_ransac(d_records, batch, d_kp3d, bp::make_pnp_cam(K), left_number, reproj_err, max_trials, samples.data(), need.data(),
                     d_poses, d_workspace, (hipStream_t)stream);
    BP_HIP(hipGetLastError());
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

// ------------------------------------------------------------------ host post-processing
int bp_solve_pnp(const double* pts3d, const double* pts2d, int n, const double* K, double* R, double* t) {
    BP_TRY
    BP_CHECK(pts3d && pts2d && K && R && t, "null argument");
    const int rc = bp::solve_pnp(pts3d, pts2d, n, K, R, t);
    if (rc != 0) throw bp::Error("solve_pnp failed (need >= 6 non-degenerate points, or >= 4 coplanar ones)");
    return 0;
    BP_CATCH
}

int bp_solve_pnp_status(const double* pts3d, const double* pts2d, int n, const double* K, double* R, double* t, int* status) {
    BP_TRY
    BP_CHECK(pts3d && pts2d && K && R && t && status, "null argument");
    *status = bp::solve_pnp(pts3d, pts2d, n, K, R, t);
    return 0;
    BP_CATCH
}

int bp_solve_pnp_refined(const double* pts3d, const double* pts2d, int n, const double* K, double* R, double* t) {
    BP_TRY
    BP_CHECK(pts3d && pts2d && K && R && t, "null argument");
    const int rc = bp::solve_pnp_refined(pts3d, pts2d, n, K, R, t);
    if (rc != 0) throw bp::Error("solve_pnp_refined failed (need >= 6 non-degenerate points)");
    return 0;
    BP_CATCH
}

int bp_solve_pnp_ransac(const double* pts3d, const double* pts2d, int n, const double* K, double reproj_err,
                        int max_trials, double confidence, double* R, double* t, unsigned char* inliers) {
    BP_TRY
    BP_CHECK(pts3d && pts2d && K && R && t, "null argument");
    bp::check_ransac_params(reproj_err, max_trials, confidence);
    const int rc = bp::solve_pnp_ransac(pts3d, pts2d, n, K, reproj_err, max_trials, confidence, R, t, inliers);
    if (rc != 0) throw bp::Error("solve_pnp_ransac failed (need >= 6 points and a 6-point consensus)");
    return 0;
    BP_CATCH
}

int bp_pose_nms(const float* bboxes, const float* bbox_scores, const float* preds, const float* scores, int n, int K,
                int* out_pick, float* out_pose, float* out_score, float* out_prop) {
    BP_TRY
    BP_CHECK(n >= 0 && K >= 1, "bad sizes");
    BP_CHECK(n == 0 || (bboxes && bbox_scores && preds && scores && out_pick && out_pose && out_score && out_prop), "null argument");
    return bp::pose_nms(bboxes, bbox_scores, preds, scores, n, K, out_pick, out_pose, out_score, out_prop);
    BP_CATCH
}

// ------------------------------------------------------------------ frame input (host)
struct bp_loader {
    std::unique_ptr<bp::FrameLoader> l;
};

static void* pinned_alloc(size_t bytes) {
    void* p = nullptr;
    if (hipHostMalloc(&p, bytes, hipHostMallocDefault) != hipSuccess) {
        (void)hipGetLastError();
        return nullptr;
    }
    return p;
}
static void pinned_free(void* p) { (void)hipHostFree(p); }

int bp_png_info(const unsigned char* data, size_t n, int* h, int* w, int* channels) {
    BP_TRY
    BP_CHECK(data, "null argument");
    bp::png_info(data, n, h, w, channels);
    return 0;
    BP_CATCH
}

int bp_png_decode_bgr(const unsigned char* data, size_t n, unsigned char* out_bgr, size_t cap, int* h, int* w) {
    BP_TRY
    BP_CHECK(data && out_bgr, "null argument");
    static thread_local std::vector<uint8_t> scratch;
    bp::png_decode_bgr(data, n, out_bgr, cap, h, w, scratch);
    return 0;
    BP_CATCH
}

int bp_loader_create(const char* const* paths, int n, int H, int W, int threads, int depth, int pinned, bp_loader** out) {
    BP_TRY
    BP_CHECK(paths && out && n >= 0, "null argument");
    std::vector<std::string> v;
    for (int i = 0; i < n; ++i) {
        BP_CHECK(paths[i], "null path");
        v.emplace_back(paths[i]);
    }
    int ndev = 0;
    const bool pin = pinned && hipGetDeviceCount(&ndev) == hipSuccess && ndev > 0;
    if (!pin) (void)hipGetLastError();
    auto* L = new bp_loader;
    try {
        L->l.reset(new bp::FrameLoader(std::move(v), H, W, threads, depth, pin ? pinned_alloc : nullptr,
                                       pin ? pinned_free : nullptr));
    } catch (...) {
        delete L;
        throw;
    }
    *out = L;
    return 0;
    BP_CATCH
}

void bp_loader_destroy(bp_loader* l) { delete l; }

int bp_loader_next(bp_loader* l, long long* index, const unsigned char** bgr) {
    BP_TRY
    BP_CHECK(l, "null argument");
    std::string err;
    const int rc = l->l->next(index, bgr, &err);
    if (rc < 0) g_err = err;
    return rc;
    BP_CATCH
}

int bp_loader_release(bp_loader* l, long long index) {
    BP_TRY
    BP_CHECK(l, "null argument");
    l->l->release(index);
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
