// What the per-frame device chains of c_api.cpp (bp_pipeline, bp_scene, bp_cands) have in common, once: the hipGraph of a
// frame and the rule that makes it stale, the lone-frame latency mode's re-run, the bicubic resize stage and the pose
// solver's state.  Host only.  A chain adds its own fields, its *_enqueue, its argument checks and its accessors.
#pragma once
#include <vector>

#include "engine.h"
#include "pose_tail.h"

namespace bp {

// ------------------------------------------------------------------ the frame's graph
// An engine of a chain and the plan version the chain's graph was captured with.  A chain lists the detector first,
// then its key-point engine(s).
struct EngineSeen {
    Net* net;
    unsigned seen = 0;
};
using EngineList = std::vector<EngineSeen>;

struct FrameGraph {
    hipGraph_t graph = nullptr;
    hipGraphExec_t exec = nullptr;
    hipStream_t cap_stream = nullptr;
    FrameGraph() = default;
    FrameGraph(const FrameGraph&) = delete;
    FrameGraph& operator=(const FrameGraph&) = delete;
    ~FrameGraph() {
        drop();
        if (cap_stream) (void)hipStreamDestroy(cap_stream);
    }
    void drop() {
        if (exec) { (void)hipGraphExecDestroy(exec); exec = nullptr; }
        if (graph) { (void)hipGraphDestroy(graph); graph = nullptr; }
    }
    int nodes() const {   // -1 before a capture
        size_t n = 0;
        if (!graph || hipGraphGetNodes(graph, nullptr, &n) != hipSuccess) return -1;
        return (int)n;
    }
    // (re)build the graph when there is none or an engine's launch plan (policy, precision) changed since the capture:
    // records the launches `enqueue(stream)` makes, executes nothing
    template <class Enqueue>
    void capture(EngineList& engines, Enqueue&& enqueue) {
        bool stale = false;
        for (const EngineSeen& e : engines) stale = stale || e.seen != e.net->plan_version();
        if (exec && stale) drop();
        if (exec) return;
        for (EngineSeen& e : engines) e.seen = e.net->plan_version();
        if (!cap_stream) BP_HIP(hipStreamCreateWithFlags(&cap_stream, hipStreamNonBlocking));
        BP_HIP(hipStreamBeginCapture(cap_stream, hipStreamCaptureModeThreadLocal));
        try {
            enqueue(cap_stream);
        } catch (...) {
            hipGraph_t g = nullptr;
            (void)hipStreamEndCapture(cap_stream, &g);
            if (g) (void)hipGraphDestroy(g);
            throw;
        }
        BP_HIP(hipStreamEndCapture(cap_stream, &graph));
        BP_HIP(hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0));
    }
    template <class Enqueue>
    void launch(int use_graph, hipStream_t s, EngineList& engines, Enqueue&& enqueue) {
        if (!use_graph) {
            enqueue(s);
            return;
        }
        capture(engines, enqueue);
        BP_HIP(hipGraphLaunch(exec, s));
    }
};

// Lone-frame latency mode (bp_*_set_prefetch), after a frame was launched on `s`: a launch that found a K slice on the wrong
// XCD raised its engine's error word and left its tile unstored, so the frame's record is void.  The mode is
// one-frame-at-a-time by definition: wait for the frame here, read (and clear) every engine's word, and on a fault switch the
// mode off for all of them and run the SAME frame again on the ordinary hand-off -- whoever drives the chain gets a valid
// record or an error.
template <class Relaunch>
void latency_rerun(EngineList& engines, int device, hipStream_t s, int& faults, Relaunch&& relaunch) {
    bool latency = false;
    for (const EngineSeen& e : engines) latency = latency || e.net->prefetch();
    if (!latency) return;
    BP_HIP(hipSetDevice(device));
    int bad = 0;
    for (EngineSeen& e : engines) bad += e.net->take_xcd_errors(s);
    if (!bad) return;
    ++faults;
    for (EngineSeen& e : engines) e.net->set_prefetch(false);
    relaunch();
}

// ------------------------------------------------------------------ resize stage
// Pillow-exact bicubic stretch of the chain's u8 BGR frames to reso x reso, BGR -> RGB, /255, straight into the detector's
// NHWC input.  frames [n][H][W][3] is the caller's buffer or the arena's.
struct ResizeStage {
    uint8_t* frames = nullptr;
    uint8_t* tmp = nullptr;
    ResizeTables t{};
    void init(Arena& arena, uint8_t* d_frames, int n_frames, int H, int W, int reso) {
        frames = d_frames ? d_frames : (uint8_t*)arena.alloc_bytes((size_t)n_frames * H * W * 3);
        tmp = (uint8_t*)arena.alloc_bytes((size_t)n_frames * H * reso * 3);
        const ResizePlan ph = make_bicubic_plan(W, reso), pv = make_bicubic_plan(H, reso);
        int* hb = (int*)arena.alloc_bytes(ph.bounds.size() * 4);
        int* hk = (int*)arena.alloc_bytes(ph.coeffs.size() * 4);
        int* vb = (int*)arena.alloc_bytes(pv.bounds.size() * 4);
        int* vk = (int*)arena.alloc_bytes(pv.coeffs.size() * 4);
        BP_HIP(hipMemcpy(hb, ph.bounds.data(), ph.bounds.size() * 4, hipMemcpyHostToDevice));
        BP_HIP(hipMemcpy(hk, ph.coeffs.data(), ph.coeffs.size() * 4, hipMemcpyHostToDevice));
        BP_HIP(hipMemcpy(vb, pv.bounds.data(), pv.bounds.size() * 4, hipMemcpyHostToDevice));
        BP_HIP(hipMemcpy(vk, pv.coeffs.data(), pv.coeffs.size() * 4, hipMemcpyHostToDevice));
        t = ResizeTables{hb, hk, ph.ksize, vb, vk, pv.ksize};
    }
    void enqueue(int n_frames, int H, int W, float* dst_nhwc, int reso, hipStream_t s) const {
        launch_resize_bicubic(frames, n_frames, H, W, tmp, dst_nhwc, nullptr, reso, reso, t, 1, s);
    }
};

// ------------------------------------------------------------------ pose solver
inline void check_pose_points(int n_kp, int left_number) {
    BP_CHECK(n_kp == 50, "the pose solver takes one 3-D point per key point (50)");
    BP_CHECK(left_number >= 0, "left_number must be >= 0");
}
inline void check_ransac_params(double reproj_err, int max_trials, double confidence) {
    BP_CHECK(reproj_err > 0 && max_trials >= 1 && confidence > 0 && confidence < 1, "RANSAC parameters out of range");
}
// points the pruning keeps, the same for every frame
inline int pose_points(int left_number) { return left_number < 50 ? left_number : 50; }

// The RANSAC pose tail: workspace = kept 3-D points [batch][64][3] f64 | kept 2-D points [batch][64][2] f64 | the
// hypotheses' masks and counts (pnp_ransac_workspace_bytes) | active [batch] i32.  Three launches: prepare (decode, NMS,
// pruning; the pose row but for the solver's slots), hypotheses, select-and-refit.
inline size_t pose_ransac_ws_bytes(int batch, int max_trials) {
    return (size_t)batch * 64 * 5 * sizeof(double) + pnp_ransac_workspace_bytes(batch, max_trials) + (size_t)batch * sizeof(int);
}
inline void pose_tail_ransac(const float* records, int batch, const double* kp3d, const PnpCam& cam, int left_number,
                             double reproj_err, int max_trials, const int* samples, const int* need, double* poses, void* ws,
                             hipStream_t s) {
    double* ws3d = (double*)ws;
    double* ws2d = ws3d + (size_t)batch * 64 * 3;
    char* hyp = (char*)(ws2d + (size_t)batch * 64 * 2);
    int* active = (int*)(hyp + pnp_ransac_workspace_bytes(batch, max_trials));
    launch_pose_tail_prepare(records, batch, kp3d, cam, left_number, poses, ws3d, ws2d, active, s);
    launch_pnp_ransac(ws3d, 64 * 3, ws2d, 64 * 2, active, pose_points(left_number), batch, cam, reproj_err, max_trials, samples,
                      need, hyp, nullptr, nullptr, nullptr, poses, s);
}
// the host's tables for n points (n > 6: below that the device code reads neither)
inline void ransac_tables(int n, int max_trials, double confidence, std::vector<int>& samples, std::vector<int>& need) {
    samples.assign((size_t)max_trials * 6, 0);
    need.assign((size_t)(n > 0 ? n : 0) + 1, 0x7fffffff);
    if (n > 6) {
        pnp_ransac_samples(n, max_trials, samples.data());
        pnp_ransac_trials_needed(n, confidence, need.data());
    }
}

// The opt-in device pose tail of a chain (or of one scene slot): on while `on`; kp3d [50][3] in the chain's arena, `poses`
// the rows it writes.  RANSAC in place of the plain PnP while ransac_trials > 0; the sampler's and the early stop's tables
// are the host's, for points() points.
struct PoseSolver {
    bool on = false;
    double* kp3d = nullptr;
    double* poses = nullptr;
    PnpCam cam{};
    int left_number = 50;
    int ransac_trials = 0;
    double ransac_err = 0, ransac_conf = 0;
    std::vector<int> ransac_samples, ransac_need;
    void* ransac_ws = nullptr;
    size_t ransac_ws_bytes = 0;

    int points() const { return pose_points(left_number); }
    void off() { on = false; }
    // h_kp3d [n_kp][3] and K [3][3] on the host; rows: the device rows the tail writes (the caller's buffer or the chain's own)
    void set(Arena& arena, int device, const double* h_kp3d, int n_kp, const double* K, int left, double* rows) {
        BP_CHECK(K, "null camera matrix");
        check_pose_points(n_kp, left);
        BP_HIP(hipSetDevice(device));
        if (!kp3d) kp3d = (double*)arena.alloc_bytes(50 * 3 * sizeof(double));
        poses = rows;
        BP_HIP(hipMemcpy(kp3d, h_kp3d, 50 * 3 * sizeof(double), hipMemcpyHostToDevice));
        cam = make_pnp_cam(K);
        left_number = left;
        on = true;
        if (ransac_trials > 0)   // the RANSAC setting stays; its tables are per point count
            ransac_tables(points(), ransac_trials, ransac_conf, ransac_samples, ransac_need);
    }
    // max_trials 0: back to the plain PnP.  Otherwise the solver must be on (the caller checks, with its own message).
    void set_ransac(Arena& arena, int device, int batch, double reproj_err, int max_trials, double confidence) {
        if (max_trials == 0) {
            ransac_trials = 0;
            return;
        }
        check_ransac_params(reproj_err, max_trials, confidence);
        BP_HIP(hipSetDevice(device));
        const size_t bytes = pose_ransac_ws_bytes(batch, max_trials);
        if (bytes > ransac_ws_bytes) {
            ransac_ws = arena.alloc_bytes(bytes);
            ransac_ws_bytes = bytes;
        }
        ransac_err = reproj_err;
        ransac_conf = confidence;
        ransac_tables(points(), max_trials, confidence, ransac_samples, ransac_need);
        ransac_trials = max_trials;
    }
    // decode, pPose-NMS, pruning and PnP on `batch` records just written (pose_tail.hip); nothing while off
    void enqueue(const float* records, int batch, hipStream_t s) const {
        if (!on) return;
        if (ransac_trials > 0)
            pose_tail_ransac(records, batch, kp3d, cam, left_number, ransac_err, ransac_trials, ransac_samples.data(),
                             ransac_need.data(), poses, ransac_ws, s);
        else launch_pose_tail(records, batch, kp3d, cam, left_number, poses, s);
    }
};

// A chain's own pose rows, for a tail that was given no buffer: n rows [166] f64, zeroed, allocated on first use.
inline double* own_pose_rows(Arena& arena, int device, double*& own, size_t n) {
    if (!own) {
        BP_HIP(hipSetDevice(device));
        const size_t bytes = n * BP_POSE_DOUBLES * sizeof(double);
        double* p = (double*)arena.alloc_bytes(bytes);
        BP_HIP(hipMemset(p, 0, bytes));
        own = p;
    }
    return own;
}

}  // namespace bp
