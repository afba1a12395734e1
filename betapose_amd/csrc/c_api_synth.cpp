// extern "C" boundary, the training-scene synthesiser: backgrounds, the composite and the depth-sensor model, host and
// device -- see include/betapose_hip.h.  Every function checks its arguments and makes one bp:: call: the host twin
// (synth_host.cpp) or the launcher (synth.hip).  What a host / device pair checks alike is stated once, in the check
// functions; the per-image tables are host memory in both, so their values are checked here for both.
#include "c_api_util.h"
#include "synth.h"

static void synth_check_images(int I, int H, int W) {
    BP_CHECK(I > 0 && H > 0 && W > 0, "I, H and W must be positive");
    BP_CHECK(H <= bp::SY_MAX_SIDE && W <= bp::SY_MAX_SIDE, "H and W must not exceed 32768");
    BP_CHECK((long long)H * W <= (1ll << 24), "H * W must not exceed 2^24");
}

static void synth_check_windows(const int* windows, int I, int Nb, int Hb, int Wb) {
    BP_CHECK(Nb > 0 && Hb > 0 && Wb > 0, "Nb, Hb and Wb must be positive");
    BP_CHECK(Hb <= bp::SY_MAX_SIDE && Wb <= bp::SY_MAX_SIDE, "Hb and Wb must not exceed 32768");
    for (int i = 0; i < I; ++i) {
        const int* w = windows + (size_t)i * bp::SY_WINDOW;
        BP_CHECK(w[0] >= 0 && w[0] < Nb, "a window names an image outside the bank");
        BP_CHECK(w[3] > 0 && w[4] > 0 && w[1] >= 0 && w[2] >= 0 && w[1] <= Wb - w[3] && w[2] <= Hb - w[4],
                 "a window must lie inside its bank image");
    }
}

static void synth_check_compose(const int* params, int I) {
    for (int i = 0; i < I; ++i) {
        const int* p = params + (size_t)i * bp::SY_PARAMS;
        BP_CHECK(p[0] == 0 || p[0] == 1, "feather must be 0 or 1");
        BP_CHECK(p[1] >= 0 && p[1] <= bp::SY_MAX_RADIUS, "the blur radius must be 0, 1 or 2");
        for (int c = 0; c < 3; ++c) {
            BP_CHECK(p[2 + c] >= 0 && p[2 + c] <= 4096, "a gain must lie in 0 .. 4096 (Q8)");
            BP_CHECK(p[5 + c] >= -255 && p[5 + c] <= 255, "an offset must lie in -255 .. 255");
        }
        BP_CHECK(p[8] >= 0 && p[8] <= 16384, "sigma must lie in 0 .. 16384 (Q8)");
    }
}

static void synth_check_sensor(const int* params, int I, double depth_scale) {
    BP_CHECK(depth_scale > 0.0, "depth_scale must be positive");
    for (int i = 0; i < I; ++i) {
        const int* p = params + (size_t)i * bp::SY_DEPTH_PARAMS;
        BP_CHECK(p[0] >= 0 && p[0] <= 65535, "noise_k must lie in 0 .. 65535");
        BP_CHECK(p[1] >= 0, "edge_counts must not be negative");
        BP_CHECK(p[2] >= 0 && p[2] <= 256, "hole_p must lie in 0 .. 256");
    }
}

static void synth_check_instances(int J, int I, int H, int W) {
    BP_CHECK(I > 0 && H > 0 && W > 0, "I, H and W must be positive");
    BP_CHECK(J >= 1 && J <= bp::SY_INST_MAX, "J must lie in 1 .. 32");
    BP_CHECK((long long)H * W <= (1ll << 24), "H * W must not exceed 2^24");
    BP_CHECK((long long)I * J < (1ll << 28), "I * J must be below 2^28");
}

extern "C" {

int bp_synth_background_host(int I, int H, int W, unsigned seed, unsigned first_image, unsigned char* out) {
    BP_TRY
    BP_CHECK(out, "null argument");
    synth_check_images(I, H, W);
    bp::synth_background_host(I, H, W, seed, first_image, out);
    return 0;
    BP_CATCH
}

int bp_synth_background(int I, int H, int W, unsigned seed, unsigned first_image, unsigned char* d_out, void* stream) {
    BP_TRY
    BP_CHECK(d_out, "null argument");
    synth_check_images(I, H, W);
    bp::launch_synth_background(I, H, W, seed, first_image, d_out, (hipStream_t)stream);
    return 0;
    BP_CATCH
}

int bp_synth_windows_host(const unsigned char* bank, int Nb, int Hb, int Wb, const int* windows, int I, int H, int W,
                          unsigned char* out) {
    BP_TRY
    BP_CHECK(bank && windows && out, "null argument");
    synth_check_images(I, H, W);
    synth_check_windows(windows, I, Nb, Hb, Wb);
    bp::synth_windows_host(bank, Hb, Wb, windows, I, H, W, out);
    return 0;
    BP_CATCH
}

int bp_synth_windows(const unsigned char* d_bank, int Nb, int Hb, int Wb, const int* windows, int I, int H, int W,
                     unsigned char* d_out, void* stream) {
    BP_TRY
    BP_CHECK(d_bank && windows && d_out, "null argument");
    synth_check_images(I, H, W);
    synth_check_windows(windows, I, Nb, Hb, Wb);
    bp::launch_synth_windows(d_bank, Hb, Wb, windows, I, H, W, d_out, (hipStream_t)stream);
    return 0;
    BP_CATCH
}

int bp_synth_compose_host(const unsigned char* background, const unsigned char* color, const float* depth, int I, int H, int W,
                          const int* params, unsigned seed, unsigned first_image, unsigned char* out) {
    BP_TRY
    BP_CHECK(background && color && depth && params && out, "null argument");
    synth_check_images(I, H, W);
    synth_check_compose(params, I);
    bp::synth_compose_host(background, color, depth, I, H, W, params, seed, first_image, out);
    return 0;
    BP_CATCH
}

int bp_synth_compose(const unsigned char* d_background, const unsigned char* d_color, const float* d_depth, int I, int H, int W,
                     const int* params, unsigned seed, unsigned first_image, unsigned char* d_out, void* stream) {
    BP_TRY
    BP_CHECK(d_background && d_color && d_depth && params && d_out, "null argument");
    BP_CHECK(d_out != d_background && d_out != d_color, "the output must not be an input: blocks read their neighbours' pixels");
    synth_check_images(I, H, W);
    synth_check_compose(params, I);
    bp::launch_synth_compose(d_background, d_color, d_depth, I, H, W, params, seed, first_image, d_out, (hipStream_t)stream);
    return 0;
    BP_CATCH
}

int bp_synth_sensor_depth_host(const float* depth, int I, int H, int W, double depth_scale, const int* params, unsigned seed,
                               unsigned first_image, uint16_t* out) {
    BP_TRY
    BP_CHECK(depth && params && out, "null argument");
    synth_check_images(I, H, W);
    synth_check_sensor(params, I, depth_scale);
    bp::synth_sensor_depth_host(depth, I, H, W, depth_scale, params, seed, first_image, out);
    return 0;
    BP_CATCH
}

int bp_synth_sensor_depth(const float* d_depth, int I, int H, int W, double depth_scale, const int* params, unsigned seed,
                          unsigned first_image, uint16_t* d_out, void* stream) {
    BP_TRY
    BP_CHECK(d_depth && params && d_out, "null argument");
    synth_check_images(I, H, W);
    synth_check_sensor(params, I, depth_scale);
    bp::launch_synth_sensor_depth(d_depth, I, H, W, depth_scale, params, seed, first_image, d_out, (hipStream_t)stream);
    return 0;
    BP_CATCH
}

int bp_synth_instances_host(const float* alone, int J, int I, int H, int W, const unsigned char* present, unsigned char* ids,
                            float* depth, int* stats) {
    BP_TRY
    BP_CHECK(alone && present && ids && depth && stats, "null argument");
    synth_check_instances(J, I, H, W);
    bp::synth_instances_host(alone, J, I, H, W, present, ids, depth, stats);
    return 0;
    BP_CATCH
}

int bp_synth_instances(const float* d_alone, int J, int I, int H, int W, const unsigned char* d_present, unsigned char* d_ids,
                       float* d_depth, int* d_stats, void* stream) {
    BP_TRY
    BP_CHECK(d_alone && d_present && d_ids && d_depth && d_stats, "null argument");
    BP_CHECK(d_depth != d_alone, "the output must not be an input: a plane is read again after the depth is written");
    synth_check_instances(J, I, H, W);
    bp::launch_synth_instances(d_alone, J, I, H, W, d_present, d_ids, d_depth, d_stats, (hipStream_t)stream);
    return 0;
    BP_CATCH
}

}  // extern "C"
