// Training-scene synthesiser: the declarations shared by synth_host.cpp, synth.hip and c_api_synth.cpp, so a signature
// that drifts fails to compile.  Needs no HIP header (synth_host.cpp is plain C++): the stream type is declared as
// hip_runtime_api.h declares it.  The arithmetic is synth_math.inc, which both units include.
#pragma once
#include <cstddef>
#include <cstdint>

typedef struct ihipStream_t* hipStream_t;

namespace bp {

constexpr int SY_PARAMS = 9;          // compose row: feather, r, gain[3] (Q8), offset[3], sigma (Q8)
constexpr int SY_DEPTH_PARAMS = 3;    // sensor row: noise_k, edge_counts, hole_p
constexpr int SY_WINDOW = 6;          // window row: bank image, x0, y0, w, h, flip
constexpr int SY_MAX_SIDE = 32768;    // H and W: a lattice node index keeps 14 bits per axis
constexpr int SY_MAX_RADIUS = 2;
constexpr int SY_INST_STATS = 10;     // instance row: px_all, px_visib, full box, visible box (xmin, xmax, ymin, ymax each)
constexpr int SY_INST_MAX = 32;       // objects of one instance call

// ---- synth_host.cpp: the host twins, all pointers host; the tables are the callers' (checked there).  Images
// [I][H][W][3] uint8, depth [I][H][W] f32, counts [I][H][W] uint16.  Image i of a call is scene first_image + i.
void synth_background_host(int I, int H, int W, uint32_t seed, uint32_t first_image, unsigned char* out);
void synth_windows_host(const unsigned char* bank, int Hb, int Wb, const int* windows, int I, int H, int W, unsigned char* out);
void synth_compose_host(const unsigned char* background, const unsigned char* color, const float* depth, int I, int H, int W,
                        const int* params, uint32_t seed, uint32_t first_image, unsigned char* out);
void synth_sensor_depth_host(const float* depth, int I, int H, int W, double depth_scale, const int* params, uint32_t seed,
                             uint32_t first_image, uint16_t* out);

// ---- synth.hip: the same on device pointers, enqueued on s; the tables stay HOST pointers (they travel as kernel
// arguments, a chunk of images per launch)
void launch_synth_background(int I, int H, int W, uint32_t seed, uint32_t first_image, unsigned char* out, hipStream_t s);
void launch_synth_windows(const unsigned char* bank, int Hb, int Wb, const int* windows, int I, int H, int W, unsigned char* out,
                          hipStream_t s);
void launch_synth_compose(const unsigned char* background, const unsigned char* color, const float* depth, int I, int H, int W,
                          const int* params, uint32_t seed, uint32_t first_image, unsigned char* out, hipStream_t s);
void launch_synth_sensor_depth(const float* depth, int I, int H, int W, double depth_scale, const int* params, uint32_t seed,
                               uint32_t first_image, uint16_t* out, hipStream_t s);

// ---- synth_inst_host.cpp / synth_inst.hip: who owns each pixel of a scene of J objects rendered alone (alone
// [J][I][H][W] f32, present [I][J] uint8 -> ids [I][H][W] uint8, depth [I][H][W] f32, stats [I][J][SY_INST_STATS] int32;
// the arithmetic is synth_inst_math.inc).  The device form accumulates in `stats` itself and needs no workspace.
void synth_instances_host(const float* alone, int J, int I, int H, int W, const unsigned char* present, unsigned char* ids,
                          float* depth, int* stats);
void launch_synth_instances(const float* alone, int J, int I, int H, int W, const unsigned char* present, unsigned char* ids,
                            float* depth, int* stats, hipStream_t s);

}  // namespace bp
