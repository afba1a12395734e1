// What the c_api*.cpp units share: the exception -> (-1, bp_last_error()) bracket of every extern "C" body and the engine
// handles.  The error text is ONE thread_local string for the whole library, defined in c_api.cpp beside bp_last_error();
// every unit sets it through set_last_error (a `static thread_local` per file would link too, and bp_last_error() would
// then answer stale text for every unit but its own).
#pragma once
#include "../../include/betapose_hip.h"

#include <exception>
#include <memory>

#include "engine.h"

namespace bp {
#pragma GCC visibility push(hidden)     // the library's own: not in its dynamic symbol table
void set_last_error(const char* text);
#pragma GCC visibility pop
}  // namespace bp

#define BP_TRY try {
#define BP_CATCH                                   \
    }                                              \
    catch (const std::exception& e) {              \
        bp::set_last_error(e.what());              \
        return -1;                                 \
    }                                              \
    catch (...) {                                  \
        bp::set_last_error("unknown error");       \
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

// The argument check of one training convolution, shared by bp_train_conv (sizes 1 and 3) and bp_kpd_train_conv (7 too):
// ONE text for the roles, the shapes, the 2^31 bounds and the launch limits.
inline bool bp_train_conv_size_ok(int size, bool admit_seven) { return size == 1 || size == 3 || (admit_seven && size == 7); }
inline void bp_check_train_conv(int role, const void* x, const void* w, const void* y, int N, int C, int H, int W, int K, int size,
                                int stride, const void* scratch, bool admit_seven) {
    BP_CHECK(role >= 0 && role <= 2, "role must be 0 (forward), 1 (filter gradient) or 2 (input gradient)");
    BP_CHECK(x && w && y && (role != 1 || scratch), "null argument");
    BP_CHECK(N > 0 && C > 0 && H > 0 && W > 0 && K > 0, "N, C, H, W and K must be positive");
    BP_CHECK(bp_train_conv_size_ok(size, admit_seven), admit_seven ? "size must be 1, 3 or 7" : "size must be 1 or 3");
    BP_CHECK(stride == 1 || stride == 2, "stride must be 1 or 2");
    const long long OH = (H + 2 * (size / 2) - size) / stride + 1, OW = (W + 2 * (size / 2) - size) / stride + 1;
    const long long lim = 1ll << 31;
    BP_CHECK((long long)N * C * H * W < lim && (long long)N * K * OH * OW < lim && (long long)K * C * size * size < lim,
             "a tensor of 2^31 elements or more");
    BP_CHECK((long long)(K > C ? K : C) <= 64ll * 65535 && (long long)N * OH * OW <= 2048ll * 65535, "shape too large for one launch");
}
