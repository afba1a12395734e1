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
