// sf_hip.hpp — the error type and macros of libsfgpu.so, and the one owner of what a context takes from the HIP runtime:
// device memory, pinned host memory, streams and events. Needs the HIP runtime API only (no device code, no RCCL), so a
// plain C++ program can compile it (tests/own_check.cpp does, against stubs of the runtime).
#pragma once
#include "../../include/sfgpu.h"
#include <hip/hip_runtime_api.h>
#include <algorithm>
#include <cstddef>
#include <string>
#include <vector>

namespace sfi {

struct Failure {
    int code;
    std::string msg;
};

#define SF_HIP(expr)                                                                               \
    do {                                                                                           \
        hipError_t _e = (expr);                                                                    \
        if (_e != hipSuccess)                                                                      \
            throw Failure{SF_ERR_HIP, std::string("Error ") + hipGetErrorString(_e) + " at line " + \
                                          std::to_string(__LINE__) + " in file " + __FILE__ +      \
                                          " (" #expr ")"};                                         \
    } while (0)

#define SF_REQUIRE(cond, text)                                          \
    do {                                                                \
        if (!(cond)) throw Failure{SF_ERR_INVALID, std::string(text)};  \
    } while (0)

// Owns everything it hands out until it dies (or, one device block, until release()). What it returns are plain
// pointers and handles: the holder may copy, swap and alias them freely, because nothing is ever freed through them.
// A call that fails throws and registers nothing; a holder whose constructor throws later loses nothing either, since
// this member's destructor still runs.
class Owned {
public:
    explicit Owned(int device) : device_(device) {}
    Owned(const Owned&) = delete;
    Owned& operator=(const Owned&) = delete;

    template <class P>
    P* dev(size_t bytes) {
        dev_.reserve(dev_.size() + 1);  // so that registering cannot fail once the block exists
        void* p = nullptr;
        SF_HIP(hipMalloc(&p, bytes));
        dev_.push_back(p);
        return static_cast<P*>(p);
    }
    template <class P>
    P* pinned(size_t bytes) {
        pinned_.reserve(pinned_.size() + 1);
        void* p = nullptr;
        SF_HIP(hipHostMalloc(&p, bytes, hipHostMallocDefault));
        pinned_.push_back(p);
        return static_cast<P*>(p);
    }
    hipStream_t stream(unsigned flags) {
        streams_.reserve(streams_.size() + 1);
        hipStream_t s = nullptr;
        SF_HIP(hipStreamCreateWithFlags(&s, flags));
        streams_.push_back(s);
        return s;
    }
    hipEvent_t event(unsigned flags) {
        events_.reserve(events_.size() + 1);
        hipEvent_t e = nullptr;
        SF_HIP(hipEventCreateWithFlags(&e, flags));
        events_.push_back(e);
        return e;
    }
    // Frees one device block now; p is the address dev() returned. The caller has made sure nothing on the device
    // still uses it.
    template <class P>
    void release(P*& p) {
        if (!p) return;
        const auto it = std::find(dev_.begin(), dev_.end(), static_cast<const void*>(p));
        SF_REQUIRE(it != dev_.end(), "internal: release of a device block this context does not own");
        dev_.erase(it);
        (void)hipFree(p);
        p = nullptr;
    }

    // Errors are ignored: there is nobody to report them to. An owner that never handed anything out touches no device.
    ~Owned() {
        if (dev_.empty() && pinned_.empty() && streams_.empty() && events_.empty()) return;
        (void)hipSetDevice(device_);
        (void)hipDeviceSynchronize();
        for (hipEvent_t e : events_) (void)hipEventDestroy(e);
        for (hipStream_t s : streams_) (void)hipStreamDestroy(s);
        for (void* p : pinned_) (void)hipHostFree(p);
        for (void* p : dev_) (void)hipFree(p);
    }

private:
    const int device_;
    std::vector<void*> dev_, pinned_;
    std::vector<hipStream_t> streams_;
    std::vector<hipEvent_t> events_;
};

}  // namespace sfi
