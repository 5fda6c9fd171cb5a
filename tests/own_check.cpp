// own_check.cpp — sfi::Owned (fluidsolvergpu_amd/csrc/sf_hip.hpp) against stubs of the HIP runtime: what is freed, when,
// in which order, and what a failing call leaves behind. Stand-alone: needs no GPU, no libamdhip64 and no libsfgpu.so.
//   g++ -std=c++17 -D__HIP_PLATFORM_AMD__ -I<rocm>/include tests/own_check.cpp -o own_check && ./own_check
// (tests/test_own_cpu.py does that.) Exit status 0: every check held and nothing is left alive.
#include "../fluidsolvergpu_amd/csrc/sf_hip.hpp"

#include <cstdio>
#include <cstdlib>
#include <set>

#define CHECK(cond)                                                              \
    do {                                                                         \
        if (!(cond)) {                                                           \
            std::fprintf(stderr, "own_check.cpp:%d: %s\n", __LINE__, #cond);     \
            std::exit(1);                                                        \
        }                                                                        \
    } while (0)

// ---- the stub runtime: malloc / free behind the eleven functions sf_hip.hpp calls ----------------------------------
namespace stub {
enum Kind { DEV, PINNED, STREAM, EVENT, NKINDS };
std::set<void*> live[NKINDS];
std::vector<std::string> calls;  // one entry per call, in order
int malloc_calls = 0;            // calls of hipMalloc so far
int fail_malloc_at = 0;          // the n-th call of hipMalloc (from 1) fails; 0: none

size_t alive(Kind k) { return live[k].size(); }
bool all_freed() { return !alive(DEV) && !alive(PINNED) && !alive(STREAM) && !alive(EVENT); }
void reset() {
    CHECK(all_freed());
    calls.clear();
    malloc_calls = fail_malloc_at = 0;
}
hipError_t make(Kind k, const char* name, void** out, size_t bytes) {
    calls.push_back(name);
    *out = std::malloc(bytes ? bytes : 1);
    live[k].insert(*out);
    return hipSuccess;
}
hipError_t drop(Kind k, const char* name, void* p) {
    calls.push_back(name);
    if (!live[k].erase(p)) {  // freed twice, or never handed out
        std::fprintf(stderr, "own_check.cpp: %s of %p, which is not alive\n", name, p);
        std::abort();
    }
    std::free(p);
    return hipSuccess;
}
size_t count(const char* name) {
    size_t n = 0;
    for (const std::string& c : calls) n += c == name;
    return n;
}
}  // namespace stub

extern "C" {
hipError_t hipMalloc(void** ptr, size_t size) {
    if (++stub::malloc_calls == stub::fail_malloc_at) {
        stub::calls.push_back("hipMalloc(failed)");
        return hipErrorOutOfMemory;
    }
    return stub::make(stub::DEV, "hipMalloc", ptr, size);
}
hipError_t hipFree(void* ptr) { return stub::drop(stub::DEV, "hipFree", ptr); }
hipError_t hipHostMalloc(void** ptr, size_t size, unsigned int) { return stub::make(stub::PINNED, "hipHostMalloc", ptr, size); }
hipError_t hipHostFree(void* ptr) { return stub::drop(stub::PINNED, "hipHostFree", ptr); }
hipError_t hipStreamCreateWithFlags(hipStream_t* s, unsigned int) {
    return stub::make(stub::STREAM, "hipStreamCreateWithFlags", reinterpret_cast<void**>(s), 1);
}
hipError_t hipStreamDestroy(hipStream_t s) { return stub::drop(stub::STREAM, "hipStreamDestroy", s); }
hipError_t hipEventCreateWithFlags(hipEvent_t* e, unsigned) {
    return stub::make(stub::EVENT, "hipEventCreateWithFlags", reinterpret_cast<void**>(e), 1);
}
hipError_t hipEventDestroy(hipEvent_t e) { return stub::drop(stub::EVENT, "hipEventDestroy", e); }
hipError_t hipSetDevice(int) {
    stub::calls.push_back("hipSetDevice");
    return hipSuccess;
}
hipError_t hipDeviceSynchronize(void) {
    stub::calls.push_back("hipDeviceSynchronize");
    return hipSuccess;
}
const char* hipGetErrorString(hipError_t e) { return e == hipErrorOutOfMemory ? "out of memory" : "error"; }
}

using sfi::Failure;
using sfi::Owned;

// ---- 1. everything goes when the owner goes: synchronise, events, streams, memory ----------------------------------
static void check_scope_exit() {
    stub::reset();
    {
        Owned own(0);
        for (int q = 0; q < 3; ++q) {  // interleaved, so the order at the end is not the order of creation
            CHECK(own.dev<float>(64) != nullptr);
            CHECK(own.stream(hipStreamNonBlocking) != nullptr);
            CHECK(own.pinned<double>(32) != nullptr);
            CHECK(own.event(hipEventDisableTiming) != nullptr);
        }
        CHECK(stub::alive(stub::DEV) == 3 && stub::alive(stub::PINNED) == 3);
        CHECK(stub::alive(stub::STREAM) == 3 && stub::alive(stub::EVENT) == 3);
        stub::calls.clear();
    }
    CHECK(stub::all_freed());
    const std::vector<std::string> want = {
        "hipSetDevice",     "hipDeviceSynchronize", "hipEventDestroy", "hipEventDestroy", "hipEventDestroy",
        "hipStreamDestroy", "hipStreamDestroy",     "hipStreamDestroy", "hipHostFree",    "hipHostFree",
        "hipHostFree",      "hipFree",              "hipFree",          "hipFree"};
    CHECK(stub::calls == want);
}

// ---- 2. a holder whose constructor throws after some allocations loses nothing -------------------------------------
struct Holder {
    Owned own;
    float* a = nullptr;
    hipStream_t s = nullptr;
    explicit Holder(bool fail) : own(0) {
        a = own.dev<float>(128);
        s = own.stream(hipStreamNonBlocking);
        (void)own.event(hipEventDisableTiming);
        (void)own.pinned<int>(16);
        SF_REQUIRE(!fail, "the constructor fails here");
    }
};
static void check_throwing_constructor() {
    stub::reset();
    bool caught = false;
    try {
        Holder h(true);
    } catch (const Failure& f) {
        caught = f.code == SF_ERR_INVALID;
    }
    CHECK(caught && stub::all_freed());
    CHECK(stub::count("hipFree") == 1 && stub::count("hipStreamDestroy") == 1);
    CHECK(stub::count("hipEventDestroy") == 1 && stub::count("hipHostFree") == 1);
}

// ---- 3. a failing allocation throws, registers nothing, and the earlier blocks are freed once ----------------------
static void check_failing_allocation() {
    stub::reset();
    stub::fail_malloc_at = 3;
    {
        Owned own(0);
        (void)own.dev<char>(8);
        (void)own.dev<char>(8);
        int code = 0;
        try {
            (void)own.dev<char>(8);
        } catch (const Failure& f) {
            code = f.code;
            CHECK(f.msg.find("out of memory") != std::string::npos);
        }
        CHECK(code == SF_ERR_HIP);
        CHECK(stub::alive(stub::DEV) == 2);
        (void)own.dev<char>(8);  // the owner is still usable
    }
    CHECK(stub::all_freed());
    CHECK(stub::count("hipMalloc") == 3 && stub::count("hipFree") == 3);  // a double free would have aborted
}

// ---- 4. release frees that block now, nulls the pointer, takes null; nothing is freed again later ------------------
static void check_release() {
    stub::reset();
    {
        Owned own(0);
        float* a = own.dev<float>(8);
        void* b = own.dev<void>(8);
        float* none = nullptr;
        own.release(none);
        CHECK(none == nullptr && stub::count("hipFree") == 0);
        void* const was = a;
        own.release(a);
        CHECK(a == nullptr && stub::count("hipFree") == 1);
        CHECK(!stub::live[stub::DEV].count(was) && stub::live[stub::DEV].count(b));
        own.release(a);  // null by now
        CHECK(stub::count("hipFree") == 1);
    }
    CHECK(stub::all_freed() && stub::count("hipFree") == 2);
}

// ---- 5. release of an address the owner never handed out throws and frees nothing ----------------------------------
static void check_release_unknown() {
    stub::reset();
    {
        Owned own(0);
        char* a = own.dev<char>(256);
        char* inside = a + 16;  // a view into a block is not the block
        char elsewhere = 0;
        char* stray = &elsewhere;
        for (char** p : {&inside, &stray}) {
            char* const before = *p;
            bool caught = false;
            try {
                own.release(*p);
            } catch (const Failure& f) {
                caught = f.code == SF_ERR_INVALID;
            }
            CHECK(caught && *p == before && stub::count("hipFree") == 0);
        }
        CHECK(stub::alive(stub::DEV) == 1);
    }
    CHECK(stub::all_freed() && stub::count("hipFree") == 1);
}

// ---- 6. allocate-if-null, repeated after a failure halfway: each block exists once ---------------------------------
struct Lazy {
    Owned own{0};
    int* a = nullptr;
    int* b = nullptr;
    int* c = nullptr;
    double* host = nullptr;
    void alloc() {
        if (!a) a = own.dev<int>(4);
        if (!b) b = own.dev<int>(4);
        if (!c) c = own.dev<int>(4);
        if (!host) host = own.pinned<double>(8);
    }
};
static void check_allocate_if_null() {
    stub::reset();
    stub::fail_malloc_at = 2;
    {
        Lazy l;
        bool caught = false;
        try {
            l.alloc();
        } catch (const Failure&) {
            caught = true;
        }
        CHECK(caught && l.a && !l.b && !l.c && !l.host);
        int* const a = l.a;
        l.alloc();
        CHECK(l.a == a && l.b && l.c && l.host);
        l.alloc();  // and a third time changes nothing
        CHECK(stub::alive(stub::DEV) == 3 && stub::alive(stub::PINNED) == 1);
        CHECK(stub::count("hipMalloc") == 3 && stub::count("hipHostMalloc") == 1);
    }
    CHECK(stub::all_freed() && stub::count("hipFree") == 3 && stub::count("hipHostFree") == 1);
}

// an owner that handed nothing out touches no device when it goes
static void check_idle_owner() {
    stub::reset();
    { Owned own(7); }
    CHECK(stub::calls.empty());
}

int main() {
    check_scope_exit();
    check_throwing_constructor();
    check_failing_allocation();
    check_release();
    check_release_unknown();
    check_allocate_if_null();
    check_idle_owner();
    CHECK(stub::all_freed());
    std::puts("own_check ok");
    return 0;
}
