// dev_shim_common.hpp -- what every exported function of the device test shims (dev_shim.hip, dev_shim_fields.hip) does
// around its one kernel: host pointers in, a stream of its own, a polling deadline instead of an unbounded synchronise.
#pragma once
#include <hip/hip_runtime.h>
#include <chrono>
#include <cstdlib>
#include <thread>
#include <vector>

namespace {

constexpr int DS_DEADLINE = 9999;   // the kernel did not finish in time (distinct from every hipError_t)
constexpr int DS_BAD_ARG = 9998;
constexpr int MAX_CHAIN = 512;      // no loop of a shim kernel runs longer, whatever the caller passes
constexpr int MAX_BLOCK = 256;      // __launch_bounds__ of every kernel: the tests launch workgroups of 64 and 256 threads

int pick_device() {
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return 0;
    if (const char *v = getenv("CKZG_HIP_DEVICE")) return atoi(v);
    if (const char *v = getenv("LOCAL_RANK")) return atoi(v) % ndev;
    return 0;
}

struct Arg {
    const void *in;   // host source (inputs), or null
    void *out;        // host destination (outputs), or null
    size_t bytes;
    void *dev;
};

template <class Launch>
int run_bounded(std::vector<Arg> &args, Launch &&launch) {
    hipError_t e = hipSetDevice(pick_device());
    if (e != hipSuccess) return (int)e;
    hipStream_t st;
    if ((e = hipStreamCreate(&st)) != hipSuccess) return (int)e;
    int rc = 0;
    for (Arg &a : args) {
        a.dev = nullptr;
        if ((e = hipMalloc(&a.dev, a.bytes ? a.bytes : 4)) != hipSuccess) { rc = (int)e; break; }
        e = a.in ? hipMemcpyAsync(a.dev, a.in, a.bytes, hipMemcpyHostToDevice, st) : hipMemsetAsync(a.dev, 0, a.bytes ? a.bytes : 4, st);
        if (e != hipSuccess) { rc = (int)e; break; }
    }
    if (rc == 0) {
        launch(st);
        if ((e = hipGetLastError()) != hipSuccess) rc = (int)e;
    }
    if (rc == 0) {
        const auto t0 = std::chrono::steady_clock::now();
        for (;;) {
            e = hipStreamQuery(st);
            if (e == hipSuccess) break;
            if (e != hipErrorNotReady) { rc = (int)e; break; }
            if (std::chrono::steady_clock::now() - t0 > std::chrono::seconds(20)) return DS_DEADLINE;   // nothing is freed under a running kernel
            std::this_thread::sleep_for(std::chrono::microseconds(200));
        }
    }
    if (rc == 0)
        for (Arg &a : args)
            if (a.out && (e = hipMemcpy(a.out, a.dev, a.bytes, hipMemcpyDeviceToHost)) != hipSuccess) { rc = (int)e; break; }
    for (Arg &a : args)
        if (a.dev) (void)hipFree(a.dev);
    (void)hipStreamDestroy(st);
    return rc;
}

bool geometry_ok(int n, int block) { return n > 0 && block >= 64 && block <= MAX_BLOCK && block % 64 == 0; }

}  // namespace
