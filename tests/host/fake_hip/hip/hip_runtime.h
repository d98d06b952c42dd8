// A stand-in for <hip/hip_runtime.h> with the host calls csrc/tm_feature_host.h makes (and hipMemcpyAsync, for a compute_async written
// out in the test), for tests/host/feature_host_test.cpp: plain g++, no GPU, no ROCm.  Device and page-locked memory are malloc'ed, so
// that AddressSanitizer sees every leak, double free and copy past an allocation; the fake keeps its own books beside that (what is
// live, how often the stream was waited for, the size of the last allocation) and can make the N-th call fail with a chosen error.
// Frees, destroys and hipGetLastError are not counted as calls and never fail.
#pragma once
#include <cstddef>
#include <cstdlib>
#include <cstring>
#include <set>
#include <string>
#include <vector>

enum hipError_t { hipSuccess = 0, hipErrorInvalidValue = 1, hipErrorOutOfMemory = 2 };
enum hipMemcpyKind { hipMemcpyHostToDevice = 1, hipMemcpyDeviceToHost = 2 };
enum { hipStreamNonBlocking = 1, hipHostMallocDefault = 0 };
struct fakeHipStream { int waits; };
typedef fakeHipStream *hipStream_t;

namespace fake_hip {

struct State {
    long calls = 0;                       // counted calls so far
    long fail_at = -1;                    // the call with this number fails ...
    hipError_t fail_with = hipSuccess;    // ... with this error
    std::string failed;                   // the name of the call that was made to fail
    std::vector<std::string> log;         // the names of the counted calls, in order
    std::set<void *> dev, pinned;         // live allocations
    std::set<hipStream_t> streams;        // live streams
    long bad_frees = 0;                   // frees and destroys of something not live
    long dev_allocs = 0, waits = 0, last_errors_read = 0;
    size_t last_dev_size = 0;
};

inline State &state()
{
    static State s;
    return s;
}

inline void reset(long fail_at = -1, hipError_t fail_with = hipSuccess)
{
    State &s = state();
    for (void *p : s.dev) free(p);
    for (void *p : s.pinned) free(p);
    for (hipStream_t p : s.streams) delete p;
    s = State();
    s.fail_at = fail_at;
    s.fail_with = fail_with;
}

// counts one call; the error it is to fail with, or hipSuccess
inline hipError_t call(const char *name)
{
    State &s = state();
    s.log.push_back(name);
    if (s.calls++ == s.fail_at) {
        s.failed = name;
        return s.fail_with;
    }
    return hipSuccess;
}

} // namespace fake_hip

#define FAKE_HIP_CALL(name)                                           \
    do {                                                              \
        const hipError_t fake_e_ = fake_hip::call(name);              \
        if (fake_e_ != hipSuccess) return fake_e_;                    \
    } while (0)

inline hipError_t hipGetLastError() { ++fake_hip::state().last_errors_read; return hipSuccess; }

inline hipError_t hipGetDevice(int *d) { FAKE_HIP_CALL("hipGetDevice"); *d = 0; return hipSuccess; }
inline hipError_t hipSetDevice(int) { FAKE_HIP_CALL("hipSetDevice"); return hipSuccess; }

inline hipError_t hipStreamCreateWithFlags(hipStream_t *s, unsigned)
{
    *s = (hipStream_t)(void *)&fake_hip::state(); // what a failing call may leave behind: not a stream
    FAKE_HIP_CALL("hipStreamCreateWithFlags");
    *s = new fakeHipStream{0};
    fake_hip::state().streams.insert(*s);
    return hipSuccess;
}

inline hipError_t hipStreamSynchronize(hipStream_t s)
{
    if (!fake_hip::state().streams.count(s)) ++fake_hip::state().bad_frees;
    FAKE_HIP_CALL("hipStreamSynchronize");
    ++fake_hip::state().waits;
    return hipSuccess;
}

inline hipError_t hipStreamDestroy(hipStream_t s)
{
    if (!fake_hip::state().streams.erase(s)) { ++fake_hip::state().bad_frees; return hipErrorInvalidValue; }
    delete s;
    return hipSuccess;
}

inline hipError_t hipMalloc(void **p, size_t n)
{
    FAKE_HIP_CALL("hipMalloc");
    *p = malloc(n);
    fake_hip::state().dev.insert(*p);
    ++fake_hip::state().dev_allocs;
    fake_hip::state().last_dev_size = n;
    return hipSuccess;
}

inline hipError_t hipFree(void *p)
{
    if (!fake_hip::state().dev.erase(p)) { ++fake_hip::state().bad_frees; return hipErrorInvalidValue; }
    free(p);
    return hipSuccess;
}

inline hipError_t hipHostMalloc(void **p, size_t n, unsigned)
{
    *p = &fake_hip::state(); // what a failing call may leave behind: not an allocation
    FAKE_HIP_CALL("hipHostMalloc");
    *p = malloc(n ? n : 1);
    fake_hip::state().pinned.insert(*p);
    return hipSuccess;
}

inline hipError_t hipHostFree(void *p)
{
    if (!fake_hip::state().pinned.erase(p)) { ++fake_hip::state().bad_frees; return hipErrorInvalidValue; }
    free(p);
    return hipSuccess;
}

inline hipError_t hipMemcpyAsync(void *dst, const void *src, size_t n, hipMemcpyKind, hipStream_t)
{
    FAKE_HIP_CALL("hipMemcpyAsync");
    memcpy(dst, src, n);
    return hipSuccess;
}

inline hipError_t hipMemcpy2DAsync(void *dst, size_t dpitch, const void *src, size_t spitch, size_t width, size_t height, hipMemcpyKind, hipStream_t)
{
    FAKE_HIP_CALL("hipMemcpy2DAsync");
    for (size_t r = 0; r < height; ++r) memcpy((char *)dst + r * dpitch, (const char *)src + r * spitch, width);
    return hipSuccess;
}
