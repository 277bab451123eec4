// abi.hpp -- the C-ABI boundary shared by every handle kind of libcarskit_mi355x.so (instance, FM, KNN, group, DAO): error
// messages, the exception barrier, the create-time device check and the device-buffer helpers.  Internal.
#pragma once
#include "../../include/carskit_mi355x.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdarg>
#include <cstdio>
#include <exception>
#include <string>
#include <utility>
#include <vector>

// a message into a handle's (or a thread's) error string; never throws: without memory for it the string is left empty
inline void abi_set_err(std::string &err, const char *msg) noexcept {
    try {
        err = msg;
    } catch (...) {
        err.clear();
    }
}

// a printf-style message into err; returns code
__attribute__((format(printf, 3, 4))) inline int abi_fail(std::string &err, int code, const char *fmt, ...) noexcept {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    abi_set_err(err, buf);
    return code;
}

// fail with a message in (h)->err: works for every handle kind (a struct with a std::string err)
#define CMI_FAIL(h, code, ...) return abi_fail((h)->err, (code), __VA_ARGS__)

#define CMI_HIP(h, expr)                                                                                \
    do {                                                                                                \
        hipError_t e_ = (expr);                                                                         \
        if (e_ != hipSuccess) CMI_FAIL(h, CMI_E_HIP, "%s failed: %s", #expr, hipGetErrorString(e_));   \
    } while (0)

// where cmi_last_error(NULL) reads: the last failure on this thread of cmi_create or of a handle-less cmi_* function (cmi_api.cpp)
std::string &cmi_thread_err();

struct abi_no_cleanup {
    void operator()() const noexcept {}
};

// The exception barrier: nothing C++ may cross into a C / JNI / ctypes host (the host pool hands a range body's exception to its
// caller, host_pool.hpp).  Runs body(); an exception that reaches this point runs on_fail(), leaves "<what>: host-side failure: ..."
// in `err` and returns `failed`.
template <typename R, typename Body, typename OnFail = abi_no_cleanup>
R abi_barrier_or(R failed, std::string &err, const char *what, Body &&body, OnFail &&on_fail = {}) noexcept {
    char buf[512];
    try {
        return body();
    } catch (const std::exception &e) {
        snprintf(buf, sizeof buf, "%s: host-side failure: %s", what, e.what());
    } catch (...) {
        snprintf(buf, sizeof buf, "%s: host-side failure (unknown exception)", what);
    }
    on_fail();
    abi_set_err(err, buf);
    return failed;
}

// the barrier of a function that returns a status: CMI_E_HOST on an exception
template <typename Body, typename OnFail = abi_no_cleanup>
int abi_barrier(std::string &err, const char *what, Body &&body, OnFail &&on_fail = {}) noexcept {
    return abi_barrier_or<int>(CMI_E_HOST, err, what, std::forward<Body>(body), std::forward<OnFail>(on_fail));
}

// create time: `device` names a visible device (there is no CPU path to fall back to)
inline int abi_check_device(std::string &err, const char *fn, int device) {
    const int ndev = cmi_device_count();
    if (ndev <= 0) return abi_fail(err, CMI_E_NO_DEVICE, "%s: no HIP device visible (libcarskit_mi355x has no CPU fallback)", fn);
    if (device < 0 || device >= ndev) return abi_fail(err, CMI_E_INVALID, "%s: device index out of range", fn);
    return CMI_OK;
}

// count elements to a new device buffer, the copy enqueued on stream s (the caller keeps src alive until s has run it).  count == 0:
// *dst = nullptr, or with min_one a one-element buffer left unwritten (for kernels that take a non-null pointer)
template <typename D, typename V>
hipError_t abi_upload(D **dst, const V *src, size_t count, hipStream_t s, bool min_one = false) {
    *dst = nullptr;
    if (!count && !min_one) return hipSuccess;
    hipError_t e = hipMalloc((void **)dst, std::max<size_t>(count, 1) * sizeof(V));
    if (e == hipSuccess && count) e = hipMemcpyAsync((void *)*dst, src, count * sizeof(V), hipMemcpyHostToDevice, s);
    return e;
}
template <typename D, typename V>
hipError_t abi_upload(D **dst, const std::vector<V> &v, hipStream_t s, bool min_one = false) {
    return abi_upload(dst, v.data(), v.size(), s, min_one);
}

// hipFree every non-null device pointer of the list and null it
template <typename... T>
void abi_free(T *&...p) {
    auto one = [](auto *&q) {
        if (q) (void)hipFree((void *)q);
        q = nullptr;
    };
    (one(p), ...);
}
