// abi.hpp -- the C-ABI boundary shared by every handle kind of libcarskit_mi355x.so (instance, FM, KNN, group, DAO): error
// messages, the exception barrier, the create-time device check, the device-buffer helpers and the prediction batch.  Internal.
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

// a HIP status as a C-ABI status: on a failure "<fn>: <HIP's message>" in err
inline int abi_hip(std::string &err, const char *fn, hipError_t e) {
    return e == hipSuccess ? CMI_OK : abi_fail(err, CMI_E_HIP, "%s: %s", fn, hipGetErrorString(e));
}

// Validated tuples on the device: two id arrays, for a contextual model the context ids, and for an evaluation the ratings and room for
// the kernel's block partials.  The transient set of a predict_batch / eval_ratings call, or the resident set of cmi_set_eval_ratings.
struct AbiTuples {
    int32_t *a = nullptr, *b = nullptr, *c = nullptr; // user, item (KNN: owner, target), context: n each; c may be null
    double *r = nullptr, *part = nullptr;             // n ratings and part_doubles partials, or both null
    int64_t n = 0;
    AbiTuples() = default;
    AbiTuples(const AbiTuples &) = delete; // the buffers have one owner, which calls release()
    AbiTuples &operator=(const AbiTuples &) = delete;
    // count > 0 tuples; the copies are enqueued on s, which the caller drains before the host arrays go.  hc and hr may be null: no
    // buffer.  Every buffer (out too: n doubles for the predictions, null: none) is allocated before the first copy is enqueued
    hipError_t upload(int64_t count, const int32_t *ha, const int32_t *hb, const int32_t *hc, const double *hr, size_t part_doubles,
                      double **out, hipStream_t s) {
        n = count;
        const size_t ids = (size_t)n * sizeof(int32_t), vals = (size_t)n * sizeof(double);
        hipError_t e = hipMalloc((void **)&a, ids);
        if (e == hipSuccess) e = hipMalloc((void **)&b, ids);
        if (e == hipSuccess && hc) e = hipMalloc((void **)&c, ids);
        if (e == hipSuccess && hr) e = hipMalloc((void **)&r, vals);
        if (e == hipSuccess && out) e = hipMalloc((void **)out, vals);
        if (e == hipSuccess && hr) e = hipMalloc((void **)&part, part_doubles * sizeof(double));
        if (e == hipSuccess) e = hipMemcpyAsync(a, ha, ids, hipMemcpyHostToDevice, s);
        if (e == hipSuccess) e = hipMemcpyAsync(b, hb, ids, hipMemcpyHostToDevice, s);
        if (e == hipSuccess && hc) e = hipMemcpyAsync(c, hc, ids, hipMemcpyHostToDevice, s);
        if (e == hipSuccess && hr) e = hipMemcpyAsync(r, hr, vals, hipMemcpyHostToDevice, s);
        return e;
    }
    void release() {
        abi_free(a, b, c, r, part);
        n = 0;
    }
};

// predict_batch (and eval_ratings) of n > 0 checked tuples, for every handle kind (a struct with err, device and stream): the tuples
// uploaded, launch(tuples, d_out) -- a C-ABI status -- enqueued on h->stream, out (n doubles; null: no d_out) copied back.  The stream is
// drained before anything is freed, whatever failed: the uploads read the host arrays until then.
template <typename H, typename Launch>
int abi_predict(H *h, const char *fn, int64_t n, const int32_t *a, const int32_t *b, const int32_t *c, const double *r, size_t part_doubles,
                double *out, Launch &&launch) {
    if (int rc = abi_hip(h->err, fn, hipSetDevice(h->device))) return rc;
    AbiTuples t;
    double *d_out = nullptr;
    int rc = CMI_OK;
    hipError_t e = t.upload(n, a, b, c, r, part_doubles, out ? &d_out : nullptr, h->stream);
    if (e == hipSuccess) rc = launch(t, d_out);
    if (e == hipSuccess && rc == CMI_OK && out) e = hipMemcpyAsync(out, d_out, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, h->stream);
    const hipError_t es = hipStreamSynchronize(h->stream);
    if (e == hipSuccess) e = es;
    t.release();
    abi_free(d_out);
    return rc != CMI_OK ? rc : abi_hip(h->err, fn, e);
}
