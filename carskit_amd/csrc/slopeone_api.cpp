// slopeone_api.cpp -- C ABI of SlopeOne (include/carskit_mi355x.h, cmi_slope_*).
#include "../../include/carskit_mi355x.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <numeric>
#include <string>
#include <vector>

#include "abi.hpp"
#include "slopeone_kernels.hpp"

using namespace cmi;

struct cmi_slope_instance {
    int n_users = 0, n_items = 0, device = 0;
    std::string err;
    hipStream_t stream = nullptr;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    // cols: item -> (user, value), for the build; rows: user -> (item, value), for the prediction.  Both CSR, ascending.
    int32_t *d_cptr = nullptr, *d_cidx = nullptr, *d_rptr = nullptr, *d_ridx = nullptr, *d_card = nullptr;
    double *d_cval = nullptr, *d_rval = nullptr, *d_dev = nullptr;
    bool have_ratings = false, built = false;
    float build_ms = 0.f;
};

static thread_local std::string g_slope_create_err;

extern "C" const char *cmi_slope_last_error(cmi_slope_handle h) { return h ? h->err.c_str() : g_slope_create_err.c_str(); }

static void slope_free_ratings(cmi_slope_instance *h) {
    abi_free(h->d_cptr, h->d_cidx, h->d_rptr, h->d_ridx, h->d_card, h->d_cval, h->d_rval, h->d_dev);
    h->have_ratings = h->built = false;
}

extern "C" int cmi_slope_destroy(cmi_slope_handle h) {
    if (!h) return CMI_OK;
    (void)hipSetDevice(h->device);
    if (h->stream) (void)hipStreamSynchronize(h->stream);
    slope_free_ratings(h);
    if (h->ev0) (void)hipEventDestroy(h->ev0);
    if (h->ev1) (void)hipEventDestroy(h->ev1);
    if (h->stream) (void)hipStreamDestroy(h->stream);
    delete h;
    return CMI_OK;
}

extern "C" int cmi_slope_create(int n_users, int n_items, int device, unsigned flags, cmi_slope_handle *out) {
    (void)flags;
    return abi_barrier(g_slope_create_err, "cmi_slope_create", [&] {
        if (out) *out = nullptr;
        if (!out || n_users <= 0 || n_items <= 0) {
            g_slope_create_err = "cmi_slope_create: invalid argument";
            return CMI_E_INVALID;
        }
        if (int rc = abi_check_device(g_slope_create_err, "cmi_slope_create", device)) return rc;
        cmi_slope_instance *h = new cmi_slope_instance();
        h->n_users = n_users;
        h->n_items = n_items;
        h->device = device;
        hipError_t e = hipSetDevice(device);
        if (e == hipSuccess) e = hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking);
        if (e == hipSuccess) e = hipEventCreate(&h->ev0);
        if (e == hipSuccess) e = hipEventCreate(&h->ev1);
        if (e != hipSuccess) {
            g_slope_create_err = std::string("cmi_slope_create: ") + hipGetErrorString(e);
            cmi_slope_destroy(h);
            return CMI_E_HIP;
        }
        *out = h;
        return CMI_OK;
    });
}

// CSR of (row, col, value) cells, rows ascending, columns ascending inside a row
static void slope_csr(int64_t n, int n_rows, const int32_t *row, const int32_t *col, const double *r, std::vector<int32_t> &ptr,
                      std::vector<int32_t> &idx, std::vector<double> &val) {
    ptr.assign((size_t)n_rows + 1, 0);
    for (int64_t t = 0; t < n; ++t) ++ptr[(size_t)row[t] + 1];
    for (int i = 0; i < n_rows; ++i) ptr[(size_t)i + 1] += ptr[(size_t)i];
    std::vector<int64_t> ord((size_t)n);
    std::iota(ord.begin(), ord.end(), 0);
    std::sort(ord.begin(), ord.end(), [&](int64_t a, int64_t b) { return row[a] != row[b] ? row[a] < row[b] : col[a] < col[b]; });
    idx.resize((size_t)n);
    val.resize((size_t)n);
    for (size_t k = 0; k < ord.size(); ++k) idx[k] = col[ord[k]], val[k] = r[ord[k]];
}

static int slope_set_ratings_impl(cmi_slope_handle h, int64_t n, const int32_t *u, const int32_t *i, const double *r) {
    if (n < 0 || (n > 0 && (!u || !i || !r))) CMI_FAIL(h, CMI_E_INVALID, "cmi_slope_set_ratings: null arrays");
    if (n >= ((int64_t)1 << 31)) CMI_FAIL(h, CMI_E_UNSUPPORTED, "cmi_slope_set_ratings: more than 2^31-1 cells");
    for (int64_t t = 0; t < n; ++t)
        if (u[t] < 0 || u[t] >= h->n_users || i[t] < 0 || i[t] >= h->n_items)
            CMI_FAIL(h, CMI_E_INVALID, "cmi_slope_set_ratings: id out of range at cell %lld", (long long)t);
    std::vector<int32_t> cptr, cidx, rptr, ridx;
    std::vector<double> cval, rval;
    slope_csr(n, h->n_users, u, i, r, rptr, ridx, rval);
    for (int a = 0; a < h->n_users; ++a)
        for (int32_t k = rptr[(size_t)a] + 1; k < rptr[(size_t)a + 1]; ++k)
            if (ridx[(size_t)k] == ridx[(size_t)k - 1])
                CMI_FAIL(h, CMI_E_INVALID, "cmi_slope_set_ratings: duplicate cell (user %d, item %d)", a, ridx[(size_t)k]);
    slope_csr(n, h->n_items, i, u, r, cptr, cidx, cval);
    CMI_HIP(h, hipSetDevice(h->device));
    CMI_HIP(h, hipStreamSynchronize(h->stream));
    slope_free_ratings(h);
    hipError_t e = abi_upload(&h->d_cptr, cptr, h->stream, true);
    if (e == hipSuccess) e = abi_upload(&h->d_cidx, cidx, h->stream, true);
    if (e == hipSuccess) e = abi_upload(&h->d_cval, cval, h->stream, true);
    if (e == hipSuccess) e = abi_upload(&h->d_rptr, rptr, h->stream, true);
    if (e == hipSuccess) e = abi_upload(&h->d_ridx, ridx, h->stream, true);
    if (e == hipSuccess) e = abi_upload(&h->d_rval, rval, h->stream, true);
    if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
    if (e != hipSuccess) {
        slope_free_ratings(h);
        CMI_FAIL(h, CMI_E_HIP, "cmi_slope_set_ratings: %s", hipGetErrorString(e));
    }
    h->have_ratings = true;
    return CMI_OK;
}

extern "C" int cmi_slope_set_ratings(cmi_slope_handle h, int64_t n, const int32_t *u, const int32_t *i, const double *r) {
    if (!h) return CMI_E_INVALID;
    return abi_barrier(h->err, "cmi_slope_set_ratings", [&] { return slope_set_ratings_impl(h, n, u, i, r); },
                       [h] { slope_free_ratings(h); });
}

extern "C" int cmi_slope_build(cmi_slope_handle h) {
    if (!h) return CMI_E_INVALID;
    if (!h->have_ratings) CMI_FAIL(h, CMI_E_INVALID, "cmi_slope_build: no ratings (cmi_slope_set_ratings first)");
    CMI_HIP(h, hipSetDevice(h->device));
    CMI_HIP(h, hipStreamSynchronize(h->stream));
    const size_t cells = (size_t)h->n_items * (size_t)h->n_items;
    const size_t bytes = cells * (sizeof(double) + sizeof(int32_t));
    if (!h->d_dev) { // the two dense n x n matrices: refused up front when they cannot fit, so a build never fails half-way
        size_t free_b = 0, total_b = 0;
        CMI_HIP(h, hipMemGetInfo(&free_b, &total_b));
        if (bytes > free_b)
            CMI_FAIL(h, CMI_E_INVALID,
                     "cmi_slope_build: the %d x %d deviation and cardinality matrices need %zu bytes of device memory, %zu are free",
                     h->n_items, h->n_items, bytes, free_b);
        hipError_t e = hipMalloc((void **)&h->d_dev, cells * sizeof(double));
        if (e == hipSuccess) e = hipMalloc((void **)&h->d_card, cells * sizeof(int32_t));
        if (e != hipSuccess) {
            abi_free(h->d_dev, h->d_card);
            CMI_FAIL(h, CMI_E_INVALID, "cmi_slope_build: the deviation and cardinality matrices need %zu bytes of device memory: %s",
                     bytes, hipGetErrorString(e));
        }
    }
    h->built = false;
    CMI_HIP(h, hipEventRecord(h->ev0, h->stream));
    CMI_HIP(h, hipMemsetAsync(h->d_dev, 0, cells * sizeof(double), h->stream)); // +0.0 and 0: "no common user"
    CMI_HIP(h, hipMemsetAsync(h->d_card, 0, cells * sizeof(int32_t), h->stream));
    CMI_HIP(h, slope_launch_build(SlopeCsr{h->d_cptr, h->d_cidx, h->d_cval}, h->n_items, h->d_dev, h->d_card, h->stream));
    CMI_HIP(h, hipEventRecord(h->ev1, h->stream));
    CMI_HIP(h, hipStreamSynchronize(h->stream));
    CMI_HIP(h, hipEventElapsedTime(&h->build_ms, h->ev0, h->ev1));
    h->built = true;
    return CMI_OK;
}

extern "C" int cmi_slope_get_deviation(cmi_slope_handle h, int32_t row0, int32_t nrows, double *dev, int32_t *card) {
    if (!h) return CMI_E_INVALID;
    if (!h->built) CMI_FAIL(h, CMI_E_INVALID, "cmi_slope_get_deviation: no deviation matrix (cmi_slope_build first)");
    if (row0 < 0 || nrows < 0 || (int64_t)row0 + nrows > h->n_items)
        CMI_FAIL(h, CMI_E_INVALID, "cmi_slope_get_deviation: rows [%d, %lld) out of range", row0, (long long)row0 + nrows);
    CMI_HIP(h, hipSetDevice(h->device));
    const size_t off = (size_t)row0 * h->n_items, cnt = (size_t)nrows * h->n_items;
    if (dev && cnt) CMI_HIP(h, hipMemcpyAsync(dev, h->d_dev + off, cnt * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    if (card && cnt) CMI_HIP(h, hipMemcpyAsync(card, h->d_card + off, cnt * sizeof(int32_t), hipMemcpyDeviceToHost, h->stream));
    CMI_HIP(h, hipStreamSynchronize(h->stream));
    return CMI_OK;
}

static int slope_predict_impl(cmi_slope_handle h, int64_t n, const int32_t *u, const int32_t *j, double gm, int bound, double lo,
                              double hi, double *out) {
    if (!h->built) CMI_FAIL(h, CMI_E_INVALID, "cmi_slope_predict_batch: no deviation matrix (cmi_slope_build first)");
    if (n < 0 || (n > 0 && (!u || !j || !out))) CMI_FAIL(h, CMI_E_INVALID, "cmi_slope_predict_batch: null arrays");
    if (n == 0) return CMI_OK;
    for (int64_t t = 0; t < n; ++t)
        if (u[t] < 0 || u[t] >= h->n_users || j[t] < 0 || j[t] >= h->n_items)
            CMI_FAIL(h, CMI_E_INVALID, "cmi_slope_predict_batch: id out of range at tuple %lld", (long long)t);
    CMI_HIP(h, hipSetDevice(h->device));
    const int nwaves = (int)std::min<int64_t>(n, 16384); // one wave per tuple in flight
    int32_t *d_u = nullptr, *d_j = nullptr;
    double *d_out = nullptr;
    hipError_t e = abi_upload(&d_u, u, (size_t)n, h->stream);
    if (e == hipSuccess) e = abi_upload(&d_j, j, (size_t)n, h->stream);
    if (e == hipSuccess) e = hipMalloc((void **)&d_out, (size_t)n * sizeof(double));
    if (e == hipSuccess)
        e = slope_launch_predict(SlopeCsr{h->d_rptr, h->d_ridx, h->d_rval}, h->d_dev, h->d_card, h->n_items, n, d_u, d_j, gm, bound, lo,
                                 hi, d_out, nwaves, h->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(out, d_out, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, h->stream);
    const hipError_t es = hipStreamSynchronize(h->stream); // the uploads read u and j until here, whatever failed
    if (e == hipSuccess) e = es;
    abi_free(d_u, d_j, d_out);
    if (e != hipSuccess) CMI_FAIL(h, CMI_E_HIP, "cmi_slope_predict_batch: %s", hipGetErrorString(e));
    return CMI_OK;
}

extern "C" int cmi_slope_predict_batch(cmi_slope_handle h, int64_t n, const int32_t *u, const int32_t *j, double global_mean, int bound,
                                       double lo, double hi, double *out) {
    if (!h) return CMI_E_INVALID;
    return abi_barrier(h->err, "cmi_slope_predict_batch", [&] { return slope_predict_impl(h, n, u, j, global_mean, bound, lo, hi, out); });
}

extern "C" int cmi_slope_last_build_ms(cmi_slope_handle h, float *ms) {
    if (!h || !ms) return CMI_E_INVALID;
    if (!h->built) CMI_FAIL(h, CMI_E_INVALID, "cmi_slope_last_build_ms: nothing built yet");
    *ms = h->build_ms;
    return CMI_OK;
}
