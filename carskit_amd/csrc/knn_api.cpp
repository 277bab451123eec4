// knn_api.cpp -- C ABI of ItemKNN / UserKNN (include/carskit_mi355x.h, cmi_knn_*).
#include "../../include/carskit_mi355x.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <strings.h>
#include <numeric>
#include <string>
#include <vector>

#include "abi.hpp"
#include "knn_kernels.hpp"

using namespace cmi;

struct cmi_knn_instance {
    int kind = CMI_KNN_ITEM, n_users = 0, n_items = 0, device = 0;
    int n_ent = 0, n_ctr = 0; // compared rows (items for ItemKNN, users for UserKNN) and the contracted index
    std::string err;
    hipStream_t stream = nullptr;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    // rows: entity -> (contracted index, value); lists: contracted index -> (entity, value).  Both CSR, ascending.
    int32_t *d_rptr = nullptr, *d_ridx = nullptr, *d_lptr = nullptr, *d_lidx = nullptr;
    uint8_t *d_rok = nullptr;
    double *d_rval = nullptr, *d_lval = nullptr, *d_mean = nullptr, *d_norm2 = nullptr, *d_S = nullptr;
    std::vector<int32_t> list_len; // per list (contracted index): its length, for the candidate limit
    bool have_ratings = false, built = false;
    float build_ms = 0.f;
};

static thread_local std::string g_knn_create_err;

extern "C" const char *cmi_knn_last_error(cmi_knn_handle h) { return h ? h->err.c_str() : g_knn_create_err.c_str(); }

extern "C" int cmi_knn_measure(const char *name) {
    const char *s = name ? name : ""; // (compared without a copy: nothing here allocates)
    if (!strcasecmp(s, "cos")) return CMI_SIM_COS;
    if (!strcasecmp(s, "cos-binary")) return CMI_SIM_COS_BINARY;
    if (!strcasecmp(s, "msd")) return CMI_SIM_MSD;
    if (!strcasecmp(s, "cpc")) return CMI_SIM_CPC;
    if (!strcasecmp(s, "exjaccard")) return CMI_SIM_EXJACCARD;
    return CMI_SIM_PCC; // "pcc" and Recommender.correlation's default: branch
}

static void knn_free_ratings(cmi_knn_instance *h) {
    abi_free(h->d_rok, h->d_rptr, h->d_ridx, h->d_lptr, h->d_lidx, h->d_rval, h->d_lval, h->d_mean, h->d_norm2, h->d_S);
    h->have_ratings = h->built = false;
}

extern "C" int cmi_knn_destroy(cmi_knn_handle h) {
    if (!h) return CMI_OK;
    (void)hipSetDevice(h->device);
    if (h->stream) (void)hipStreamSynchronize(h->stream);
    knn_free_ratings(h);
    if (h->ev0) (void)hipEventDestroy(h->ev0);
    if (h->ev1) (void)hipEventDestroy(h->ev1);
    if (h->stream) (void)hipStreamDestroy(h->stream);
    delete h;
    return CMI_OK;
}

extern "C" int cmi_knn_create(int kind, int n_users, int n_items, int device, unsigned flags, cmi_knn_handle *out) {
    (void)flags;
    return abi_barrier(g_knn_create_err, "cmi_knn_create", [&] {
        if (out) *out = nullptr;
        if (!out || (kind != CMI_KNN_USER && kind != CMI_KNN_ITEM) || n_users <= 0 || n_items <= 0) {
            g_knn_create_err = "cmi_knn_create: invalid argument";
            return CMI_E_INVALID;
        }
        if (int rc = abi_check_device(g_knn_create_err, "cmi_knn_create", device)) return rc;
        cmi_knn_instance *h = new cmi_knn_instance();
        h->kind = kind;
        h->n_users = n_users;
        h->n_items = n_items;
        h->device = device;
        h->n_ent = kind == CMI_KNN_ITEM ? n_items : n_users;
        h->n_ctr = kind == CMI_KNN_ITEM ? n_users : n_items;
        hipError_t e = hipSetDevice(device);
        if (e == hipSuccess) e = hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking);
        if (e == hipSuccess) e = hipEventCreate(&h->ev0);
        if (e == hipSuccess) e = hipEventCreate(&h->ev1);
        if (e != hipSuccess) {
            g_knn_create_err = std::string("cmi_knn_create: ") + hipGetErrorString(e);
            cmi_knn_destroy(h);
            return CMI_E_HIP;
        }
        *out = h;
        return CMI_OK;
    });
}

// CSR of (row, col, value) cells, rows ascending, columns ascending inside a row
static void knn_csr(int64_t n, int n_rows, const int32_t *row, const int32_t *col, const double *r, std::vector<int32_t> &ptr,
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

static int knn_set_ratings_impl(cmi_knn_handle h, int64_t n, const int32_t *u, const int32_t *i, const double *r) {
    if (n < 0 || (n > 0 && (!u || !i || !r))) CMI_FAIL(h, CMI_E_INVALID, "cmi_knn_set_ratings: null arrays");
    if (n >= ((int64_t)1 << 31)) CMI_FAIL(h, CMI_E_UNSUPPORTED, "cmi_knn_set_ratings: more than 2^31-1 cells");
    for (int64_t t = 0; t < n; ++t)
        if (u[t] < 0 || u[t] >= h->n_users || i[t] < 0 || i[t] >= h->n_items)
            CMI_FAIL(h, CMI_E_INVALID, "cmi_knn_set_ratings: id out of range at cell %lld", (long long)t);
    const bool item = h->kind == CMI_KNN_ITEM;
    const int32_t *ent = item ? i : u, *ctr = item ? u : i;
    std::vector<int32_t> rptr, ridx, lptr, lidx;
    std::vector<double> rval, lval;
    knn_csr(n, h->n_ent, ent, ctr, r, rptr, ridx, rval);
    for (int e = 0; e < h->n_ent; ++e)
        for (int32_t k = rptr[(size_t)e] + 1; k < rptr[(size_t)e + 1]; ++k)
            if (ridx[(size_t)k] == ridx[(size_t)k - 1])
                CMI_FAIL(h, CMI_E_INVALID, "cmi_knn_set_ratings: duplicate cell (user %d, item %d)", item ? ridx[(size_t)k] : e,
                         item ? e : ridx[(size_t)k]);
    knn_csr(n, h->n_ctr, ctr, ent, r, lptr, lidx, lval);
    // librec SparseVector.contains: Arrays.binarySearch over the whole index array of a vector built by set() -- capacity the next
    // power of two >= count, the tail zero.  Per entry of every row: does the row's own contains() find it?
    std::vector<uint8_t> rok((size_t)n, 0);
    for (int e = 0; e < h->n_ent; ++e) {
        const int32_t b0 = rptr[(size_t)e], cnt = rptr[(size_t)e + 1] - b0;
        int32_t cap = 1;
        while (cap < cnt) cap <<= 1;
        for (int32_t k = 0; k < cnt; ++k) {
            const int32_t key = ridx[(size_t)(b0 + k)];
            int32_t low = 0, high = cap - 1;
            while (low <= high) {
                const int32_t mid = (int32_t)((uint32_t)(low + high) >> 1);
                const int32_t v = mid < cnt ? ridx[(size_t)(b0 + mid)] : 0;
                if (v < key) low = mid + 1;
                else if (v > key) high = mid - 1;
                else {
                    rok[(size_t)(b0 + k)] = 1;
                    break;
                }
            }
        }
    }
    CMI_HIP(h, hipSetDevice(h->device));
    CMI_HIP(h, hipStreamSynchronize(h->stream));
    knn_free_ratings(h);
    hipError_t e = abi_upload(&h->d_rptr, rptr, h->stream, true);
    if (e == hipSuccess) e = abi_upload(&h->d_ridx, ridx, h->stream, true);
    if (e == hipSuccess) e = abi_upload(&h->d_rval, rval, h->stream, true);
    if (e == hipSuccess) e = abi_upload(&h->d_rok, rok, h->stream, true);
    if (e == hipSuccess) e = abi_upload(&h->d_lptr, lptr, h->stream, true);
    if (e == hipSuccess) e = abi_upload(&h->d_lidx, lidx, h->stream, true);
    if (e == hipSuccess) e = abi_upload(&h->d_lval, lval, h->stream, true);
    if (e == hipSuccess) e = hipMalloc((void **)&h->d_mean, (size_t)h->n_ent * sizeof(double));
    if (e == hipSuccess) e = hipMalloc((void **)&h->d_norm2, (size_t)h->n_ent * sizeof(double));
    if (e == hipSuccess) e = knn_launch_row_stats(KnnCsr{h->d_rptr, h->d_ridx, h->d_rval, h->d_rok}, h->n_ent, h->d_mean, h->d_norm2, h->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
    if (e != hipSuccess) {
        knn_free_ratings(h);
        CMI_FAIL(h, CMI_E_HIP, "cmi_knn_set_ratings: %s", hipGetErrorString(e));
    }
    h->list_len.resize((size_t)h->n_ctr);
    for (int c = 0; c < h->n_ctr; ++c) h->list_len[(size_t)c] = lptr[(size_t)c + 1] - lptr[(size_t)c];
    h->have_ratings = true;
    return CMI_OK;
}

extern "C" int cmi_knn_set_ratings(cmi_knn_handle h, int64_t n, const int32_t *u, const int32_t *i, const double *r) {
    if (!h) return CMI_E_INVALID;
    return abi_barrier(h->err, "cmi_knn_set_ratings", [&] { return knn_set_ratings_impl(h, n, u, i, r); }, [h] { knn_free_ratings(h); });
}

extern "C" int cmi_knn_build(cmi_knn_handle h, int measure, int shrinkage, double min_rate, double max_rate) {
    if (!h) return CMI_E_INVALID;
    if (!h->have_ratings) CMI_FAIL(h, CMI_E_INVALID, "cmi_knn_build: no ratings (cmi_knn_set_ratings first)");
    if (measure < CMI_SIM_PCC || measure > CMI_SIM_EXJACCARD) CMI_FAIL(h, CMI_E_INVALID, "cmi_knn_build: unknown measure %d", measure);
    CMI_HIP(h, hipSetDevice(h->device));
    CMI_HIP(h, hipStreamSynchronize(h->stream));
    const size_t bytes = (size_t)h->n_ent * (size_t)h->n_ent * sizeof(double);
    if (!h->d_S) { // the dense n x n matrix: refused up front when it cannot fit, so a build never fails half-way
        size_t free_b = 0, total_b = 0;
        CMI_HIP(h, hipMemGetInfo(&free_b, &total_b));
        if (bytes > free_b)
            CMI_FAIL(h, CMI_E_INVALID, "cmi_knn_build: the %d x %d similarity matrix needs %zu bytes of device memory, %zu are free",
                     h->n_ent, h->n_ent, bytes, free_b);
        hipError_t e = hipMalloc((void **)&h->d_S, std::max<size_t>(bytes, 8));
        if (e != hipSuccess) {
            h->d_S = nullptr;
            CMI_FAIL(h, CMI_E_INVALID, "cmi_knn_build: the similarity matrix needs %zu bytes of device memory: %s", bytes,
                     hipGetErrorString(e));
        }
    }
    h->built = false;
    CMI_HIP(h, hipEventRecord(h->ev0, h->stream));
    CMI_HIP(h, hipMemsetAsync(h->d_S, 0xff, bytes, h->stream)); // all-ones bits: NaN, "unset"
    CMI_HIP(h, knn_launch_build(KnnCsr{h->d_rptr, h->d_ridx, h->d_rval, h->d_rok}, h->n_ent, h->d_norm2, measure, shrinkage,
                                (min_rate + max_rate) / 2.0, h->d_S, h->stream));
    CMI_HIP(h, hipEventRecord(h->ev1, h->stream));
    CMI_HIP(h, hipStreamSynchronize(h->stream));
    CMI_HIP(h, hipEventElapsedTime(&h->build_ms, h->ev0, h->ev1));
    h->built = true;
    return CMI_OK;
}

extern "C" int cmi_knn_get_similarity(cmi_knn_handle h, int32_t row0, int32_t nrows, double *dst) {
    if (!h) return CMI_E_INVALID;
    if (!h->built) CMI_FAIL(h, CMI_E_INVALID, "cmi_knn_get_similarity: no similarity matrix (cmi_knn_build first)");
    if (row0 < 0 || nrows < 0 || (int64_t)row0 + nrows > h->n_ent || (nrows > 0 && !dst))
        CMI_FAIL(h, CMI_E_INVALID, "cmi_knn_get_similarity: rows [%d, %d) out of range", row0, row0 + nrows);
    CMI_HIP(h, hipSetDevice(h->device));
    CMI_HIP(h, hipMemcpyAsync(dst, h->d_S + (size_t)row0 * h->n_ent, (size_t)nrows * h->n_ent * sizeof(double), hipMemcpyDeviceToHost,
                              h->stream));
    CMI_HIP(h, hipStreamSynchronize(h->stream));
    return CMI_OK;
}

static int knn_predict_impl(cmi_knn_handle h, int64_t n, const int32_t *u, const int32_t *j, int knn, double gm, int bound, double lo,
                            double hi, double *out) {
    if (!h->built) CMI_FAIL(h, CMI_E_INVALID, "cmi_knn_predict_batch: no similarity matrix (cmi_knn_build first)");
    if (n < 0 || (n > 0 && (!u || !j || !out))) CMI_FAIL(h, CMI_E_INVALID, "cmi_knn_predict_batch: null arrays");
    if (n == 0) return CMI_OK;
    for (int64_t t = 0; t < n; ++t)
        if (u[t] < 0 || u[t] >= h->n_users || j[t] < 0 || j[t] >= h->n_items)
            CMI_FAIL(h, CMI_E_INVALID, "cmi_knn_predict_batch: id out of range at tuple %lld", (long long)t);
    const bool item = h->kind == CMI_KNN_ITEM;
    const int32_t *owner = item ? u : j, *target = item ? j : u; // ItemKNN: the user's items scored against item j; UserKNN: the reverse
    int cap = 1;
    for (int64_t t = 0; t < n; ++t) {
        const int len = h->list_len[(size_t)owner[t]];
        if (len > CMI_KNN_MAX_CANDIDATES)
            CMI_FAIL(h, CMI_E_UNSUPPORTED, "cmi_knn_predict_batch: tuple %lld has %d candidates, more than CMI_KNN_MAX_CANDIDATES (%d)",
                     (long long)t, len, CMI_KNN_MAX_CANDIDATES);
        cap = std::max(cap, len);
    }
    CMI_HIP(h, hipSetDevice(h->device));
    // one wave per tuple in flight; every wave owns `cap` entries (the longest list of the batch) of each scratch array (32 bytes an
    // entry), at most ~1 GiB
    const int64_t by_mem = std::max<int64_t>(1, ((int64_t)1 << 30) / ((int64_t)cap * 32));
    const int nwaves = (int)std::max<int64_t>(1, std::min<int64_t>({n, 8192, by_mem}));
    int32_t *d_owner = nullptr, *d_target = nullptr, *d_bad = nullptr, *s_key = nullptr, *s_pos = nullptr, *s_sel = nullptr;
    double *d_out = nullptr, *s_sim = nullptr, *s_rate = nullptr;
    const size_t ns = (size_t)nwaves * cap;
    hipError_t e = hipMalloc((void **)&d_owner, (size_t)n * 4);
    if (e == hipSuccess) e = hipMalloc((void **)&d_target, (size_t)n * 4);
    if (e == hipSuccess) e = hipMalloc((void **)&d_out, (size_t)n * 8);
    if (e == hipSuccess) e = hipMalloc((void **)&d_bad, 4);
    if (e == hipSuccess) e = hipMalloc((void **)&s_key, ns * 4);
    if (e == hipSuccess) e = hipMalloc((void **)&s_pos, ns * 4);
    if (e == hipSuccess) e = hipMalloc((void **)&s_sel, ns * 4);
    if (e == hipSuccess) e = hipMalloc((void **)&s_sim, ns * 8);
    if (e == hipSuccess) e = hipMalloc((void **)&s_rate, ns * 8);
    if (e == hipSuccess) e = hipMemcpyAsync(d_owner, owner, (size_t)n * 4, hipMemcpyHostToDevice, h->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(d_target, target, (size_t)n * 4, hipMemcpyHostToDevice, h->stream);
    if (e == hipSuccess) e = hipMemsetAsync(d_bad, 0, 4, h->stream);
    if (e == hipSuccess)
        e = knn_launch_predict(KnnCsr{h->d_lptr, h->d_lidx, h->d_lval}, h->d_S, h->n_ent, h->d_mean, n, d_owner, d_target, knn, gm, bound,
                               lo, hi, d_out, nwaves, cap, s_key, s_sim, s_rate, s_pos, s_sel, d_bad, h->stream);
    int32_t bad = 0;
    if (e == hipSuccess) e = hipMemcpyAsync(out, d_out, (size_t)n * 8, hipMemcpyDeviceToHost, h->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(&bad, d_bad, 4, hipMemcpyDeviceToHost, h->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
    abi_free(d_owner, d_target, d_out, d_bad, s_key, s_pos, s_sel, s_sim, s_rate);
    if (e != hipSuccess) CMI_FAIL(h, CMI_E_HIP, "cmi_knn_predict_batch: %s", hipGetErrorString(e));
    if (bad)
        CMI_FAIL(h, CMI_E_UNSUPPORTED,
                 "cmi_knn_predict_batch: %d tuple(s) would treeify a java.util.HashMap bin, whose iteration order is not modelled", bad);
    return CMI_OK;
}

extern "C" int cmi_knn_predict_batch(cmi_knn_handle h, int64_t n, const int32_t *u, const int32_t *j, int knn, double global_mean,
                                     int bound, double lo, double hi, double *out) {
    if (!h) return CMI_E_INVALID;
    return abi_barrier(h->err, "cmi_knn_predict_batch", [&] { return knn_predict_impl(h, n, u, j, knn, global_mean, bound, lo, hi, out); });
}

extern "C" int cmi_knn_last_build_ms(cmi_knn_handle h, float *ms) {
    if (!h || !ms) return CMI_E_INVALID;
    if (!h->built) CMI_FAIL(h, CMI_E_INVALID, "cmi_knn_last_build_ms: nothing built yet");
    *ms = h->build_ms;
    return CMI_OK;
}
