// knn_api.cpp -- C ABI of ItemKNN / UserKNN (include/carskit_mi355x.h, cmi_knn_*).
#include "../../include/carskit_mi355x.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <strings.h>
#include <string>
#include <vector>

#include "knn_kernels.hpp"
#include "pair_host.hpp"

using namespace cmi;

struct cmi_knn_instance : PairModelBase {
    int kind = CMI_KNN_ITEM;
    int n_ent = 0, n_ctr = 0; // compared rows (items for ItemKNN, users for UserKNN) and the contracted index
    // rows: entity -> (contracted index, value); lists: contracted index -> (entity, value).  Both CSR, ascending.
    int32_t *d_rptr = nullptr, *d_ridx = nullptr, *d_lptr = nullptr, *d_lidx = nullptr;
    uint8_t *d_rok = nullptr;
    double *d_rval = nullptr, *d_lval = nullptr, *d_mean = nullptr, *d_norm2 = nullptr, *d_S = nullptr;
    std::vector<int32_t> list_len; // per list (contracted index): its length, for the candidate limit
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

extern "C" int cmi_knn_destroy(cmi_knn_handle h) { return pair_destroy(h, knn_free_ratings); }

extern "C" int cmi_knn_create(int kind, int n_users, int n_items, int device, unsigned flags, cmi_knn_handle *out) {
    (void)flags;
    const bool valid = kind == CMI_KNN_USER || kind == CMI_KNN_ITEM;
    return pair_create(g_knn_create_err, "cmi_knn_create", valid, n_users, n_items, device, out, cmi_knn_destroy,
                       [&](cmi_knn_instance *h) {
                           h->kind = kind;
                           h->n_ent = kind == CMI_KNN_ITEM ? n_items : n_users;
                           h->n_ctr = kind == CMI_KNN_ITEM ? n_users : n_items;
                       });
}

static int knn_set_ratings_impl(cmi_knn_handle h, int64_t n, const int32_t *u, const int32_t *i, const double *r) {
    const bool item = h->kind == CMI_KNN_ITEM;
    PairHostCsr by_user, by_item;
    if (int rc = pair_ingest(h, "cmi_knn_set_ratings", n, u, i, r, /*scan_items=*/item, by_user, by_item)) return rc;
    const PairHostCsr &rows = item ? by_item : by_user, &lists = item ? by_user : by_item;
    const std::vector<int32_t> &lptr = lists.ptr;
    const std::vector<uint8_t> rok = pair_contains_flags(rows);
    CMI_HIP(h, hipSetDevice(h->device));
    CMI_HIP(h, hipStreamSynchronize(h->stream));
    knn_free_ratings(h);
    hipError_t e = pair_upload(rows, &h->d_rptr, &h->d_ridx, &h->d_rval, h->stream);
    if (e == hipSuccess) e = abi_upload(&h->d_rok, rok, h->stream, true);
    if (e == hipSuccess) e = pair_upload(lists, &h->d_lptr, &h->d_lidx, &h->d_lval, h->stream);
    if (e == hipSuccess) e = hipMalloc((void **)&h->d_mean, (size_t)h->n_ent * sizeof(double));
    if (e == hipSuccess) e = hipMalloc((void **)&h->d_norm2, (size_t)h->n_ent * sizeof(double));
    if (e == hipSuccess) e = knn_launch_row_stats(PairCsr{h->d_rptr, h->d_ridx, h->d_rval, h->d_rok}, h->n_ent, h->d_mean, h->d_norm2, h->stream);
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
    const size_t bytes = (size_t)h->n_ent * (size_t)h->n_ent * sizeof(double);
    const auto alloc = [&] { // the dense n x n matrix
        const hipError_t e = hipMalloc((void **)&h->d_S, std::max<size_t>(bytes, 8));
        if (e != hipSuccess) h->d_S = nullptr;
        return e;
    };
    if (!h->d_S)
        if (int rc = pair_reserve_dense(h, "cmi_knn_build", h->n_ent, bytes, "similarity matrix", /*plural=*/false, alloc)) return rc;
    return pair_timed_build(h, [&] {
        CMI_HIP(h, hipMemsetAsync(h->d_S, 0xff, bytes, h->stream)); // all-ones bits: NaN, "unset"
        CMI_HIP(h, knn_launch_build(PairCsr{h->d_rptr, h->d_ridx, h->d_rval, h->d_rok}, h->n_ent, h->d_norm2, measure, shrinkage,
                                    (min_rate + max_rate) / 2.0, h->d_S, h->stream));
        return CMI_OK;
    });
}

extern "C" int cmi_knn_get_similarity(cmi_knn_handle h, int32_t row0, int32_t nrows, double *dst) {
    if (!h) return CMI_E_INVALID;
    if (!h->built) CMI_FAIL(h, CMI_E_INVALID, "cmi_knn_get_similarity: no similarity matrix (cmi_knn_build first)");
    if (row0 < 0 || nrows < 0 || (int64_t)row0 + nrows > h->n_ent || (nrows > 0 && !dst))
        CMI_FAIL(h, CMI_E_INVALID, "cmi_knn_get_similarity: rows [%d, %lld) out of range", row0, (long long)row0 + nrows);
    CMI_HIP(h, hipSetDevice(h->device));
    CMI_HIP(h, hipMemcpyAsync(dst, h->d_S + (size_t)row0 * h->n_ent, (size_t)nrows * h->n_ent * sizeof(double), hipMemcpyDeviceToHost,
                              h->stream));
    CMI_HIP(h, hipStreamSynchronize(h->stream));
    return CMI_OK;
}

static int knn_predict_impl(cmi_knn_handle h, int64_t n, const int32_t *u, const int32_t *j, int knn, double gm, int bound, double lo,
                            double hi, double *out) {
    if (!h->built) CMI_FAIL(h, CMI_E_INVALID, "cmi_knn_predict_batch: no similarity matrix (cmi_knn_build first)");
    if (int rc = pair_check_tuples(h, "cmi_knn_predict_batch", n, u, j, out)) return rc;
    if (n == 0) return CMI_OK;
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
    // one wave per tuple in flight; every wave owns `cap` entries (the longest list of the batch) of each scratch array (32 bytes an
    // entry), at most ~1 GiB
    const int64_t by_mem = std::max<int64_t>(1, ((int64_t)1 << 30) / ((int64_t)cap * 32));
    const int nwaves = (int)std::max<int64_t>(1, std::min<int64_t>({n, 8192, by_mem}));
    int32_t *d_bad = nullptr, *s_key = nullptr, *s_pos = nullptr, *s_sel = nullptr;
    double *s_sim = nullptr, *s_rate = nullptr;
    const size_t ns = (size_t)nwaves * cap;
    int32_t bad = 0;
    const int rc = abi_predict(h, "cmi_knn_predict_batch", n, owner, target, nullptr, nullptr, 0, out, [&](const AbiTuples &t, double *d_out) {
        hipError_t e = hipMalloc((void **)&d_bad, 4);
        if (e == hipSuccess) e = hipMalloc((void **)&s_key, ns * 4);
        if (e == hipSuccess) e = hipMalloc((void **)&s_pos, ns * 4);
        if (e == hipSuccess) e = hipMalloc((void **)&s_sel, ns * 4);
        if (e == hipSuccess) e = hipMalloc((void **)&s_sim, ns * 8);
        if (e == hipSuccess) e = hipMalloc((void **)&s_rate, ns * 8);
        if (e == hipSuccess) e = hipMemsetAsync(d_bad, 0, 4, h->stream);
        if (e == hipSuccess)
            e = knn_launch_predict(PairCsr{h->d_lptr, h->d_lidx, h->d_lval}, h->d_S, h->n_ent, h->d_mean, n, t.a, t.b, knn, gm,
                                   bound, lo, hi, d_out, nwaves, cap, s_key, s_sim, s_rate, s_pos, s_sel, d_bad, h->stream);
        if (e == hipSuccess) e = hipMemcpyAsync(&bad, d_bad, 4, hipMemcpyDeviceToHost, h->stream);
        return abi_hip(h->err, "cmi_knn_predict_batch", e);
    });
    abi_free(d_bad, s_key, s_pos, s_sel, s_sim, s_rate); // the stream is drained
    if (rc != CMI_OK) return rc;
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

extern "C" int cmi_knn_last_build_ms(cmi_knn_handle h, float *ms) { return pair_last_build_ms(h, "cmi_knn_last_build_ms", ms); }
