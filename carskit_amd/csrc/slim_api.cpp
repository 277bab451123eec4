// slim_api.cpp -- C ABI of SLIM (include/carskit_mi355x.h, cmi_slim_*).
#include "../../include/carskit_mi355x.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdio>
#include <numeric>
#include <string>
#include <vector>

#include "host_pool.hpp"
#include "java_hash.hpp"
#include "knn_kernels.hpp"
#include "pair_host.hpp"
#include "rank_host.hpp"
#include "slim_kernels.hpp"

using namespace cmi;

struct cmi_slim_instance : PairModelBase {
    // rows: user -> (item, value, ok); cols: item -> (user, value, ok); both CSR, ascending, without the zero-valued cells
    int32_t *d_rptr = nullptr, *d_ridx = nullptr, *d_cptr = nullptr, *d_cidx = nullptr;
    uint8_t *d_rok = nullptr, *d_cok = nullptr;
    double *d_rval = nullptr, *d_cval = nullptr, *d_mean = nullptr, *d_norm2 = nullptr;
    std::vector<int32_t> col_len; // per item: its live entries
    // the lists (cmi_slim_build_neighbors) and what is aligned with them
    std::vector<int64_t> nptr;
    std::vector<int32_t> nidx;
    int64_t *d_nptr = nullptr;
    int32_t *d_nidx = nullptr, *d_order = nullptr; // order: the columns with a list, by descending work; first the n_lds short lists
    double *d_w = nullptr, *d_term = nullptr, *d_loss = nullptr;
    int n_lds = 0, n_big = 0, lds_len = 0; // lds_len: the longest of the n_lds short lists (the sweep's LDS, in doubles)
    bool have_lists = false, have_weights = false, iterated = false;
    hipEvent_t ev2 = nullptr;
    float iter_ms[2] = {0.f, 0.f};
    RankWorkspace rank_ws;
};

static thread_local std::string g_slim_create_err;

extern "C" const char *cmi_slim_last_error(cmi_slim_handle h) { return h ? h->err.c_str() : g_slim_create_err.c_str(); }

static void slim_free_lists(cmi_slim_instance *h) {
    abi_free(h->d_nptr, h->d_nidx, h->d_order, h->d_w, h->d_term, h->d_loss);
    h->nptr.clear(), h->nidx.clear();
    h->have_lists = h->have_weights = h->iterated = h->built = false;
}

static void slim_free_ratings(cmi_slim_instance *h) {
    slim_free_lists(h);
    abi_free(h->d_rptr, h->d_ridx, h->d_cptr, h->d_cidx, h->d_rok, h->d_cok, h->d_rval, h->d_cval, h->d_mean, h->d_norm2);
    h->have_ratings = false;
}

static void slim_free_all(cmi_slim_instance *h) {
    slim_free_ratings(h);
    h->rank_ws.release();
    if (h->ev2) (void)hipEventDestroy(h->ev2);
    h->ev2 = nullptr;
}

extern "C" int cmi_slim_destroy(cmi_slim_handle h) { return pair_destroy(h, slim_free_all); }

extern "C" int cmi_slim_create(int n_users, int n_items, int device, unsigned flags, cmi_slim_handle *out) {
    (void)flags;
    int rc = pair_create(g_slim_create_err, "cmi_slim_create", true, n_users, n_items, device, out, cmi_slim_destroy, [](cmi_slim_instance *) {});
    if (rc != CMI_OK) return rc;
    const hipError_t e = hipEventCreate(&(*out)->ev2);
    if (e != hipSuccess) {
        cmi_slim_destroy(*out);
        *out = nullptr;
        return abi_fail(g_slim_create_err, CMI_E_HIP, "cmi_slim_create: %s", hipGetErrorString(e));
    }
    return CMI_OK;
}

static int slim_set_ratings_impl(cmi_slim_handle h, int64_t n, const int32_t *u, const int32_t *i, const double *r) {
    PairHostCsr rows, cols;
    if (int rc = pair_ingest(h, "cmi_slim_set_ratings", n, u, i, r, /*scan_items=*/false, rows, cols)) return rc;
    // a stored 0.0: row() and column() leave it out, and get() returns the 0.0 of an absent cell
    rows = pair_drop_zeros(rows), cols = pair_drop_zeros(cols);
    const std::vector<uint8_t> rok = pair_contains_flags(rows), cok = pair_contains_flags(cols);
    CMI_HIP(h, hipSetDevice(h->device));
    CMI_HIP(h, hipStreamSynchronize(h->stream));
    slim_free_ratings(h);
    hipError_t e = pair_upload(rows, &h->d_rptr, &h->d_ridx, &h->d_rval, h->stream);
    if (e == hipSuccess) e = abi_upload(&h->d_rok, rok, h->stream, true);
    if (e == hipSuccess) e = pair_upload(cols, &h->d_cptr, &h->d_cidx, &h->d_cval, h->stream);
    if (e == hipSuccess) e = abi_upload(&h->d_cok, cok, h->stream, true);
    if (e == hipSuccess) e = hipMalloc((void **)&h->d_mean, (size_t)h->n_items * sizeof(double));
    if (e == hipSuccess) e = hipMalloc((void **)&h->d_norm2, (size_t)h->n_items * sizeof(double));
    if (e == hipSuccess)
        e = knn_launch_row_stats(PairCsr{h->d_cptr, h->d_cidx, h->d_cval, h->d_cok}, h->n_items, h->d_mean, h->d_norm2, h->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
    if (e != hipSuccess) {
        slim_free_ratings(h);
        CMI_FAIL(h, CMI_E_HIP, "cmi_slim_set_ratings: %s", hipGetErrorString(e));
    }
    h->col_len.resize((size_t)h->n_items);
    for (int j = 0; j < h->n_items; ++j) h->col_len[(size_t)j] = cols.ptr[(size_t)j + 1] - cols.ptr[(size_t)j];
    h->have_ratings = true;
    return CMI_OK;
}

extern "C" int cmi_slim_set_ratings(cmi_slim_handle h, int64_t n, const int32_t *u, const int32_t *i, const double *r) {
    if (!h) return CMI_E_INVALID;
    return abi_barrier(h->err, "cmi_slim_set_ratings", [&] { return slim_set_ratings_impl(h, n, u, i, r); }, [h] { slim_free_ratings(h); });
}

namespace {
// SLIM.java:96-109 for one item: `sims` is the item's row of the similarity matrix (NaN unset).  Three tables of java_hash.hpp: the
// map nns, the same map kept by clear() and refilled with the survivors of the cut, and the set guava keeps per key.  false: a bin
// would treeify.
bool slim_cut(const double *sims, int n, int knn, std::vector<int32_t> &out) {
    std::vector<int32_t> key; // the keys of the table being filled, in put order
    const auto hash_at = [&](size_t t) { return (uint32_t)key[t]; };
    for (int i = 0; i < n; ++i)
        if (sims[i] == sims[i] && sims[i] != 0.0) key.push_back(i);
    JavaHashTable nns(16);
    nns.fill(hash_at, key.size());
    if (nns.tree) return false;
    std::vector<size_t> pos = nns.order(hash_at, key.size());
    if (knn < (int)key.size()) { // Lists.sortMap(nns, true): stable, descending by value; nns.clear(); the first knn are put back
        std::stable_sort(pos.begin(), pos.end(), [&](size_t a, size_t b) { return sims[key[a]] > sims[key[b]]; });
        std::vector<int32_t> kept((size_t)knn);
        for (size_t t = 0; t < kept.size(); ++t) kept[t] = key[pos[t]];
        key.swap(kept);
        nns.fill(hash_at, key.size());
        if (nns.tree) return false;
        pos = nns.order(hash_at, key.size());
    }
    std::vector<int32_t> in_map(key.size()); // the set receives the keys in the map's order
    for (size_t t = 0; t < in_map.size(); ++t) in_map[t] = key[pos[t]];
    key.swap(in_map);
    JavaHashTable set(4);
    set.fill(hash_at, key.size());
    if (set.tree) return false;
    out.clear();
    for (size_t p : set.order(hash_at, key.size())) out.push_back(key[p]);
    return true;
}
} // namespace

// host-only: SLIM.java:96-109 for one item, without a device (the cut and the two hash orders of cmi_slim_build_neighbors)
extern "C" int cmi_slim_cut_neighbors(int32_t n, const double *sims, int knn, int32_t *out, int32_t *n_out) {
    return abi_barrier(cmi_thread_err(), "cmi_slim_cut_neighbors", [&] {
        if (n < 0 || knn < 1 || (n > 0 && (!sims || !out)) || !n_out)
            return abi_fail(cmi_thread_err(), CMI_E_INVALID, "cmi_slim_cut_neighbors: invalid argument");
        std::vector<int32_t> lst;
        if (!slim_cut(sims, n, knn, lst))
            return abi_fail(cmi_thread_err(), CMI_E_UNSUPPORTED,
                            "cmi_slim_cut_neighbors: the list would treeify a java.util.HashMap bin, whose iteration order is not modelled");
        std::copy(lst.begin(), lst.end(), out);
        *n_out = (int32_t)lst.size();
        return CMI_OK;
    });
}

static int slim_build_impl(cmi_slim_handle h, int knn, int measure, int shrinkage, double min_rate, double max_rate) {
    const char *fn = "cmi_slim_build_neighbors";
    if (!h->have_ratings) CMI_FAIL(h, CMI_E_INVALID, "%s: no ratings (cmi_slim_set_ratings first)", fn);
    if (measure < CMI_SIM_PCC || measure > CMI_SIM_EXJACCARD) CMI_FAIL(h, CMI_E_INVALID, "%s: unknown measure %d", fn, measure);
    CMI_HIP(h, hipSetDevice(h->device));
    CMI_HIP(h, hipStreamSynchronize(h->stream));
    slim_free_lists(h);
    const int n = h->n_items;
    std::vector<int32_t> live; // train.columns()
    for (int j = 0; j < n; ++j)
        if (h->col_len[(size_t)j] > 0) live.push_back(j);
    // reserved before anything runs: the similarity matrix and, per list entry, its index, weight and loss term
    const size_t per = knn > 0 ? (size_t)std::min<int64_t>(knn, std::max(0, (int)live.size() - 1)) : live.size();
    const size_t sim_bytes = knn > 0 ? (size_t)n * (size_t)n * sizeof(double) : 0;
    const size_t bytes = sim_bytes + (size_t)n * per * 20 + ((size_t)n + 1) * 12 + 8;
    size_t free_b = 0, total_b = 0;
    CMI_HIP(h, hipMemGetInfo(&free_b, &total_b));
    if (bytes > free_b)
        CMI_FAIL(h, CMI_E_INVALID, "%s: the lists and weights of %d items (%zu entries a list%s) need %zu bytes of device memory, %zu are free", fn,
                 n, per, knn > 0 ? ", and the similarity matrix" : "", bytes, free_b);
    // the device buffers of the lists, allocated now: a build never fails half-way for memory
    const size_t cap = (size_t)n * per; // list entries at most
    struct Scratch { // the similarity matrix lives for this call only, whatever ends it
        double *S = nullptr;
        ~Scratch() { abi_free(S); }
    } sim;
    hipError_t e = hipMalloc((void **)&h->d_nptr, ((size_t)n + 1) * sizeof(int64_t));
    if (e == hipSuccess) e = hipMalloc((void **)&h->d_order, std::max<size_t>((size_t)n, 1) * sizeof(int32_t));
    if (e == hipSuccess) e = hipMalloc((void **)&h->d_nidx, std::max<size_t>(cap, 1) * sizeof(int32_t));
    if (e == hipSuccess) e = hipMalloc((void **)&h->d_w, std::max<size_t>(cap, 1) * sizeof(double));
    if (e == hipSuccess) e = hipMalloc((void **)&h->d_term, std::max<size_t>(cap, 1) * sizeof(double));
    if (e == hipSuccess) e = hipMalloc((void **)&h->d_loss, sizeof(double));
    if (e == hipSuccess && knn > 0) e = hipMalloc((void **)&sim.S, std::max<size_t>(sim_bytes, 8));
    if (e != hipSuccess) {
        slim_free_lists(h);
        CMI_FAIL(h, CMI_E_INVALID, "%s: the lists and weights of %d items%s need %zu bytes of device memory: %s", fn, n,
                 knn > 0 ? " and the similarity matrix" : "", bytes, hipGetErrorString(e));
    }
    h->nptr.assign((size_t)n + 1, 0);
    if (knn > 0) {
        std::vector<std::vector<int32_t>> lists((size_t)n); // at most knn entries each
        int rc = pair_timed_build(h, [&] {
            CMI_HIP(h, hipMemsetAsync(sim.S, 0xff, sim_bytes, h->stream)); // all-ones bits: NaN, "unset"
            CMI_HIP(h, knn_launch_build(PairCsr{h->d_cptr, h->d_cidx, h->d_cval, h->d_cok}, n, h->d_norm2, measure, shrinkage,
                                        (min_rate + max_rate) / 2.0, sim.S, h->stream));
            return CMI_OK;
        });
        // the cut, on the host, over blocks of rows of about 64 MiB
        const int block = (int)std::max<int64_t>(1, std::min<int64_t>(n, ((int64_t)64 << 20) / ((int64_t)n * 8)));
        std::vector<double> S((size_t)block * (size_t)n);
        std::atomic<int> tree{0};
        for (int j0 = 0; j0 < n && rc == CMI_OK; j0 += block) {
            const int nb = std::min(block, n - j0);
            rc = abi_hip(h->err, fn, hipMemcpy(S.data(), sim.S + (size_t)j0 * n, (size_t)nb * n * sizeof(double), hipMemcpyDeviceToHost));
            if (rc != CMI_OK) break;
            parallel_ranges(nb, host_threads((int64_t)nb * n), [&](int, int64_t b, int64_t e2) {
                for (int64_t a = b; a < e2; ++a)
                    if (!slim_cut(S.data() + (size_t)a * n, n, knn, lists[(size_t)(j0 + a)])) ++tree;
            });
        }
        if (rc == CMI_OK && tree.load())
            rc = abi_fail(h->err, CMI_E_UNSUPPORTED, "%s: %d list(s) would treeify a java.util.HashMap bin, whose iteration order is not modelled",
                          fn, tree.load());
        if (rc != CMI_OK) {
            slim_free_lists(h);
            return rc;
        }
        for (int j = 0; j < n; ++j) h->nptr[(size_t)j + 1] = h->nptr[(size_t)j] + (int64_t)lists[(size_t)j].size();
        h->nidx.resize((size_t)h->nptr[(size_t)n]);
        for (int j = 0; j < n; ++j) std::copy(lists[(size_t)j].begin(), lists[(size_t)j].end(), h->nidx.begin() + h->nptr[(size_t)j]);
    } else { // every list is train.columns(), written where it stays
        for (int j = 0; j < n; ++j) h->nptr[(size_t)j + 1] = h->nptr[(size_t)j] + (int64_t)live.size();
        h->nidx.resize((size_t)h->nptr[(size_t)n]);
        for (int j = 0; j < n; ++j) std::copy(live.begin(), live.end(), h->nidx.begin() + h->nptr[(size_t)j]);
        h->build_ms = 0.f;
        h->built = true;
    }
    // the columns with a list, by descending work (the entries its coordinates walk); the short lists (weights in LDS) first
    const auto len_of = [&](int32_t j) { return h->nptr[(size_t)j + 1] - h->nptr[(size_t)j]; };
    std::vector<int64_t> work((size_t)n, 0);
    std::vector<int32_t> order;
    h->lds_len = 0;
    for (int j = 0; j < n; ++j) {
        for (int64_t p = h->nptr[(size_t)j]; p < h->nptr[(size_t)j + 1]; ++p) work[(size_t)j] += h->col_len[(size_t)h->nidx[(size_t)p]];
        if (len_of(j) > 0) order.push_back(j);
        if (len_of(j) <= SLIM_WTILE) h->lds_len = std::max(h->lds_len, (int)len_of(j));
    }
    std::stable_sort(order.begin(), order.end(), [&](int32_t a, int32_t b) { return work[(size_t)a] > work[(size_t)b]; });
    h->n_lds = (int)(std::stable_partition(order.begin(), order.end(), [&](int32_t j) { return len_of(j) <= SLIM_WTILE; }) - order.begin());
    h->n_big = (int)order.size() - h->n_lds;
    const size_t ne = h->nidx.size();
    e = hipMemcpyAsync(h->d_nptr, h->nptr.data(), h->nptr.size() * sizeof(int64_t), hipMemcpyHostToDevice, h->stream);
    if (e == hipSuccess && ne) e = hipMemcpyAsync(h->d_nidx, h->nidx.data(), ne * sizeof(int32_t), hipMemcpyHostToDevice, h->stream);
    if (e == hipSuccess && !order.empty())
        e = hipMemcpyAsync(h->d_order, order.data(), order.size() * sizeof(int32_t), hipMemcpyHostToDevice, h->stream);
    if (e == hipSuccess) e = hipMemsetAsync(h->d_w, 0, std::max<size_t>(ne, 1) * sizeof(double), h->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
    if (e != hipSuccess) {
        slim_free_lists(h);
        CMI_FAIL(h, CMI_E_HIP, "%s: %s", fn, hipGetErrorString(e));
    }
    h->have_lists = true;
    return CMI_OK;
}

extern "C" int cmi_slim_build_neighbors(cmi_slim_handle h, int knn, int measure, int shrinkage, double min_rate, double max_rate) {
    if (!h) return CMI_E_INVALID;
    return abi_barrier(h->err, "cmi_slim_build_neighbors", [&] { return slim_build_impl(h, knn, measure, shrinkage, min_rate, max_rate); },
                       [h] { slim_free_lists(h); });
}

extern "C" int cmi_slim_get_neighbors(cmi_slim_handle h, int64_t *ptr, int32_t *idx) {
    if (!h) return CMI_E_INVALID;
    if (!h->have_lists) CMI_FAIL(h, CMI_E_INVALID, "cmi_slim_get_neighbors: no lists (cmi_slim_build_neighbors first)");
    if (!ptr) CMI_FAIL(h, CMI_E_INVALID, "cmi_slim_get_neighbors: null ptr");
    std::copy(h->nptr.begin(), h->nptr.end(), ptr);
    if (idx) std::copy(h->nidx.begin(), h->nidx.end(), idx);
    return CMI_OK;
}

extern "C" int cmi_slim_set_weights(cmi_slim_handle h, const double *w) {
    if (!h) return CMI_E_INVALID;
    if (!h->have_lists) CMI_FAIL(h, CMI_E_INVALID, "cmi_slim_set_weights: no lists (cmi_slim_build_neighbors first)");
    if (!w && !h->nidx.empty()) CMI_FAIL(h, CMI_E_INVALID, "cmi_slim_set_weights: null weights");
    CMI_HIP(h, hipSetDevice(h->device));
    if (!h->nidx.empty()) CMI_HIP(h, hipMemcpyAsync(h->d_w, w, h->nidx.size() * sizeof(double), hipMemcpyHostToDevice, h->stream));
    CMI_HIP(h, hipStreamSynchronize(h->stream));
    h->have_weights = true;
    return CMI_OK;
}

extern "C" int cmi_slim_get_weights(cmi_slim_handle h, double *w) {
    if (!h) return CMI_E_INVALID;
    if (!h->have_lists) CMI_FAIL(h, CMI_E_INVALID, "cmi_slim_get_weights: no lists (cmi_slim_build_neighbors first)");
    if (!w && !h->nidx.empty()) CMI_FAIL(h, CMI_E_INVALID, "cmi_slim_get_weights: null weights");
    CMI_HIP(h, hipSetDevice(h->device));
    if (!h->nidx.empty()) CMI_HIP(h, hipMemcpyAsync(w, h->d_w, h->nidx.size() * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    CMI_HIP(h, hipStreamSynchronize(h->stream));
    return CMI_OK;
}

static PairCsr slim_rows(const cmi_slim_instance *h) { return PairCsr{h->d_rptr, h->d_ridx, h->d_rval, h->d_rok}; }
static SlimLists slim_lists(const cmi_slim_instance *h) { return SlimLists{h->d_nptr, h->d_nidx, h->d_w}; }

extern "C" int cmi_slim_iterate(cmi_slim_handle h, double l1, double l2, double *loss) {
    if (!h) return CMI_E_INVALID;
    if (!h->have_lists) CMI_FAIL(h, CMI_E_INVALID, "cmi_slim_iterate: no lists (cmi_slim_build_neighbors first)");
    if (!h->have_weights) CMI_FAIL(h, CMI_E_INVALID, "cmi_slim_iterate: no weights (cmi_slim_set_weights first)");
    CMI_HIP(h, hipSetDevice(h->device));
    const PairCsr rows = slim_rows(h), cols{h->d_cptr, h->d_cidx, h->d_cval};
    const SlimLists L = slim_lists(h);
    CMI_HIP(h, hipEventRecord(h->ev0, h->stream));
    CMI_HIP(h, slim_launch_sweep(rows, cols, L, h->d_term, h->d_order, h->n_lds, h->lds_len, l1, l2, h->stream));
    CMI_HIP(h, slim_launch_sweep(rows, cols, L, h->d_term, h->d_order + h->n_lds, h->n_big, /*lds_len=*/0, l1, l2, h->stream));
    CMI_HIP(h, hipEventRecord(h->ev1, h->stream));
    CMI_HIP(h, slim_launch_loss(h->d_term, (int64_t)h->nidx.size(), h->d_loss, h->stream));
    CMI_HIP(h, hipEventRecord(h->ev2, h->stream));
    double l = 0.0;
    CMI_HIP(h, hipMemcpyAsync(&l, h->d_loss, sizeof l, hipMemcpyDeviceToHost, h->stream));
    CMI_HIP(h, hipStreamSynchronize(h->stream));
    CMI_HIP(h, hipEventElapsedTime(&h->iter_ms[0], h->ev0, h->ev1));
    CMI_HIP(h, hipEventElapsedTime(&h->iter_ms[1], h->ev1, h->ev2));
    h->iterated = true;
    if (loss) *loss = l;
    if (std::isnan(l) || std::isinf(l)) CMI_FAIL(h, CMI_E_NUMERIC, "cmi_slim_iterate: loss is NaN or Infinity");
    return CMI_OK;
}

static int slim_predict_impl(cmi_slim_handle h, int64_t n, const int32_t *u, const int32_t *j, double *out) {
    if (!h->have_weights) CMI_FAIL(h, CMI_E_INVALID, "cmi_slim_predict_batch: no weights (cmi_slim_build_neighbors and cmi_slim_set_weights first)");
    if (int rc = pair_check_tuples(h, "cmi_slim_predict_batch", n, u, j, out)) return rc;
    if (n == 0) return CMI_OK;
    return abi_predict(h, "cmi_slim_predict_batch", n, u, j, nullptr, nullptr, 0, out, [&](const AbiTuples &t, double *d_out) {
        return abi_hip(h->err, "cmi_slim_predict_batch", slim_launch_predict(slim_rows(h), slim_lists(h), n, t.a, t.b, d_out, h->stream));
    });
}

extern "C" int cmi_slim_predict_batch(cmi_slim_handle h, int64_t n, const int32_t *u, const int32_t *j, double *out) {
    if (!h) return CMI_E_INVALID;
    return abi_barrier(h->err, "cmi_slim_predict_batch", [&] { return slim_predict_impl(h, n, u, j, out); });
}

extern "C" int cmi_slim_eval_rankings(cmi_slim_handle h, int64_t n_train, const int32_t *tu, const int32_t *tj, const int32_t *tctx,
                                      const double *tr, int64_t n_test, const int32_t *su, const int32_t *sj, const int32_t *sctx,
                                      const double *sr, double bin_thold, int num_recs, int num_ignore, int strategy, double out[21],
                                      int64_t *n_queries, int32_t *q_user, int32_t *q_ctx, int32_t *q_count, int32_t *top_items,
                                      double *top_scores) {
    if (!h) return CMI_E_INVALID;
    return abi_barrier(h->err, "slim_eval_rankings", [&] {
        auto ready = [h]() -> int {
            if (!h->have_weights) CMI_FAIL(h, CMI_E_INVALID, "slim: call cmi_slim_build_neighbors and cmi_slim_set_weights first");
            CMI_HIP(h, hipSetDevice(h->device));
            return CMI_OK;
        };
        auto score = [&](const RankPlan &plan, const RankBatchFn &on_batch) {
            const RankSlabFn fill = [h](double *dS, const int32_t *dcand, int nc, const int32_t *dgu, const int32_t *dgq0, int g0, int g1,
                                        int64_t q0, int64_t nq, hipStream_t s) {
                return slim_launch_score(slim_rows(h), slim_lists(h), dcand, nc, dgu, dgq0, g0, g1, q0, nq, dS, s);
            };
            return rank_run_device_slab(h->stream, h->rank_ws, plan, fill, bin_thold, num_recs, on_batch, nullptr);
        };
        const RankEvalIO io{{n_train, tu, tj, tctx, tr}, {n_test, su, sj, sctx, sr}, bin_thold, num_recs, num_ignore, strategy, out, n_queries,
                            q_user, q_ctx, q_count, top_items, top_scores};
        return rank_evaluate(h->err, "slim_eval_rankings", h->rank_ws, h->n_users, h->n_items, INT64_MAX, io, ready, score);
    });
}

extern "C" int cmi_slim_last_build_ms(cmi_slim_handle h, float *ms) { return pair_last_build_ms(h, "cmi_slim_last_build_ms", ms); }

extern "C" int cmi_slim_last_iter_ms(cmi_slim_handle h, float *ms) {
    if (!h || !ms) return CMI_E_INVALID;
    if (!h->iterated) CMI_FAIL(h, CMI_E_INVALID, "cmi_slim_last_iter_ms: no iteration yet");
    ms[0] = h->iter_ms[0], ms[1] = h->iter_ms[1];
    return CMI_OK;
}
