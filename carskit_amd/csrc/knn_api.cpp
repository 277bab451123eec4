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
#include "rank_host.hpp"

using namespace cmi;

struct cmi_knn_instance : PairModelBase {
    int kind = CMI_KNN_ITEM;
    int n_ent = 0, n_ctr = 0; // compared rows (items for ItemKNN, users for UserKNN) and the contracted index
    // rows: entity -> (contracted index, value); lists: contracted index -> (entity, value).  Both CSR, ascending.
    int32_t *d_rptr = nullptr, *d_ridx = nullptr, *d_lptr = nullptr, *d_lidx = nullptr;
    uint8_t *d_rok = nullptr;
    double *d_rval = nullptr, *d_lval = nullptr, *d_mean = nullptr, *d_norm2 = nullptr, *d_S = nullptr;
    std::vector<int32_t> list_len; // per list (contracted index): its length, for the candidate limit
    RankWorkspace rank_ws;
    float rank_ms = 0.f; // scoring and selection of the last cmi_knn_eval_rankings
    bool evaluated = false;
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

static void knn_free_all(cmi_knn_instance *h) {
    knn_free_ratings(h);
    h->rank_ws.release();
}

extern "C" int cmi_knn_destroy(cmi_knn_handle h) { return pair_destroy(h, knn_free_all); }

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

namespace {
// the scratch of a prediction or an evaluation and its treeify record, freed with the call whatever ends it (the stream is drained then)
struct KnnCallScratch {
    KnnScratch s{nullptr, nullptr, nullptr, nullptr, nullptr};
    int32_t *d_bad = nullptr;
    int nwaves = 1, cap = 1;
    // one wave per unit of work in flight; every wave owns `cap` entries (the longest list it may meet) of each scratch array (32 bytes
    // an entry), at most ~1 GiB
    hipError_t alloc(int64_t units, int longest, hipStream_t stream) {
        cap = std::max(1, longest);
        const int64_t by_mem = std::max<int64_t>(1, ((int64_t)1 << 30) / ((int64_t)cap * 32));
        nwaves = (int)std::max<int64_t>(1, std::min<int64_t>({units, 8192, by_mem}));
        const size_t ns = (size_t)nwaves * cap;
        hipError_t e = hipMalloc((void **)&d_bad, 3 * sizeof(int32_t));
        if (e == hipSuccess) e = hipMalloc((void **)&s.key, ns * 4);
        if (e == hipSuccess) e = hipMalloc((void **)&s.pos, ns * 4);
        if (e == hipSuccess) e = hipMalloc((void **)&s.sel, ns * 4);
        if (e == hipSuccess) e = hipMalloc((void **)&s.sim, ns * 8);
        if (e == hipSuccess) e = hipMalloc((void **)&s.dlt, ns * 8);
        if (e == hipSuccess) e = hipMemsetAsync(d_bad, 0, 3 * sizeof(int32_t), stream);
        return e;
    }
    ~KnnCallScratch() { abi_free(d_bad, s.key, s.pos, s.sel, s.sim, s.dlt); }
};
} // namespace

static PairCsr knn_lists(const cmi_knn_instance *h) { return PairCsr{h->d_lptr, h->d_lidx, h->d_lval}; }

// fn: cmi_knn_predict_batch (ranking false) or cmi_knn_ranking_batch (ranking true, unbounded)
static int knn_predict_impl(cmi_knn_handle h, const char *fn, int64_t n, const int32_t *u, const int32_t *j, int knn, double gm, bool ranking,
                            int bound, double lo, double hi, double *out) {
    if (!h->built) CMI_FAIL(h, CMI_E_INVALID, "%s: no similarity matrix (cmi_knn_build first)", fn);
    if (int rc = pair_check_tuples(h, fn, n, u, j, out)) return rc;
    if (n == 0) return CMI_OK;
    const bool item = h->kind == CMI_KNN_ITEM;
    const int32_t *owner = item ? u : j, *target = item ? j : u; // ItemKNN: the user's items scored against item j; UserKNN: the reverse
    int cap = 1;
    for (int64_t t = 0; t < n; ++t) {
        const int len = h->list_len[(size_t)owner[t]];
        if (len > CMI_KNN_MAX_CANDIDATES)
            CMI_FAIL(h, CMI_E_UNSUPPORTED, "%s: tuple %lld has %d candidates, more than CMI_KNN_MAX_CANDIDATES (%d)", fn, (long long)t, len,
                     CMI_KNN_MAX_CANDIDATES);
        cap = std::max(cap, len);
    }
    KnnCallScratch k;
    int32_t bad[3] = {0, 0, 0};
    const int rc = abi_predict(h, fn, n, owner, target, nullptr, nullptr, 0, out, [&](const AbiTuples &t, double *d_out) {
        hipError_t e = k.alloc(n, cap, h->stream);
        if (e == hipSuccess)
            e = knn_launch_predict(knn_lists(h), h->d_S, h->n_ent, h->d_mean, n, t.a, t.b, knn, gm, ranking, bound, lo, hi, d_out, k.nwaves,
                                   k.cap, k.s, k.d_bad, h->stream);
        if (e == hipSuccess) e = hipMemcpyAsync(bad, k.d_bad, sizeof bad, hipMemcpyDeviceToHost, h->stream);
        return abi_hip(h->err, fn, e);
    });
    if (rc != CMI_OK) return rc;
    if (bad[0] && ranking)
        CMI_FAIL(h, CMI_E_UNSUPPORTED,
                 "%s: %d tuple(s) would treeify a java.util.HashMap bin, whose iteration order is not modelled, (user %d, item %d) among them",
                 fn, bad[0], item ? bad[1] : bad[2], item ? bad[2] : bad[1]);
    if (bad[0])
        CMI_FAIL(h, CMI_E_UNSUPPORTED, "%s: %d tuple(s) would treeify a java.util.HashMap bin, whose iteration order is not modelled", fn,
                 bad[0]);
    return CMI_OK;
}

extern "C" int cmi_knn_predict_batch(cmi_knn_handle h, int64_t n, const int32_t *u, const int32_t *j, int knn, double global_mean,
                                     int bound, double lo, double hi, double *out) {
    if (!h) return CMI_E_INVALID;
    return abi_barrier(h->err, "cmi_knn_predict_batch",
                       [&] { return knn_predict_impl(h, "cmi_knn_predict_batch", n, u, j, knn, global_mean, false, bound, lo, hi, out); });
}

// Recommender.ranking(u, j, c) = predict(u, j, c, false) (Recommender.java:1016-1018) with isRankingPred set (ItemKNN.java:92-95,
// UserKNN.java:94-97)
extern "C" int cmi_knn_ranking_batch(cmi_knn_handle h, int64_t n, const int32_t *u, const int32_t *j, int knn, double global_mean,
                                     double *out) {
    if (!h) return CMI_E_INVALID;
    return abi_barrier(h->err, "cmi_knn_ranking_batch",
                       [&] { return knn_predict_impl(h, "cmi_knn_ranking_batch", n, u, j, knn, global_mean, true, 0, 0.0, 0.0, out); });
}

// Recommender.evalRankings (Recommender.java:668-964) with that ranking(u, j) as the scorer
extern "C" int cmi_knn_eval_rankings(cmi_knn_handle h, int knn, double global_mean, int64_t n_train, const int32_t *tu, const int32_t *tj,
                                     const int32_t *tctx, const double *tr, int64_t n_test, const int32_t *su, const int32_t *sj,
                                     const int32_t *sctx, const double *sr, double bin_thold, int num_recs, int num_ignore, int strategy,
                                     double out[21], int64_t *n_queries, int32_t *q_user, int32_t *q_ctx, int32_t *q_count,
                                     int32_t *top_items, double *top_scores) {
    if (!h) return CMI_E_INVALID;
    return abi_barrier(h->err, "knn_eval_rankings", [&] {
        const bool item = h->kind == CMI_KNN_ITEM;
        auto ready = [h]() -> int {
            if (!h->built) CMI_FAIL(h, CMI_E_INVALID, "knn: call cmi_knn_set_ratings and cmi_knn_build first");
            CMI_HIP(h, hipSetDevice(h->device));
            return CMI_OK;
        };
        KnnCallScratch k;
        std::string refused; // a list past the limit: nothing runs
        auto score = [&](const RankPlan &plan, const RankBatchFn &on_batch) -> hipError_t {
            // the owner lists of this evaluation: the query users' rows (ItemKNN) or the candidates' columns (UserKNN)
            const std::vector<int32_t> &owners = item ? plan.gu : plan.cand;
            int longest = 1;
            for (int32_t o : owners) {
                const int len = h->list_len[(size_t)o];
                if (len > CMI_KNN_MAX_CANDIDATES) {
                    char msg[160];
                    snprintf(msg, sizeof msg, "%s %d has %d candidates, more than CMI_KNN_MAX_CANDIDATES (%d)", item ? "user" : "item", o, len,
                             CMI_KNN_MAX_CANDIDATES);
                    refused = msg;
                    return hipErrorInvalidValue;
                }
                longest = std::max(longest, len);
            }
            const int64_t tiles = ((int64_t)plan.cand.size() + KNN_SCORE_TILE - 1) / KNN_SCORE_TILE;
            if (hipError_t e = k.alloc((int64_t)plan.gu.size() * tiles, longest, h->stream)) return e;
            const RankSlabFn fill = [&](double *dS, const int32_t *dcand, int nc, const int32_t *dgu, const int32_t *dgq0, int g0, int g1,
                                        int64_t q0, int64_t nq, hipStream_t s) {
                return knn_launch_score(item, knn_lists(h), h->d_S, h->n_ent, h->d_mean, knn, global_mean, k.nwaves, k.cap, k.s, k.d_bad, dcand,
                                        nc, dgu, dgq0, g0, g1, q0, nq, dS, s);
            };
            return rank_run_device_slab(h->stream, h->rank_ws, plan, fill, bin_thold, num_recs, on_batch, &h->rank_ms);
        };
        const RankEvalIO io{{n_train, tu, tj, tctx, tr}, {n_test, su, sj, sctx, sr}, bin_thold, num_recs, num_ignore, strategy, out, n_queries,
                            q_user, q_ctx, q_count, top_items, top_scores};
        const int rc = rank_evaluate(h->err, "knn_eval_rankings", h->rank_ws, h->n_users, h->n_items, INT64_MAX, io, ready, score);
        if (!refused.empty()) CMI_FAIL(h, CMI_E_UNSUPPORTED, "knn_eval_rankings: %s", refused.c_str());
        if (rc != CMI_OK) return rc;
        if (k.d_bad) { // (no queries or no candidates: nothing was scored)
            int32_t bad[3] = {0, 0, 0};
            CMI_HIP(h, hipMemcpyAsync(bad, k.d_bad, sizeof bad, hipMemcpyDeviceToHost, h->stream));
            CMI_HIP(h, hipStreamSynchronize(h->stream));
            if (bad[0])
                CMI_FAIL(h, CMI_E_UNSUPPORTED,
                         "knn_eval_rankings: %d tuple(s) would treeify a java.util.HashMap bin, whose iteration order is not modelled, (user "
                         "%d, item %d) among them",
                         bad[0], bad[1], bad[2]);
        }
        h->evaluated = true;
        return CMI_OK;
    });
}

extern "C" int cmi_knn_last_rank_ms(cmi_knn_handle h, float *ms) {
    if (!h || !ms) return CMI_E_INVALID;
    if (!h->evaluated) CMI_FAIL(h, CMI_E_INVALID, "cmi_knn_last_rank_ms: no evaluation yet");
    *ms = h->rank_ms;
    return CMI_OK;
}

extern "C" int cmi_knn_last_build_ms(cmi_knn_handle h, float *ms) { return pair_last_build_ms(h, "cmi_knn_last_build_ms", ms); }
