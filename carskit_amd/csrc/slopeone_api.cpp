// slopeone_api.cpp -- C ABI of SlopeOne (include/carskit_mi355x.h, cmi_slope_*).
#include "../../include/carskit_mi355x.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <string>
#include <vector>

#include "pair_host.hpp"
#include "rank_host.hpp"
#include "slopeone_kernels.hpp"

using namespace cmi;

struct cmi_slope_instance : PairModelBase {
    // cols: item -> (user, value), for the build; rows: user -> (item, value), for the prediction.  Both CSR, ascending.
    int32_t *d_cptr = nullptr, *d_cidx = nullptr, *d_rptr = nullptr, *d_ridx = nullptr, *d_card = nullptr;
    double *d_cval = nullptr, *d_rval = nullptr, *d_dev = nullptr;
    RankWorkspace rank_ws;
    float rank_ms = 0.f; // scoring and selection of the last cmi_slope_eval_rankings
    bool evaluated = false;
};

static thread_local std::string g_slope_create_err;

extern "C" const char *cmi_slope_last_error(cmi_slope_handle h) { return h ? h->err.c_str() : g_slope_create_err.c_str(); }

static void slope_free_ratings(cmi_slope_instance *h) {
    abi_free(h->d_cptr, h->d_cidx, h->d_rptr, h->d_ridx, h->d_card, h->d_cval, h->d_rval, h->d_dev);
    h->have_ratings = h->built = false;
}

static void slope_free_all(cmi_slope_instance *h) {
    slope_free_ratings(h);
    h->rank_ws.release();
}

extern "C" int cmi_slope_destroy(cmi_slope_handle h) { return pair_destroy(h, slope_free_all); }

extern "C" int cmi_slope_create(int n_users, int n_items, int device, unsigned flags, cmi_slope_handle *out) {
    (void)flags;
    return pair_create(g_slope_create_err, "cmi_slope_create", /*valid=*/true, n_users, n_items, device, out, cmi_slope_destroy,
                       [](cmi_slope_instance *) {});
}

static int slope_set_ratings_impl(cmi_slope_handle h, int64_t n, const int32_t *u, const int32_t *i, const double *r) {
    PairHostCsr rows, cols;
    if (int rc = pair_ingest(h, "cmi_slope_set_ratings", n, u, i, r, /*scan_items=*/false, rows, cols)) return rc;
    CMI_HIP(h, hipSetDevice(h->device));
    CMI_HIP(h, hipStreamSynchronize(h->stream));
    slope_free_ratings(h);
    hipError_t e = pair_upload(cols, &h->d_cptr, &h->d_cidx, &h->d_cval, h->stream);
    if (e == hipSuccess) e = pair_upload(rows, &h->d_rptr, &h->d_ridx, &h->d_rval, h->stream);
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
    const size_t cells = (size_t)h->n_items * (size_t)h->n_items;
    const auto alloc = [&] { // the two dense n x n matrices
        hipError_t e = hipMalloc((void **)&h->d_dev, cells * sizeof(double));
        if (e == hipSuccess) e = hipMalloc((void **)&h->d_card, cells * sizeof(int32_t));
        if (e != hipSuccess) abi_free(h->d_dev, h->d_card);
        return e;
    };
    if (!h->d_dev)
        if (int rc = pair_reserve_dense(h, "cmi_slope_build", h->n_items, cells * (sizeof(double) + sizeof(int32_t)),
                                        "deviation and cardinality matrices", /*plural=*/true, alloc))
            return rc;
    return pair_timed_build(h, [&] {
        CMI_HIP(h, hipMemsetAsync(h->d_dev, 0, cells * sizeof(double), h->stream)); // +0.0 and 0: "no common user"
        CMI_HIP(h, hipMemsetAsync(h->d_card, 0, cells * sizeof(int32_t), h->stream));
        CMI_HIP(h, slope_launch_build(PairCsr{h->d_cptr, h->d_cidx, h->d_cval}, h->n_items, h->d_dev, h->d_card, h->stream));
        return CMI_OK;
    });
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
    if (int rc = pair_check_tuples(h, "cmi_slope_predict_batch", n, u, j, out)) return rc;
    if (n == 0) return CMI_OK;
    const int nwaves = (int)std::min<int64_t>(n, 16384); // one wave per tuple in flight
    return abi_predict(h, "cmi_slope_predict_batch", n, u, j, nullptr, nullptr, 0, out, [&](const AbiTuples &t, double *d_out) {
        return abi_hip(h->err, "cmi_slope_predict_batch",
                       slope_launch_predict(PairCsr{h->d_rptr, h->d_ridx, h->d_rval}, h->d_dev, h->d_card, h->n_items, n, t.a, t.b, gm, bound,
                                            lo, hi, d_out, nwaves, h->stream));
    });
}

extern "C" int cmi_slope_predict_batch(cmi_slope_handle h, int64_t n, const int32_t *u, const int32_t *j, double global_mean, int bound,
                                       double lo, double hi, double *out) {
    if (!h) return CMI_E_INVALID;
    return abi_barrier(h->err, "cmi_slope_predict_batch", [&] { return slope_predict_impl(h, n, u, j, global_mean, bound, lo, hi, out); });
}

// Recommender.evalRankings (Recommender.java:668-964) with ranking(u, j, c) = predict(u, j, c, false) (Recommender.java:1016-1018),
// SlopeOne.predict unbounded, as the scorer
extern "C" int cmi_slope_eval_rankings(cmi_slope_handle h, double global_mean, int64_t n_train, const int32_t *tu, const int32_t *tj,
                                       const int32_t *tctx, const double *tr, int64_t n_test, const int32_t *su, const int32_t *sj,
                                       const int32_t *sctx, const double *sr, double bin_thold, int num_recs, int num_ignore, int strategy,
                                       double out[21], int64_t *n_queries, int32_t *q_user, int32_t *q_ctx, int32_t *q_count,
                                       int32_t *top_items, double *top_scores) {
    if (!h) return CMI_E_INVALID;
    return abi_barrier(h->err, "slope_eval_rankings", [&] {
        auto ready = [h]() -> int {
            if (!h->built) CMI_FAIL(h, CMI_E_INVALID, "slope: call cmi_slope_set_ratings and cmi_slope_build first");
            CMI_HIP(h, hipSetDevice(h->device));
            return CMI_OK;
        };
        auto score = [&](const RankPlan &plan, const RankBatchFn &on_batch) {
            const RankSlabFn fill = [h, global_mean](double *dS, const int32_t *dcand, int nc, const int32_t *dgu, const int32_t *dgq0, int g0,
                                                     int g1, int64_t q0, int64_t nq, hipStream_t s) {
                return slope_launch_score(PairCsr{h->d_rptr, h->d_ridx, h->d_rval}, h->d_dev, h->d_card, h->n_items, global_mean, dcand, nc,
                                          dgu, dgq0, g0, g1, q0, nq, dS, s);
            };
            return rank_run_device_slab(h->stream, h->rank_ws, plan, fill, bin_thold, num_recs, on_batch, &h->rank_ms);
        };
        const RankEvalIO io{{n_train, tu, tj, tctx, tr}, {n_test, su, sj, sctx, sr}, bin_thold, num_recs, num_ignore, strategy, out, n_queries,
                            q_user, q_ctx, q_count, top_items, top_scores};
        const int rc = rank_evaluate(h->err, "slope_eval_rankings", h->rank_ws, h->n_users, h->n_items, INT64_MAX, io, ready, score);
        if (rc == CMI_OK) h->evaluated = true;
        return rc;
    });
}

extern "C" int cmi_slope_last_rank_ms(cmi_slope_handle h, float *ms) {
    if (!h || !ms) return CMI_E_INVALID;
    if (!h->evaluated) CMI_FAIL(h, CMI_E_INVALID, "cmi_slope_last_rank_ms: no evaluation yet");
    *ms = h->rank_ms;
    return CMI_OK;
}

extern "C" int cmi_slope_last_build_ms(cmi_slope_handle h, float *ms) { return pair_last_build_ms(h, "cmi_slope_last_build_ms", ms); }
