// rankals_api.cpp -- C ABI of RankALS (include/carskit_mi355x.h, cmi_rankals_*).
#include "../../include/carskit_mi355x.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <string>
#include <vector>

#include "pair_host.hpp"
#include "rank_host.hpp"
#include "rankals_kernels.hpp"

using namespace cmi;

struct cmi_rankals_instance : PairModelBase {
    int k = 0, n_rows = 0;
    // rows: user -> (item, value); cols: item -> (user, value); both CSR, ascending, without the zero-valued cells; users: train.rows()
    int32_t *d_rptr = nullptr, *d_ridx = nullptr, *d_cptr = nullptr, *d_cidx = nullptr, *d_users = nullptr;
    double *d_rval = nullptr, *d_cval = nullptr;
    double *d_s[2] = {nullptr, nullptr}; // s_i without and with support weighting
    double sum_s[2] = {0.0, 0.0};
    double *d_P = nullptr, *d_Q = nullptr;
    double *d_work = nullptr; // one allocation: sum_sq, sum_sqq, the m_* arrays, the item-independent sums (rankals_state)
    bool have_model = false, iterated = false, evaluated = false; // iterated / evaluated: iter_ms[0..3] / iter_ms[4] hold a time
    hipEvent_t ev[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    float iter_ms[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
    RankWorkspace rank_ws;
};

static thread_local std::string g_rankals_create_err;

extern "C" const char *cmi_rankals_last_error(cmi_rankals_handle h) { return h ? h->err.c_str() : g_rankals_create_err.c_str(); }

static void rankals_free_ratings(cmi_rankals_instance *h) {
    abi_free(h->d_rptr, h->d_ridx, h->d_cptr, h->d_cidx, h->d_users, h->d_rval, h->d_cval, h->d_s[0], h->d_s[1]);
    h->have_ratings = h->iterated = false;
}

static void rankals_free_all(cmi_rankals_instance *h) {
    rankals_free_ratings(h);
    abi_free(h->d_P, h->d_Q, h->d_work);
    h->have_model = false;
    h->rank_ws.release();
    for (hipEvent_t &e : h->ev) {
        if (e) (void)hipEventDestroy(e);
        e = nullptr;
    }
}

extern "C" int cmi_rankals_destroy(cmi_rankals_handle h) { return pair_destroy(h, rankals_free_all); }

// doubles of d_work
static size_t rankals_work_doubles(const cmi_rankals_instance *h) {
    const size_t k = (size_t)h->k, nu = (size_t)h->n_users;
    return k + k * k + 3 * nu + 2 * nu * k + 2 * k * k + 2 * k;
}

// RankALS.java:47-79 (numFactors, the shapes of P and Q).  The solve keeps two k x k matrices in LDS: k <= 64
extern "C" int cmi_rankals_create(int k, int n_users, int n_items, int device, unsigned flags, cmi_rankals_handle *out) {
    (void)flags;
    if (out && k > RANKALS_MAX_K) {
        *out = nullptr;
        return abi_fail(g_rankals_create_err, CMI_E_UNSUPPORTED,
                        "cmi_rankals_create: %d factors: the solve keeps two k x k matrices of doubles in LDS (16 k^2 bytes), k <= %d", k,
                        RANKALS_MAX_K);
    }
    int rc = pair_create(g_rankals_create_err, "cmi_rankals_create", k >= 1, n_users, n_items, device, out, cmi_rankals_destroy,
                         [k](cmi_rankals_instance *h) { h->k = k; });
    if (rc != CMI_OK) return rc;
    cmi_rankals_instance *h = *out;
    hipError_t e = hipSuccess;
    for (hipEvent_t &ev : h->ev)
        if (e == hipSuccess) e = hipEventCreate(&ev);
    if (e == hipSuccess) e = hipMalloc((void **)&h->d_work, rankals_work_doubles(h) * sizeof(double));
    if (e != hipSuccess) {
        cmi_rankals_destroy(h);
        *out = nullptr;
        return abi_fail(g_rankals_create_err, CMI_E_HIP, "cmi_rankals_create: %s", hipGetErrorString(e));
    }
    return CMI_OK;
}

static int rankals_set_ratings_impl(cmi_rankals_handle h, int64_t n, const int32_t *u, const int32_t *i, const double *r) {
    PairHostCsr rows, cols;
    if (int rc = pair_ingest(h, "cmi_rankals_set_ratings", n, u, i, r, /*scan_items=*/false, rows, cols)) return rc;
    // a stored 0.0 takes no part: librec's row(u), its getCount(), rows(), columnSize(i) and get(u, i) > 0 all see the non-zero cells only
    rows = pair_drop_zeros(rows), cols = pair_drop_zeros(cols);
    std::vector<int32_t> users; // train.rows()
    for (int a = 0; a < h->n_users; ++a)
        if (rows.ptr[(size_t)a + 1] > rows.ptr[(size_t)a]) users.push_back(a);
    std::vector<double> s_off((size_t)h->n_items, 1.0), s_on((size_t)h->n_items);
    double sum_off = 0.0, sum_on = 0.0; // RankALS.java:73-79: one chain over the items ascending
    for (int j = 0; j < h->n_items; ++j) {
        s_on[(size_t)j] = (double)(cols.ptr[(size_t)j + 1] - cols.ptr[(size_t)j]);
        sum_off += 1.0;
        sum_on += s_on[(size_t)j];
    }
    CMI_HIP(h, hipSetDevice(h->device));
    CMI_HIP(h, hipStreamSynchronize(h->stream));
    rankals_free_ratings(h);
    hipError_t e = pair_upload(rows, &h->d_rptr, &h->d_ridx, &h->d_rval, h->stream);
    if (e == hipSuccess) e = pair_upload(cols, &h->d_cptr, &h->d_cidx, &h->d_cval, h->stream);
    if (e == hipSuccess) e = abi_upload(&h->d_users, users, h->stream, true);
    if (e == hipSuccess) e = abi_upload(&h->d_s[0], s_off, h->stream, true);
    if (e == hipSuccess) e = abi_upload(&h->d_s[1], s_on, h->stream, true);
    if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
    if (e != hipSuccess) {
        rankals_free_ratings(h);
        CMI_FAIL(h, CMI_E_HIP, "cmi_rankals_set_ratings: %s", hipGetErrorString(e));
    }
    h->n_rows = (int)users.size();
    h->sum_s[0] = sum_off, h->sum_s[1] = sum_on;
    h->have_ratings = true;
    return CMI_OK;
}

// RankALS.java:67-79 (train, s, sum_s): the 2-D train matrix as n cells
extern "C" int cmi_rankals_set_ratings(cmi_rankals_handle h, int64_t n, const int32_t *u, const int32_t *i, const double *r) {
    if (!h) return CMI_E_INVALID;
    return abi_barrier(h->err, "cmi_rankals_set_ratings", [&] { return rankals_set_ratings_impl(h, n, u, i, r); },
                       [h] { rankals_free_ratings(h); });
}

static int rankals_set_model_impl(cmi_rankals_handle h, const double *P, const double *Q) {
    if (!h->have_model && (!P || !Q)) CMI_FAIL(h, CMI_E_INVALID, "cmi_rankals_set_model: the first call sets both P and Q");
    CMI_HIP(h, hipSetDevice(h->device));
    const size_t pn = (size_t)h->n_users * h->k, qn = (size_t)h->n_items * h->k;
    if (!h->d_P) {
        hipError_t e = hipMalloc((void **)&h->d_P, pn * sizeof(double));
        if (e == hipSuccess) e = hipMalloc((void **)&h->d_Q, qn * sizeof(double));
        if (e != hipSuccess) {
            abi_free(h->d_P, h->d_Q);
            CMI_FAIL(h, CMI_E_HIP, "cmi_rankals_set_model: %s", hipGetErrorString(e));
        }
    }
    if (P) CMI_HIP(h, hipMemcpyAsync(h->d_P, P, pn * sizeof(double), hipMemcpyHostToDevice, h->stream));
    if (Q) CMI_HIP(h, hipMemcpyAsync(h->d_Q, Q, qn * sizeof(double), hipMemcpyHostToDevice, h->stream));
    CMI_HIP(h, hipStreamSynchronize(h->stream));
    h->have_model = true;
    return CMI_OK;
}

// IterativeRecommender.java:235-241 (P and Q, drawn by the host) and any later injection
extern "C" int cmi_rankals_set_model(cmi_rankals_handle h, const double *P, const double *Q) {
    if (!h) return CMI_E_INVALID;
    return abi_barrier(h->err, "cmi_rankals_set_model", [&] { return rankals_set_model_impl(h, P, Q); });
}

extern "C" int cmi_rankals_get_model(cmi_rankals_handle h, double *P, double *Q) {
    if (!h) return CMI_E_INVALID;
    return abi_barrier(h->err, "cmi_rankals_get_model", [&] {
        if (!h->have_model) CMI_FAIL(h, CMI_E_INVALID, "cmi_rankals_get_model: no model (cmi_rankals_set_model first)");
        CMI_HIP(h, hipSetDevice(h->device));
        if (P) CMI_HIP(h, hipMemcpyAsync(P, h->d_P, (size_t)h->n_users * h->k * sizeof(double), hipMemcpyDeviceToHost, h->stream));
        if (Q) CMI_HIP(h, hipMemcpyAsync(Q, h->d_Q, (size_t)h->n_items * h->k * sizeof(double), hipMemcpyDeviceToHost, h->stream));
        CMI_HIP(h, hipStreamSynchronize(h->stream));
        return CMI_OK;
    });
}

static RankAlsState rankals_state(const cmi_rankals_instance *h, int sw) {
    RankAlsState a;
    const size_t k = (size_t)h->k, nu = (size_t)h->n_users;
    a.k = h->k, a.n_users = h->n_users, a.n_items = h->n_items, a.n_rows = h->n_rows;
    a.rows = PairCsr{h->d_rptr, h->d_ridx, h->d_rval}, a.cols = PairCsr{h->d_cptr, h->d_cidx, h->d_cval};
    a.users = h->d_users, a.s = h->d_s[sw], a.sum_s = h->sum_s[sw];
    a.P = h->d_P, a.Q = h->d_Q;
    double *w = h->d_work;
    a.sum_sq = w, w += k;
    a.sum_sqq = w, w += k * k;
    a.m_sr = w, w += nu;
    a.m_cr = w, w += nu;
    a.m_c = w, w += nu;
    a.m_cq = w, w += nu * k;
    a.ppcq_u = w, w += nu * k;
    a.cpp = w, w += k * k;
    a.ppc = w, w += k * k;
    a.ppcq = w, w += k;
    a.crp = w;
    return a;
}

// one pass of RankALS.buildModel's loop body (RankALS.java:84-205): sum_sq / sum_sqq (:91-98), the P step (:100-137) with step 3's maps
// (:140-166), the item-independent sums of the Q step (:184-189, formed once), the Q step (:168-204)
extern "C" int cmi_rankals_iterate(cmi_rankals_handle h, int support_weight) {
    if (!h) return CMI_E_INVALID;
    if (!h->have_ratings) CMI_FAIL(h, CMI_E_INVALID, "cmi_rankals_iterate: no ratings (cmi_rankals_set_ratings first)");
    if (!h->have_model) CMI_FAIL(h, CMI_E_INVALID, "cmi_rankals_iterate: no model (cmi_rankals_set_model first)");
    CMI_HIP(h, hipSetDevice(h->device));
    const RankAlsState a = rankals_state(h, support_weight ? 1 : 0);
    CMI_HIP(h, hipEventRecord(h->ev[0], h->stream));
    CMI_HIP(h, rankals_launch_item_moments(a, h->stream));
    CMI_HIP(h, hipEventRecord(h->ev[1], h->stream));
    CMI_HIP(h, rankals_launch_user_solve(a, h->stream));
    CMI_HIP(h, hipEventRecord(h->ev[2], h->stream));
    CMI_HIP(h, rankals_launch_user_moments(a, h->stream));
    CMI_HIP(h, hipEventRecord(h->ev[3], h->stream));
    CMI_HIP(h, rankals_launch_item_solve(a, h->stream));
    CMI_HIP(h, hipEventRecord(h->ev[4], h->stream));
    CMI_HIP(h, hipStreamSynchronize(h->stream));
    for (int p = 0; p < 4; ++p) CMI_HIP(h, hipEventElapsedTime(&h->iter_ms[p], h->ev[p], h->ev[p + 1]));
    h->iterated = true;
    return CMI_OK;
}

static int rankals_predict_impl(cmi_rankals_handle h, int64_t n, const int32_t *u, const int32_t *j, double *out) {
    if (!h->have_model) CMI_FAIL(h, CMI_E_INVALID, "cmi_rankals_predict_batch: no model (cmi_rankals_set_model first)");
    if (int rc = pair_check_tuples(h, "cmi_rankals_predict_batch", n, u, j, out)) return rc;
    if (n == 0) return CMI_OK;
    return abi_predict(h, "cmi_rankals_predict_batch", n, u, j, nullptr, nullptr, 0, out, [&](const AbiTuples &t, double *d_out) {
        return abi_hip(h->err, "cmi_rankals_predict_batch", rankals_launch_predict(h->d_P, h->d_Q, h->k, n, t.a, t.b, d_out, h->stream));
    });
}

// IterativeRecommender.predict(u, j) = DenseMatrix.rowMult(P, u, Q, j) of n tuples
extern "C" int cmi_rankals_predict_batch(cmi_rankals_handle h, int64_t n, const int32_t *u, const int32_t *j, double *out) {
    if (!h) return CMI_E_INVALID;
    return abi_barrier(h->err, "cmi_rankals_predict_batch", [&] { return rankals_predict_impl(h, n, u, j, out); });
}

extern "C" int cmi_rankals_eval_rankings(cmi_rankals_handle h, int64_t n_train, const int32_t *tu, const int32_t *tj, const int32_t *tctx,
                                         const double *tr, int64_t n_test, const int32_t *su, const int32_t *sj, const int32_t *sctx,
                                         const double *sr, double bin_thold, int num_recs, int num_ignore, int strategy, double out[21],
                                         int64_t *n_queries, int32_t *q_user, int32_t *q_ctx, int32_t *q_count, int32_t *top_items,
                                         double *top_scores) {
    if (!h) return CMI_E_INVALID;
    return abi_barrier(h->err, "rankals_eval_rankings", [&] {
        auto ready = [h]() -> int {
            if (!h->have_model) CMI_FAIL(h, CMI_E_INVALID, "rankals: call cmi_rankals_set_model first");
            CMI_HIP(h, hipSetDevice(h->device));
            return CMI_OK;
        };
        auto score = [&](const RankPlan &plan, const RankBatchFn &on_batch) {
            const RankSlabFn fill = [h](double *dS, const int32_t *dcand, int nc, const int32_t *dgu, const int32_t *dgq0, int g0, int g1,
                                        int64_t q0, int64_t nq, hipStream_t s) {
                return rankals_launch_score(h->d_P, h->d_Q, h->k, dcand, nc, dgu, dgq0, g0, g1, q0, nq, dS, s);
            };
            return rank_run_device_slab(h->stream, h->rank_ws, plan, fill, bin_thold, num_recs, on_batch, &h->iter_ms[4]);
        };
        const RankEvalIO io{{n_train, tu, tj, tctx, tr}, {n_test, su, sj, sctx, sr}, bin_thold, num_recs, num_ignore, strategy, out, n_queries,
                            q_user, q_ctx, q_count, top_items, top_scores};
        const int rc = rank_evaluate(h->err, "rankals_eval_rankings", h->rank_ws, h->n_users, h->n_items, INT64_MAX, io, ready, score);
        if (rc == CMI_OK) h->evaluated = true;
        return rc;
    });
}

extern "C" int cmi_rankals_last_iter_ms(cmi_rankals_handle h, float *ms) {
    if (!h || !ms) return CMI_E_INVALID;
    if (!h->iterated && !h->evaluated) CMI_FAIL(h, CMI_E_INVALID, "cmi_rankals_last_iter_ms: no iteration and no evaluation yet");
    for (int p = 0; p < 4; ++p) ms[p] = h->iterated ? h->iter_ms[p] : 0.f;
    ms[4] = h->evaluated ? h->iter_ms[4] : 0.f;
    return CMI_OK;
}

static int rankals_invert_impl(cmi_rankals_handle h, int n_mats, int n, const double *A, double *out) {
    const char *fn = "cmi_rankals_invert";
    if (n_mats < 0 || n < 1 || (n_mats > 0 && (!A || !out))) CMI_FAIL(h, CMI_E_INVALID, "%s: invalid argument", fn);
    if (n > RANKALS_MAX_K)
        CMI_FAIL(h, CMI_E_UNSUPPORTED, "%s: n = %d: the two n x n matrices of doubles stay in LDS (16 n^2 bytes), n <= %d", fn, n, RANKALS_MAX_K);
    if (n_mats == 0) return CMI_OK;
    CMI_HIP(h, hipSetDevice(h->device));
    const size_t bytes = (size_t)n_mats * n * n * sizeof(double);
    double *dA = nullptr, *dO = nullptr;
    hipError_t e = hipMalloc((void **)&dA, bytes);
    if (e == hipSuccess) e = hipMalloc((void **)&dO, bytes);
    if (e == hipSuccess) e = hipMemcpyAsync(dA, A, bytes, hipMemcpyHostToDevice, h->stream);
    if (e == hipSuccess) e = rankals_launch_invert(dA, dO, n_mats, n, h->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(out, dO, bytes, hipMemcpyDeviceToHost, h->stream);
    const hipError_t es = hipStreamSynchronize(h->stream);
    if (e == hipSuccess) e = es;
    abi_free(dA, dO);
    return abi_hip(h->err, fn, e);
}

// librec DenseMatrix.inv() of n_mats n x n matrices by the device routine both solves use
extern "C" int cmi_rankals_invert(cmi_rankals_handle h, int n_mats, int n, const double *A, double *out) {
    if (!h) return CMI_E_INVALID;
    return abi_barrier(h->err, "cmi_rankals_invert", [&] { return rankals_invert_impl(h, n_mats, n, A, out); });
}
