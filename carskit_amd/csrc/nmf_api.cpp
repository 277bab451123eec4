// nmf_api.cpp -- C ABI of NMF (include/carskit_mi355x.h, cmi_nmf_*).
#include "../../include/carskit_mi355x.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <numeric>
#include <string>
#include <vector>

#include "nmf_kernels.hpp"
#include "pair_host.hpp"
#include "rank_host.hpp"
#include "rank_kernels.hpp"
#include "rankals_kernels.hpp"

using namespace cmi;

struct cmi_nmf_instance : PairModelBase {
    int k = 0;
    int64_t nnz = 0;      // cells with a non-zero value: the others take no part (SparseMatrix.row() / column() leave them out)
    int n_uorder = 0, n_iorder = 0;
    // rows: user -> (item, value), cols: item -> (user, value), both CSR, ascending; cu: the user of every cell of rows; uorder / iorder:
    // the users / items with entries, longest first
    int32_t *d_rptr = nullptr, *d_ridx = nullptr, *d_cptr = nullptr, *d_cidx = nullptr, *d_cu = nullptr, *d_uorder = nullptr,
            *d_iorder = nullptr;
    double *d_rval = nullptr, *d_cval = nullptr, *d_part = nullptr, *d_loss = nullptr;
    double *d_W = nullptr, *d_Ht = nullptr; // W: n_users x k; Ht: n_items x k (H item-major)
    bool have_model = false, iterated = false;
    hipEvent_t ev2 = nullptr, ev3 = nullptr;
    float iter_ms[3] = {0.f, 0.f, 0.f};
    RankWorkspace rank_ws;
    float rank_ms = 0.f; // scoring and selection of the last cmi_topn_nmf_eval_rankings
    bool evaluated = false;
};

static thread_local std::string g_nmf_create_err;

extern "C" const char *cmi_nmf_last_error(cmi_nmf_handle h) { return h ? h->err.c_str() : g_nmf_create_err.c_str(); }

static void nmf_free_ratings(cmi_nmf_instance *h) {
    abi_free(h->d_rptr, h->d_ridx, h->d_cptr, h->d_cidx, h->d_cu, h->d_uorder, h->d_iorder, h->d_rval, h->d_cval, h->d_part, h->d_loss);
    h->have_ratings = h->iterated = false;
}

static void nmf_free_all(cmi_nmf_instance *h) {
    nmf_free_ratings(h);
    abi_free(h->d_W, h->d_Ht);
    h->have_model = false;
    h->rank_ws.release();
    if (h->ev2) (void)hipEventDestroy(h->ev2);
    if (h->ev3) (void)hipEventDestroy(h->ev3);
    h->ev2 = h->ev3 = nullptr;
}

extern "C" int cmi_nmf_destroy(cmi_nmf_handle h) { return pair_destroy(h, nmf_free_all); }

extern "C" int cmi_nmf_create(int k, int n_users, int n_items, int device, unsigned flags, cmi_nmf_handle *out) {
    (void)flags;
    int rc = pair_create(g_nmf_create_err, "cmi_nmf_create", k >= 1 && k <= NMF_MAX_K, n_users, n_items, device, out, cmi_nmf_destroy,
                         [k](cmi_nmf_instance *h) { h->k = k; });
    if (rc != CMI_OK) return rc;
    cmi_nmf_instance *h = *out;
    hipError_t e = hipEventCreate(&h->ev2);
    if (e == hipSuccess) e = hipEventCreate(&h->ev3);
    if (e != hipSuccess) {
        cmi_nmf_destroy(h);
        *out = nullptr;
        return abi_fail(g_nmf_create_err, CMI_E_HIP, "cmi_nmf_create: %s", hipGetErrorString(e));
    }
    return CMI_OK;
}

// the rows with entries, longest first (equal lengths in index order): the longest chain starts first
static std::vector<int32_t> nmf_order(const PairHostCsr &m) {
    std::vector<int32_t> ord;
    for (size_t row = 0; row + 1 < m.ptr.size(); ++row)
        if (m.ptr[row + 1] > m.ptr[row]) ord.push_back((int32_t)row);
    std::stable_sort(ord.begin(), ord.end(), [&](int32_t a, int32_t b) {
        return m.ptr[(size_t)a + 1] - m.ptr[(size_t)a] > m.ptr[(size_t)b + 1] - m.ptr[(size_t)b];
    });
    return ord;
}

static int nmf_set_ratings_impl(cmi_nmf_handle h, int64_t n, const int32_t *u, const int32_t *i, const double *r) {
    PairHostCsr rows, cols;
    if (int rc = pair_ingest(h, "cmi_nmf_set_ratings", n, u, i, r, /*scan_items=*/false, rows, cols)) return rc;
    rows = pair_drop_zeros(rows), cols = pair_drop_zeros(cols);
    const std::vector<int32_t> uorder = nmf_order(rows), iorder = nmf_order(cols);
    std::vector<int32_t> cu(rows.idx.size());
    for (int a = 0; a < h->n_users; ++a) std::fill(cu.begin() + rows.ptr[(size_t)a], cu.begin() + rows.ptr[(size_t)a + 1], a);
    CMI_HIP(h, hipSetDevice(h->device));
    CMI_HIP(h, hipStreamSynchronize(h->stream));
    nmf_free_ratings(h);
    const size_t n_part = (size_t)nmf_loss_blocks((int64_t)rows.idx.size());
    hipError_t e = pair_upload(rows, &h->d_rptr, &h->d_ridx, &h->d_rval, h->stream);
    if (e == hipSuccess) e = pair_upload(cols, &h->d_cptr, &h->d_cidx, &h->d_cval, h->stream);
    if (e == hipSuccess) e = abi_upload(&h->d_cu, cu, h->stream, true);
    if (e == hipSuccess) e = abi_upload(&h->d_uorder, uorder, h->stream, true);
    if (e == hipSuccess) e = abi_upload(&h->d_iorder, iorder, h->stream, true);
    if (e == hipSuccess) e = hipMalloc((void **)&h->d_part, std::max<size_t>(n_part, 1) * sizeof(double));
    if (e == hipSuccess) e = hipMalloc((void **)&h->d_loss, sizeof(double));
    if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
    if (e != hipSuccess) {
        nmf_free_ratings(h);
        CMI_FAIL(h, CMI_E_HIP, "cmi_nmf_set_ratings: %s", hipGetErrorString(e));
    }
    h->nnz = (int64_t)rows.idx.size();
    h->n_uorder = (int)uorder.size(), h->n_iorder = (int)iorder.size();
    h->have_ratings = true;
    return CMI_OK;
}

extern "C" int cmi_nmf_set_ratings(cmi_nmf_handle h, int64_t n, const int32_t *u, const int32_t *i, const double *r) {
    if (!h) return CMI_E_INVALID;
    return abi_barrier(h->err, "cmi_nmf_set_ratings", [&] { return nmf_set_ratings_impl(h, n, u, i, r); }, [h] { nmf_free_ratings(h); });
}

// H (k x n_items, the reference's layout) <-> Ht (n_items x k, the device's)
static std::vector<double> nmf_transpose(const double *src, int rows, int cols) {
    std::vector<double> t((size_t)rows * cols);
    for (int a = 0; a < rows; ++a)
        for (int b = 0; b < cols; ++b) t[(size_t)b * rows + a] = src[(size_t)a * cols + b];
    return t;
}

static int nmf_set_model_impl(cmi_nmf_handle h, const double *W, const double *H) {
    if (!h->have_model && (!W || !H)) CMI_FAIL(h, CMI_E_INVALID, "cmi_nmf_set_model: the first call sets both W and H");
    CMI_HIP(h, hipSetDevice(h->device));
    const size_t wn = (size_t)h->n_users * h->k, hn = (size_t)h->n_items * h->k;
    if (!h->d_W) {
        hipError_t e = hipMalloc((void **)&h->d_W, wn * sizeof(double));
        if (e == hipSuccess) e = hipMalloc((void **)&h->d_Ht, hn * sizeof(double));
        if (e != hipSuccess) {
            abi_free(h->d_W, h->d_Ht);
            CMI_FAIL(h, CMI_E_HIP, "cmi_nmf_set_model: %s", hipGetErrorString(e));
        }
    }
    std::vector<double> ht;
    if (H) ht = nmf_transpose(H, h->k, h->n_items);
    if (W) CMI_HIP(h, hipMemcpyAsync(h->d_W, W, wn * sizeof(double), hipMemcpyHostToDevice, h->stream));
    if (H) CMI_HIP(h, hipMemcpyAsync(h->d_Ht, ht.data(), hn * sizeof(double), hipMemcpyHostToDevice, h->stream));
    CMI_HIP(h, hipStreamSynchronize(h->stream));
    h->have_model = true;
    return CMI_OK;
}

// NMF.java:56-65 (initModel's W and H, drawn by the host) and any later injection
extern "C" int cmi_nmf_set_model(cmi_nmf_handle h, const double *W, const double *H) {
    if (!h) return CMI_E_INVALID;
    return abi_barrier(h->err, "cmi_nmf_set_model", [&] { return nmf_set_model_impl(h, W, H); });
}

static int nmf_get_model_impl(cmi_nmf_handle h, double *W, double *H) {
    if (!h->have_model) CMI_FAIL(h, CMI_E_INVALID, "cmi_nmf_get_model: no model (cmi_nmf_set_model first)");
    CMI_HIP(h, hipSetDevice(h->device));
    const size_t wn = (size_t)h->n_users * h->k, hn = (size_t)h->n_items * h->k;
    std::vector<double> ht(H ? hn : 0);
    if (W) CMI_HIP(h, hipMemcpyAsync(W, h->d_W, wn * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    if (H) CMI_HIP(h, hipMemcpyAsync(ht.data(), h->d_Ht, hn * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    CMI_HIP(h, hipStreamSynchronize(h->stream));
    if (H) {
        const std::vector<double> t = nmf_transpose(ht.data(), h->n_items, h->k);
        std::copy(t.begin(), t.end(), H);
    }
    return CMI_OK;
}

extern "C" int cmi_nmf_get_model(cmi_nmf_handle h, double *W, double *H) {
    if (!h) return CMI_E_INVALID;
    return abi_barrier(h->err, "cmi_nmf_get_model", [&] { return nmf_get_model_impl(h, W, H); });
}

// one pass of NMF.buildModel's loop body (NMF.java:71-126): the W phase, the H phase with the new W, the loss
extern "C" int cmi_nmf_iterate(cmi_nmf_handle h, double *loss) {
    if (!h) return CMI_E_INVALID;
    if (!h->have_ratings) CMI_FAIL(h, CMI_E_INVALID, "cmi_nmf_iterate: no ratings (cmi_nmf_set_ratings first)");
    if (!h->have_model) CMI_FAIL(h, CMI_E_INVALID, "cmi_nmf_iterate: no model (cmi_nmf_set_model first)");
    CMI_HIP(h, hipSetDevice(h->device));
    const PairCsr rows{h->d_rptr, h->d_ridx, h->d_rval}, cols{h->d_cptr, h->d_cidx, h->d_cval};
    CMI_HIP(h, hipEventRecord(h->ev0, h->stream));
    CMI_HIP(h, nmf_launch_rows(h->d_W, h->d_Ht, rows, h->d_uorder, h->n_uorder, h->k, h->stream));
    CMI_HIP(h, hipEventRecord(h->ev1, h->stream));
    CMI_HIP(h, nmf_launch_rows(h->d_Ht, h->d_W, cols, h->d_iorder, h->n_iorder, h->k, h->stream));
    CMI_HIP(h, hipEventRecord(h->ev2, h->stream));
    CMI_HIP(h, nmf_launch_loss(h->d_W, h->d_Ht, rows, h->d_cu, h->nnz, h->k, h->d_part, h->d_loss, h->stream));
    CMI_HIP(h, hipEventRecord(h->ev3, h->stream));
    double l = 0.0;
    CMI_HIP(h, hipMemcpyAsync(&l, h->d_loss, sizeof l, hipMemcpyDeviceToHost, h->stream));
    CMI_HIP(h, hipStreamSynchronize(h->stream));
    CMI_HIP(h, hipEventElapsedTime(&h->iter_ms[0], h->ev0, h->ev1));
    CMI_HIP(h, hipEventElapsedTime(&h->iter_ms[1], h->ev1, h->ev2));
    CMI_HIP(h, hipEventElapsedTime(&h->iter_ms[2], h->ev2, h->ev3));
    h->iterated = true;
    if (loss) *loss = l;
    if (std::isnan(l) || std::isinf(l)) CMI_FAIL(h, CMI_E_NUMERIC, "cmi_nmf_iterate: loss is NaN or Infinity");
    return CMI_OK;
}

static int nmf_predict_impl(cmi_nmf_handle h, int64_t n, const int32_t *u, const int32_t *j, int bound, double lo, double hi, double *out) {
    if (!h->have_model) CMI_FAIL(h, CMI_E_INVALID, "cmi_nmf_predict_batch: no model (cmi_nmf_set_model first)");
    if (int rc = pair_check_tuples(h, "cmi_nmf_predict_batch", n, u, j, out)) return rc;
    if (n == 0) return CMI_OK;
    return abi_predict(h, "cmi_nmf_predict_batch", n, u, j, nullptr, nullptr, 0, out, [&](const AbiTuples &t, double *d_out) {
        return abi_hip(h->err, "cmi_nmf_predict_batch", nmf_launch_predict(h->d_W, h->d_Ht, h->k, n, t.a, t.b, bound, lo, hi, d_out, h->stream));
    });
}

// NMF.java:142-145 (predict) and Recommender.predict(u, j, c, true)'s bound
extern "C" int cmi_nmf_predict_batch(cmi_nmf_handle h, int64_t n, const int32_t *u, const int32_t *j, int bound, double lo, double hi,
                                     double *out) {
    if (!h) return CMI_E_INVALID;
    return abi_barrier(h->err, "cmi_nmf_predict_batch", [&] { return nmf_predict_impl(h, n, u, j, bound, lo, hi, out); });
}

// NMF scores its slabs with rankals_launch_score, whose kernel keeps a row of W in an LDS array of RANK_SCORE_MAX_K doubles: the wider
// models NMF trains (up to NMF_MAX_K) are refused by cmi_topn_nmf_eval_rankings
static_assert(RANK_SCORE_MAX_K < NMF_MAX_K, "every k NMF trains fits rankals_launch_score: drop the refusal in cmi_topn_nmf_eval_rankings");

// Recommender.evalRankings (Recommender.java:668-964) with ranking(u, j, c) = predict(u, j, c, false) (Recommender.java:1016-1018),
// NMF.predict (NMF.java:142-145) = product(W, u, H, j) unbounded, as the scorer
extern "C" int cmi_topn_nmf_eval_rankings(cmi_nmf_handle h, int64_t n_train, const int32_t *tu, const int32_t *tj, const int32_t *tctx,
                                     const double *tr, int64_t n_test, const int32_t *su, const int32_t *sj, const int32_t *sctx,
                                     const double *sr, double bin_thold, int num_recs, int num_ignore, int strategy, double out[21],
                                     int64_t *n_queries, int32_t *q_user, int32_t *q_ctx, int32_t *q_count, int32_t *top_items,
                                     double *top_scores) {
    if (!h) return CMI_E_INVALID;
    return abi_barrier(h->err, "nmf_eval_rankings", [&] {
        auto ready = [h]() -> int {
            if (!h->have_model) CMI_FAIL(h, CMI_E_INVALID, "nmf: call cmi_nmf_set_model first");
            if (h->k > RANK_SCORE_MAX_K)
                CMI_FAIL(h, CMI_E_UNSUPPORTED, "nmf_eval_rankings: k = %d: the scoring kernel keeps a user's row of W in LDS, k <= %d", h->k,
                         RANK_SCORE_MAX_K);
            CMI_HIP(h, hipSetDevice(h->device));
            return CMI_OK;
        };
        auto score = [&](const RankPlan &plan, const RankBatchFn &on_batch) {
            const RankSlabFn fill = [h](double *dS, const int32_t *dcand, int nc, const int32_t *dgu, const int32_t *dgq0, int g0, int g1,
                                        int64_t q0, int64_t nq, hipStream_t s) {
                return rankals_launch_score(h->d_W, h->d_Ht, h->k, dcand, nc, dgu, dgq0, g0, g1, q0, nq, dS, s);
            };
            return rank_run_device_slab(h->stream, h->rank_ws, plan, fill, bin_thold, num_recs, on_batch, &h->rank_ms);
        };
        const RankEvalIO io{{n_train, tu, tj, tctx, tr}, {n_test, su, sj, sctx, sr}, bin_thold, num_recs, num_ignore, strategy, out, n_queries,
                            q_user, q_ctx, q_count, top_items, top_scores};
        const int rc = rank_evaluate(h->err, "nmf_eval_rankings", h->rank_ws, h->n_users, h->n_items, INT64_MAX, io, ready, score);
        if (rc == CMI_OK) h->evaluated = true;
        return rc;
    });
}

extern "C" int cmi_topn_nmf_last_rank_ms(cmi_nmf_handle h, float *ms) {
    if (!h || !ms) return CMI_E_INVALID;
    if (!h->evaluated) CMI_FAIL(h, CMI_E_INVALID, "cmi_topn_nmf_last_rank_ms: no evaluation yet");
    *ms = h->rank_ms;
    return CMI_OK;
}

extern "C" int cmi_nmf_last_iter_ms(cmi_nmf_handle h, float *ms) {
    if (!h || !ms) return CMI_E_INVALID;
    if (!h->iterated) CMI_FAIL(h, CMI_E_INVALID, "cmi_nmf_last_iter_ms: no iteration yet");
    std::copy(h->iter_ms, h->iter_ms + 3, ms);
    return CMI_OK;
}
