// lrmf_api.cpp -- C ABI of LRMF (include/carskit_mi355x.h, cmi_lrmf_*): the host preparation of a matrix (lrmf_host.hpp), the launches
// of its unit schedule, the loss, prediction and top-N evaluation over the shared pipeline.
#include "../../include/carskit_mi355x.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <string>
#include <vector>

#include "bpr_kernels.hpp"
#include "lrmf_kernels.hpp"
#include "pair_host.hpp"
#include "rank_host.hpp"
#include "rankals_kernels.hpp"

using namespace cmi;

struct cmi_lrmf_instance : PairModelBase {
    int k = 0;
    unsigned flags = 0;
    int64_t n = 0; // cells
    LrmfPlan plan;
    int32_t *d_ptr = nullptr, *d_col = nullptr, *d_order = nullptr;
    double *d_A = nullptr;
    uint8_t *d_nz = nullptr;
    double *d_slots = nullptr, *d_parts = nullptr, *d_loss = nullptr;
    double *d_P = nullptr, *d_Q = nullptr;
    bool have_model = false, iterated = false, evaluated = false;
    hipEvent_t ev[3] = {nullptr, nullptr, nullptr};
    float iter_ms[3] = {0.f, 0.f, 0.f};
    RankWorkspace rank_ws;
};

static thread_local std::string g_lrmf_err;

extern "C" const char *cmi_lrmf_last_error(cmi_lrmf_handle h) { return h ? h->err.c_str() : g_lrmf_err.c_str(); }
extern "C" int cmi_lrmf_lds_rows(int k) { return k >= 1 && k <= LRMF_MAX_K ? lrmf_lds_rows(k) : 0; }
extern "C" int cmi_lrmf_block(void) { return LRMF_BLOCK; }

static void lrmf_free_ratings(cmi_lrmf_instance *h) {
    abi_free(h->d_ptr, h->d_col, h->d_order, h->d_A, h->d_nz, h->d_slots, h->d_parts, h->d_loss);
    h->have_ratings = h->iterated = false;
}

static void lrmf_free_all(cmi_lrmf_instance *h) {
    lrmf_free_ratings(h);
    abi_free(h->d_P, h->d_Q);
    h->have_model = false;
    h->rank_ws.release();
    for (hipEvent_t &e : h->ev) {
        if (e) (void)hipEventDestroy(e);
        e = nullptr;
    }
}

extern "C" int cmi_lrmf_destroy(cmi_lrmf_handle h) { return pair_destroy(h, lrmf_free_all); }

// LRMF.java:46-53.  A lane per factor applies a cell's update and P[u] has LRMF_MAX_K doubles of LDS: k <= 128
extern "C" int cmi_lrmf_create(int k, int n_users, int n_items, int device, unsigned flags, cmi_lrmf_handle *out) {
    if (out && k > LRMF_MAX_K) {
        *out = nullptr;
        return abi_fail(g_lrmf_err, CMI_E_UNSUPPORTED, "cmi_lrmf_create: %d factors: a workgroup holds P[u] in %d doubles of LDS, k <= %d", k,
                        LRMF_MAX_K, LRMF_MAX_K);
    }
    const bool valid = k >= 1 && (flags & ~(CMI_LRMF_FLAG_STRICT | CMI_LRMF_FLAG_GLOBAL_ROWS)) == 0;
    int rc = pair_create(g_lrmf_err, "cmi_lrmf_create", valid, n_users, n_items, device, out, cmi_lrmf_destroy,
                         [k, flags](cmi_lrmf_instance *h) { h->k = k, h->flags = flags; });
    if (rc != CMI_OK) return rc;
    cmi_lrmf_instance *h = *out;
    hipError_t e = hipSuccess;
    for (hipEvent_t &ev : h->ev)
        if (e == hipSuccess) e = hipEventCreate(&ev);
    if (e != hipSuccess) {
        cmi_lrmf_destroy(h);
        *out = nullptr;
        return abi_fail(g_lrmf_err, CMI_E_HIP, "cmi_lrmf_create: %s", hipGetErrorString(e));
    }
    return CMI_OK;
}

// LRMF.java:55-67 and the model-independent part of :70-110, once per matrix
static int lrmf_set_ratings_impl(cmi_lrmf_handle h, int64_t n, const int32_t *u, const int32_t *i, const double *r) {
    const char *fn = "cmi_lrmf_set_ratings";
    PairHostCsr all, cols;
    if (int rc = pair_ingest(h, fn, n, u, i, r, /*scan_items=*/false, all, cols)) return rc;
    if (n * (int64_t)(h->k + 1) >= ((int64_t)1 << 40)) CMI_FAIL(h, CMI_E_UNSUPPORTED, "%s: %lld cells of %d loss terms each", fn, (long long)n, h->k + 1);
    CMI_HIP(h, hipSetDevice(h->device));
    CMI_HIP(h, hipStreamSynchronize(h->stream));
    lrmf_free_ratings(h);
    const int32_t lds_rows = (h->flags & CMI_LRMF_FLAG_GLOBAL_ROWS) ? 0 : lrmf_lds_rows(h->k);
    lrmf_prepare(h->n_users, h->n_items, all.ptr.data(), all.idx.data(), all.val.data(), lds_rows, h->plan);
    h->n = n;
    hipError_t e = abi_upload(&h->d_ptr, all.ptr, h->stream, true);
    if (e == hipSuccess) e = abi_upload(&h->d_col, all.idx, h->stream, true);
    if (e == hipSuccess) e = abi_upload(&h->d_order, h->plan.order, h->stream, true);
    if (e == hipSuccess) e = abi_upload(&h->d_A, h->plan.A, h->stream, true);
    if (e == hipSuccess) e = abi_upload(&h->d_nz, h->plan.nz, h->stream, true);
    if (e == hipSuccess) e = hipMalloc((void **)&h->d_slots, std::max<size_t>((size_t)n * (size_t)(h->k + 1), 1) * sizeof(double));
    if (e == hipSuccess) e = hipMalloc((void **)&h->d_parts, BPR_LOSS_PARTS * sizeof(double));
    if (e == hipSuccess) e = hipMalloc((void **)&h->d_loss, sizeof(double));
    if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
    if (e != hipSuccess) {
        lrmf_free_ratings(h);
        CMI_FAIL(h, CMI_E_HIP, "%s: %s", fn, hipGetErrorString(e));
    }
    h->have_ratings = true;
    return CMI_OK;
}

extern "C" int cmi_lrmf_set_ratings(cmi_lrmf_handle h, int64_t n, const int32_t *u, const int32_t *i, const double *r) {
    if (!h) return CMI_E_INVALID;
    return abi_barrier(h->err, "cmi_lrmf_set_ratings", [&] { return lrmf_set_ratings_impl(h, n, u, i, r); }, [h] { lrmf_free_ratings(h); });
}

static int lrmf_set_model_impl(cmi_lrmf_handle h, const double *P, const double *Q) {
    if (!h->have_model && (!P || !Q)) CMI_FAIL(h, CMI_E_INVALID, "cmi_lrmf_set_model: the first call sets both P and Q");
    CMI_HIP(h, hipSetDevice(h->device));
    const size_t pn = (size_t)h->n_users * h->k, qn = (size_t)h->n_items * h->k;
    if (!h->d_P) {
        hipError_t e = hipMalloc((void **)&h->d_P, pn * sizeof(double));
        if (e == hipSuccess) e = hipMalloc((void **)&h->d_Q, qn * sizeof(double));
        if (e != hipSuccess) {
            abi_free(h->d_P, h->d_Q);
            CMI_FAIL(h, CMI_E_HIP, "cmi_lrmf_set_model: %s", hipGetErrorString(e));
        }
    }
    if (P) CMI_HIP(h, hipMemcpyAsync(h->d_P, P, pn * sizeof(double), hipMemcpyHostToDevice, h->stream));
    if (Q) CMI_HIP(h, hipMemcpyAsync(h->d_Q, Q, qn * sizeof(double), hipMemcpyHostToDevice, h->stream));
    CMI_HIP(h, hipStreamSynchronize(h->stream));
    h->have_model = true;
    return CMI_OK;
}

// IterativeRecommender.java:239-245 with initByNorm = false (P and Q uniform, drawn by the host) and any later injection
extern "C" int cmi_lrmf_set_model(cmi_lrmf_handle h, const double *P, const double *Q) {
    if (!h) return CMI_E_INVALID;
    return abi_barrier(h->err, "cmi_lrmf_set_model", [&] { return lrmf_set_model_impl(h, P, Q); });
}

extern "C" int cmi_lrmf_get_model(cmi_lrmf_handle h, double *P, double *Q) {
    if (!h) return CMI_E_INVALID;
    return abi_barrier(h->err, "cmi_lrmf_get_model", [&] {
        if (!h->have_model) CMI_FAIL(h, CMI_E_INVALID, "cmi_lrmf_get_model: no model (cmi_lrmf_set_model first)");
        CMI_HIP(h, hipSetDevice(h->device));
        if (P) CMI_HIP(h, hipMemcpyAsync(P, h->d_P, (size_t)h->n_users * h->k * sizeof(double), hipMemcpyDeviceToHost, h->stream));
        if (Q) CMI_HIP(h, hipMemcpyAsync(Q, h->d_Q, (size_t)h->n_items * h->k * sizeof(double), hipMemcpyDeviceToHost, h->stream));
        CMI_HIP(h, hipStreamSynchronize(h->stream));
        return CMI_OK;
    });
}

// LRMF.java:74-104: one iteration, the launches of the unit schedule in level order, then the loss
static int lrmf_iterate_impl(cmi_lrmf_handle h, double lrate, double regU, double regI, double *loss) {
    const char *fn = "cmi_lrmf_iterate";
    if (!h->have_ratings) CMI_FAIL(h, CMI_E_INVALID, "%s: no ratings (cmi_lrmf_set_ratings first)", fn);
    if (!h->have_model) CMI_FAIL(h, CMI_E_INVALID, "%s: no model (cmi_lrmf_set_model first)", fn);
    CMI_HIP(h, hipSetDevice(h->device));
    LrmfEpoch a;
    a.k = h->k, a.P = h->d_P, a.Q = h->d_Q, a.ptr = h->d_ptr, a.col = h->d_col, a.A = h->d_A, a.nz = h->d_nz, a.order = h->d_order;
    a.slots = h->d_slots, a.lrate = lrate, a.regU = regU, a.regI = regI;
    a.lds_rows = (h->flags & CMI_LRMF_FLAG_GLOBAL_ROWS) ? 0 : lrmf_lds_rows(h->k);
    CMI_HIP(h, hipEventRecord(h->ev[0], h->stream));
    for (const LrmfLaunch &l : h->plan.launches)
        CMI_HIP(h, l.run ? lrmf_launch_run(a, l.x0, l.x1, l.rows, h->stream) : lrmf_launch_level(a, l.x0, l.x1, l.rows, h->stream));
    CMI_HIP(h, hipEventRecord(h->ev[1], h->stream));
    CMI_HIP(h, bpr_launch_loss(h->d_slots, h->n * (int64_t)(h->k + 1), (h->flags & CMI_LRMF_FLAG_STRICT) != 0, h->d_parts, h->d_loss, h->stream));
    CMI_HIP(h, hipEventRecord(h->ev[2], h->stream));
    double l = 0.0;
    CMI_HIP(h, hipMemcpyAsync(&l, h->d_loss, sizeof(double), hipMemcpyDeviceToHost, h->stream));
    CMI_HIP(h, hipStreamSynchronize(h->stream));
    CMI_HIP(h, hipEventElapsedTime(&h->iter_ms[0], h->ev[0], h->ev[1]));
    CMI_HIP(h, hipEventElapsedTime(&h->iter_ms[1], h->ev[1], h->ev[2]));
    h->iterated = true;
    if (loss) *loss = l;
    if (!std::isfinite(l)) CMI_FAIL(h, CMI_E_NUMERIC, "%s: loss = %g", fn, l);
    return CMI_OK;
}

extern "C" int cmi_lrmf_iterate(cmi_lrmf_handle h, double lrate, double regU, double regI, double *loss) {
    if (!h) return CMI_E_INVALID;
    return abi_barrier(h->err, "cmi_lrmf_iterate", [&] { return lrmf_iterate_impl(h, lrate, regU, regI, loss); });
}

static int lrmf_predict_impl(cmi_lrmf_handle h, int64_t n, const int32_t *u, const int32_t *j, double *out) {
    if (!h->have_model) CMI_FAIL(h, CMI_E_INVALID, "cmi_lrmf_predict_batch: no model (cmi_lrmf_set_model first)");
    if (int rc = pair_check_tuples(h, "cmi_lrmf_predict_batch", n, u, j, out)) return rc;
    if (n == 0) return CMI_OK;
    return abi_predict(h, "cmi_lrmf_predict_batch", n, u, j, nullptr, nullptr, 0, out, [&](const AbiTuples &t, double *d_out) {
        return abi_hip(h->err, "cmi_lrmf_predict_batch", rankals_launch_predict(h->d_P, h->d_Q, h->k, n, t.a, t.b, d_out, h->stream));
    });
}

// IterativeRecommender.predict(u, j) = DenseMatrix.rowMult(P, u, Q, j) of n tuples: RankALS's kernel
extern "C" int cmi_lrmf_predict_batch(cmi_lrmf_handle h, int64_t n, const int32_t *u, const int32_t *j, double *out) {
    if (!h) return CMI_E_INVALID;
    return abi_barrier(h->err, "cmi_lrmf_predict_batch", [&] { return lrmf_predict_impl(h, n, u, j, out); });
}

// Recommender.evalRankings (Recommender.java:630-860) with ranking(u, j, c) = predict(u, j): the shared batch pipeline
extern "C" int cmi_lrmf_eval_rankings(cmi_lrmf_handle h, int64_t n_train, const int32_t *tu, const int32_t *tj, const int32_t *tctx,
                                      const double *tr, int64_t n_test, const int32_t *su, const int32_t *sj, const int32_t *sctx,
                                      const double *sr, double bin_thold, int num_recs, int num_ignore, int strategy, double out[21],
                                      int64_t *n_queries, int32_t *q_user, int32_t *q_ctx, int32_t *q_count, int32_t *top_items,
                                      double *top_scores) {
    if (!h) return CMI_E_INVALID;
    return abi_barrier(h->err, "lrmf_eval_rankings", [&] {
        auto ready = [h]() -> int {
            if (!h->have_model) CMI_FAIL(h, CMI_E_INVALID, "lrmf: call cmi_lrmf_set_model first");
            CMI_HIP(h, hipSetDevice(h->device));
            return CMI_OK;
        };
        auto score = [&](const RankPlan &plan, const RankBatchFn &on_batch) {
            const RankSlabFn fill = [h](double *dS, const int32_t *dcand, int nc, const int32_t *dgu, const int32_t *dgq0, int g0, int g1,
                                        int64_t q0, int64_t nq, hipStream_t s) {
                static_assert(LRMF_MAX_K <= RANK_SCORE_MAX_K, "LRMF scores with RankALS's kernel: its rows must fit that kernel's LDS row");
                return rankals_launch_score(h->d_P, h->d_Q, h->k, dcand, nc, dgu, dgq0, g0, g1, q0, nq, dS, s);
            };
            return rank_run_device_slab(h->stream, h->rank_ws, plan, fill, bin_thold, num_recs, on_batch, &h->iter_ms[2]);
        };
        const RankEvalIO io{{n_train, tu, tj, tctx, tr}, {n_test, su, sj, sctx, sr}, bin_thold, num_recs, num_ignore, strategy, out, n_queries,
                            q_user, q_ctx, q_count, top_items, top_scores};
        const int rc = rank_evaluate(h->err, "lrmf_eval_rankings", h->rank_ws, h->n_users, h->n_items, INT64_MAX, io, ready, score);
        if (rc == CMI_OK) h->evaluated = true;
        return rc;
    });
}

extern "C" int cmi_lrmf_last_iter_ms(cmi_lrmf_handle h, float *ms) {
    if (!h || !ms) return CMI_E_INVALID;
    if (!h->iterated && !h->evaluated) CMI_FAIL(h, CMI_E_INVALID, "cmi_lrmf_last_iter_ms: no iteration and no evaluation yet");
    for (int p = 0; p < 2; ++p) ms[p] = h->iterated ? h->iter_ms[p] : 0.f;
    ms[2] = h->evaluated ? h->iter_ms[2] : 0.f;
    return CMI_OK;
}

extern "C" int cmi_lrmf_last_schedule(cmi_lrmf_handle h, int64_t *out) {
    if (!h || !out) return CMI_E_INVALID;
    if (!h->have_ratings) CMI_FAIL(h, CMI_E_INVALID, "cmi_lrmf_last_schedule: no ratings (cmi_lrmf_set_ratings first)");
    const LrmfPlan &p = h->plan;
    out[0] = p.n_levels, out[1] = p.alone, out[2] = p.runs, out[3] = p.widest, out[4] = p.global_units;
    return CMI_OK;
}

// ---- without a device ---------------------------------------------------------------------------------------------------------------
extern "C" int cmi_lrmf_levels(int n_users, int n_items, int64_t n, const int32_t *u, const int32_t *i, int32_t *order, int32_t *level_of,
                               int32_t *n_levels, int64_t *max_chain) {
    return abi_barrier(g_lrmf_err, "cmi_lrmf_levels", [&] {
        const char *fn = "cmi_lrmf_levels";
        if (n_users <= 0 || n_items <= 0 || n < 0 || n >= ((int64_t)1 << 31) || (n > 0 && (!u || !i)))
            return abi_fail(g_lrmf_err, CMI_E_INVALID, "%s: invalid argument", fn);
        for (int64_t t = 0; t < n; ++t)
            if (u[t] < 0 || u[t] >= n_users || i[t] < 0 || i[t] >= n_items)
                return abi_fail(g_lrmf_err, CMI_E_INVALID, "%s: id out of range at cell %lld", fn, (long long)t);
        const std::vector<double> ones((size_t)n, 1.0);
        const PairHostCsr m = pair_csr(n, n_users, u, i, ones.data());
        for (int a = 0; a < n_users; ++a)
            for (int32_t c = m.ptr[(size_t)a] + 1; c < m.ptr[(size_t)a + 1]; ++c)
                if (m.idx[(size_t)c] == m.idx[(size_t)c - 1])
                    return abi_fail(g_lrmf_err, CMI_E_INVALID, "%s: duplicate cell (user %d, item %d)", fn, a, m.idx[(size_t)c]);
        std::vector<int32_t> ord, ptr, lv;
        int64_t chain = 0;
        const int32_t nl = build_unit_levels(n_users, n_items, m.ptr.data(), m.idx.data(), ord, ptr, &lv, &chain);
        if (order) std::copy(ord.begin(), ord.end(), order);
        if (level_of) std::copy(lv.begin(), lv.end(), level_of);
        if (n_levels) *n_levels = nl;
        if (max_chain) *max_chain = chain;
        return (int)CMI_OK;
    });
}
