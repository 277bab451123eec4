// cptf_api.cpp -- C ABI of CPTF (include/carskit_mi355x.h, cmi_cptf_*): the checked entries and ranking keys, the model, the one-wave
// epoch and its loss, prediction of key tuples and the top-N evaluation through the slab form of the batch pipeline.
#include "../../include/carskit_mi355x.h"

#include <hip/hip_runtime.h>

#include <cmath>
#include <string>
#include <vector>

#include "cptf_host.hpp"
#include "cptf_kernels.hpp"
#include "pair_host.hpp"
#include "rank_host.hpp"

using namespace cmi;

struct cmi_cptf_instance : PairModelBase { // n_users = dims[0], n_items = dims[1]
    int k = 0, n_dims = 0;
    unsigned flags = 0;
    std::vector<int32_t> dims;
    CptfModel m{};                  // m.M: the device model
    int64_t n_entries = 0;          // those with rate > 0
    int64_t *d_row = nullptr;
    double *d_r = nullptr, *d_slots = nullptr, *d_parts = nullptr, *d_loss = nullptr, *d_Qt = nullptr;
    int32_t n_ctx = 0;
    std::vector<int32_t> ctx_keys;  // n_ctx x (n_dims - 2)
    int32_t *d_qu = nullptr, *d_qkeys = nullptr;
    size_t qu_cap = 0, qkeys_cap = 0;
    double min_rate = 0.0, max_rate = 0.0;
    bool have_model = false, have_range = false, iterated = false, evaluated = false, lds_ctx = false;
    hipEvent_t ev[3] = {nullptr, nullptr, nullptr};
    float iter_ms[3] = {0.f, 0.f, 0.f};
    RankWorkspace rank_ws;
};

static thread_local std::string g_cptf_err;

extern "C" const char *cmi_cptf_last_error(cmi_cptf_handle h) { return h ? h->err.c_str() : g_cptf_err.c_str(); }

static void cptf_free_entries(cmi_cptf_instance *h) {
    abi_free(h->d_row, h->d_r, h->d_slots);
    h->have_ratings = false;
}

static void cptf_free_all(cmi_cptf_instance *h) {
    cptf_free_entries(h);
    abi_free(h->m.M, h->d_parts, h->d_loss, h->d_Qt, h->d_qu, h->d_qkeys);
    h->qu_cap = h->qkeys_cap = 0;
    h->have_model = false;
    h->rank_ws.release();
    for (hipEvent_t &e : h->ev) {
        if (e) (void)hipEventDestroy(e);
        e = nullptr;
    }
}

extern "C" int cmi_cptf_destroy(cmi_cptf_handle h) { return pair_destroy(h, cptf_free_all); }

// CPTF.java:46-55, TensorRecommender.java:62-84
extern "C" int cmi_cptf_create(int k, int n_dims, const int32_t *dims, int device, unsigned flags, cmi_cptf_handle *out) {
    if (out) *out = nullptr;
    if (out && (k > CPTF_MAX_K || n_dims < CPTF_MIN_DIMS || n_dims > CPTF_MAX_DIMS))
        return abi_fail(g_cptf_err, CMI_E_UNSUPPORTED,
                        "cmi_cptf_create: %d factors, %d dimensions: a lane holds the rows of an entry in registers, k <= %d and %d <= n_dims <= %d",
                        k, n_dims, CPTF_MAX_K, CPTF_MIN_DIMS, CPTF_MAX_DIMS);
    bool valid = out && k >= 1 && dims && (flags & ~(CMI_CPTF_FLAG_STRICT | CMI_CPTF_FLAG_GLOBAL_CTX)) == 0;
    for (int d = 0; valid && d < n_dims; ++d) valid = dims[d] > 0;
    int rc = pair_create(g_cptf_err, "cmi_cptf_create", valid, valid ? dims[0] : 0, valid ? dims[1] : 0, device, out, cmi_cptf_destroy,
                         [&](cmi_cptf_instance *h) {
                             h->k = k, h->n_dims = n_dims, h->flags = flags;
                             h->dims.assign(dims, dims + n_dims);
                             h->m.k = k, h->m.n_dims = n_dims;
                             h->m.off[0] = 0;
                             for (int d = 0; d < n_dims; ++d) h->m.off[d + 1] = h->m.off[d] + (int64_t)dims[d] * k;
                             for (int d = n_dims + 1; d <= CPTF_MAX_DIMS; ++d) h->m.off[d] = h->m.off[n_dims];
                         });
    if (rc != CMI_OK) return rc;
    cmi_cptf_instance *h = *out;
    hipError_t e = hipSuccess;
    for (hipEvent_t &ev : h->ev)
        if (e == hipSuccess) e = hipEventCreate(&ev);
    if (e == hipSuccess) e = hipMalloc((void **)&h->d_parts, (size_t)(k + 1) * sizeof(double));
    if (e == hipSuccess) e = hipMalloc((void **)&h->d_loss, sizeof(double));
    if (e != hipSuccess) {
        cmi_cptf_destroy(h);
        *out = nullptr;
        return abi_fail(g_cptf_err, CMI_E_HIP, "cmi_cptf_create: %s", hipGetErrorString(e));
    }
    return CMI_OK;
}

// every key of n tuples of `width` keys, the first of them of dimension d0, inside its dimension: nothing the device indexes with is
// unchecked
static int cptf_check_keys(cmi_cptf_instance *h, const char *fn, const char *unit, int64_t n, int d0, int width, const int32_t *keys) {
    for (int64_t t = 0; t < n; ++t)
        for (int x = 0; x < width; ++x) {
            const int32_t key = keys[t * width + x];
            if (key < 0 || key >= h->dims[(size_t)(d0 + x)])
                CMI_FAIL(h, CMI_E_INVALID, "%s: key %d of dimension %d (size %d) out of range at %s %lld", fn, key, d0 + x,
                         h->dims[(size_t)(d0 + x)], unit, (long long)t);
        }
    return CMI_OK;
}

static int cptf_set_entries_impl(cmi_cptf_handle h, int64_t n, const int32_t *keys, const double *r) {
    const char *fn = "cmi_cptf_set_entries";
    if (n < 0 || (n > 0 && (!keys || !r))) CMI_FAIL(h, CMI_E_INVALID, "%s: null arrays", fn);
    if (n >= ((int64_t)1 << 31)) CMI_FAIL(h, CMI_E_UNSUPPORTED, "%s: more than 2^31-1 entries", fn);
    if (int rc = cptf_check_keys(h, fn, "entry", n, 0, h->n_dims, keys)) return rc;
    std::vector<int64_t> row;
    std::vector<double> rate;
    for (int64_t t = 0; t < n; ++t) {
        if (r[t] <= 0.0) continue; // CPTF.java:85-86
        for (int d = 0; d < h->n_dims; ++d) row.push_back(h->m.off[d] + (int64_t)keys[t * h->n_dims + d] * h->k);
        rate.push_back(r[t]);
    }
    if ((h->flags & CMI_CPTF_FLAG_STRICT) && (int64_t)rate.size() * (1 + (int64_t)h->k * h->n_dims) > CMI_CPTF_STRICT_MAX_TERMS)
        CMI_FAIL(h, CMI_E_UNSUPPORTED, "%s: %lld entries need %lld loss slots in the strict form, more than %lld", fn, (long long)rate.size(),
                 (long long)rate.size() * (1 + (long long)h->k * h->n_dims), (long long)CMI_CPTF_STRICT_MAX_TERMS);
    CMI_HIP(h, hipSetDevice(h->device));
    CMI_HIP(h, hipStreamSynchronize(h->stream));
    cptf_free_entries(h);
    h->n_entries = (int64_t)rate.size();
    hipError_t e = abi_upload(&h->d_row, row, h->stream, true);
    if (e == hipSuccess) e = abi_upload(&h->d_r, rate, h->stream, true);
    if (e == hipSuccess && (h->flags & CMI_CPTF_FLAG_STRICT))
        e = hipMalloc((void **)&h->d_slots, std::max<size_t>((size_t)h->n_entries * (size_t)(1 + h->k * h->n_dims), 1) * sizeof(double));
    if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
    if (e != hipSuccess) {
        cptf_free_entries(h);
        CMI_FAIL(h, CMI_E_HIP, "%s: %s", fn, hipGetErrorString(e));
    }
    h->have_ratings = true;
    return CMI_OK;
}

// TensorRecommender.java:62-84's trainTensor in the order CPTF.java:81 iterates it
extern "C" int cmi_cptf_set_entries(cmi_cptf_handle h, int64_t n, const int32_t *keys, const double *r) {
    if (!h) return CMI_E_INVALID;
    return abi_barrier(h->err, "cmi_cptf_set_entries", [&] { return cptf_set_entries_impl(h, n, keys, r); }, [h] { cptf_free_entries(h); });
}

// TensorRecommender.java:189-205
extern "C" int cmi_cptf_set_context_keys(cmi_cptf_handle h, int32_t n_ctx, const int32_t *ctx_keys) {
    if (!h) return CMI_E_INVALID;
    return abi_barrier(h->err, "cmi_cptf_set_context_keys", [&] {
        const char *fn = "cmi_cptf_set_context_keys";
        const int w = h->n_dims - 2;
        if (n_ctx < 0 || (n_ctx > 0 && w > 0 && !ctx_keys)) CMI_FAIL(h, CMI_E_INVALID, "%s: invalid argument", fn);
        if (int rc = cptf_check_keys(h, fn, "context", n_ctx, 2, w, ctx_keys)) return rc;
        h->ctx_keys.assign(ctx_keys, ctx_keys + (size_t)n_ctx * (size_t)w);
        h->n_ctx = n_ctx;
        return (int)CMI_OK;
    });
}

// Recommender.java's minRate / maxRate, which CPTF.java:133-136 clamps to
extern "C" int cmi_cptf_set_rating_range(cmi_cptf_handle h, double min_rate, double max_rate) {
    if (!h) return CMI_E_INVALID;
    if (std::isnan(min_rate) || std::isnan(max_rate) || min_rate > max_rate)
        CMI_FAIL(h, CMI_E_INVALID, "cmi_cptf_set_rating_range: not a range");
    h->min_rate = min_rate, h->max_rate = max_rate, h->have_range = true;
    return CMI_OK;
}

// CPTF.java:46-55: M[d].init(1, 0.1) per dimension, drawn by the host, and any later injection
extern "C" int cmi_cptf_set_model(cmi_cptf_handle h, const double *M) {
    if (!h) return CMI_E_INVALID;
    return abi_barrier(h->err, "cmi_cptf_set_model", [&] {
        if (!M) CMI_FAIL(h, CMI_E_INVALID, "cmi_cptf_set_model: null model");
        CMI_HIP(h, hipSetDevice(h->device));
        const size_t bytes = (size_t)h->m.off[h->n_dims] * sizeof(double);
        if (!h->m.M) CMI_HIP(h, hipMalloc((void **)&h->m.M, bytes));
        CMI_HIP(h, hipMemcpyAsync(h->m.M, M, bytes, hipMemcpyHostToDevice, h->stream));
        CMI_HIP(h, hipStreamSynchronize(h->stream));
        h->have_model = true;
        return (int)CMI_OK;
    });
}

extern "C" int cmi_cptf_get_model(cmi_cptf_handle h, double *M) {
    if (!h) return CMI_E_INVALID;
    return abi_barrier(h->err, "cmi_cptf_get_model", [&] {
        if (!M) CMI_FAIL(h, CMI_E_INVALID, "cmi_cptf_get_model: null model");
        if (!h->have_model) CMI_FAIL(h, CMI_E_INVALID, "cmi_cptf_get_model: no model (cmi_cptf_set_model first)");
        CMI_HIP(h, hipSetDevice(h->device));
        CMI_HIP(h, hipMemcpyAsync(M, h->m.M, (size_t)h->m.off[h->n_dims] * sizeof(double), hipMemcpyDeviceToHost, h->stream));
        CMI_HIP(h, hipStreamSynchronize(h->stream));
        return (int)CMI_OK;
    });
}

static int cptf_iterate_impl(cmi_cptf_handle h, double lrate, double reg, double *loss) {
    const char *fn = "cmi_cptf_iterate";
    if (!h->have_ratings) CMI_FAIL(h, CMI_E_INVALID, "%s: no entries (cmi_cptf_set_entries first)", fn);
    if (!h->have_model) CMI_FAIL(h, CMI_E_INVALID, "%s: no model (cmi_cptf_set_model first)", fn);
    CMI_HIP(h, hipSetDevice(h->device));
    const bool strict = (h->flags & CMI_CPTF_FLAG_STRICT) != 0;
    const size_t ctx_bytes = (size_t)(h->m.off[h->n_dims] - h->m.off[2]) * sizeof(double);
    CptfEpoch a;
    a.m = h->m, a.row = h->d_row, a.r = h->d_r, a.n = h->n_entries, a.lrate = lrate, a.reg = reg, a.strict = strict;
    a.lds_ctx = ctx_bytes > 0 && ctx_bytes <= CPTF_LDS_CTX_BYTES && !(h->flags & CMI_CPTF_FLAG_GLOBAL_CTX);
    a.slots = h->d_slots, a.parts = h->d_parts;
    const int64_t n_terms = strict ? h->n_entries * (1 + (int64_t)h->k * h->n_dims) : (h->n_entries ? h->k + 1 : 0);
    CMI_HIP(h, hipEventRecord(h->ev[0], h->stream));
    CMI_HIP(h, cptf_launch_epoch(a, h->stream));
    CMI_HIP(h, hipEventRecord(h->ev[1], h->stream));
    CMI_HIP(h, cptf_launch_loss(strict ? h->d_slots : h->d_parts, n_terms, h->d_loss, h->stream));
    CMI_HIP(h, hipEventRecord(h->ev[2], h->stream));
    double l = 0.0;
    CMI_HIP(h, hipMemcpyAsync(&l, h->d_loss, sizeof(double), hipMemcpyDeviceToHost, h->stream));
    CMI_HIP(h, hipStreamSynchronize(h->stream));
    CMI_HIP(h, hipEventElapsedTime(&h->iter_ms[0], h->ev[0], h->ev[1]));
    CMI_HIP(h, hipEventElapsedTime(&h->iter_ms[1], h->ev[1], h->ev[2]));
    l *= 0.5; // CPTF.java:111
    h->iterated = true, h->lds_ctx = a.lds_ctx;
    if (loss) *loss = l;
    if (!std::isfinite(l)) CMI_FAIL(h, CMI_E_NUMERIC, "%s: loss = %g", fn, l);
    return CMI_OK;
}

// CPTF.java:80-111: one iteration
extern "C" int cmi_cptf_iterate(cmi_cptf_handle h, double lrate, double reg, double *loss) {
    if (!h) return CMI_E_INVALID;
    return abi_barrier(h->err, "cmi_cptf_iterate", [&] { return cptf_iterate_impl(h, lrate, reg, loss); });
}

static int cptf_predict_impl(cmi_cptf_handle h, int64_t n, const int32_t *keys, int bound, double lo, double hi, double *out) {
    const char *fn = "cmi_cptf_predict_batch";
    if (!h->have_model) CMI_FAIL(h, CMI_E_INVALID, "%s: no model (cmi_cptf_set_model first)", fn);
    if (n < 0 || (n > 0 && (!keys || !out))) CMI_FAIL(h, CMI_E_INVALID, "%s: null arrays", fn);
    if (int rc = cptf_check_keys(h, fn, "tuple", n, 0, h->n_dims, keys)) return rc;
    if (n == 0) return CMI_OK;
    CMI_HIP(h, hipSetDevice(h->device));
    int32_t *d_keys = nullptr;
    double *d_out = nullptr;
    hipError_t e = abi_upload(&d_keys, keys, (size_t)n * (size_t)h->n_dims, h->stream);
    if (e == hipSuccess) e = hipMalloc((void **)&d_out, (size_t)n * sizeof(double));
    if (e == hipSuccess) e = cptf_launch_predict(h->m, n, d_keys, bound != 0, lo, hi, d_out, h->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(out, d_out, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, h->stream);
    const hipError_t es = hipStreamSynchronize(h->stream); // the upload reads `keys` until then
    if (e == hipSuccess) e = es;
    abi_free(d_keys, d_out);
    return abi_hip(h->err, fn, e);
}

// CPTF.java:141-155 of n key tuples, bounded as TensorRecommender.java:86-164 bounds what it evaluates
extern "C" int cmi_cptf_predict_batch(cmi_cptf_handle h, int64_t n, const int32_t *keys, int bound, double lo, double hi, double *out) {
    if (!h) return CMI_E_INVALID;
    return abi_barrier(h->err, "cmi_cptf_predict_batch", [&] { return cptf_predict_impl(h, n, keys, bound, lo, hi, out); });
}

template <typename T>
static hipError_t cptf_grow(T *&p, size_t &cap, size_t n) {
    if (n <= cap) return hipSuccess;
    abi_free(p);
    cap = 0;
    const hipError_t e = hipMalloc((void **)&p, n * sizeof(T));
    if (e == hipSuccess) cap = n;
    return e;
}

// Recommender.java:630-860 with ranking(u, j, c) = CPTF.predict(u, j, c) (CPTF.java:119-139)
extern "C" int cmi_cptf_eval_rankings(cmi_cptf_handle h, int64_t n_train, const int32_t *tu, const int32_t *tj, const int32_t *tctx,
                                      const double *tr, int64_t n_test, const int32_t *su, const int32_t *sj, const int32_t *sctx,
                                      const double *sr, double bin_thold, int num_recs, int num_ignore, int strategy, double out[21],
                                      int64_t *n_queries, int32_t *q_user, int32_t *q_ctx, int32_t *q_count, int32_t *top_items,
                                      double *top_scores) {
    if (!h) return CMI_E_INVALID;
    return abi_barrier(h->err, "cptf_eval_rankings", [&] {
        auto ready = [h]() -> int {
            if (!h->have_model) CMI_FAIL(h, CMI_E_INVALID, "cptf: call cmi_cptf_set_model first");
            if (!h->have_range) CMI_FAIL(h, CMI_E_INVALID, "cptf: call cmi_cptf_set_rating_range first");
            if (h->n_ctx <= 0) CMI_FAIL(h, CMI_E_INVALID, "cptf: call cmi_cptf_set_context_keys first");
            CMI_HIP(h, hipSetDevice(h->device));
            return CMI_OK;
        };
        std::vector<int32_t> qkeys; // outlives the device loop: its upload reads it
        auto score = [&](const RankPlan &plan, const RankBatchFn &on_batch) {
            // the queries' users and getKeys' context keys (ids checked below n_ctx by rank_evaluate), the item matrix transposed
            const size_t nq = plan.qu.size(), w = (size_t)(h->n_dims - 2);
            qkeys.resize(nq * w);
            for (size_t q = 0; q < nq; ++q)
                for (size_t x = 0; x < w; ++x) qkeys[q * w + x] = h->ctx_keys[(size_t)plan.qc[q] * w + x];
            hipError_t e = cptf_grow(h->d_qu, h->qu_cap, std::max<size_t>(nq, 1));
            if (e == hipSuccess) e = cptf_grow(h->d_qkeys, h->qkeys_cap, std::max<size_t>(nq * w, 1));
            if (e == hipSuccess && !h->d_Qt) e = hipMalloc((void **)&h->d_Qt, (size_t)h->n_items * h->k * sizeof(double));
            if (e == hipSuccess && nq) e = hipMemcpyAsync(h->d_qu, plan.qu.data(), nq * sizeof(int32_t), hipMemcpyHostToDevice, h->stream);
            if (e == hipSuccess && nq * w)
                e = hipMemcpyAsync(h->d_qkeys, qkeys.data(), nq * w * sizeof(int32_t), hipMemcpyHostToDevice, h->stream);
            if (e == hipSuccess) e = cptf_launch_transpose_items(h->m, h->n_items, h->d_Qt, h->stream);
            if (e != hipSuccess) return e;
            const RankSlabFn fill = [h](double *dS, const int32_t *dcand, int nc, const int32_t *, const int32_t *, int, int, int64_t q0,
                                        int64_t nq_b, hipStream_t s) {
                return cptf_launch_score(h->m, h->d_Qt, h->n_items, dcand, nc, h->d_qu, h->d_qkeys, q0, nq_b, h->min_rate, h->max_rate, dS,
                                         s);
            };
            return rank_run_device_slab(h->stream, h->rank_ws, plan, fill, bin_thold, num_recs, on_batch, &h->iter_ms[2]);
        };
        const RankEvalIO io{{n_train, tu, tj, tctx, tr}, {n_test, su, sj, sctx, sr}, bin_thold, num_recs, num_ignore, strategy, out, n_queries,
                            q_user, q_ctx, q_count, top_items, top_scores};
        const int rc = rank_evaluate(h->err, "cptf_eval_rankings", h->rank_ws, h->n_users, h->n_items, h->n_ctx > 0 ? h->n_ctx : 1, io, ready,
                                     score);
        (void)hipStreamSynchronize(h->stream);
        if (rc == CMI_OK) h->evaluated = true;
        return rc;
    });
}

extern "C" int cmi_cptf_last_iter_ms(cmi_cptf_handle h, float *ms) {
    if (!h || !ms) return CMI_E_INVALID;
    if (!h->iterated && !h->evaluated) CMI_FAIL(h, CMI_E_INVALID, "cmi_cptf_last_iter_ms: no iteration and no evaluation yet");
    for (int p = 0; p < 2; ++p) ms[p] = h->iterated ? h->iter_ms[p] : 0.f;
    ms[2] = h->evaluated ? h->iter_ms[2] : 0.f;
    return CMI_OK;
}

extern "C" int cmi_cptf_ctx_in_lds(cmi_cptf_handle h) { return h && h->iterated && h->lds_ctx ? 1 : 0; }

// ---- without a device ---------------------------------------------------------------------------------------------------------------
// DataDAO.java:423-481, TensorRecommender.java:62-84 and :189-205 (cptf_host.hpp)
extern "C" int cmi_cptf_tensor_build(int64_t n_cells, const int32_t *pair, const int32_t *ctx, const double *rate, int32_t n_pairs,
                                     const int32_t *pair_user, const int32_t *pair_item, int32_t n_ctx, const int32_t *ctx_ptr,
                                     const int32_t *ctx_conds, int32_t n_conds, const int32_t *cond_dim, int64_t n_test,
                                     const int32_t *test_pair, unsigned flags, int32_t *n_dims, int32_t *dims, int32_t *dim_list_ptr,
                                     int32_t *dim_list, int32_t *keys, double *vals, int64_t *n_train, int32_t *train_keys,
                                     double *train_vals, int64_t *n_test_out, int32_t *test_keys, double *test_vals, int32_t *ctx_keys) {
    return abi_barrier(g_cptf_err, "cmi_cptf_tensor_build", [&] {
        const char *fn = "cmi_cptf_tensor_build";
        if ((flags & ~CMI_CPTF_FLAG_KEYS_INDEXOF) != 0 || !n_dims || !dims || !dim_list_ptr || !dim_list || !keys || !vals || !n_train ||
            !train_keys || !train_vals || !n_test_out || !test_keys || !test_vals || !ctx_keys)
            return abi_fail(g_cptf_err, CMI_E_INVALID, "%s: invalid argument", fn);
        CptfTensorIn in;
        in.n_cells = n_cells, in.pair = pair, in.ctx = ctx, in.rate = rate, in.n_pairs = n_pairs, in.pair_user = pair_user;
        in.pair_item = pair_item, in.n_ctx = n_ctx, in.ctx_ptr = ctx_ptr, in.ctx_conds = ctx_conds, in.n_conds = n_conds;
        in.cond_dim = cond_dim, in.n_test = n_test, in.test_pair = test_pair, in.keys_indexof = (flags & CMI_CPTF_FLAG_KEYS_INDEXOF) != 0;
        CptfTensorOut o;
        std::string why;
        if (const int rc = cptf_tensor_build(in, o, why))
            return abi_fail(g_cptf_err, rc == CPTF_BUILD_UNSUPPORTED ? CMI_E_UNSUPPORTED : CMI_E_INVALID, "%s: %s", fn, why.c_str());
        *n_dims = (int32_t)o.dims.size();
        std::copy(o.dims.begin(), o.dims.end(), dims);
        dim_list_ptr[0] = 0;
        for (size_t d = 0; d < o.dim_lists.size(); ++d) {
            std::copy(o.dim_lists[d].begin(), o.dim_lists[d].end(), dim_list + dim_list_ptr[d]);
            dim_list_ptr[d + 1] = dim_list_ptr[d] + (int32_t)o.dim_lists[d].size();
        }
        std::copy(o.keys.begin(), o.keys.end(), keys);
        std::copy(o.vals.begin(), o.vals.end(), vals);
        *n_train = (int64_t)o.train_vals.size(), *n_test_out = (int64_t)o.test_vals.size();
        std::copy(o.train_keys.begin(), o.train_keys.end(), train_keys);
        std::copy(o.train_vals.begin(), o.train_vals.end(), train_vals);
        std::copy(o.test_keys.begin(), o.test_keys.end(), test_keys);
        std::copy(o.test_vals.begin(), o.test_vals.end(), test_vals);
        std::copy(o.ctx_keys.begin(), o.ctx_keys.end(), ctx_keys);
        return (int)CMI_OK;
    });
}
