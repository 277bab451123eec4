// ranksgd_api.cpp -- C ABI of RankSGD (include/carskit_mi355x.h, cmi_ranksgd_*): the item list, the device tries and the host walk that
// consumes them, the per-iteration level schedule and its launches.
#include "../../include/carskit_mi355x.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <string>
#include <vector>

#include "level_schedule.hpp"
#include "pair_host.hpp"
#include "rank_host.hpp"
#include "rankals_kernels.hpp"
#include "ranksgd_host.hpp"
#include "ranksgd_kernels.hpp"

using namespace cmi;

constexpr int64_t RANKSGD_MAX_TRIES = ((int64_t)1 << 31) - 1;

struct cmi_ranksgd_instance : PairModelBase {
    int k = 0;
    unsigned flags = 0;
    PairHostCsr rows; // train.row(u): the non-zero cells, items ascending
    RanksgdTable table;
    int64_t n_cells = 0, L = 0;
    uint64_t state = java_lcg_scramble(0);
    JavaLcgJump jump = java_lcg_jump_table();
    int32_t *d_item = nullptr, *d_try = nullptr;
    double *d_cum = nullptr;
    // the samples (u, i, r fixed by the matrix, j per iteration) and the iteration's schedule
    int32_t *d_u = nullptr, *d_i = nullptr, *d_j = nullptr, *d_order = nullptr, *d_level_ptr = nullptr;
    double *d_r = nullptr;
    std::vector<int32_t> tu, ti, tj, tries, order, level_ptr;
    double *d_slots = nullptr, *d_parts = nullptr, *d_loss = nullptr;
    double *d_P = nullptr, *d_Q = nullptr;
    bool have_model = false, iterated = false, evaluated = false;
    hipEvent_t ev[3] = {nullptr, nullptr, nullptr};
    float iter_ms[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    int64_t sched[4] = {0, 0, 0, 0}, host_tries = 0;
    RankWorkspace rank_ws;
};

static thread_local std::string g_ranksgd_err;

extern "C" const char *cmi_ranksgd_last_error(cmi_ranksgd_handle h) { return h ? h->err.c_str() : g_ranksgd_err.c_str(); }

static void ranksgd_free_ratings(cmi_ranksgd_instance *h) {
    abi_free(h->d_item, h->d_try, h->d_cum, h->d_u, h->d_i, h->d_j, h->d_order, h->d_level_ptr, h->d_r, h->d_slots, h->d_parts, h->d_loss);
    h->have_ratings = h->iterated = false;
}

static void ranksgd_free_all(cmi_ranksgd_instance *h) {
    ranksgd_free_ratings(h);
    abi_free(h->d_P, h->d_Q);
    h->have_model = false;
    h->rank_ws.release();
    for (hipEvent_t &e : h->ev) {
        if (e) (void)hipEventDestroy(e);
        e = nullptr;
    }
}

extern "C" int cmi_ranksgd_destroy(cmi_ranksgd_handle h) { return pair_destroy(h, ranksgd_free_all); }

// RankSGD.java:53-59.  A 16-lane group holds a row in 8 registers per lane: k <= 128
extern "C" int cmi_ranksgd_create(int k, int n_users, int n_items, int device, unsigned flags, cmi_ranksgd_handle *out) {
    if (out && k > BPR_MAX_K) {
        *out = nullptr;
        return abi_fail(g_ranksgd_err, CMI_E_UNSUPPORTED,
                        "cmi_ranksgd_create: %d factors: a 16-lane group holds a sample's rows in registers, k <= %d", k, BPR_MAX_K);
    }
    const bool valid =
        k >= 1 && (flags & ~(CMI_RANKSGD_FLAG_STRICT | CMI_RANKSGD_FLAG_HOST_SAMPLER | CMI_RANKSGD_FLAG_NUM_RATES_SIZE)) == 0;
    int rc = pair_create(g_ranksgd_err, "cmi_ranksgd_create", valid, n_users, n_items, device, out, cmi_ranksgd_destroy,
                         [k, flags](cmi_ranksgd_instance *h) { h->k = k, h->flags = flags; });
    if (rc != CMI_OK) return rc;
    cmi_ranksgd_instance *h = *out;
    hipError_t e = hipSuccess;
    for (hipEvent_t &ev : h->ev)
        if (e == hipSuccess) e = hipEventCreate(&ev);
    if (e != hipSuccess) {
        cmi_ranksgd_destroy(h);
        *out = nullptr;
        return abi_fail(g_ranksgd_err, CMI_E_HIP, "cmi_ranksgd_create: %s", hipGetErrorString(e));
    }
    return CMI_OK;
}

// the checked cells as train's rows without the zero-valued cells, and the item list; the matrices the reference cannot finish are
// refused here
static int ranksgd_prepare(std::string &err, const char *fn, const PairHostCsr &all, int n_users, int n_items, unsigned flags,
                           PairHostCsr &rows, RanksgdTable &table) {
    rows = pair_drop_zeros(all);
    if (rows.idx.empty()) return abi_fail(err, CMI_E_INVALID, "%s: no non-zero cell: RankSGD.java:85 has nothing to visit", fn);
    std::vector<int32_t> col((size_t)n_items, 0);
    for (int32_t i : rows.idx) ++col[(size_t)i];
    table = ranksgd_item_table(n_items, col.data(), (flags & CMI_RANKSGD_FLAG_NUM_RATES_SIZE) ? (int64_t)rows.idx.size() : 0);
    if (table.tree)
        return abi_fail(err, CMI_E_UNSUPPORTED,
                        "%s: the items with a cell would treeify a java.util.HashMap bin, whose iteration order is not modelled", fn);
    const int32_t endless = ranksgd_endless_user(n_users, rows.ptr.data(), rows.idx.data(), table);
    if (endless >= 0)
        return abi_fail(err, CMI_E_INVALID,
                        "%s: user %d holds every item a draw can return (the first of them item %d): RankSGD.java:94-112 would draw j for "
                        "ever%s",
                        fn, endless, table.item[0],
                        (flags & CMI_RANKSGD_FLAG_NUM_RATES_SIZE)
                            ? ""
                            : " (the reference never assigns numRates, so every draw returns the first item of the list; "
                              "CMI_RANKSGD_FLAG_NUM_RATES_SIZE divides by the number of ratings instead)");
    return CMI_OK;
}

static int ranksgd_set_ratings_impl(cmi_ranksgd_handle h, int64_t n, const int32_t *u, const int32_t *i, const double *r) {
    const char *fn = "cmi_ranksgd_set_ratings";
    PairHostCsr all, cols;
    if (int rc = pair_ingest(h, fn, n, u, i, r, /*scan_items=*/false, all, cols)) return rc;
    PairHostCsr rows;
    RanksgdTable table;
    if (int rc = ranksgd_prepare(h->err, fn, all, h->n_users, h->n_items, h->flags, rows, table)) return rc;
    const double want = ranksgd_reservation(h->n_users, h->n_items, rows.ptr.data(), rows.idx.data(), table);
    if (want > (double)RANKSGD_MAX_TRIES) CMI_FAIL(h, CMI_E_UNSUPPORTED, "%s: more than 2^31-1 tries an iteration are expected", fn);
    CMI_HIP(h, hipSetDevice(h->device));
    CMI_HIP(h, hipStreamSynchronize(h->stream));
    ranksgd_free_ratings(h);
    h->rows = std::move(rows), h->table = std::move(table);
    h->n_cells = (int64_t)h->rows.idx.size();
    h->L = (int64_t)want;
    const size_t S = (size_t)h->n_cells;
    h->tu.resize(S), h->ti = h->rows.idx, h->tj.assign(S, 0);
    for (int32_t a = 0; a < h->n_users; ++a)
        for (int32_t q = h->rows.ptr[(size_t)a]; q < h->rows.ptr[(size_t)a + 1]; ++q) h->tu[(size_t)q] = a;
    hipError_t e = abi_upload(&h->d_item, h->table.item, h->stream, true);
    if (e == hipSuccess) e = abi_upload(&h->d_cum, h->table.cum, h->stream, true);
    if (e == hipSuccess) e = abi_upload(&h->d_u, h->tu, h->stream, true);
    if (e == hipSuccess) e = abi_upload(&h->d_i, h->ti, h->stream, true);
    if (e == hipSuccess) e = abi_upload(&h->d_r, h->rows.val, h->stream, true);
    if (e == hipSuccess) e = hipMalloc((void **)&h->d_j, S * sizeof(int32_t));
    if (e == hipSuccess) e = hipMalloc((void **)&h->d_order, S * sizeof(int32_t));
    if (e == hipSuccess) e = hipMalloc((void **)&h->d_level_ptr, (S + 1) * sizeof(int32_t));
    if (e == hipSuccess) e = hipMalloc((void **)&h->d_slots, S * sizeof(double));
    if (e == hipSuccess) e = hipMalloc((void **)&h->d_parts, BPR_LOSS_PARTS * sizeof(double));
    if (e == hipSuccess) e = hipMalloc((void **)&h->d_loss, sizeof(double));
    if (e == hipSuccess && !(h->flags & CMI_RANKSGD_FLAG_HOST_SAMPLER)) e = hipMalloc((void **)&h->d_try, (size_t)h->L * sizeof(int32_t));
    if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
    if (e != hipSuccess) {
        ranksgd_free_ratings(h);
        CMI_FAIL(h, CMI_E_HIP, "%s: %s", fn, hipGetErrorString(e));
    }
    h->have_ratings = true;
    return CMI_OK;
}

extern "C" int cmi_ranksgd_set_ratings(cmi_ranksgd_handle h, int64_t n, const int32_t *u, const int32_t *i, const double *r) {
    if (!h) return CMI_E_INVALID;
    return abi_barrier(h->err, "cmi_ranksgd_set_ratings", [&] { return ranksgd_set_ratings_impl(h, n, u, i, r); },
                       [h] { ranksgd_free_ratings(h); });
}

static int ranksgd_set_model_impl(cmi_ranksgd_handle h, const double *P, const double *Q) {
    if (!h->have_model && (!P || !Q)) CMI_FAIL(h, CMI_E_INVALID, "cmi_ranksgd_set_model: the first call sets both P and Q");
    CMI_HIP(h, hipSetDevice(h->device));
    const size_t pn = (size_t)h->n_users * h->k, qn = (size_t)h->n_items * h->k;
    if (!h->d_P) {
        hipError_t e = hipMalloc((void **)&h->d_P, pn * sizeof(double));
        if (e == hipSuccess) e = hipMalloc((void **)&h->d_Q, qn * sizeof(double));
        if (e != hipSuccess) {
            abi_free(h->d_P, h->d_Q);
            CMI_FAIL(h, CMI_E_HIP, "cmi_ranksgd_set_model: %s", hipGetErrorString(e));
        }
    }
    if (P) CMI_HIP(h, hipMemcpyAsync(h->d_P, P, pn * sizeof(double), hipMemcpyHostToDevice, h->stream));
    if (Q) CMI_HIP(h, hipMemcpyAsync(h->d_Q, Q, qn * sizeof(double), hipMemcpyHostToDevice, h->stream));
    CMI_HIP(h, hipStreamSynchronize(h->stream));
    h->have_model = true;
    return CMI_OK;
}

// IterativeRecommender.java:235-241 with initByNorm = true (P and Q gaussian, drawn by the host) and any later injection
extern "C" int cmi_ranksgd_set_model(cmi_ranksgd_handle h, const double *P, const double *Q) {
    if (!h) return CMI_E_INVALID;
    return abi_barrier(h->err, "cmi_ranksgd_set_model", [&] { return ranksgd_set_model_impl(h, P, Q); });
}

extern "C" int cmi_ranksgd_get_model(cmi_ranksgd_handle h, double *P, double *Q) {
    if (!h) return CMI_E_INVALID;
    return abi_barrier(h->err, "cmi_ranksgd_get_model", [&] {
        if (!h->have_model) CMI_FAIL(h, CMI_E_INVALID, "cmi_ranksgd_get_model: no model (cmi_ranksgd_set_model first)");
        CMI_HIP(h, hipSetDevice(h->device));
        if (P) CMI_HIP(h, hipMemcpyAsync(P, h->d_P, (size_t)h->n_users * h->k * sizeof(double), hipMemcpyDeviceToHost, h->stream));
        if (Q) CMI_HIP(h, hipMemcpyAsync(Q, h->d_Q, (size_t)h->n_items * h->k * sizeof(double), hipMemcpyDeviceToHost, h->stream));
        CMI_HIP(h, hipStreamSynchronize(h->stream));
        return CMI_OK;
    });
}

extern "C" int cmi_ranksgd_set_random_state(cmi_ranksgd_handle h, int64_t state) {
    if (!h) return CMI_E_INVALID;
    if (state < 0 || (uint64_t)state > JAVA_LCG_MASK) CMI_FAIL(h, CMI_E_INVALID, "cmi_ranksgd_set_random_state: not a 48-bit state");
    h->state = (uint64_t)state;
    return CMI_OK;
}
extern "C" int cmi_ranksgd_get_random_state(cmi_ranksgd_handle h, int64_t *state) {
    if (!h || !state) return CMI_E_INVALID;
    *state = (int64_t)h->state;
    return CMI_OK;
}

// the try at position t of the stream that starts at state0, in sequence where the caller asks in sequence (the walk does), else by
// jump-ahead
struct RanksgdHostTries {
    const RanksgdTable &table;
    const JavaLcgJump &jump;
    uint64_t state0, at_state;
    int64_t at = -1, supplied = 0;
    int32_t operator()(int64_t t) {
        if (t != at) at_state = java_lcg_jump(jump, state0, 2 * (uint64_t)t);
        const int32_t x = ranksgd_try(at_state, table.item.data(), table.cum.data(), (int32_t)table.item.size());
        at_state = (at_state * JAVA_LCG_A + JAVA_LCG_C) & JAVA_LCG_MASK; // the try's two draws
        at_state = (at_state * JAVA_LCG_A + JAVA_LCG_C) & JAVA_LCG_MASK;
        at = t + 1, ++supplied;
        return x;
    }
};

static float ms_since(std::chrono::steady_clock::time_point t0) {
    return std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
}

static int ranksgd_walk_error(std::string &err, const char *fn, int rc, int64_t bad, int64_t used) {
    if (rc == RANKSGD_FIRST_TRY_MISS)
        return abi_fail(err, CMI_E_NUMERIC,
                        "%s: no entry of the item list reached the random number on the first try of cell %lld: RankSGD.java:116 would "
                        "predict(u, -1)",
                        fn, (long long)bad);
    return abi_fail(err, CMI_E_UNSUPPORTED, "%s: cell %lld needs a try past %lld", fn, (long long)bad, (long long)used);
}

// one iteration's j per cell from h->state into h->tj and d_j; *after: the state after the last consumed draw.  n_device: the tries
// computed on the device (0: all on the host); ms: the device tries, the host walk
static int ranksgd_sample_impl(cmi_ranksgd_handle h, const char *fn, int64_t n_device, uint64_t *after, float ms[2]) {
    const size_t S = (size_t)h->n_cells;
    n_device = h->d_try ? std::min(n_device, h->L) : 0;
    auto t0 = std::chrono::steady_clock::now();
    if (n_device > 0) {
        h->tries.resize((size_t)n_device);
        CMI_HIP(h, ranksgd_launch_tries(h->state, h->jump, h->d_item, h->d_cum, (int32_t)h->table.item.size(), n_device, h->d_try, h->stream));
        CMI_HIP(h, hipMemcpyAsync(h->tries.data(), h->d_try, (size_t)n_device * sizeof(int32_t), hipMemcpyDeviceToHost, h->stream));
        CMI_HIP(h, hipStreamSynchronize(h->stream));
    }
    ms[0] = ms_since(t0);
    t0 = std::chrono::steady_clock::now();
    RanksgdHostTries host{h->table, h->jump, h->state, h->state};
    const int32_t *dev = h->tries.data();
    int64_t used = 0, bad = 0;
    const int rc = ranksgd_assign(
        h->n_users, h->rows.ptr.data(), h->rows.idx.data(), [&](int64_t t) { return t < n_device ? dev[t] : host(t); }, RANKSGD_MAX_TRIES,
        h->tj.data(), &used, &bad);
    ms[1] = ms_since(t0);
    if (rc != RANKSGD_OK) return ranksgd_walk_error(h->err, fn, rc, bad, used);
    // exactness never depends on the reservation: what the walk needed past it came from the same function on the host.  (With
    // CMI_RANKSGD_FLAG_HOST_SAMPLER the device form is switched off: nothing was supplied in its place)
    if (n_device > 0) h->host_tries += host.supplied;
    CMI_HIP(h, hipMemcpyAsync(h->d_j, h->tj.data(), S * sizeof(int32_t), hipMemcpyHostToDevice, h->stream));
    CMI_HIP(h, hipStreamSynchronize(h->stream));
    *after = java_lcg_jump(h->jump, h->state, 2 * (uint64_t)used);
    return CMI_OK;
}

extern "C" int cmi_ranksgd_sample(cmi_ranksgd_handle h, int on_device, int64_t max_device_tries, int32_t *u, int32_t *i, int32_t *j,
                                  double *r, int64_t *state_after) {
    if (!h) return CMI_E_INVALID;
    return abi_barrier(h->err, "cmi_ranksgd_sample", [&] {
        if (!u || !i || !j || !r || max_device_tries < 0) CMI_FAIL(h, CMI_E_INVALID, "cmi_ranksgd_sample: invalid argument");
        if (!h->have_ratings) CMI_FAIL(h, CMI_E_INVALID, "cmi_ranksgd_sample: no ratings (cmi_ranksgd_set_ratings first)");
        CMI_HIP(h, hipSetDevice(h->device));
        uint64_t after = 0;
        float ms[2];
        const int64_t nd = !on_device ? 0 : (max_device_tries ? max_device_tries : h->L);
        if (int rc = ranksgd_sample_impl(h, "cmi_ranksgd_sample", nd, &after, ms)) return rc;
        std::copy(h->tu.begin(), h->tu.end(), u);
        std::copy(h->ti.begin(), h->ti.end(), i);
        std::copy(h->tj.begin(), h->tj.end(), j);
        std::copy(h->rows.val.begin(), h->rows.val.end(), r);
        if (state_after) *state_after = (int64_t)after;
        return CMI_OK;
    });
}

static int ranksgd_iterate_impl(cmi_ranksgd_handle h, double lrate, double *loss) {
    const char *fn = "cmi_ranksgd_iterate";
    if (!h->have_ratings) CMI_FAIL(h, CMI_E_INVALID, "%s: no ratings (cmi_ranksgd_set_ratings first)", fn);
    if (!h->have_model) CMI_FAIL(h, CMI_E_INVALID, "%s: no model (cmi_ranksgd_set_model first)", fn);
    CMI_HIP(h, hipSetDevice(h->device));
    uint64_t after = 0;
    if (int rc = ranksgd_sample_impl(h, fn, (h->flags & CMI_RANKSGD_FLAG_HOST_SAMPLER) ? 0 : h->L, &after, h->iter_ms)) return rc;

    auto t0 = std::chrono::steady_clock::now();
    const int32_t n_levels =
        build_triple_levels(h->n_cells, h->tu.data(), h->ti.data(), h->tj.data(), h->n_users, h->n_items, h->order, h->level_ptr);
    h->iter_ms[2] = ms_since(t0);

    RanksgdEpoch a;
    a.k = h->k, a.P = h->d_P, a.Q = h->d_Q, a.u = h->d_u, a.i = h->d_i, a.j = h->d_j, a.r = h->d_r, a.order = h->d_order;
    a.level_ptr = h->d_level_ptr, a.slots = h->d_slots, a.lrate = lrate;
    CMI_HIP(h, hipMemcpyAsync(h->d_order, h->order.data(), h->order.size() * sizeof(int32_t), hipMemcpyHostToDevice, h->stream));
    CMI_HIP(h, hipMemcpyAsync(h->d_level_ptr, h->level_ptr.data(), h->level_ptr.size() * sizeof(int32_t), hipMemcpyHostToDevice, h->stream));
    CMI_HIP(h, hipEventRecord(h->ev[0], h->stream));
    int64_t sched[4] = {0, 0, 0, 0};
    CMI_HIP(h, launch_triple_levels(
                   h->level_ptr, n_levels, BPR_WG_SAMPLES, [&](int32_t b0, int32_t b1) { return ranksgd_launch_level(a, b0, b1, h->stream); },
                   [&](int32_t l0, int32_t l1) { return ranksgd_launch_run(a, l0, l1, h->stream); }, sched));
    CMI_HIP(h, hipEventRecord(h->ev[1], h->stream));
    CMI_HIP(h, bpr_launch_loss(h->d_slots, h->n_cells, (h->flags & CMI_RANKSGD_FLAG_STRICT) != 0, h->d_parts, h->d_loss, h->stream));
    CMI_HIP(h, hipEventRecord(h->ev[2], h->stream));
    double l = 0.0;
    CMI_HIP(h, hipMemcpyAsync(&l, h->d_loss, sizeof(double), hipMemcpyDeviceToHost, h->stream));
    CMI_HIP(h, hipStreamSynchronize(h->stream));
    CMI_HIP(h, hipEventElapsedTime(&h->iter_ms[3], h->ev[0], h->ev[1]));
    CMI_HIP(h, hipEventElapsedTime(&h->iter_ms[4], h->ev[1], h->ev[2]));
    l *= 0.5; // RankSGD.java:136
    h->state = after;
    std::copy(sched, sched + 4, h->sched);
    h->iterated = true;
    if (loss) *loss = l;
    if (!std::isfinite(l)) CMI_FAIL(h, CMI_E_NUMERIC, "%s: loss = %g", fn, l);
    return CMI_OK;
}

// RankSGD.java:80-137: one iteration
extern "C" int cmi_ranksgd_iterate(cmi_ranksgd_handle h, double lrate, double *loss) {
    if (!h) return CMI_E_INVALID;
    return abi_barrier(h->err, "cmi_ranksgd_iterate", [&] { return ranksgd_iterate_impl(h, lrate, loss); });
}

static int ranksgd_predict_impl(cmi_ranksgd_handle h, int64_t n, const int32_t *u, const int32_t *j, double *out) {
    if (!h->have_model) CMI_FAIL(h, CMI_E_INVALID, "cmi_ranksgd_predict_batch: no model (cmi_ranksgd_set_model first)");
    if (int rc = pair_check_tuples(h, "cmi_ranksgd_predict_batch", n, u, j, out)) return rc;
    if (n == 0) return CMI_OK;
    return abi_predict(h, "cmi_ranksgd_predict_batch", n, u, j, nullptr, nullptr, 0, out, [&](const AbiTuples &t, double *d_out) {
        return abi_hip(h->err, "cmi_ranksgd_predict_batch", rankals_launch_predict(h->d_P, h->d_Q, h->k, n, t.a, t.b, d_out, h->stream));
    });
}

// IterativeRecommender.predict(u, j) = DenseMatrix.rowMult(P, u, Q, j) of n tuples: RankALS's kernel
extern "C" int cmi_ranksgd_predict_batch(cmi_ranksgd_handle h, int64_t n, const int32_t *u, const int32_t *j, double *out) {
    if (!h) return CMI_E_INVALID;
    return abi_barrier(h->err, "cmi_ranksgd_predict_batch", [&] { return ranksgd_predict_impl(h, n, u, j, out); });
}

extern "C" int cmi_ranksgd_eval_rankings(cmi_ranksgd_handle h, int64_t n_train, const int32_t *tu, const int32_t *tj, const int32_t *tctx,
                                         const double *tr, int64_t n_test, const int32_t *su, const int32_t *sj, const int32_t *sctx,
                                         const double *sr, double bin_thold, int num_recs, int num_ignore, int strategy, double out[21],
                                         int64_t *n_queries, int32_t *q_user, int32_t *q_ctx, int32_t *q_count, int32_t *top_items,
                                         double *top_scores) {
    if (!h) return CMI_E_INVALID;
    return abi_barrier(h->err, "ranksgd_eval_rankings", [&] {
        auto ready = [h]() -> int {
            if (!h->have_model) CMI_FAIL(h, CMI_E_INVALID, "ranksgd: call cmi_ranksgd_set_model first");
            CMI_HIP(h, hipSetDevice(h->device));
            return CMI_OK;
        };
        auto score = [&](const RankPlan &plan, const RankBatchFn &on_batch) {
            const RankSlabFn fill = [h](double *dS, const int32_t *dcand, int nc, const int32_t *dgu, const int32_t *dgq0, int g0, int g1,
                                        int64_t q0, int64_t nq, hipStream_t s) {
                static_assert(BPR_MAX_K <= RANK_SCORE_MAX_K, "RankSGD scores with RankALS's kernel: its rows must fit that kernel's LDS row");
                return rankals_launch_score(h->d_P, h->d_Q, h->k, dcand, nc, dgu, dgq0, g0, g1, q0, nq, dS, s);
            };
            return rank_run_device_slab(h->stream, h->rank_ws, plan, fill, bin_thold, num_recs, on_batch, &h->iter_ms[5]);
        };
        const RankEvalIO io{{n_train, tu, tj, tctx, tr}, {n_test, su, sj, sctx, sr}, bin_thold, num_recs, num_ignore, strategy, out, n_queries,
                            q_user, q_ctx, q_count, top_items, top_scores};
        const int rc = rank_evaluate(h->err, "ranksgd_eval_rankings", h->rank_ws, h->n_users, h->n_items, INT64_MAX, io, ready, score);
        if (rc == CMI_OK) h->evaluated = true;
        return rc;
    });
}

extern "C" int cmi_ranksgd_last_iter_ms(cmi_ranksgd_handle h, float *ms) {
    if (!h || !ms) return CMI_E_INVALID;
    if (!h->iterated && !h->evaluated) CMI_FAIL(h, CMI_E_INVALID, "cmi_ranksgd_last_iter_ms: no iteration and no evaluation yet");
    for (int p = 0; p < 5; ++p) ms[p] = h->iterated ? h->iter_ms[p] : 0.f;
    ms[5] = h->evaluated ? h->iter_ms[5] : 0.f;
    return CMI_OK;
}

extern "C" int cmi_ranksgd_last_schedule(cmi_ranksgd_handle h, int64_t *out) {
    if (!h || !out) return CMI_E_INVALID;
    for (int p = 0; p < 4; ++p) out[p] = h->iterated ? h->sched[p] : 0;
    out[4] = h->host_tries;
    return CMI_OK;
}

// ---- without a device ---------------------------------------------------------------------------------------------------------------
static int ranksgd_check_cells(const char *fn, int n_users, int n_items, int64_t n, const int32_t *u, const int32_t *i, const double *r,
                               unsigned flags) {
    if (n_users <= 0 || n_items <= 0 || n < 0 || n >= ((int64_t)1 << 31) || (n > 0 && (!u || !i || !r)) ||
        (flags & ~CMI_RANKSGD_FLAG_NUM_RATES_SIZE) != 0)
        return abi_fail(g_ranksgd_err, CMI_E_INVALID, "%s: invalid argument", fn);
    for (int64_t t = 0; t < n; ++t)
        if (u[t] < 0 || u[t] >= n_users || i[t] < 0 || i[t] >= n_items)
            return abi_fail(g_ranksgd_err, CMI_E_INVALID, "%s: id out of range at %lld", fn, (long long)t);
    return CMI_OK;
}

extern "C" int cmi_ranksgd_item_table(int n_users, int n_items, int64_t n, const int32_t *u, const int32_t *i, const double *r,
                                      unsigned flags, int32_t *item_out, double *cum_out, int32_t *n_out) {
    return abi_barrier(g_ranksgd_err, "cmi_ranksgd_item_table", [&] {
        const char *fn = "cmi_ranksgd_item_table";
        if (int rc = ranksgd_check_cells(fn, n_users, n_items, n, u, i, r, flags)) return rc;
        if (!item_out || !cum_out || !n_out) return abi_fail(g_ranksgd_err, CMI_E_INVALID, "%s: invalid argument", fn);
        std::vector<int32_t> col((size_t)n_items, 0);
        int64_t nz = 0;
        for (int64_t t = 0; t < n; ++t)
            if (r[t] != 0.0) ++col[(size_t)i[t]], ++nz;
        const RanksgdTable table = ranksgd_item_table(n_items, col.data(), (flags & CMI_RANKSGD_FLAG_NUM_RATES_SIZE) ? nz : 0);
        if (table.tree)
            return abi_fail(g_ranksgd_err, CMI_E_UNSUPPORTED,
                            "%s: the items with a cell would treeify a java.util.HashMap bin, whose iteration order is not modelled", fn);
        std::copy(table.item.begin(), table.item.end(), item_out);
        std::copy(table.cum.begin(), table.cum.end(), cum_out);
        *n_out = (int32_t)table.item.size();
        return (int)CMI_OK;
    });
}

static int ranksgd_tries_device(uint64_t state, int32_t n_table, const int32_t *item, const double *cum, int64_t n, int32_t *out) {
    const char *fn = "cmi_ranksgd_tries";
    if (int rc = abi_check_device(g_ranksgd_err, fn, 0)) return rc;
    const JavaLcgJump jump = java_lcg_jump_table();
    int32_t *d_item = nullptr, *d_out = nullptr;
    double *d_cum = nullptr;
    hipError_t e = hipSetDevice(0);
    if (e == hipSuccess) e = hipMalloc((void **)&d_item, (size_t)n_table * sizeof(int32_t));
    if (e == hipSuccess) e = hipMalloc((void **)&d_cum, (size_t)n_table * sizeof(double));
    if (e == hipSuccess) e = hipMalloc((void **)&d_out, (size_t)n * sizeof(int32_t));
    if (e == hipSuccess) e = hipMemcpy(d_item, item, (size_t)n_table * sizeof(int32_t), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(d_cum, cum, (size_t)n_table * sizeof(double), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = ranksgd_launch_tries(state, jump, d_item, d_cum, n_table, n, d_out, nullptr);
    if (e == hipSuccess) e = hipMemcpy(out, d_out, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost);
    abi_free(d_item, d_cum, d_out);
    return abi_hip(g_ranksgd_err, fn, e);
}

extern "C" int cmi_ranksgd_tries(int64_t state, int32_t n_table, const int32_t *item, const double *cum, int64_t n, int32_t *out,
                                 int on_device) {
    return abi_barrier(g_ranksgd_err, "cmi_ranksgd_tries", [&] {
        const char *fn = "cmi_ranksgd_tries";
        if (state < 0 || (uint64_t)state > JAVA_LCG_MASK || n_table <= 0 || !item || !cum || n < 0 || n > (1 << 24) || (n > 0 && !out))
            return abi_fail(g_ranksgd_err, CMI_E_INVALID, "%s: invalid argument", fn);
        for (int32_t x = 0; x < n_table; ++x)
            if (item[x] < 0 || std::isnan(cum[x]) || (x > 0 && cum[x] < cum[x - 1]))
                return abi_fail(g_ranksgd_err, CMI_E_INVALID, "%s: entry %d: a negative item, or sums that are not non-decreasing", fn, x);
        if (n == 0) return (int)CMI_OK;
        if (on_device) return ranksgd_tries_device((uint64_t)state, n_table, item, cum, n, out);
        const JavaLcgJump jump = java_lcg_jump_table();
        for (int64_t t = 0; t < n; ++t) out[t] = ranksgd_try(java_lcg_jump(jump, (uint64_t)state, 2 * (uint64_t)t), item, cum, n_table);
        return (int)CMI_OK;
    });
}

extern "C" int cmi_ranksgd_assign_host(int n_users, int n_items, int64_t n, const int32_t *u, const int32_t *i, const double *r,
                                       int64_t n_tries, const int32_t *try_item, int32_t *j_out, int64_t *tries_used) {
    return abi_barrier(g_ranksgd_err, "cmi_ranksgd_assign_host", [&] {
        const char *fn = "cmi_ranksgd_assign_host";
        if (int rc = ranksgd_check_cells(fn, n_users, n_items, n, u, i, r, 0)) return rc;
        if (n_tries < 0 || (n_tries > 0 && !try_item) || !j_out || !tries_used)
            return abi_fail(g_ranksgd_err, CMI_E_INVALID, "%s: invalid argument", fn);
        for (int64_t t = 0; t < n_tries; ++t)
            if (try_item[t] < -1 || try_item[t] >= n_items)
                return abi_fail(g_ranksgd_err, CMI_E_INVALID, "%s: try %lld is no item and not -1", fn, (long long)t);
        const PairHostCsr rows = pair_drop_zeros(pair_csr(n, n_users, u, i, r));
        int64_t bad = 0;
        const int rc = ranksgd_assign(
            n_users, rows.ptr.data(), rows.idx.data(), [&](int64_t t) { return try_item[t]; }, n_tries, j_out, tries_used, &bad);
        if (rc != RANKSGD_OK) return ranksgd_walk_error(g_ranksgd_err, fn, rc, bad, *tries_used);
        return (int)CMI_OK;
    });
}

extern "C" int cmi_ranksgd_sample_host(int n_users, int n_items, int64_t n, const int32_t *u, const int32_t *i, const double *r,
                                       unsigned flags, int64_t *state, int32_t *ou, int32_t *oi, int32_t *oj, double *orr,
                                       int64_t *n_cells, int64_t *tries_used) {
    return abi_barrier(g_ranksgd_err, "cmi_ranksgd_sample_host", [&] {
        const char *fn = "cmi_ranksgd_sample_host";
        if (int rc = ranksgd_check_cells(fn, n_users, n_items, n, u, i, r, flags)) return rc;
        if (!state || *state < 0 || (uint64_t)*state > JAVA_LCG_MASK || !ou || !oi || !oj || !orr || !n_cells)
            return abi_fail(g_ranksgd_err, CMI_E_INVALID, "%s: invalid argument", fn);
        const PairHostCsr all = pair_csr(n, n_users, u, i, r);
        for (int a = 0; a < n_users; ++a)
            for (int32_t q = all.ptr[(size_t)a] + 1; q < all.ptr[(size_t)a + 1]; ++q)
                if (all.idx[(size_t)q] == all.idx[(size_t)q - 1])
                    return abi_fail(g_ranksgd_err, CMI_E_INVALID, "%s: duplicate cell (user %d, item %d)", fn, a, all.idx[(size_t)q]);
        PairHostCsr rows;
        RanksgdTable table;
        if (int rc = ranksgd_prepare(g_ranksgd_err, fn, all, n_users, n_items, flags, rows, table)) return rc;
        const JavaLcgJump jump = java_lcg_jump_table();
        RanksgdHostTries host{table, jump, (uint64_t)*state, (uint64_t)*state};
        int64_t used = 0, bad = 0;
        const int rc = ranksgd_assign(n_users, rows.ptr.data(), rows.idx.data(), host, RANKSGD_MAX_TRIES, oj, &used, &bad);
        if (rc != RANKSGD_OK) return ranksgd_walk_error(g_ranksgd_err, fn, rc, bad, used);
        for (int32_t a = 0; a < n_users; ++a)
            for (int32_t q = rows.ptr[(size_t)a]; q < rows.ptr[(size_t)a + 1]; ++q) ou[q] = a;
        std::copy(rows.idx.begin(), rows.idx.end(), oi);
        std::copy(rows.val.begin(), rows.val.end(), orr);
        *n_cells = (int64_t)rows.idx.size();
        if (tries_used) *tries_used = used;
        *state = (int64_t)java_lcg_jump(jump, (uint64_t)*state, 2 * (uint64_t)used);
        return (int)CMI_OK;
    });
}
