// bpr_api.cpp -- C ABI of BPR (include/carskit_mi355x.h, cmi_bpr_*, cmi_java_*): the host walk that defines the sampler, the device
// sampler's reservation and fallback, the per-iteration level schedule and its launches.
#include "../../include/carskit_mi355x.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <string>
#include <vector>

#include "bpr_kernels.hpp"
#include "level_schedule.hpp"
#include "pair_host.hpp"
#include "rank_host.hpp"
#include "rankals_kernels.hpp"

using namespace cmi;

struct cmi_bpr_instance : PairModelBase {
    int k = 0;
    unsigned flags = 0;
    PairHostCsr rows; // train.row(u): the non-zero cells, items ascending
    int64_t S = 0, L = 0, n_blocks = 0;
    uint64_t state = java_lcg_scramble(0);
    JavaLcgJump jump = java_lcg_jump_table();
    int32_t *d_rptr = nullptr, *d_ridx = nullptr;
    // the device sampler's reservation (absent: every iteration is sampled by the host walk)
    bool device_sampler = false;
    uint8_t *d_len = nullptr;
    uint16_t *d_exit = nullptr, *d_cnt = nullptr;
    int32_t *d_entry = nullptr;
    int64_t *d_base = nullptr, *d_result = nullptr, *d_pos = nullptr;
    // the iteration's triples and schedule
    int32_t *d_u = nullptr, *d_i = nullptr, *d_j = nullptr, *d_order = nullptr, *d_level_ptr = nullptr;
    std::vector<int32_t> tu, ti, tj, order, level_ptr;
    double *d_slots = nullptr, *d_parts = nullptr, *d_loss = nullptr;
    double *d_P = nullptr, *d_Q = nullptr;
    bool have_model = false, iterated = false, evaluated = false;
    hipEvent_t ev[3] = {nullptr, nullptr, nullptr};
    float iter_ms[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
    int64_t sched[4] = {0, 0, 0, 0}, fallbacks = 0;
    RankWorkspace rank_ws;
};

static thread_local std::string g_bpr_err;

extern "C" const char *cmi_bpr_last_error(cmi_bpr_handle h) { return h ? h->err.c_str() : g_bpr_err.c_str(); }
extern "C" int cmi_bpr_rank_block(void) { return BPR_RANK_BLOCK; }

static void bpr_free_ratings(cmi_bpr_instance *h) {
    abi_free(h->d_rptr, h->d_ridx, h->d_len, h->d_exit, h->d_cnt, h->d_entry, h->d_base, h->d_result, h->d_pos);
    abi_free(h->d_u, h->d_i, h->d_j, h->d_order, h->d_level_ptr, h->d_slots, h->d_parts, h->d_loss);
    h->have_ratings = h->iterated = h->device_sampler = false;
}

static void bpr_free_all(cmi_bpr_instance *h) {
    bpr_free_ratings(h);
    abi_free(h->d_P, h->d_Q);
    h->have_model = false;
    h->rank_ws.release();
    for (hipEvent_t &e : h->ev) {
        if (e) (void)hipEventDestroy(e);
        e = nullptr;
    }
}

extern "C" int cmi_bpr_destroy(cmi_bpr_handle h) { return pair_destroy(h, bpr_free_all); }

// BPR.java:39-52.  A 16-lane group holds a row in 8 registers per lane: k <= 128
extern "C" int cmi_bpr_create(int k, int n_users, int n_items, int device, unsigned flags, cmi_bpr_handle *out) {
    if (out && k > BPR_MAX_K) {
        *out = nullptr;
        return abi_fail(g_bpr_err, CMI_E_UNSUPPORTED, "cmi_bpr_create: %d factors: a 16-lane group holds a sample's rows in registers, k <= %d",
                        k, BPR_MAX_K);
    }
    if (out && n_users > 0 && (int64_t)n_users * 100 >= ((int64_t)1 << 31)) {
        *out = nullptr;
        return abi_fail(g_bpr_err, CMI_E_UNSUPPORTED, "cmi_bpr_create: %d users: more than 2^31-1 samples an iteration", n_users);
    }
    const bool valid = k >= 1 && (flags & ~(CMI_BPR_FLAG_STRICT | CMI_BPR_FLAG_HOST_SAMPLER | CMI_BPR_FLAG_MIN_SLACK)) == 0;
    int rc = pair_create(g_bpr_err, "cmi_bpr_create", valid, n_users, n_items, device, out, cmi_bpr_destroy,
                         [k, flags](cmi_bpr_instance *h) { h->k = k, h->flags = flags; });
    if (rc != CMI_OK) return rc;
    cmi_bpr_instance *h = *out;
    hipError_t e = hipSuccess;
    for (hipEvent_t &ev : h->ev)
        if (e == hipSuccess) e = hipEventCreate(&ev);
    if (e != hipSuccess) {
        cmi_bpr_destroy(h);
        *out = nullptr;
        return abi_fail(g_bpr_err, CMI_E_HIP, "cmi_bpr_create: %s", hipGetErrorString(e));
    }
    return CMI_OK;
}

// the checked cells as train's rows without the zero-valued cells; the reference's endless loops are refused here
static int bpr_rows(std::string &err, const char *fn, const PairHostCsr &all, int n_users, int n_items, PairHostCsr &rows) {
    rows = pair_drop_zeros(all);
    bool any = false;
    for (int a = 0; a < n_users; ++a) {
        const int32_t cnt = rows.ptr[(size_t)a + 1] - rows.ptr[(size_t)a];
        any = any || cnt > 0;
        if (cnt >= n_items)
            return abi_fail(err, CMI_E_INVALID, "%s: user %d holds every item: BPR.java:75-77 would draw j for ever", fn, a);
    }
    if (!any) return abi_fail(err, CMI_E_INVALID, "%s: no user with a non-zero cell: BPR.java:65-70 would draw u for ever", fn);
    return CMI_OK;
}

// BPR.java:60-80 for n_samples samples: the definition of the sampler
static void bpr_host_walk(const PairHostCsr &rows, int n_users, int n_items, uint64_t *state, int64_t n_samples, int32_t *u, int32_t *i,
                          int32_t *j) {
    JavaStream rng{*state, 0};
    for (int64_t s = 0; s < n_samples; ++s) (void)bpr_draw(rng, n_users, n_items, rows.ptr.data(), rows.idx.data(), INT64_MAX, u[s], i[s], j[s]);
    *state = rng.state;
}

// stream positions to speculate on: the expected draws of S samples (one u draw per non-empty pick, one i, the j draws of a row that
// holds cnt of the items), a twentieth more, and room for the variance of a few long rows
static int64_t bpr_reservation(const cmi_bpr_instance *h) {
    if (h->flags & CMI_BPR_FLAG_MIN_SLACK) return 3 * h->S;
    int64_t nonempty = 0;
    double ej = 0.0;
    for (int a = 0; a < h->n_users; ++a) {
        const int32_t cnt = h->rows.ptr[(size_t)a + 1] - h->rows.ptr[(size_t)a];
        if (cnt == 0) continue;
        ++nonempty;
        ej += (double)h->n_items / (double)(h->n_items - cnt);
    }
    const double per = (double)h->n_users / (double)nonempty + 1.0 + ej / (double)nonempty;
    return (int64_t)std::ceil((double)h->S * per * 1.05) + 16 * BPR_RANK_BLOCK;
}

static int bpr_set_ratings_impl(cmi_bpr_handle h, int64_t n, const int32_t *u, const int32_t *i, const double *r) {
    const char *fn = "cmi_bpr_set_ratings";
    PairHostCsr all, cols;
    if (int rc = pair_ingest(h, fn, n, u, i, r, /*scan_items=*/false, all, cols)) return rc;
    PairHostCsr rows;
    if (int rc = bpr_rows(h->err, fn, all, h->n_users, h->n_items, rows)) return rc;
    CMI_HIP(h, hipSetDevice(h->device));
    CMI_HIP(h, hipStreamSynchronize(h->stream));
    bpr_free_ratings(h);
    h->rows = std::move(rows);
    h->S = (int64_t)h->n_users * 100;
    h->L = bpr_reservation(h);
    h->n_blocks = (h->L + BPR_RANK_BLOCK - 1) / BPR_RANK_BLOCK;
    const size_t S = (size_t)h->S;
    hipError_t e = abi_upload(&h->d_rptr, h->rows.ptr, h->stream, true);
    if (e == hipSuccess) e = abi_upload(&h->d_ridx, h->rows.idx, h->stream, true);
    if (e == hipSuccess) e = hipMalloc((void **)&h->d_u, S * sizeof(int32_t));
    if (e == hipSuccess) e = hipMalloc((void **)&h->d_i, S * sizeof(int32_t));
    if (e == hipSuccess) e = hipMalloc((void **)&h->d_j, S * sizeof(int32_t));
    if (e == hipSuccess) e = hipMalloc((void **)&h->d_order, S * sizeof(int32_t));
    if (e == hipSuccess) e = hipMalloc((void **)&h->d_level_ptr, (S + 1) * sizeof(int32_t));
    if (e == hipSuccess) e = hipMalloc((void **)&h->d_slots, S * (size_t)(h->k + 1) * sizeof(double));
    if (e == hipSuccess) e = hipMalloc((void **)&h->d_parts, BPR_LOSS_PARTS * sizeof(double));
    if (e == hipSuccess) e = hipMalloc((void **)&h->d_loss, sizeof(double));
    if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
    if (e != hipSuccess) {
        bpr_free_ratings(h);
        CMI_FAIL(h, CMI_E_HIP, "%s: %s", fn, hipGetErrorString(e));
    }
    if (!(h->flags & CMI_BPR_FLAG_HOST_SAMPLER)) { // the sampler's reservation: without it the host walk serves
        const size_t nb = (size_t)h->n_blocks;
        e = hipMalloc((void **)&h->d_len, (size_t)h->L);
        if (e == hipSuccess) e = hipMalloc((void **)&h->d_exit, nb * BPR_RANK_ENTRIES * sizeof(uint16_t));
        if (e == hipSuccess) e = hipMalloc((void **)&h->d_cnt, nb * BPR_RANK_ENTRIES * sizeof(uint16_t));
        if (e == hipSuccess) e = hipMalloc((void **)&h->d_entry, nb * sizeof(int32_t));
        if (e == hipSuccess) e = hipMalloc((void **)&h->d_base, nb * sizeof(int64_t));
        if (e == hipSuccess) e = hipMalloc((void **)&h->d_result, 2 * sizeof(int64_t));
        if (e == hipSuccess) e = hipMalloc((void **)&h->d_pos, S * sizeof(int64_t));
        h->device_sampler = e == hipSuccess;
        if (e != hipSuccess) {
            (void)hipGetLastError();
            abi_free(h->d_len, h->d_exit, h->d_cnt, h->d_entry, h->d_base, h->d_result, h->d_pos);
        }
    }
    h->tu.resize(S), h->ti.resize(S), h->tj.resize(S);
    h->have_ratings = true;
    return CMI_OK;
}

extern "C" int cmi_bpr_set_ratings(cmi_bpr_handle h, int64_t n, const int32_t *u, const int32_t *i, const double *r) {
    if (!h) return CMI_E_INVALID;
    return abi_barrier(h->err, "cmi_bpr_set_ratings", [&] { return bpr_set_ratings_impl(h, n, u, i, r); }, [h] { bpr_free_ratings(h); });
}

static int bpr_set_model_impl(cmi_bpr_handle h, const double *P, const double *Q) {
    if (!h->have_model && (!P || !Q)) CMI_FAIL(h, CMI_E_INVALID, "cmi_bpr_set_model: the first call sets both P and Q");
    CMI_HIP(h, hipSetDevice(h->device));
    const size_t pn = (size_t)h->n_users * h->k, qn = (size_t)h->n_items * h->k;
    if (!h->d_P) {
        hipError_t e = hipMalloc((void **)&h->d_P, pn * sizeof(double));
        if (e == hipSuccess) e = hipMalloc((void **)&h->d_Q, qn * sizeof(double));
        if (e != hipSuccess) {
            abi_free(h->d_P, h->d_Q);
            CMI_FAIL(h, CMI_E_HIP, "cmi_bpr_set_model: %s", hipGetErrorString(e));
        }
    }
    if (P) CMI_HIP(h, hipMemcpyAsync(h->d_P, P, pn * sizeof(double), hipMemcpyHostToDevice, h->stream));
    if (Q) CMI_HIP(h, hipMemcpyAsync(h->d_Q, Q, qn * sizeof(double), hipMemcpyHostToDevice, h->stream));
    CMI_HIP(h, hipStreamSynchronize(h->stream));
    h->have_model = true;
    return CMI_OK;
}

// IterativeRecommender.java:235-241 with initByNorm = false (P and Q uniform, drawn by the host) and any later injection
extern "C" int cmi_bpr_set_model(cmi_bpr_handle h, const double *P, const double *Q) {
    if (!h) return CMI_E_INVALID;
    return abi_barrier(h->err, "cmi_bpr_set_model", [&] { return bpr_set_model_impl(h, P, Q); });
}

extern "C" int cmi_bpr_get_model(cmi_bpr_handle h, double *P, double *Q) {
    if (!h) return CMI_E_INVALID;
    return abi_barrier(h->err, "cmi_bpr_get_model", [&] {
        if (!h->have_model) CMI_FAIL(h, CMI_E_INVALID, "cmi_bpr_get_model: no model (cmi_bpr_set_model first)");
        CMI_HIP(h, hipSetDevice(h->device));
        if (P) CMI_HIP(h, hipMemcpyAsync(P, h->d_P, (size_t)h->n_users * h->k * sizeof(double), hipMemcpyDeviceToHost, h->stream));
        if (Q) CMI_HIP(h, hipMemcpyAsync(Q, h->d_Q, (size_t)h->n_items * h->k * sizeof(double), hipMemcpyDeviceToHost, h->stream));
        CMI_HIP(h, hipStreamSynchronize(h->stream));
        return CMI_OK;
    });
}

extern "C" int cmi_bpr_set_random_state(cmi_bpr_handle h, int64_t state) {
    if (!h) return CMI_E_INVALID;
    if (state < 0 || (uint64_t)state > JAVA_LCG_MASK) CMI_FAIL(h, CMI_E_INVALID, "cmi_bpr_set_random_state: not a 48-bit state");
    h->state = (uint64_t)state;
    return CMI_OK;
}
extern "C" int cmi_bpr_get_random_state(cmi_bpr_handle h, int64_t *state) {
    if (!h || !state) return CMI_E_INVALID;
    *state = (int64_t)h->state;
    return CMI_OK;
}

// one iteration's triples from h->state into h->tu / ti / tj and d_u / d_i / d_j; *after: the state after the last consumed draw
static int bpr_sample_impl(cmi_bpr_handle h, bool on_device, uint64_t *after) {
    const size_t S = (size_t)h->S;
    if (on_device && h->device_sampler) {
        BprSampler a;
        a.n_users = h->n_users, a.n_items = h->n_items, a.rptr = h->d_rptr, a.ridx = h->d_ridx, a.state0 = h->state;
        a.L = h->L, a.S = h->S, a.n_blocks = h->n_blocks;
        a.len = h->d_len, a.exit_off = h->d_exit, a.cnt = h->d_cnt, a.entry = h->d_entry, a.base = h->d_base, a.result = h->d_result;
        a.pos = h->d_pos, a.u = h->d_u, a.i = h->d_i, a.j = h->d_j;
        int64_t result[2] = {0, 0};
        CMI_HIP(h, bpr_launch_sampler(a, h->jump, h->stream));
        CMI_HIP(h, hipMemcpyAsync(result, h->d_result, sizeof(int64_t), hipMemcpyDeviceToHost, h->stream));
        CMI_HIP(h, hipStreamSynchronize(h->stream));
        if (result[0] >= h->S) { // the list holds S samples inside L and meets no overflow before the last of them
            CMI_HIP(h, bpr_launch_emit(a, h->jump, h->stream));
            CMI_HIP(h, hipMemcpyAsync(result, h->d_result, 2 * sizeof(int64_t), hipMemcpyDeviceToHost, h->stream));
            CMI_HIP(h, hipMemcpyAsync(h->tu.data(), h->d_u, S * sizeof(int32_t), hipMemcpyDeviceToHost, h->stream));
            CMI_HIP(h, hipMemcpyAsync(h->ti.data(), h->d_i, S * sizeof(int32_t), hipMemcpyDeviceToHost, h->stream));
            CMI_HIP(h, hipMemcpyAsync(h->tj.data(), h->d_j, S * sizeof(int32_t), hipMemcpyDeviceToHost, h->stream));
            CMI_HIP(h, hipStreamSynchronize(h->stream));
            *after = java_lcg_jump(h->jump, h->state, (uint64_t)result[1]);
            return CMI_OK;
        }
    }
    // the reservation could not be allocated, the list left L, or it met an overflow mark: exactness never depends on the guess.  (With
    // CMI_BPR_FLAG_HOST_SAMPLER the device form is switched off: nothing fell back)
    if (on_device && !(h->flags & CMI_BPR_FLAG_HOST_SAMPLER)) ++h->fallbacks;
    uint64_t st = h->state;
    bpr_host_walk(h->rows, h->n_users, h->n_items, &st, h->S, h->tu.data(), h->ti.data(), h->tj.data());
    CMI_HIP(h, hipMemcpyAsync(h->d_u, h->tu.data(), S * sizeof(int32_t), hipMemcpyHostToDevice, h->stream));
    CMI_HIP(h, hipMemcpyAsync(h->d_i, h->ti.data(), S * sizeof(int32_t), hipMemcpyHostToDevice, h->stream));
    CMI_HIP(h, hipMemcpyAsync(h->d_j, h->tj.data(), S * sizeof(int32_t), hipMemcpyHostToDevice, h->stream));
    CMI_HIP(h, hipStreamSynchronize(h->stream));
    *after = st;
    return CMI_OK;
}

extern "C" int cmi_bpr_sample(cmi_bpr_handle h, int on_device, int32_t *u, int32_t *i, int32_t *j, int64_t *state_after) {
    if (!h) return CMI_E_INVALID;
    return abi_barrier(h->err, "cmi_bpr_sample", [&] {
        if (!u || !i || !j) CMI_FAIL(h, CMI_E_INVALID, "cmi_bpr_sample: null arrays");
        if (!h->have_ratings) CMI_FAIL(h, CMI_E_INVALID, "cmi_bpr_sample: no ratings (cmi_bpr_set_ratings first)");
        CMI_HIP(h, hipSetDevice(h->device));
        uint64_t after = 0;
        if (int rc = bpr_sample_impl(h, on_device != 0, &after)) return rc;
        std::copy(h->tu.begin(), h->tu.end(), u);
        std::copy(h->ti.begin(), h->ti.end(), i);
        std::copy(h->tj.begin(), h->tj.end(), j);
        if (state_after) *state_after = (int64_t)after;
        return CMI_OK;
    });
}

static float ms_since(std::chrono::steady_clock::time_point t0) {
    return std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
}

static int bpr_iterate_impl(cmi_bpr_handle h, double lrate, double regU, double regI, double *loss) {
    const char *fn = "cmi_bpr_iterate";
    if (!h->have_ratings) CMI_FAIL(h, CMI_E_INVALID, "%s: no ratings (cmi_bpr_set_ratings first)", fn);
    if (!h->have_model) CMI_FAIL(h, CMI_E_INVALID, "%s: no model (cmi_bpr_set_model first)", fn);
    CMI_HIP(h, hipSetDevice(h->device));
    auto t0 = std::chrono::steady_clock::now();
    uint64_t after = 0;
    if (int rc = bpr_sample_impl(h, !(h->flags & CMI_BPR_FLAG_HOST_SAMPLER), &after)) return rc;
    h->iter_ms[0] = ms_since(t0);

    t0 = std::chrono::steady_clock::now();
    const int32_t n_levels =
        build_triple_levels(h->S, h->tu.data(), h->ti.data(), h->tj.data(), h->n_users, h->n_items, h->order, h->level_ptr);
    h->iter_ms[1] = ms_since(t0);

    BprEpoch a;
    a.k = h->k, a.P = h->d_P, a.Q = h->d_Q, a.u = h->d_u, a.i = h->d_i, a.j = h->d_j, a.order = h->d_order, a.level_ptr = h->d_level_ptr;
    a.slots = h->d_slots, a.lrate = lrate, a.regU = regU, a.regI = regI;
    CMI_HIP(h, hipMemcpyAsync(h->d_order, h->order.data(), h->order.size() * sizeof(int32_t), hipMemcpyHostToDevice, h->stream));
    CMI_HIP(h, hipMemcpyAsync(h->d_level_ptr, h->level_ptr.data(), h->level_ptr.size() * sizeof(int32_t), hipMemcpyHostToDevice, h->stream));
    CMI_HIP(h, hipEventRecord(h->ev[0], h->stream));
    // a level wider than one workgroup's samples on its own; a run of consecutive narrower levels in one launch of one workgroup
    int64_t sched[4] = {0, 0, 0, 0};
    CMI_HIP(h, launch_triple_levels(
                   h->level_ptr, n_levels, BPR_WG_SAMPLES, [&](int32_t b0, int32_t b1) { return bpr_launch_level(a, b0, b1, h->stream); },
                   [&](int32_t l0, int32_t l1) { return bpr_launch_run(a, l0, l1, h->stream); }, sched));
    CMI_HIP(h, hipEventRecord(h->ev[1], h->stream));
    CMI_HIP(h, bpr_launch_loss(h->d_slots, h->S * (int64_t)(h->k + 1), (h->flags & CMI_BPR_FLAG_STRICT) != 0, h->d_parts, h->d_loss, h->stream));
    CMI_HIP(h, hipEventRecord(h->ev[2], h->stream));
    double l = 0.0;
    CMI_HIP(h, hipMemcpyAsync(&l, h->d_loss, sizeof(double), hipMemcpyDeviceToHost, h->stream));
    CMI_HIP(h, hipStreamSynchronize(h->stream));
    CMI_HIP(h, hipEventElapsedTime(&h->iter_ms[2], h->ev[0], h->ev[1]));
    CMI_HIP(h, hipEventElapsedTime(&h->iter_ms[3], h->ev[1], h->ev[2]));
    h->state = after;
    std::copy(sched, sched + 4, h->sched);
    h->iterated = true;
    if (loss) *loss = l;
    if (!std::isfinite(l)) CMI_FAIL(h, CMI_E_NUMERIC, "%s: loss = %g", fn, l);
    return CMI_OK;
}

extern "C" int cmi_bpr_iterate(cmi_bpr_handle h, double lrate, double regU, double regI, double *loss) {
    if (!h) return CMI_E_INVALID;
    return abi_barrier(h->err, "cmi_bpr_iterate", [&] { return bpr_iterate_impl(h, lrate, regU, regI, loss); });
}

static int bpr_predict_impl(cmi_bpr_handle h, int64_t n, const int32_t *u, const int32_t *j, double *out) {
    if (!h->have_model) CMI_FAIL(h, CMI_E_INVALID, "cmi_bpr_predict_batch: no model (cmi_bpr_set_model first)");
    if (int rc = pair_check_tuples(h, "cmi_bpr_predict_batch", n, u, j, out)) return rc;
    if (n == 0) return CMI_OK;
    return abi_predict(h, "cmi_bpr_predict_batch", n, u, j, nullptr, nullptr, 0, out, [&](const AbiTuples &t, double *d_out) {
        return abi_hip(h->err, "cmi_bpr_predict_batch", rankals_launch_predict(h->d_P, h->d_Q, h->k, n, t.a, t.b, d_out, h->stream));
    });
}

// IterativeRecommender.predict(u, j) = DenseMatrix.rowMult(P, u, Q, j) of n tuples: RankALS's kernel
extern "C" int cmi_bpr_predict_batch(cmi_bpr_handle h, int64_t n, const int32_t *u, const int32_t *j, double *out) {
    if (!h) return CMI_E_INVALID;
    return abi_barrier(h->err, "cmi_bpr_predict_batch", [&] { return bpr_predict_impl(h, n, u, j, out); });
}

extern "C" int cmi_bpr_eval_rankings(cmi_bpr_handle h, int64_t n_train, const int32_t *tu, const int32_t *tj, const int32_t *tctx,
                                     const double *tr, int64_t n_test, const int32_t *su, const int32_t *sj, const int32_t *sctx,
                                     const double *sr, double bin_thold, int num_recs, int num_ignore, int strategy, double out[21],
                                     int64_t *n_queries, int32_t *q_user, int32_t *q_ctx, int32_t *q_count, int32_t *top_items,
                                     double *top_scores) {
    if (!h) return CMI_E_INVALID;
    return abi_barrier(h->err, "bpr_eval_rankings", [&] {
        auto ready = [h]() -> int {
            if (!h->have_model) CMI_FAIL(h, CMI_E_INVALID, "bpr: call cmi_bpr_set_model first");
            CMI_HIP(h, hipSetDevice(h->device));
            return CMI_OK;
        };
        auto score = [&](const RankPlan &plan, const RankBatchFn &on_batch) {
            const RankSlabFn fill = [h](double *dS, const int32_t *dcand, int nc, const int32_t *dgu, const int32_t *dgq0, int g0, int g1,
                                        int64_t q0, int64_t nq, hipStream_t s) {
                static_assert(BPR_MAX_K <= RANK_SCORE_MAX_K, "BPR scores with RankALS's kernel: its rows must fit that kernel's LDS row");
                return rankals_launch_score(h->d_P, h->d_Q, h->k, dcand, nc, dgu, dgq0, g0, g1, q0, nq, dS, s);
            };
            return rank_run_device_slab(h->stream, h->rank_ws, plan, fill, bin_thold, num_recs, on_batch, &h->iter_ms[4]);
        };
        const RankEvalIO io{{n_train, tu, tj, tctx, tr}, {n_test, su, sj, sctx, sr}, bin_thold, num_recs, num_ignore, strategy, out, n_queries,
                            q_user, q_ctx, q_count, top_items, top_scores};
        const int rc = rank_evaluate(h->err, "bpr_eval_rankings", h->rank_ws, h->n_users, h->n_items, INT64_MAX, io, ready, score);
        if (rc == CMI_OK) h->evaluated = true;
        return rc;
    });
}

extern "C" int cmi_bpr_last_iter_ms(cmi_bpr_handle h, float *ms) {
    if (!h || !ms) return CMI_E_INVALID;
    if (!h->iterated && !h->evaluated) CMI_FAIL(h, CMI_E_INVALID, "cmi_bpr_last_iter_ms: no iteration and no evaluation yet");
    for (int p = 0; p < 4; ++p) ms[p] = h->iterated ? h->iter_ms[p] : 0.f;
    ms[4] = h->evaluated ? h->iter_ms[4] : 0.f;
    return CMI_OK;
}

extern "C" int cmi_bpr_last_schedule(cmi_bpr_handle h, int64_t *out) {
    if (!h || !out) return CMI_E_INVALID;
    for (int p = 0; p < 4; ++p) out[p] = h->iterated ? h->sched[p] : 0;
    out[4] = h->fallbacks;
    return CMI_OK;
}

// ---- without a device ---------------------------------------------------------------------------------------------------------------
static int bpr_check_ids(const char *fn, int64_t n, int n_users, int n_items, const int32_t *u, const int32_t *i, const int32_t *j) {
    for (int64_t t = 0; t < n; ++t)
        if (u[t] < 0 || u[t] >= n_users || i[t] < 0 || i[t] >= n_items || (j && (j[t] < 0 || j[t] >= n_items)))
            return abi_fail(g_bpr_err, CMI_E_INVALID, "%s: id out of range at %lld", fn, (long long)t);
    return CMI_OK;
}

extern "C" int cmi_bpr_levels(int n_users, int n_items, int64_t n, const int32_t *u, const int32_t *i, const int32_t *j, int32_t *order,
                              int32_t *level_of, int32_t *n_levels, int64_t *max_chain) {
    return abi_barrier(g_bpr_err, "cmi_bpr_levels", [&] {
        const char *fn = "cmi_bpr_levels";
        if (n_users <= 0 || n_items <= 0 || n < 0 || n >= ((int64_t)1 << 31) || (n > 0 && (!u || !i || !j || !order)))
            return abi_fail(g_bpr_err, CMI_E_INVALID, "%s: invalid argument", fn);
        if (int rc = bpr_check_ids(fn, n, n_users, n_items, u, i, j)) return rc;
        std::vector<int32_t> ord, ptr;
        int64_t chain = 0;
        const int32_t nl = build_triple_levels(n, u, i, j, n_users, n_items, ord, ptr, &chain);
        std::copy(ord.begin(), ord.end(), order);
        if (level_of)
            for (int32_t l = 0; l < nl; ++l)
                for (int32_t x = ptr[(size_t)l]; x < ptr[(size_t)l + 1]; ++x) level_of[ord[(size_t)x]] = l + 1;
        if (n_levels) *n_levels = nl;
        if (max_chain) *max_chain = chain;
        return (int)CMI_OK;
    });
}

extern "C" int cmi_bpr_sample_host(int n_users, int n_items, int64_t n, const int32_t *u, const int32_t *i, const double *r, int64_t *state,
                                   int64_t n_samples, int32_t *ou, int32_t *oi, int32_t *oj) {
    return abi_barrier(g_bpr_err, "cmi_bpr_sample_host", [&] {
        const char *fn = "cmi_bpr_sample_host";
        if (n_users <= 0 || n_items <= 0 || n < 0 || n >= ((int64_t)1 << 31) || (n > 0 && (!u || !i || !r)) || !state || *state < 0 ||
            (uint64_t)*state > JAVA_LCG_MASK || n_samples < 0 || (n_samples > 0 && (!ou || !oi || !oj)))
            return abi_fail(g_bpr_err, CMI_E_INVALID, "%s: invalid argument", fn);
        if (int rc = bpr_check_ids(fn, n, n_users, n_items, u, i, nullptr)) return rc;
        PairHostCsr rows;
        if (int rc = bpr_rows(g_bpr_err, fn, pair_csr(n, n_users, u, i, r), n_users, n_items, rows)) return rc;
        uint64_t st = (uint64_t)*state;
        bpr_host_walk(rows, n_users, n_items, &st, n_samples, ou, oi, oj);
        *state = (int64_t)st;
        return (int)CMI_OK;
    });
}

// ---- probes of java_math.hpp ------------------------------------------------------------------------------------------------------
static int java_next_ints_device(uint64_t *state, int32_t bound, int64_t n, int32_t *out) {
    const char *fn = "cmi_java_next_ints";
    if (int rc = abi_check_device(g_bpr_err, fn, 0)) return rc;
    const JavaLcgJump jump = java_lcg_jump_table();
    const int64_t L = 4 * n + 64; // positions speculated on: a value takes two draws on average at the worst bound
    int32_t *d_val = nullptr, *d_used = nullptr;
    std::vector<int32_t> val((size_t)L), used((size_t)L);
    hipError_t e = hipSetDevice(0);
    if (e == hipSuccess) e = hipMalloc((void **)&d_val, (size_t)L * sizeof(int32_t));
    if (e == hipSuccess) e = hipMalloc((void **)&d_used, (size_t)L * sizeof(int32_t));
    if (e == hipSuccess) e = bpr_launch_next_ints(*state, bound, L, jump, d_val, d_used, nullptr);
    if (e == hipSuccess) e = hipMemcpy(val.data(), d_val, (size_t)L * sizeof(int32_t), hipMemcpyDeviceToHost);
    if (e == hipSuccess) e = hipMemcpy(used.data(), d_used, (size_t)L * sizeof(int32_t), hipMemcpyDeviceToHost);
    abi_free(d_val, d_used);
    if (e != hipSuccess) return abi_fail(g_bpr_err, CMI_E_HIP, "%s: %s", fn, hipGetErrorString(e));
    int64_t pos = 0;
    for (int64_t t = 0; t < n; ++t) {
        if (pos >= L || val[(size_t)pos] < 0) return abi_fail(g_bpr_err, CMI_E_HOST, "%s: the list left the %lld positions speculated on", fn, (long long)L);
        out[t] = val[(size_t)pos];
        pos += used[(size_t)pos];
    }
    *state = java_lcg_jump(jump, *state, (uint64_t)pos);
    return CMI_OK;
}

extern "C" int cmi_java_next_ints(int64_t *state, int32_t bound, int64_t n, int32_t *out, int on_device) {
    return abi_barrier(g_bpr_err, "cmi_java_next_ints", [&] {
        if (!state || *state < 0 || (uint64_t)*state > JAVA_LCG_MASK || bound <= 0 || n < 0 || n > (1 << 24) || (n > 0 && !out))
            return abi_fail(g_bpr_err, CMI_E_INVALID, "cmi_java_next_ints: invalid argument");
        uint64_t st = (uint64_t)*state;
        if (on_device) {
            if (int rc = java_next_ints_device(&st, bound, n, out)) return rc;
        } else {
            JavaStream rng{st, 0};
            for (int64_t t = 0; t < n; ++t) out[t] = rng.nextInt(bound, INT64_MAX);
            st = rng.state;
        }
        *state = (int64_t)st;
        return (int)CMI_OK;
    });
}

extern "C" int cmi_java_exp_log(int64_t n, const double *x, double *exp_out, double *log_out, int on_device) {
    return abi_barrier(g_bpr_err, "cmi_java_exp_log", [&] {
        const char *fn = "cmi_java_exp_log";
        if (n < 0 || (n > 0 && (!x || !exp_out || !log_out))) return abi_fail(g_bpr_err, CMI_E_INVALID, "%s: invalid argument", fn);
        if (!on_device) {
            for (int64_t t = 0; t < n; ++t) exp_out[t] = fdlibm_exp(x[t]), log_out[t] = fdlibm_log(x[t]);
            return (int)CMI_OK;
        }
        if (int rc = abi_check_device(g_bpr_err, fn, 0)) return rc;
        if (n == 0) return (int)CMI_OK;
        double *d_x = nullptr, *d_e = nullptr, *d_l = nullptr;
        const size_t bytes = (size_t)n * sizeof(double);
        hipError_t e = hipSetDevice(0);
        if (e == hipSuccess) e = hipMalloc((void **)&d_x, bytes);
        if (e == hipSuccess) e = hipMalloc((void **)&d_e, bytes);
        if (e == hipSuccess) e = hipMalloc((void **)&d_l, bytes);
        if (e == hipSuccess) e = hipMemcpy(d_x, x, bytes, hipMemcpyHostToDevice);
        if (e == hipSuccess) e = bpr_launch_exp_log(n, d_x, d_e, d_l, nullptr);
        if (e == hipSuccess) e = hipMemcpy(exp_out, d_e, bytes, hipMemcpyDeviceToHost);
        if (e == hipSuccess) e = hipMemcpy(log_out, d_l, bytes, hipMemcpyDeviceToHost);
        abi_free(d_x, d_e, d_l);
        return abi_hip(g_bpr_err, fn, e);
    });
}
