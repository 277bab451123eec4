// bpmf_api.cpp -- C ABI of BPMF (include/carskit_mi355x.h, cmi_bpmf_*, cmi_java_next_gaussians).
#include "../../include/carskit_mi355x.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <climits>
#include <cmath>
#include <cstdio>
#include <string>
#include <vector>

#include "bpmf_host.hpp"
#include "bpmf_kernels.hpp"
#include "pair_host.hpp"

using namespace cmi;

// the device buffers of the gaussian stream: a count and an offset per workgroup of attempts, and where the round ended
struct BpmfGaussWork {
    int32_t *d_cnt = nullptr, *d_off = nullptr;
    BpmfGaussTail *d_tail = nullptr;
    int64_t blocks = 0;
    void release() {
        abi_free(d_cnt, d_off, d_tail);
        blocks = 0;
    }
    hipError_t reserve(int64_t n_blocks) {
        hipError_t e = hipSuccess;
        if (!d_tail) e = hipMalloc((void **)&d_tail, sizeof(BpmfGaussTail));
        if (e != hipSuccess || n_blocks <= blocks) return e;
        abi_free(d_cnt, d_off);
        blocks = 0;
        e = hipMalloc((void **)&d_cnt, (size_t)n_blocks * sizeof(int32_t));
        if (e == hipSuccess) e = hipMalloc((void **)&d_off, (size_t)n_blocks * sizeof(int32_t));
        if (e == hipSuccess) blocks = n_blocks;
        return e;
    }
};

struct cmi_bpmf_instance : PairModelBase {
    int k = 0;
    unsigned flags = 0;
    double gm = 0.0;
    // [0]: user -> (item, value), [1]: item -> (user, value): CSR, ascending, without the zero-valued cells; slots: the rows with entries
    int32_t *d_ptr[2] = {nullptr, nullptr}, *d_idx[2] = {nullptr, nullptr}, *d_slots[2] = {nullptr, nullptr};
    double *d_val[2] = {nullptr, nullptr};
    std::vector<int32_t> slot_rows[2];
    // every stored cell in CRS order (the loss), with its user
    int32_t *d_lptr = nullptr, *d_lidx = nullptr, *d_lu = nullptr;
    double *d_lval = nullptr, *d_term = nullptr, *d_part = nullptr, *d_loss = nullptr;
    int64_t n_cells = 0;
    double *d_X[2] = {nullptr, nullptr};                   // P, Q
    double *d_alpha[2] = {nullptr, nullptr}, *d_mu[2] = {nullptr, nullptr}; // the hyper-parameters of the two sides
    std::vector<double> alpha[2], mu[2];
    double *d_mom = nullptr;                               // per side: mean (k), Stats.mean (k), cov (k x k)
    double *d_Z = nullptr;                                 // the gaussians of a pass: k x the larger side's slots
    int32_t *d_null = nullptr, *d_first = nullptr, *d_rslot = nullptr, *d_rrank = nullptr; // per slot; one; the rerun's lists
    BpmfGaussWork gw;
    BpmfStream st;
    bool have_model = false, have_hyper = false, have_stream = false, iterated = false;
    float iter_ms[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
};

static thread_local std::string g_bpmf_err;

extern "C" const char *cmi_bpmf_last_error(cmi_bpmf_handle h) { return h ? h->err.c_str() : g_bpmf_err.c_str(); }

static void bpmf_free_ratings(cmi_bpmf_instance *h) {
    for (int s = 0; s < 2; ++s) abi_free(h->d_ptr[s], h->d_idx[s], h->d_slots[s], h->d_val[s]);
    abi_free(h->d_lptr, h->d_lidx, h->d_lu, h->d_lval, h->d_term, h->d_part, h->d_Z, h->d_null, h->d_rslot, h->d_rrank);
    h->have_ratings = h->iterated = false;
}

static void bpmf_free_all(cmi_bpmf_instance *h) {
    bpmf_free_ratings(h);
    for (int s = 0; s < 2; ++s) abi_free(h->d_X[s], h->d_alpha[s], h->d_mu[s]);
    abi_free(h->d_mom, h->d_loss, h->d_first);
    h->gw.release();
    h->have_model = h->have_hyper = false;
}

extern "C" int cmi_bpmf_destroy(cmi_bpmf_handle h) { return pair_destroy(h, bpmf_free_all); }

extern "C" int cmi_bpmf_create(int k, int n_users, int n_items, int device, unsigned flags, cmi_bpmf_handle *out) {
    if (out && k > BPMF_MAX_K) {
        *out = nullptr;
        return abi_fail(g_bpmf_err, CMI_E_UNSUPPORTED,
                        "cmi_bpmf_create: %d factors: a row's posterior keeps two k x k matrices of doubles in LDS (16 k^2 bytes), k <= %d", k,
                        BPMF_MAX_K);
    }
    int rc = pair_create(g_bpmf_err, "cmi_bpmf_create", k >= 1 && (flags & ~CMI_BPMF_FLAG_STRICT) == 0, n_users, n_items, device, out,
                         cmi_bpmf_destroy, [k, flags](cmi_bpmf_instance *h) { h->k = k, h->flags = flags; });
    if (rc != CMI_OK) return rc;
    cmi_bpmf_instance *h = *out;
    const size_t kk = (size_t)k * k;
    hipError_t e = hipMalloc((void **)&h->d_mom, 2 * (2 * (size_t)k + kk) * sizeof(double));
    for (int s = 0; s < 2 && e == hipSuccess; ++s) {
        e = hipMalloc((void **)&h->d_alpha[s], kk * sizeof(double));
        if (e == hipSuccess) e = hipMalloc((void **)&h->d_mu[s], (size_t)k * sizeof(double));
    }
    if (e == hipSuccess) e = hipMalloc((void **)&h->d_loss, sizeof(double));
    if (e == hipSuccess) e = hipMalloc((void **)&h->d_first, sizeof(int32_t));
    if (e != hipSuccess) {
        cmi_bpmf_destroy(h);
        *out = nullptr;
        return abi_fail(g_bpmf_err, CMI_E_HIP, "cmi_bpmf_create: %s", hipGetErrorString(e));
    }
    return CMI_OK;
}

static int bpmf_set_ratings_impl(cmi_bpmf_handle h, int64_t n, const int32_t *u, const int32_t *i, const double *r) {
    PairHostCsr all, all_cols;
    if (int rc = pair_ingest(h, "cmi_bpmf_set_ratings", n, u, i, r, /*scan_items=*/false, all, all_cols)) return rc;
    const PairHostCsr side[2] = {pair_drop_zeros(all), pair_drop_zeros(all_cols)};
    std::vector<int32_t> lu(all.idx.size());
    for (int a = 0; a < h->n_users; ++a) std::fill(lu.begin() + all.ptr[(size_t)a], lu.begin() + all.ptr[(size_t)a + 1], a);
    double sum = 0.0; // the mean of the non-zero cells, one chain in CRS order
    for (double v : side[0].val) sum += v;
    CMI_HIP(h, hipSetDevice(h->device));
    CMI_HIP(h, hipStreamSynchronize(h->stream));
    bpmf_free_ratings(h);
    size_t widest = 1;
    hipError_t e = hipSuccess;
    for (int s = 0; s < 2 && e == hipSuccess; ++s) {
        h->slot_rows[s].clear();
        for (size_t a = 0; a + 1 < side[s].ptr.size(); ++a)
            if (side[s].ptr[a + 1] > side[s].ptr[a]) h->slot_rows[s].push_back((int32_t)a);
        widest = std::max(widest, h->slot_rows[s].size());
        e = pair_upload(side[s], &h->d_ptr[s], &h->d_idx[s], &h->d_val[s], h->stream);
        if (e == hipSuccess) e = abi_upload(&h->d_slots[s], h->slot_rows[s], h->stream, true);
    }
    if (e == hipSuccess) e = pair_upload(all, &h->d_lptr, &h->d_lidx, &h->d_lval, h->stream);
    if (e == hipSuccess) e = abi_upload(&h->d_lu, lu, h->stream, true);
    if (e == hipSuccess) e = hipMalloc((void **)&h->d_term, std::max<size_t>(lu.size(), 1) * sizeof(double));
    if (e == hipSuccess) e = hipMalloc((void **)&h->d_part, std::max<size_t>((size_t)bpmf_loss_blocks((int64_t)lu.size()), 1) * sizeof(double));
    if (e == hipSuccess) e = hipMalloc((void **)&h->d_Z, widest * (size_t)h->k * sizeof(double));
    if (e == hipSuccess) e = hipMalloc((void **)&h->d_null, widest * sizeof(int32_t));
    if (e == hipSuccess) e = hipMalloc((void **)&h->d_rslot, widest * sizeof(int32_t));
    if (e == hipSuccess) e = hipMalloc((void **)&h->d_rrank, widest * sizeof(int32_t));
    if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
    if (e != hipSuccess) {
        bpmf_free_ratings(h);
        CMI_FAIL(h, CMI_E_HIP, "cmi_bpmf_set_ratings: %s", hipGetErrorString(e));
    }
    h->n_cells = (int64_t)lu.size();
    h->gm = sum / (double)side[0].val.size();
    h->have_ratings = true;
    return CMI_OK;
}

extern "C" int cmi_bpmf_set_ratings(cmi_bpmf_handle h, int64_t n, const int32_t *u, const int32_t *i, const double *r) {
    if (!h) return CMI_E_INVALID;
    return abi_barrier(h->err, "cmi_bpmf_set_ratings", [&] { return bpmf_set_ratings_impl(h, n, u, i, r); }, [h] { bpmf_free_ratings(h); });
}

extern "C" int cmi_bpmf_set_global_mean(cmi_bpmf_handle h, double global_mean) {
    if (!h) return CMI_E_INVALID;
    h->gm = global_mean;
    return CMI_OK;
}

extern "C" int cmi_bpmf_get_global_mean(cmi_bpmf_handle h, double *global_mean) {
    if (!h || !global_mean) return CMI_E_INVALID;
    *global_mean = h->gm;
    return CMI_OK;
}

static int bpmf_set_model_impl(cmi_bpmf_handle h, const double *P, const double *Q) {
    if (!h->have_model && (!P || !Q)) CMI_FAIL(h, CMI_E_INVALID, "cmi_bpmf_set_model: the first call sets both P and Q");
    CMI_HIP(h, hipSetDevice(h->device));
    const size_t pn = (size_t)h->n_users * h->k, qn = (size_t)h->n_items * h->k;
    if (!h->d_X[0]) {
        hipError_t e = hipMalloc((void **)&h->d_X[0], pn * sizeof(double));
        if (e == hipSuccess) e = hipMalloc((void **)&h->d_X[1], qn * sizeof(double));
        if (e != hipSuccess) {
            abi_free(h->d_X[0], h->d_X[1]);
            CMI_FAIL(h, CMI_E_HIP, "cmi_bpmf_set_model: %s", hipGetErrorString(e));
        }
    }
    if (P) CMI_HIP(h, hipMemcpyAsync(h->d_X[0], P, pn * sizeof(double), hipMemcpyHostToDevice, h->stream));
    if (Q) CMI_HIP(h, hipMemcpyAsync(h->d_X[1], Q, qn * sizeof(double), hipMemcpyHostToDevice, h->stream));
    CMI_HIP(h, hipStreamSynchronize(h->stream));
    h->have_model = true;
    return CMI_OK;
}

extern "C" int cmi_bpmf_set_model(cmi_bpmf_handle h, const double *P, const double *Q) {
    if (!h) return CMI_E_INVALID;
    return abi_barrier(h->err, "cmi_bpmf_set_model", [&] { return bpmf_set_model_impl(h, P, Q); });
}

extern "C" int cmi_bpmf_get_model(cmi_bpmf_handle h, double *P, double *Q) {
    if (!h) return CMI_E_INVALID;
    return abi_barrier(h->err, "cmi_bpmf_get_model", [&] {
        if (!h->have_model) CMI_FAIL(h, CMI_E_INVALID, "cmi_bpmf_get_model: no model (cmi_bpmf_set_model first)");
        CMI_HIP(h, hipSetDevice(h->device));
        if (P) CMI_HIP(h, hipMemcpyAsync(P, h->d_X[0], (size_t)h->n_users * h->k * sizeof(double), hipMemcpyDeviceToHost, h->stream));
        if (Q) CMI_HIP(h, hipMemcpyAsync(Q, h->d_X[1], (size_t)h->n_items * h->k * sizeof(double), hipMemcpyDeviceToHost, h->stream));
        CMI_HIP(h, hipStreamSynchronize(h->stream));
        return CMI_OK;
    });
}

extern "C" int cmi_bpmf_set_stream(cmi_bpmf_handle h, int64_t state, int have_cached, double cached) {
    if (!h) return CMI_E_INVALID;
    if (state < 0 || (uint64_t)state > JAVA_LCG_MASK) CMI_FAIL(h, CMI_E_INVALID, "cmi_bpmf_set_stream: the state has 48 bits");
    h->st.state = (uint64_t)state, h->st.have = have_cached ? 1 : 0, h->st.cached = cached;
    h->have_stream = true;
    return CMI_OK;
}

extern "C" int cmi_bpmf_get_stream(cmi_bpmf_handle h, int64_t *state, int *have_cached, double *cached) {
    if (!h || !state || !have_cached || !cached) return CMI_E_INVALID;
    *state = (int64_t)h->st.state, *have_cached = h->st.have, *cached = h->st.cached;
    return CMI_OK;
}

// ---- the gaussian stream ----------------------------------------------------------------------------------------------------------------
// the next n values of st into d_out on stream s; st is left as after them.  Rounds of attempts until the pairs needed are there: a
// round that accepts too few is followed by one that starts where it ended
static hipError_t bpmf_generate(BpmfStream &st, int64_t n, double *d_out, BpmfGaussWork &w, hipStream_t s) {
    if (n <= 0) return hipSuccess;
    static const JavaLcgJump jump = java_lcg_jump_table();
    const int lead = st.have ? 1 : 0;
    const int64_t need = (n - lead + 1) / 2;
    if (need == 0) { // n == 1 and the cached value serves it
        const double v = st.cached;
        hipError_t e = hipMemcpyAsync(d_out, &v, sizeof v, hipMemcpyHostToDevice, s);
        if (e == hipSuccess) e = hipStreamSynchronize(s);
        st.have = 0;
        return e;
    }
    const uint64_t state0 = st.state;
    int64_t t0 = 0, pair0 = 0;
    for (;;) {
        const int64_t att = std::min<int64_t>(bpmf_gauss_attempts(need - pair0), (int64_t)1 << 30);
        hipError_t e = w.reserve((att + BPMF_GAUSS_BLOCK - 1) / BPMF_GAUSS_BLOCK);
        if (e == hipSuccess) e = bpmf_launch_gauss_round(state0, jump, t0, att, pair0, need, lead, st.cached, n, d_out, w.d_cnt, w.d_off, w.d_tail, s);
        BpmfGaussTail tail{};
        if (e == hipSuccess) e = hipMemcpyAsync(&tail, w.d_tail, sizeof tail, hipMemcpyDeviceToHost, s);
        if (e == hipSuccess) e = hipStreamSynchronize(s);
        if (e != hipSuccess) return e;
        if (tail.last_t >= 0) {
            st.state = java_lcg_jump(jump, state0, (uint64_t)(tail.last_t + 1) * 4u);
            st.have = tail.have, st.cached = tail.have ? tail.cached : 0.0;
            return hipSuccess;
        }
        pair0 += tail.accepted, t0 += att;
    }
}

extern "C" int cmi_java_next_gaussians(int64_t *state, int *have_cached, double *cached, int64_t n, double *out) {
    return abi_barrier(g_bpmf_err, "cmi_java_next_gaussians", [&] {
        const char *fn = "cmi_java_next_gaussians";
        if (!state || !have_cached || !cached || *state < 0 || (uint64_t)*state > JAVA_LCG_MASK || n < 0 || n > ((int64_t)1 << 28) ||
            (n > 0 && !out))
            return abi_fail(g_bpmf_err, CMI_E_INVALID, "%s: invalid argument", fn);
        if (int rc = abi_check_device(g_bpmf_err, fn, 0)) return rc;
        if (n == 0) return (int)CMI_OK;
        BpmfStream st;
        st.state = (uint64_t)*state, st.have = *have_cached ? 1 : 0, st.cached = *cached;
        BpmfGaussWork w;
        double *d_out = nullptr;
        hipError_t e = hipSetDevice(0);
        if (e == hipSuccess) e = hipMalloc((void **)&d_out, (size_t)n * sizeof(double));
        if (e == hipSuccess) e = bpmf_generate(st, n, d_out, w, nullptr);
        if (e == hipSuccess) e = hipMemcpy(out, d_out, (size_t)n * sizeof(double), hipMemcpyDeviceToHost);
        abi_free(d_out);
        w.release();
        if (e != hipSuccess) return abi_fail(g_bpmf_err, CMI_E_HIP, "%s: %s", fn, hipGetErrorString(e));
        *state = (int64_t)st.state, *have_cached = st.have, *cached = st.cached;
        return (int)CMI_OK;
    });
}

extern "C" int64_t cmi_bpmf_gauss_attempts(int64_t n_pairs) { return bpmf_gauss_attempts(n_pairs); }

// ---- the moments and the hyper step ---------------------------------------------------------------------------------------------------
extern "C" int cmi_bpmf_moments(const double *X, int rows, int k, double *mean, double *cov, int on_device) {
    return abi_barrier(g_bpmf_err, "cmi_bpmf_moments", [&] {
        const char *fn = "cmi_bpmf_moments";
        if (!X || !mean || !cov || rows < 1 || k < 1) return abi_fail(g_bpmf_err, CMI_E_INVALID, "%s: invalid argument", fn);
        if (k > BPMF_MAX_K) return abi_fail(g_bpmf_err, CMI_E_UNSUPPORTED, "%s: k = %d: k <= %d", fn, k, BPMF_MAX_K);
        if (!on_device) {
            bpmf_moments_host(X, rows, k, mean, cov);
            return (int)CMI_OK;
        }
        if (int rc = abi_check_device(g_bpmf_err, fn, 0)) return rc;
        const size_t xn = (size_t)rows * k, kk = (size_t)k * k;
        double *d_x = nullptr, *d_m = nullptr;
        hipError_t e = hipSetDevice(0);
        if (e == hipSuccess) e = hipMalloc((void **)&d_x, xn * sizeof(double));
        if (e == hipSuccess) e = hipMalloc((void **)&d_m, (2 * (size_t)k + kk) * sizeof(double));
        if (e == hipSuccess) e = hipMemcpy(d_x, X, xn * sizeof(double), hipMemcpyHostToDevice);
        if (e == hipSuccess) e = bpmf_launch_moments(d_x, rows, k, d_m, d_m + k, d_m + 2 * k, nullptr);
        if (e == hipSuccess) e = hipMemcpy(mean, d_m, (size_t)k * sizeof(double), hipMemcpyDeviceToHost);
        if (e == hipSuccess) e = hipMemcpy(cov, d_m + 2 * k, kk * sizeof(double), hipMemcpyDeviceToHost);
        abi_free(d_x, d_m);
        return abi_hip(g_bpmf_err, fn, e);
    });
}

extern "C" int cmi_bpmf_hyper_host(int k, int rows, const double *mean, const double *cov, double *alpha, double *mu, int64_t *state,
                                   int *have_cached, double *cached) {
    return abi_barrier(g_bpmf_err, "cmi_bpmf_hyper_host", [&] {
        const char *fn = "cmi_bpmf_hyper_host";
        if (k < 1 || rows < 1 || !mean || !cov || !alpha || !mu || !state || !have_cached || !cached || *state < 0 ||
            (uint64_t)*state > JAVA_LCG_MASK)
            return abi_fail(g_bpmf_err, CMI_E_INVALID, "%s: invalid argument", fn);
        if (k > BPMF_MAX_K) return abi_fail(g_bpmf_err, CMI_E_UNSUPPORTED, "%s: k = %d: k <= %d", fn, k, BPMF_MAX_K);
        BpmfStream st;
        st.state = (uint64_t)*state, st.have = *have_cached ? 1 : 0, st.cached = *cached;
        const size_t kk = (size_t)k * k;
        BpmfMat a(alpha, alpha + kk);
        std::vector<double> m(mu, mu + k);
        bpmf_hyper_side(st, k, rows, std::vector<double>(mean, mean + k), BpmfMat(cov, cov + kk), a, m);
        std::copy(a.begin(), a.end(), alpha);
        std::copy(m.begin(), m.end(), mu);
        *state = (int64_t)st.state, *have_cached = st.have, *cached = st.cached;
        return (int)CMI_OK;
    });
}

// the moments of both sides: mean and cov of side s at mom[s]
struct BpmfMoments {
    std::vector<double> mean[2], cov[2];
};
static int bpmf_moments_of_model(cmi_bpmf_instance *h, BpmfMoments &m) {
    const size_t k = (size_t)h->k, kk = k * k, per = 2 * k + kk;
    for (int s = 0; s < 2; ++s) {
        double *d = h->d_mom + s * per;
        CMI_HIP(h, bpmf_launch_moments(h->d_X[s], s == 0 ? h->n_users : h->n_items, h->k, d, d + k, d + 2 * k, h->stream));
    }
    CMI_HIP(h, hipEventRecord(h->ev1, h->stream));
    for (int s = 0; s < 2; ++s) {
        const double *d = h->d_mom + s * per;
        m.mean[s].resize(k), m.cov[s].resize(kk);
        CMI_HIP(h, hipMemcpyAsync(m.mean[s].data(), d, k * sizeof(double), hipMemcpyDeviceToHost, h->stream));
        CMI_HIP(h, hipMemcpyAsync(m.cov[s].data(), d + 2 * k, kk * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    }
    CMI_HIP(h, hipStreamSynchronize(h->stream));
    return CMI_OK;
}

static int bpmf_upload_hyper(cmi_bpmf_instance *h) {
    for (int s = 0; s < 2; ++s) {
        CMI_HIP(h, hipMemcpyAsync(h->d_alpha[s], h->alpha[s].data(), h->alpha[s].size() * sizeof(double), hipMemcpyHostToDevice, h->stream));
        CMI_HIP(h, hipMemcpyAsync(h->d_mu[s], h->mu[s].data(), h->mu[s].size() * sizeof(double), hipMemcpyHostToDevice, h->stream));
    }
    CMI_HIP(h, hipStreamSynchronize(h->stream));
    return CMI_OK;
}

extern "C" int cmi_bpmf_init_hyper(cmi_bpmf_handle h) {
    if (!h) return CMI_E_INVALID;
    return abi_barrier(h->err, "cmi_bpmf_init_hyper", [&] {
        if (!h->have_model) CMI_FAIL(h, CMI_E_INVALID, "cmi_bpmf_init_hyper: no model (cmi_bpmf_set_model first)");
        CMI_HIP(h, hipSetDevice(h->device));
        BpmfMoments m;
        if (int rc = bpmf_moments_of_model(h, m)) return rc;
        for (int s = 0; s < 2; ++s) h->mu[s] = m.mean[s], h->alpha[s] = bpmf_inv(m.cov[s], h->k);
        if (int rc = bpmf_upload_hyper(h)) return rc;
        h->have_hyper = true;
        return CMI_OK;
    });
}

extern "C" int cmi_bpmf_get_hyper(cmi_bpmf_handle h, double *alpha_u, double *mu_u, double *alpha_m, double *mu_m) {
    if (!h) return CMI_E_INVALID;
    if (!h->have_hyper) CMI_FAIL(h, CMI_E_INVALID, "cmi_bpmf_get_hyper: no hyper-parameters (cmi_bpmf_init_hyper first)");
    double *a[2] = {alpha_u, alpha_m}, *m[2] = {mu_u, mu_m};
    for (int s = 0; s < 2; ++s) {
        if (a[s]) std::copy(h->alpha[s].begin(), h->alpha[s].end(), a[s]);
        if (m[s]) std::copy(h->mu[s].begin(), h->mu[s].end(), m[s]);
    }
    return CMI_OK;
}

extern "C" int cmi_bpmf_set_hyper(cmi_bpmf_handle h, const double *alpha_u, const double *mu_u, const double *alpha_m, const double *mu_m) {
    if (!h) return CMI_E_INVALID;
    return abi_barrier(h->err, "cmi_bpmf_set_hyper", [&] {
        if (!alpha_u || !mu_u || !alpha_m || !mu_m) CMI_FAIL(h, CMI_E_INVALID, "cmi_bpmf_set_hyper: null argument");
        CMI_HIP(h, hipSetDevice(h->device));
        const size_t k = (size_t)h->k;
        h->alpha[0].assign(alpha_u, alpha_u + k * k), h->mu[0].assign(mu_u, mu_u + k);
        h->alpha[1].assign(alpha_m, alpha_m + k * k), h->mu[1].assign(mu_m, mu_m + k);
        if (int rc = bpmf_upload_hyper(h)) return rc;
        h->have_hyper = true;
        return CMI_OK;
    });
}

// ---- a Gibbs pass ----------------------------------------------------------------------------------------------------------------------
// One pass of one side with the hyper-parameters at d_alpha / d_mu.  The first launch gives slot s the draws at k * s; if a slot came
// back null, the slots after the first null one run again at their exact ranks, and the stream is advanced by the draws really taken.
// slot_null (may be null): the slots' flags.
static int bpmf_pass(cmi_bpmf_instance *h, int side, const double *d_alpha, const double *d_mu, std::vector<int32_t> *slot_null,
                     int64_t *draws) {
    const int R = (int)h->slot_rows[side].size();
    if (draws) *draws = 0;
    if (slot_null) slot_null->assign((size_t)R, 0);
    if (R == 0) return CMI_OK;
    const BpmfStream st0 = h->st;
    BpmfStream st = st0;
    CMI_HIP(h, bpmf_generate(st, (int64_t)R * h->k, h->d_Z, h->gw, h->stream));
    BpmfRowArgs a;
    a.k = h->k, a.n = R;
    a.C = PairCsr{h->d_ptr[side], h->d_idx[side], h->d_val[side]};
    a.rows = h->d_slots[side], a.other = h->d_X[1 - side], a.own = h->d_X[side];
    a.alpha = d_alpha, a.mu = d_mu, a.gm = h->gm, a.Z = h->d_Z, a.null_flag = h->d_null, a.first_null = h->d_first;
    int32_t first = INT_MAX;
    CMI_HIP(h, hipMemcpyAsync(h->d_first, &first, sizeof first, hipMemcpyHostToDevice, h->stream));
    CMI_HIP(h, bpmf_launch_rows(a, h->stream));
    CMI_HIP(h, hipMemcpyAsync(&first, h->d_first, sizeof first, hipMemcpyDeviceToHost, h->stream));
    CMI_HIP(h, hipStreamSynchronize(h->stream));
    int64_t taken = R;
    if (first < R) {
        std::vector<int32_t> null((size_t)R);
        CMI_HIP(h, hipMemcpyAsync(null.data(), h->d_null, (size_t)R * sizeof(int32_t), hipMemcpyDeviceToHost, h->stream));
        CMI_HIP(h, hipStreamSynchronize(h->stream));
        const BpmfRerun plan = bpmf_rerun_plan(null);
        taken = plan.taken;
        if (!plan.slot.empty()) {
            CMI_HIP(h, hipMemcpyAsync(h->d_rslot, plan.slot.data(), plan.slot.size() * sizeof(int32_t), hipMemcpyHostToDevice, h->stream));
            CMI_HIP(h, hipMemcpyAsync(h->d_rrank, plan.rank.data(), plan.rank.size() * sizeof(int32_t), hipMemcpyHostToDevice, h->stream));
            a.n = (int)plan.slot.size(), a.slots = h->d_rslot, a.rank = h->d_rrank;
            CMI_HIP(h, bpmf_launch_rows(a, h->stream));
            CMI_HIP(h, hipStreamSynchronize(h->stream));
        }
        st = st0; // the state after the draws really taken: the same values again, fewer of them
        CMI_HIP(h, bpmf_generate(st, taken * h->k, h->d_Z, h->gw, h->stream));
        if (slot_null) *slot_null = null;
    }
    h->st = st;
    if (draws) *draws = taken * h->k;
    return CMI_OK;
}

static int bpmf_ready(cmi_bpmf_instance *h, const char *fn, bool hyper) {
    if (!h->have_ratings) CMI_FAIL(h, CMI_E_INVALID, "%s: no ratings (cmi_bpmf_set_ratings first)", fn);
    if (!h->have_model) CMI_FAIL(h, CMI_E_INVALID, "%s: no model (cmi_bpmf_set_model first)", fn);
    if (hyper && !h->have_hyper) CMI_FAIL(h, CMI_E_INVALID, "%s: no hyper-parameters (cmi_bpmf_init_hyper first)", fn);
    if (!h->have_stream) CMI_FAIL(h, CMI_E_INVALID, "%s: no stream (cmi_bpmf_set_stream first)", fn);
    CMI_HIP(h, hipSetDevice(h->device));
    return CMI_OK;
}

extern "C" int cmi_bpmf_sample_side(cmi_bpmf_handle h, int side, const double *alpha, const double *mu, int32_t *null_flags, int64_t *draws) {
    if (!h) return CMI_E_INVALID;
    return abi_barrier(h->err, "cmi_bpmf_sample_side", [&] {
        const char *fn = "cmi_bpmf_sample_side";
        if ((side != 0 && side != 1) || !alpha || !mu) CMI_FAIL(h, CMI_E_INVALID, "%s: invalid argument", fn);
        if (int rc = bpmf_ready(h, fn, false)) return rc;
        const size_t k = (size_t)h->k;
        double *d_a = nullptr, *d_m = nullptr;
        hipError_t e = hipMalloc((void **)&d_a, k * k * sizeof(double));
        if (e == hipSuccess) e = hipMalloc((void **)&d_m, k * sizeof(double));
        if (e == hipSuccess) e = hipMemcpyAsync(d_a, alpha, k * k * sizeof(double), hipMemcpyHostToDevice, h->stream);
        if (e == hipSuccess) e = hipMemcpyAsync(d_m, mu, k * sizeof(double), hipMemcpyHostToDevice, h->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
        int rc = abi_hip(h->err, fn, e);
        std::vector<int32_t> slot_null;
        if (rc == CMI_OK) rc = bpmf_pass(h, side, d_a, d_m, &slot_null, draws);
        (void)hipStreamSynchronize(h->stream);
        abi_free(d_a, d_m);
        if (rc == CMI_OK && null_flags) {
            std::fill(null_flags, null_flags + (side == 0 ? h->n_users : h->n_items), 0);
            for (size_t s = 0; s < slot_null.size(); ++s) null_flags[h->slot_rows[side][s]] = slot_null[s];
        }
        return rc;
    });
}

static int bpmf_iterate_impl(cmi_bpmf_handle h, double *loss) {
    if (int rc = bpmf_ready(h, "cmi_bpmf_iterate", true)) return rc;
    float ms[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
    // the moments of both sides first: the item step reads Q, which the user step does not write
    CMI_HIP(h, hipEventRecord(h->ev0, h->stream));
    BpmfMoments m;
    if (int rc = bpmf_moments_of_model(h, m)) return rc; // records ev1 behind the kernels
    CMI_HIP(h, hipEventElapsedTime(&ms[0], h->ev0, h->ev1));
    const auto w0 = std::chrono::steady_clock::now();
    bpmf_hyper_side(h->st, h->k, h->n_users, m.mean[0], m.cov[0], h->alpha[0], h->mu[0]);
    bpmf_hyper_side(h->st, h->k, h->n_items, m.mean[1], m.cov[1], h->alpha[1], h->mu[1]);
    ms[1] = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - w0).count();
    if (int rc = bpmf_upload_hyper(h)) return rc;
    for (int gibbs = 0; gibbs < 2; ++gibbs)
        for (int side = 0; side < 2; ++side) {
            float t = 0.f;
            CMI_HIP(h, hipEventRecord(h->ev0, h->stream));
            if (int rc = bpmf_pass(h, side, h->d_alpha[side], h->d_mu[side], nullptr, nullptr)) return rc;
            CMI_HIP(h, hipEventRecord(h->ev1, h->stream));
            CMI_HIP(h, hipEventSynchronize(h->ev1));
            CMI_HIP(h, hipEventElapsedTime(&t, h->ev0, h->ev1));
            ms[2 + side] += t;
        }
    CMI_HIP(h, hipEventRecord(h->ev0, h->stream));
    CMI_HIP(h, bpmf_launch_loss(h->d_X[0], h->d_X[1], PairCsr{h->d_lptr, h->d_lidx, h->d_lval}, h->d_lu, h->n_cells, h->k, h->gm,
                                (h->flags & CMI_BPMF_FLAG_STRICT) != 0, h->d_term, h->d_part, h->d_loss, h->stream));
    CMI_HIP(h, hipEventRecord(h->ev1, h->stream));
    double l = 0.0;
    CMI_HIP(h, hipMemcpyAsync(&l, h->d_loss, sizeof l, hipMemcpyDeviceToHost, h->stream));
    CMI_HIP(h, hipStreamSynchronize(h->stream));
    CMI_HIP(h, hipEventElapsedTime(&ms[4], h->ev0, h->ev1));
    std::copy(ms, ms + 5, h->iter_ms);
    h->iterated = true;
    if (loss) *loss = l;
    if (std::isnan(l) || std::isinf(l)) CMI_FAIL(h, CMI_E_NUMERIC, "cmi_bpmf_iterate: loss is NaN or Infinity");
    return CMI_OK;
}

extern "C" int cmi_bpmf_iterate(cmi_bpmf_handle h, double *loss) {
    if (!h) return CMI_E_INVALID;
    return abi_barrier(h->err, "cmi_bpmf_iterate", [&] { return bpmf_iterate_impl(h, loss); });
}

extern "C" int cmi_bpmf_last_iter_ms(cmi_bpmf_handle h, float *ms) {
    if (!h || !ms) return CMI_E_INVALID;
    if (!h->iterated) CMI_FAIL(h, CMI_E_INVALID, "cmi_bpmf_last_iter_ms: no iteration yet");
    std::copy(h->iter_ms, h->iter_ms + 5, ms);
    return CMI_OK;
}

static int bpmf_predict_impl(cmi_bpmf_handle h, int64_t n, const int32_t *u, const int32_t *j, int bound, double lo, double hi, double *out) {
    if (!h->have_model) CMI_FAIL(h, CMI_E_INVALID, "cmi_bpmf_predict_batch: no model (cmi_bpmf_set_model first)");
    if (int rc = pair_check_tuples(h, "cmi_bpmf_predict_batch", n, u, j, out)) return rc;
    if (n == 0) return CMI_OK;
    return abi_predict(h, "cmi_bpmf_predict_batch", n, u, j, nullptr, nullptr, 0, out, [&](const AbiTuples &t, double *d_out) {
        return abi_hip(h->err, "cmi_bpmf_predict_batch",
                       bpmf_launch_predict(h->d_X[0], h->d_X[1], h->k, h->gm, n, t.a, t.b, bound, lo, hi, d_out, h->stream));
    });
}

extern "C" int cmi_bpmf_predict_batch(cmi_bpmf_handle h, int64_t n, const int32_t *u, const int32_t *j, int bound, double lo, double hi,
                                      double *out) {
    if (!h) return CMI_E_INVALID;
    return abi_barrier(h->err, "cmi_bpmf_predict_batch", [&] { return bpmf_predict_impl(h, n, u, j, bound, lo, hi, out); });
}
