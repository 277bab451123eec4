// pair_host.hpp -- the host side that the pair-co-occurrence handles share (cmi_knn_*: knn_api.cpp, cmi_slope_*: slopeone_api.cpp,
// cmi_nmf_*: nmf_api.cpp, cmi_slim_*: slim_api.cpp, cmi_rankals_*: rankals_api.cpp): the handle's common state, the ingest of the 2-D
// train matrix, librec's contains() flags and its zero-cell filter, the dense-matrix reservation and the timed build (the prediction
// batch is abi_predict).
// Every function that can fail takes the C function's name, `fn`, which opens its messages.  Internal.
#pragma once
#include <algorithm>
#include <numeric>
#include <string>
#include <vector>

#include "abi.hpp"

struct PairModelBase {
    int n_users = 0, n_items = 0, device = 0;
    std::string err;
    hipStream_t stream = nullptr;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    bool have_ratings = false, built = false;
    float build_ms = 0.f;
};

// create: valid says whether the model's own arguments are; init(h) sets the model's fields of the new handle.  err is the thread's
// message, which *_last_error(NULL) reads.
template <typename Inst, typename Init>
int pair_create(std::string &err, const char *fn, bool valid, int n_users, int n_items, int device, Inst **out, int (*destroy)(Inst *),
                Init &&init) {
    return abi_barrier(err, fn, [&] {
        if (out) *out = nullptr;
        if (!out || !valid || n_users <= 0 || n_items <= 0) return abi_fail(err, CMI_E_INVALID, "%s: invalid argument", fn);
        if (int rc = abi_check_device(err, fn, device)) return rc;
        Inst *h = new Inst();
        h->n_users = n_users, h->n_items = n_items, h->device = device;
        init(h);
        hipError_t e = hipSetDevice(device);
        if (e == hipSuccess) e = hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking);
        if (e == hipSuccess) e = hipEventCreate(&h->ev0);
        if (e == hipSuccess) e = hipEventCreate(&h->ev1);
        if (e != hipSuccess) {
            destroy(h);
            return abi_fail(err, CMI_E_HIP, "%s: %s", fn, hipGetErrorString(e));
        }
        *out = h;
        return CMI_OK;
    });
}

// destroy: the stream drained, the model's device buffers freed, then the events, the stream and the handle
template <typename Inst>
int pair_destroy(Inst *h, void (*free_buffers)(Inst *)) {
    if (!h) return CMI_OK;
    (void)hipSetDevice(h->device);
    if (h->stream) (void)hipStreamSynchronize(h->stream);
    free_buffers(h);
    if (h->ev0) (void)hipEventDestroy(h->ev0);
    if (h->ev1) (void)hipEventDestroy(h->ev1);
    if (h->stream) (void)hipStreamDestroy(h->stream);
    delete h;
    return CMI_OK;
}

struct PairHostCsr {
    std::vector<int32_t> ptr, idx;
    std::vector<double> val;
};

// CSR of (row, col, value) cells, rows ascending, columns ascending inside a row
inline PairHostCsr pair_csr(int64_t n, int n_rows, const int32_t *row, const int32_t *col, const double *r) {
    PairHostCsr m;
    m.ptr.assign((size_t)n_rows + 1, 0);
    for (int64_t t = 0; t < n; ++t) ++m.ptr[(size_t)row[t] + 1];
    for (int i = 0; i < n_rows; ++i) m.ptr[(size_t)i + 1] += m.ptr[(size_t)i];
    std::vector<int64_t> ord((size_t)n);
    std::iota(ord.begin(), ord.end(), 0);
    std::sort(ord.begin(), ord.end(), [&](int64_t a, int64_t b) { return row[a] != row[b] ? row[a] < row[b] : col[a] < col[b]; });
    m.idx.resize((size_t)n);
    m.val.resize((size_t)n);
    for (size_t k = 0; k < ord.size(); ++k) m.idx[k] = col[ord[k]], m.val[k] = r[ord[k]];
    return m;
}

// every id of n cells or tuples (`unit` names them in the message) inside the handle's sizes
inline int pair_check_range(PairModelBase *h, const char *fn, const char *unit, int64_t n, const int32_t *u, const int32_t *i) {
    for (int64_t t = 0; t < n; ++t)
        if (u[t] < 0 || u[t] >= h->n_users || i[t] < 0 || i[t] >= h->n_items)
            CMI_FAIL(h, CMI_E_INVALID, "%s: id out of range at %s %lld", fn, unit, (long long)t);
    return CMI_OK;
}
// the arguments of set_ratings
inline int pair_check_cells(PairModelBase *h, const char *fn, int64_t n, const int32_t *u, const int32_t *i, const double *r) {
    if (n < 0 || (n > 0 && (!u || !i || !r))) CMI_FAIL(h, CMI_E_INVALID, "%s: null arrays", fn);
    if (n >= ((int64_t)1 << 31)) CMI_FAIL(h, CMI_E_UNSUPPORTED, "%s: more than 2^31-1 cells", fn);
    return pair_check_range(h, fn, "cell", n, u, i);
}
// the arguments of predict_batch
inline int pair_check_tuples(PairModelBase *h, const char *fn, int64_t n, const int32_t *u, const int32_t *j, const double *out) {
    if (n < 0 || (n > 0 && (!u || !j || !out))) CMI_FAIL(h, CMI_E_INVALID, "%s: null arrays", fn);
    return pair_check_range(h, fn, "tuple", n, u, j);
}

// set_ratings: the checked cells as both CSRs, by_user (user -> items) and by_item (item -> users).  A duplicate cell is looked for in
// by_item if scan_items, else in by_user, and reported as (user, item) either way.
inline int pair_ingest(PairModelBase *h, const char *fn, int64_t n, const int32_t *u, const int32_t *i, const double *r, bool scan_items,
                       PairHostCsr &by_user, PairHostCsr &by_item) {
    if (int rc = pair_check_cells(h, fn, n, u, i, r)) return rc;
    by_user = pair_csr(n, h->n_users, u, i, r);
    by_item = pair_csr(n, h->n_items, i, u, r);
    const PairHostCsr &m = scan_items ? by_item : by_user;
    for (int e = 0; e + 1 < (int)m.ptr.size(); ++e)
        for (int32_t k = m.ptr[(size_t)e] + 1; k < m.ptr[(size_t)e + 1]; ++k)
            if (m.idx[(size_t)k] == m.idx[(size_t)k - 1])
                CMI_FAIL(h, CMI_E_INVALID, "%s: duplicate cell (user %d, item %d)", fn, scan_items ? m.idx[(size_t)k] : e,
                         scan_items ? e : m.idx[(size_t)k]);
    return CMI_OK;
}

// librec SparseVector.contains: Arrays.binarySearch over the whole index array of a vector built by set() -- capacity the next power
// of two >= count, the tail zero.  Per entry of every row: does the row's own contains() find it?
inline std::vector<uint8_t> pair_contains_flags(const PairHostCsr &m) {
    std::vector<uint8_t> ok(m.idx.size(), 0);
    for (size_t e = 0; e + 1 < m.ptr.size(); ++e) {
        const int32_t b0 = m.ptr[e], cnt = m.ptr[e + 1] - b0;
        int32_t cap = 1;
        while (cap < cnt) cap <<= 1;
        for (int32_t k = 0; k < cnt; ++k) {
            const int32_t key = m.idx[(size_t)(b0 + k)];
            int32_t low = 0, high = cap - 1;
            while (low <= high) {
                const int32_t mid = (int32_t)((uint32_t)(low + high) >> 1);
                const int32_t v = mid < cnt ? m.idx[(size_t)(b0 + mid)] : 0;
                if (v < key) low = mid + 1;
                else if (v > key) high = mid - 1;
                else {
                    ok[(size_t)(b0 + k)] = 1;
                    break;
                }
            }
        }
    }
    return ok;
}

// the CSR without its zero-valued cells (librec's SparseMatrix.row() / column() leave them out)
inline PairHostCsr pair_drop_zeros(const PairHostCsr &m) {
    PairHostCsr o;
    o.ptr.assign(m.ptr.size(), 0);
    for (size_t row = 0; row + 1 < m.ptr.size(); ++row) {
        for (int32_t q = m.ptr[row]; q < m.ptr[row + 1]; ++q)
            if (m.val[(size_t)q] != 0.0) o.idx.push_back(m.idx[(size_t)q]), o.val.push_back(m.val[(size_t)q]);
        o.ptr[row + 1] = (int32_t)o.idx.size();
    }
    return o;
}

inline hipError_t pair_upload(const PairHostCsr &m, int32_t **ptr, int32_t **idx, double **val, hipStream_t s) {
    hipError_t e = abi_upload(ptr, m.ptr, s, true);
    if (e == hipSuccess) e = abi_upload(idx, m.idx, s, true);
    if (e == hipSuccess) e = abi_upload(val, m.val, s, true);
    return e;
}

// build: the dense n x n matrices (`what`: "similarity matrix"; plural: more than one), refused up front when they cannot fit, so a
// build never fails half-way.  alloc() allocates them and leaves none behind when it fails.
template <typename Alloc>
int pair_reserve_dense(PairModelBase *h, const char *fn, int n, size_t bytes, const char *what, bool plural, Alloc &&alloc) {
    const char *need = plural ? "need" : "needs";
    size_t free_b = 0, total_b = 0;
    CMI_HIP(h, hipMemGetInfo(&free_b, &total_b));
    if (bytes > free_b)
        CMI_FAIL(h, CMI_E_INVALID, "%s: the %d x %d %s %s %zu bytes of device memory, %zu are free", fn, n, n, what, need, bytes, free_b);
    const hipError_t e = alloc();
    if (e != hipSuccess)
        CMI_FAIL(h, CMI_E_INVALID, "%s: the %s %s %zu bytes of device memory: %s", fn, what, need, bytes, hipGetErrorString(e));
    return CMI_OK;
}

// build: body() enqueues the fill and the kernels on h->stream; the time between the two events becomes build_ms
template <typename Body>
int pair_timed_build(PairModelBase *h, Body &&body) {
    CMI_HIP(h, hipStreamSynchronize(h->stream));
    h->built = false;
    CMI_HIP(h, hipEventRecord(h->ev0, h->stream));
    if (int rc = body()) return rc;
    CMI_HIP(h, hipEventRecord(h->ev1, h->stream));
    CMI_HIP(h, hipStreamSynchronize(h->stream));
    CMI_HIP(h, hipEventElapsedTime(&h->build_ms, h->ev0, h->ev1));
    h->built = true;
    return CMI_OK;
}

inline int pair_last_build_ms(PairModelBase *h, const char *fn, float *ms) {
    if (!h || !ms) return CMI_E_INVALID;
    if (!h->built) CMI_FAIL(h, CMI_E_INVALID, "%s: nothing built yet", fn);
    *ms = h->build_ms;
    return CMI_OK;
}
