// slim_kernels.hip -- SLIM on gfx950: the coordinate-descent sweep (SLIM.buildModel), its loss and the score (SLIM.predict).
// Everything is fp64 with the reference's operation order: every sum is one left-to-right chain from 0.0 with a rounding per multiply and
// per add (no FMA: -ffp-contract=off), and division is the correctly rounded IEEE operation Java uses.  Column j of W is read and
// written by column j's coordinates alone, so columns never meet: no cross-column sums, no atomic adds, the same bits on every run.
#include "slim_kernels.hpp"

#include <algorithm>
#include <cstdlib>

namespace cmi {

// lane `l`'s value of a wave-uniform lane index, through the scalar unit (v_readlane)
__device__ __forceinline__ double slim_lane_d(double v, int l) {
    const int lo = __builtin_amdgcn_readlane(__double2loint(v), l), hi = __builtin_amdgcn_readlane(__double2hiint(v), l);
    return __hiloint2double(hi, lo);
}

// the place of `key` in the ascending idx[lo, hi), or -1
__device__ __forceinline__ int slim_find(const int32_t *idx, int lo, int hi, int key) {
    const int end = hi;
    while (lo < hi) {
        const int m = (lo + hi) >> 1;
        if (idx[m] < key) lo = m + 1;
        else hi = m;
    }
    return lo < end && idx[lo] == key ? lo : -1;
}

// SLIM.predict(u, j, true, j): the ordered sum over nns(j) of Ru.get(k) * W[k][j] where Ru.contains(k), k == j left out.  The user's row
// is (idx, val, ok)[r0, r1).
__device__ __forceinline__ double slim_score_one(const int32_t *idx, const double *val, const uint8_t *ok, int r0, int r1, const SlimLists &L,
                                                 int j) {
    double pred = 0.0;
    for (int64_t p = L.ptr[j], p1 = L.ptr[j + 1]; p < p1; ++p) {
        const int k = L.idx[p];
        if (k == j) continue;
        const int q = slim_find(idx, r0, r1, k);
        if (q >= 0 && ok[q]) pred += val[q] * L.w[p];
    }
    return pred;
}

// ---- the sweep -------------------------------------------------------------------------------------------------------------------
// A wave owns column j and walks its coordinates t = 0 .. len-1 in list order (the Gauss-Seidel chain: coordinate t + 1 reads the weight
// coordinate t wrote).  The column's weights stay in LDS for the whole sweep (LDSW: dynamic LDS, the launch's longest list or
// SLIM_SWEEP_LDS_MIN, whichever is more; a list longer than SLIM_WTILE keeps them in global memory, read and written past the vector L1
// at agent scope) and go back once.  Per coordinate, the entries of column i = nns(j)[t] are
// taken 64 at a time:
//   1. a lane per USER: its own r_uj (train.get: a plain search of the row), and its own prediction chain over the list's other
//      positions in order -- per neighbour k a binary search of the user's row with the entry's `ok` flag (SparseVector.contains);
//   2. the three sums over the users (grad, rate, errs) in user order, one chain each, carried from chunk to chunk: every lane adds the
//      products lane after lane through v_readlane, so the sums are wave-uniform and no sum is split.
template <bool LDSW>
__global__ __launch_bounds__(64) void slim_sweep_kernel(PairCsr rows, PairCsr cols, SlimLists L, double *term, const int32_t *order, int n_order,
                                                        double l1, double l2) {
    extern __shared__ double s_w[]; // LDSW: the launch's longest list (slim_launch_sweep); else none
    const int lane = threadIdx.x;
    if ((int)blockIdx.x >= n_order) return;
    const int j = order[blockIdx.x];
    const int64_t p0 = L.ptr[j];
    const int len = (int)(L.ptr[j + 1] - p0);
    const int32_t *lst = L.idx + p0;
    double *wj = L.w + p0;
    if constexpr (LDSW) {
        for (int s = lane; s < len; s += 64) s_w[s] = wj[s];
        __syncthreads();
    }
    const auto wget = [&](int s) -> double {
        if constexpr (LDSW) return s_w[s];
        else return __hip_atomic_load(wj + s, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    };
    for (int t = 0; t < len; ++t) {
        const int i = lst[t];
        const int c0 = cols.ptr[i], c1 = cols.ptr[i + 1];
        double grad = 0.0, rate = 0.0, errs = 0.0;
        for (int base = c0; base < c1; base += 64) {
            const int cnt = min(64, c1 - base);
            const int q = base + min(lane, cnt - 1); // the lanes past the column's end repeat its last entry; step 2 never reads them
            const int u = cols.idx[q];
            const double rui = cols.val[q];
            const int r0 = rows.ptr[u], r1 = rows.ptr[u + 1];
            const int pj = slim_find(rows.idx, r0, r1, j);
            const double ruj = pj >= 0 ? rows.val[pj] : 0.0;
            double pred = 0.0;
            for (int s = 0; s < len; ++s) {
                if (s == t) continue;
                const int p = slim_find(rows.idx, r0, r1, lst[s]);
                if (p >= 0 && rows.ok[p]) pred += rows.val[p] * wget(s);
            }
            const double e = ruj - pred;
            const double pg = rui * e, pr = rui * rui, pe = e * e;
            for (int l = 0; l < cnt; ++l) {
                grad += slim_lane_d(pg, l);
                rate += slim_lane_d(pr, l);
                errs += slim_lane_d(pe, l);
            }
        }
        const double n = (double)(c1 - c0);
        grad /= n;
        rate /= n;
        errs /= n;
        const double wij = wget(t);
        const double tm = errs + 0.5 * l2 * wij * wij + l1 * wij;
        double nw = 0.0;
        if (l1 < fabs(grad)) nw = (grad > 0 ? grad - l1 : grad + l1) / (l2 + rate);
        if (lane == 0) {
            term[p0 + t] = tm;
            if constexpr (LDSW) s_w[t] = nw;
            else __hip_atomic_store(wj + t, nw, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        if constexpr (LDSW) __syncthreads();
        else __threadfence(); // the store has reached the L2 before the wave's next loads leave
    }
    if constexpr (LDSW)
        for (int s = lane; s < len; s += 64) wj[s] = s_w[s];
}

hipError_t slim_launch_sweep(PairCsr rows, PairCsr cols, SlimLists L, double *term, const int32_t *order, int n_order, int lds_len, double l1,
                             double l2, hipStream_t s) {
    if (n_order <= 0) return hipSuccess;
    if (lds_len > SLIM_WTILE) return hipErrorInvalidValue;
    // the LDS a wave asks for also sets how many waves share a CU's caches (160 KiB / bytes); SLIM_SWEEP_LDS_MIN is the measured choice
    // (DESIGN.md section 14), CMI_SLIM_SWEEP_LDS overrides it for measurements
    size_t lds_min = SLIM_SWEEP_LDS_MIN;
    if (const char *e = getenv("CMI_SLIM_SWEEP_LDS")) lds_min = (size_t)std::max(0, std::min(atoi(e), SLIM_WTILE * 8));
    const size_t lds = std::max((size_t)lds_len * sizeof(double), lds_min);
    if (lds_len > 0)
        slim_sweep_kernel<true><<<dim3((unsigned)n_order), dim3(64), lds, s>>>(rows, cols, L, term, order, n_order, l1, l2);
    else slim_sweep_kernel<false><<<dim3((unsigned)n_order), dim3(64), 0, s>>>(rows, cols, L, term, order, n_order, l1, l2);
    return hipGetLastError();
}

// ---- loss ------------------------------------------------------------------------------------------------------------------------
// `loss += term` in (j, t) order decides isConverged, so it is one chain: one wave loads 64 terms at a time (coalesced, the next load in
// flight) and adds them lane after lane, every lane alike.
__global__ __launch_bounds__(64) void slim_loss_kernel(const double *term, int64_t n, double *loss) {
    const int lane = threadIdx.x;
    double s = 0.0;
    double next = lane < n ? term[lane] : 0.0;
    for (int64_t base = 0; base < n; base += 64) {
        const double cur = next;
        const int64_t p = base + 64 + lane;
        next = p < n ? term[p] : 0.0;
        const int cnt = (int)min<int64_t>(64, n - base);
        for (int l = 0; l < cnt; ++l) s += slim_lane_d(cur, l);
    }
    if (lane == 0) *loss = s;
}

hipError_t slim_launch_loss(const double *term, int64_t n, double *loss, hipStream_t s) {
    slim_loss_kernel<<<1, 64, 0, s>>>(term, n, loss);
    return hipGetLastError();
}

// ---- scores ----------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(SLIM_SCORE_BLOCK) void slim_predict_kernel(PairCsr rows, SlimLists L, int64_t n, const int32_t *tu, const int32_t *tj,
                                                                        double *out) {
    const int64_t t = (int64_t)blockIdx.x * SLIM_SCORE_BLOCK + threadIdx.x;
    if (t >= n) return;
    const int u = tu[t];
    out[t] = slim_score_one(rows.idx, rows.val, rows.ok, rows.ptr[u], rows.ptr[u + 1], L, tj[t]);
}

hipError_t slim_launch_predict(PairCsr rows, SlimLists L, int64_t n, const int32_t *u, const int32_t *j, double *out, hipStream_t s) {
    if (n <= 0) return hipSuccess;
    slim_predict_kernel<<<dim3((unsigned)((n + SLIM_SCORE_BLOCK - 1) / SLIM_SCORE_BLOCK)), dim3(SLIM_SCORE_BLOCK), 0, s>>>(rows, L, n, u, j, out);
    return hipGetLastError();
}

// A workgroup per (group of queries of one user, block of SLIM_SCORE_BLOCK candidates): the user's row is staged in LDS (a row longer than
// SLIM_RTILE is read from global memory), a lane per candidate walks nns(j) in order with its own chain, and the score goes to every query
// of the group inside [q0, q0 + nq).
__global__ __launch_bounds__(SLIM_SCORE_BLOCK) void slim_score_kernel(PairCsr rows, SlimLists L, const int32_t *cand, int nc, const int32_t *gu,
                                                                      const int32_t *gq0, int g0, int64_t q0, int64_t nq, double *S) {
    __shared__ int32_t s_idx[SLIM_RTILE];
    __shared__ double s_val[SLIM_RTILE];
    __shared__ uint8_t s_ok[SLIM_RTILE];
    const int g = g0 + (int)blockIdx.x;
    const int u = gu[g];
    const int r0 = rows.ptr[u], r1 = rows.ptr[u + 1];
    const bool staged = r1 - r0 <= SLIM_RTILE;
    if (staged) {
        for (int e = threadIdx.x; e < r1 - r0; e += SLIM_SCORE_BLOCK) s_idx[e] = rows.idx[r0 + e], s_val[e] = rows.val[r0 + e], s_ok[e] = rows.ok[r0 + e];
        __syncthreads();
    }
    const int c = (int)blockIdx.y * SLIM_SCORE_BLOCK + (int)threadIdx.x;
    if (c >= nc) return;
    const int j = cand[c];
    const double pred = staged ? slim_score_one(s_idx, s_val, s_ok, 0, r1 - r0, L, j) : slim_score_one(rows.idx, rows.val, rows.ok, r0, r1, L, j);
    const int64_t qa = max((int64_t)gq0[g], q0), qb = min((int64_t)gq0[g + 1], q0 + nq);
    for (int64_t q = qa; q < qb; ++q) S[(size_t)(q - q0) * (size_t)nc + (size_t)c] = pred;
}

hipError_t slim_launch_score(PairCsr rows, SlimLists L, const int32_t *cand, int nc, const int32_t *gu, const int32_t *gq0, int g0, int g1,
                             int64_t q0, int64_t nq, double *S, hipStream_t s) {
    if (g1 <= g0 || nc <= 0 || nq <= 0) return hipSuccess;
    const dim3 grid((unsigned)(g1 - g0), (unsigned)((nc + SLIM_SCORE_BLOCK - 1) / SLIM_SCORE_BLOCK));
    slim_score_kernel<<<grid, dim3(SLIM_SCORE_BLOCK), 0, s>>>(rows, L, cand, nc, gu, gq0, g0, q0, nq, S);
    return hipGetLastError();
}

} // namespace cmi
