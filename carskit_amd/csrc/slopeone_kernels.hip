// slopeone_kernels.hip -- SlopeOne on gfx950: the deviation build (SlopeOne.buildModel) and the prediction (SlopeOne.predict).
// Everything is fp64 with the reference's operation order: a pair's sum runs sequentially in one lane along the ascending user index, a
// prediction's sum in one chain along the ascending item index (no lane-split reductions, no FMA: -ffp-contract=off), and division is
// the correctly rounded IEEE operation Java uses.
#include "slopeone_kernels.hpp"
#include "eval_device.hpp"

namespace cmi {

// ---- deviation build -----------------------------------------------------------------------------------------------------------
// A workgroup owns an anchor column a and its partners b > a, one per lane (chunks of PAIR_BUILD_BLOCK), and meets every pair's common
// users in ascending order by the shared walk (pair_walk.hpp); the running sum stays in the lane's registers.
__global__ __launch_bounds__(PAIR_BUILD_BLOCK) void slope_build_kernel(PairCsr C, int n, double *dev, int32_t *card) {
    __shared__ PairTile<PairOk::ALL> T;
    const int a = blockIdx.x;
    const int a0 = C.ptr[a], a1 = C.ptr[a + 1];
    if (a0 == a1 || a + 1 >= n) return; // no user rated a: no pair of a has a common user
    pair_tile_init(T);
    int gen = 0;
    for (int c = a + 1; c < n; c += blockDim.x) {
        const int b = c + (int)threadIdx.x;
        const int b0 = b < n ? C.ptr[b] : 0, b1 = b < n ? C.ptr[b + 1] : 0;
        const bool act = b0 < b1;
        int k = 0;
        double sum = 0.0;
        pair_sweep(C, a0, a1, b0, b1, act, T, gen, [&](double va, double vb, int, int) {
            sum += va - vb; // devMatrix.add(a, b, r_ua - r_ub)
            ++k;
        });
        if (!act || k == 0) continue;
        const double d = sum / (double)k;
        dev[(int64_t)a * n + b] = d;
        // the reference sums r_ub - r_ua from +0.0 on the other side: the negated sum, except that a zero sum is +0.0 there too
        dev[(int64_t)b * n + a] = sum == 0.0 ? 0.0 : -d;
        card[(int64_t)a * n + b] = k;
        card[(int64_t)b * n + a] = k;
    }
}

hipError_t slope_launch_build(PairCsr cols, int n, double *dev, int32_t *card, hipStream_t s) {
    if (n <= 1) return hipSuccess;
    slope_build_kernel<<<dim3(n), dim3(PAIR_BUILD_BLOCK), 0, s>>>(cols, n, dev, card);
    return hipGetLastError();
}

// ---- prediction ----------------------------------------------------------------------------------------------------------------
// A wave per tuple (u, j).  The user's items are taken 64 at a time: every lane loads its item's rating and the entries of row j of dev
// and card, and forms its own term (dev + r) * card; then the whole wave adds the valid terms (card > 0, i != j) lane after lane, i.e.
// in item order, in one chain that is carried from chunk to chunk.
__global__ __launch_bounds__(64) void slope_predict_kernel(PairCsr R, const double *dev, const int32_t *card, int n_items, int64_t n,
                                                           const int32_t *tu, const int32_t *tj, double gm, int bound, double lo,
                                                           double hi, double *out) {
    const int lane = threadIdx.x;
    for (int64_t t = blockIdx.x; t < n; t += gridDim.x) {
        const int u = tu[t], j = tj[t];
        const double *dj = dev + (int64_t)j * n_items;
        const int32_t *cj = card + (int64_t)j * n_items;
        const int e1 = R.ptr[u + 1];
        double preds = 0.0, cards = 0.0;
        for (int base = R.ptr[u]; base < e1; base += 64) {
            const int q = base + lane;
            double term = 0.0, c = 0.0;
            bool keep = false;
            if (q < e1) {
                const int i = R.idx[q];
                const int32_t ci = cj[i];
                keep = i != j && ci > 0; // train.row(u, j) leaves column j out
                c = (double)ci;
                term = (dj[i] + R.val[q]) * c;
            }
            for (uint64_t m = __ballot(keep); m; m &= m - 1) {
                const int l = __ffsll((unsigned long long)m) - 1;
                preds += __shfl(term, l);
                cards += __shfl(c, l);
            }
        }
        if (lane == 0) {
            out[t] = bound_to_scale(cards > 0.0 ? preds / cards : gm, bound, lo, hi);
        }
    }
}

hipError_t slope_launch_predict(PairCsr rows, const double *dev, const int32_t *card, int n_items, int64_t n, const int32_t *u,
                                const int32_t *j, double global_mean, int bound, double lo, double hi, double *out, int nwaves,
                                hipStream_t s) {
    if (n <= 0) return hipSuccess;
    slope_predict_kernel<<<nwaves, 64, 0, s>>>(rows, dev, card, n_items, n, u, j, global_mean, bound, lo, hi, out);
    return hipGetLastError();
}

// ---- top-N scores --------------------------------------------------------------------------------------------------------------
// ranking(u, j) = predict(u, j), unbounded (SlopeOne has no ranking branch).  A workgroup per (group of queries of one user, block of
// SLOPE_SCORE_BLOCK candidates): the user's row is staged in LDS (a row longer than SLOPE_RTILE is read from global memory), a lane per
// candidate walks it in ascending item order with slope_predict_kernel's chain, and the score goes to every query of the group inside
// [q0, q0 + nq).
template <class Idx, class Val>
__device__ double slope_score_one(Idx idx, Val val, int len, const double *dj, const int32_t *cj, int j, double gm) {
    double preds = 0.0, cards = 0.0;
    for (int q = 0; q < len; ++q) {
        const int i = idx[q];
        const int32_t ci = cj[i];
        if (i != j && ci > 0) { // train.row(u, j) leaves column j out
            const double c = (double)ci;
            preds += (dj[i] + val[q]) * c;
            cards += c;
        }
    }
    return cards > 0.0 ? preds / cards : gm;
}

__global__ __launch_bounds__(SLOPE_SCORE_BLOCK) void slope_score_kernel(PairCsr R, const double *dev, const int32_t *card, int n_items,
                                                                        double gm, const int32_t *cand, int nc, const int32_t *gu,
                                                                        const int32_t *gq0, int g0, int64_t q0, int64_t nq, double *S) {
    __shared__ int32_t s_idx[SLOPE_RTILE];
    __shared__ double s_val[SLOPE_RTILE];
    const int g = g0 + (int)blockIdx.x;
    const int u = gu[g];
    const int r0 = R.ptr[u], len = R.ptr[u + 1] - r0;
    const bool staged = len <= SLOPE_RTILE;
    if (staged) {
        for (int e = threadIdx.x; e < len; e += SLOPE_SCORE_BLOCK) s_idx[e] = R.idx[r0 + e], s_val[e] = R.val[r0 + e];
        __syncthreads();
    }
    const int c = (int)blockIdx.y * SLOPE_SCORE_BLOCK + (int)threadIdx.x;
    if (c >= nc) return;
    const int j = cand[c];
    const double *dj = dev + (int64_t)j * n_items;
    const int32_t *cj = card + (int64_t)j * n_items;
    const double pred = staged ? slope_score_one(s_idx, s_val, len, dj, cj, j, gm) : slope_score_one(R.idx + r0, R.val + r0, len, dj, cj, j, gm);
    const int64_t qa = max((int64_t)gq0[g], q0), qb = min((int64_t)gq0[g + 1], q0 + nq);
    for (int64_t q = qa; q < qb; ++q) S[(size_t)(q - q0) * (size_t)nc + (size_t)c] = pred;
}

hipError_t slope_launch_score(PairCsr rows, const double *dev, const int32_t *card, int n_items, double global_mean, const int32_t *cand,
                              int nc, const int32_t *gu, const int32_t *gq0, int g0, int g1, int64_t q0, int64_t nq, double *S,
                              hipStream_t s) {
    if (g1 <= g0 || nc <= 0 || nq <= 0) return hipSuccess;
    const dim3 grid((unsigned)(g1 - g0), (unsigned)((nc + SLOPE_SCORE_BLOCK - 1) / SLOPE_SCORE_BLOCK));
    slope_score_kernel<<<grid, dim3(SLOPE_SCORE_BLOCK), 0, s>>>(rows, dev, card, n_items, global_mean, cand, nc, gu, gq0, g0, q0, nq, S);
    return hipGetLastError();
}

} // namespace cmi
