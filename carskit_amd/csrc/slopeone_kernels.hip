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

} // namespace cmi
