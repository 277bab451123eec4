// slopeone_kernels.hip -- SlopeOne on gfx950: the deviation build (SlopeOne.buildModel) and the prediction (SlopeOne.predict).
// Everything is fp64 with the reference's operation order: a pair's sum runs sequentially in one lane along the ascending user index, a
// prediction's sum in one chain along the ascending item index (no lane-split reductions, no FMA: -ffp-contract=off), and division is
// the correctly rounded IEEE operation Java uses.
#include "slopeone_kernels.hpp"

namespace cmi {

// ---- deviation build -----------------------------------------------------------------------------------------------------------
// A workgroup owns an anchor column a and its partners b > a, one per lane (chunks of SLOPE_BUILD_BLOCK).  The anchor's column is
// scattered into LDS one tile of SLOPE_TILE users at a time (only tiles where the anchor has entries: no common user lies elsewhere);
// every lane walks its partner's entries of that tile in ascending order and probes the tile, so the common users are met in ascending
// order and the running sum stays in the lane's registers across tiles.  A tile entry is valid when its tag equals the current
// generation, so a tile is never cleared.
__global__ __launch_bounds__(SLOPE_BUILD_BLOCK) void slope_build_kernel(SlopeCsr C, int n, double *dev, int32_t *card) {
    __shared__ double lv[SLOPE_TILE];
    __shared__ int32_t tag[SLOPE_TILE];
    __shared__ int32_t s_qb;
    const int a = blockIdx.x;
    const int a0 = C.ptr[a], a1 = C.ptr[a + 1];
    if (a0 == a1 || a + 1 >= n) return; // no user rated a: no pair of a has a common user
    for (int i = threadIdx.x; i < SLOPE_TILE; i += blockDim.x) tag[i] = -1;
    int gen = 0;
    for (int c = a + 1; c < n; c += blockDim.x) {
        const int b = c + (int)threadIdx.x;
        const int b0 = b < n ? C.ptr[b] : 0, b1 = b < n ? C.ptr[b + 1] : 0;
        const bool act = b0 < b1;
        int k = 0;
        double sum = 0.0;
        int cur = b0;
        for (int qa = a0; qa < a1;) {
            const int lo = C.idx[qa] / SLOPE_TILE * SLOPE_TILE, hi = lo + SLOPE_TILE;
            __syncthreads(); // the previous tile's readers are done
            if (threadIdx.x == 0) { // the anchor's entries of this tile: [qa, qb)
                int l = qa, r = a1;
                while (l < r) {
                    const int m = (l + r) >> 1;
                    if (C.idx[m] < hi) l = m + 1;
                    else r = m;
                }
                s_qb = l;
            }
            __syncthreads();
            const int qb = s_qb;
            for (int q = qa + (int)threadIdx.x; q < qb; q += blockDim.x) {
                lv[C.idx[q] - lo] = C.val[q];
                tag[C.idx[q] - lo] = gen;
            }
            __syncthreads();
            if (act) {
                int l = cur, r = b1; // skip the partner's entries below the tile
                while (l < r) {
                    const int m = (l + r) >> 1;
                    if (C.idx[m] < lo) l = m + 1;
                    else r = m;
                }
                for (cur = l; cur < b1; ++cur) {
                    const int x = C.idx[cur];
                    if (x >= hi) break;
                    if (tag[x - lo] != gen) continue;
                    sum += lv[x - lo] - C.val[cur]; // devMatrix.add(a, b, r_ua - r_ub)
                    ++k;
                }
            }
            ++gen;
            qa = qb;
        }
        if (!act || k == 0) continue;
        const double d = sum / (double)k;
        dev[(int64_t)a * n + b] = d;
        // the reference sums r_ub - r_ua from +0.0 on the other side: the negated sum, except that a zero sum is +0.0 there too
        dev[(int64_t)b * n + a] = sum == 0.0 ? 0.0 : -d;
        card[(int64_t)a * n + b] = k;
        card[(int64_t)b * n + a] = k;
    }
}

hipError_t slope_launch_build(SlopeCsr cols, int n, double *dev, int32_t *card, hipStream_t s) {
    if (n <= 1) return hipSuccess;
    slope_build_kernel<<<dim3(n), dim3(SLOPE_BUILD_BLOCK), 0, s>>>(cols, n, dev, card);
    return hipGetLastError();
}

// ---- prediction ----------------------------------------------------------------------------------------------------------------
// A wave per tuple (u, j).  The user's items are taken 64 at a time: every lane loads its item's rating and the entries of row j of dev
// and card, and forms its own term (dev + r) * card; then the whole wave adds the valid terms (card > 0, i != j) lane after lane, i.e.
// in item order, in one chain that is carried from chunk to chunk.
__global__ __launch_bounds__(64) void slope_predict_kernel(SlopeCsr R, const double *dev, const int32_t *card, int n_items, int64_t n,
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
            double pred = cards > 0.0 ? preds / cards : gm;
            if (bound) {
                if (pred > hi) pred = hi;
                if (pred < lo) pred = lo;
            }
            out[t] = pred;
        }
    }
}

hipError_t slope_launch_predict(SlopeCsr rows, const double *dev, const int32_t *card, int n_items, int64_t n, const int32_t *u,
                                const int32_t *j, double global_mean, int bound, double lo, double hi, double *out, int nwaves,
                                hipStream_t s) {
    if (n <= 0) return hipSuccess;
    slope_predict_kernel<<<nwaves, 64, 0, s>>>(rows, dev, card, n_items, n, u, j, global_mean, bound, lo, hi, out);
    return hipGetLastError();
}

} // namespace cmi
