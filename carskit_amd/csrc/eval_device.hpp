// eval_device.hpp -- what every predict / evalRatings kernel ends in (eval_kernel: mf_sgd_kernels.hip, ext_eval_kernel: ext_kernels.hip,
// fm_predict_kernel, knn_predict_kernel, slope_predict_kernel): the bound to the rating scale, and for the two evaluation kernels the
// tuple / output / scale fields, the five running sums of Recommender.evalRatings and their hand-over to the block's partials.  Internal.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

namespace cmi {

// Recommender.predict(u, j, c, true): the prediction bounded to the rating scale.  Two comparisons, so that NaN stays NaN
__device__ __forceinline__ double bound_to_scale(double pred, int bound, double lo, double hi) {
    if (bound) {
        if (pred > hi) pred = hi;
        if (pred < lo) pred = lo;
    }
    return pred;
}

// the tuples an evaluation kernel reads, what it writes and the rating scale: the part of EvalArgs and ExtEvalArgs that is the same
struct EvalIO {
    const int32_t *u, *j, *ctx; // n tuples (ctx null for a 2-D model)
    const double *r;            // may be null (predict only)
    double *preds;              // may be null
    double *part;               // [blocks x 5] partial sums (abs, sq, rabs, rsq, count); may be null
    double gm, lo, hi, min_rate;
    int32_t bound;
};

struct EvalSums { // of one wave, over its tuples in order
    double abs = 0, sq = 0, rabs = 0, rsq = 0, cnt = 0;
};

// the end of tuple t, whose wave holds `pred` in every lane: bounded, stored, and (Recommender.java:532-545) unless it is NaN compared
// with the rating as it is and rounded to a rating level
__device__ __forceinline__ void eval_tuple(const EvalIO &io, int64_t t, int lane, double pred, EvalSums &s) {
    pred = bound_to_scale(pred, io.bound, io.lo, io.hi);
    if (io.preds && lane == 0) io.preds[t] = pred;
    if (io.r && !isnan(pred)) {
        const double rate = io.r[t];
        const double rpred = floor(pred / io.min_rate + 0.5) * io.min_rate; // Math.round(x)*minRate
        const double err = fabs(rate - pred), rerr = fabs(rate - rpred);
        s.abs += err;
        s.sq += err * err;
        s.rabs += rerr;
        s.rsq += rerr * rerr;
        s.cnt += 1.0;
    }
}

// the end of a 256-thread block: its four waves' sums added in wave order into part[block * 5 + c]
__device__ __forceinline__ void eval_block_store(const EvalIO &io, int wave, int lane, const EvalSums &s) {
    __shared__ double s_part[4][5];
    if (!io.part) return;
    if (lane == 0) {
        s_part[wave][0] = s.abs;
        s_part[wave][1] = s.sq;
        s_part[wave][2] = s.rabs;
        s_part[wave][3] = s.rsq;
        s_part[wave][4] = s.cnt;
    }
    __syncthreads();
    if (threadIdx.x < 5) {
        const int c = threadIdx.x;
        io.part[(size_t)blockIdx.x * 5 + c] = ((s_part[0][c] + s_part[1][c]) + s_part[2][c]) + s_part[3][c];
    }
}

} // namespace cmi
