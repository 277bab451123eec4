// slopeone_kernels.hpp -- device side of SlopeOne (slopeone_kernels.hip), launched by slopeone_api.cpp.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

#include "pair_walk.hpp"

namespace cmi {

// SlopeOne.buildModel: for every pair a < b of columns with a common user, dev[a][b] = (sum over the common users, ascending, of
// r_ua - r_ub) / k, dev[b][a] its mirror (+0.0 where the sum is zero) and card[a][b] = card[b][a] = k.  dev and card (n x n) must be
// zero-filled before.
// cols: item -> users, for the build; rows: user -> items, for the prediction
hipError_t slope_launch_build(PairCsr cols, int n, double *dev, int32_t *card, hipStream_t s);
// SlopeOne.predict(u, j) of n tuples, a wave each (nwaves waves take the tuples in turn)
hipError_t slope_launch_predict(PairCsr rows, const double *dev, const int32_t *card, int n_items, int64_t n, const int32_t *u,
                                const int32_t *j, double global_mean, int bound, double lo, double hi, double *out, int nwaves,
                                hipStream_t s);
// the candidates of a workgroup of slope_launch_score, and the entries of a user's row it stages in LDS (12 bytes each)
constexpr int SLOPE_SCORE_BLOCK = 64, SLOPE_RTILE = 1024;
// predict(gu[g], cand[c]), unbounded, of the groups g0 .. g1 -> S[(q - q0) * nc + c] for every query q of group g inside
// [q0, q0 + nq): the fill of rank_run_device_slab
hipError_t slope_launch_score(PairCsr rows, const double *dev, const int32_t *card, int n_items, double global_mean, const int32_t *cand,
                              int nc, const int32_t *gu, const int32_t *gq0, int g0, int g1, int64_t q0, int64_t nq, double *S,
                              hipStream_t s);

} // namespace cmi
