// knn_kernels.hpp -- device side of ItemKNN / UserKNN (knn_kernels.hip), launched by knn_api.cpp.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

#include "pair_walk.hpp"

namespace cmi {

// Recommender.buildCorrs: S[a][b] = S[b][a] = correlation(row a, row b) for a < b, both rows non-empty; NaN stays where it is unset
// (S must be NaN-filled before).  norm2: inner(v, v) of every row (cos-binary).
hipError_t knn_launch_build(PairCsr rows, int n, const double *norm2, int measure, int shrinkage, double median, double *S,
                            hipStream_t s);
// SparseVector.mean() (and inner(v, v)) of every row; empty rows get NaN
hipError_t knn_launch_row_stats(PairCsr rows, int n, double *mean, double *norm2, hipStream_t s);
// predict(u, j) of n tuples (one wave each).  owner[t] names the list the candidates come from (ItemKNN: the user's items, UserKNN:
// the item's users: a row of `lists`), target[t] the row of S they are scored against.  scratch: nwaves * cap entries of each array.
// bad[0] counts tuples whose HashMap would treeify a bin.
hipError_t knn_launch_predict(PairCsr lists, const double *S, int n_ent, const double *mean, int64_t n, const int32_t *owner,
                              const int32_t *target, int knn, double global_mean, int bound, double lo, double hi, double *out,
                              int nwaves, int cap, int32_t *s_key, double *s_sim, double *s_rate, int32_t *s_pos, int32_t *s_sel,
                              int32_t *bad, hipStream_t s);

} // namespace cmi
