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
// The scratch of the prediction: every wave owns `cap` entries (the longest list it may meet) of each array, 32 bytes an entry.
struct KnnScratch {
    int32_t *key, *pos, *sel;
    double *sim, *dlt; // dlt: rating - mean[key], the neighbour's term of the weighted sum
};
// predict(u, j) of n tuples (one wave each).  owner[t] names the list the candidates come from (ItemKNN: the user's items, UserKNN:
// the item's users: a row of `lists`), target[t] the row of S they are scored against.  ranking: the keep rule of isRankingPred (a set,
// non-zero similarity of either sign) instead of sim > 0.  scratch: nwaves * cap entries of each array.  bad[0] counts the tuples whose
// HashMap would treeify a bin; bad[1], bad[2]: the (owner, target) of the first one counted.
hipError_t knn_launch_predict(PairCsr lists, const double *S, int n_ent, const double *mean, int64_t n, const int32_t *owner,
                              const int32_t *target, int knn, double global_mean, bool ranking, int bound, double lo, double hi,
                              double *out, int nwaves, int cap, KnnScratch scratch, int32_t *bad, hipStream_t s);
// the candidates of a unit of knn_launch_score, and the entries of a user's row that ItemKNN stages in LDS (20 bytes each)
constexpr int KNN_SCORE_TILE = 64, KNN_STAGE = 512;
// ranking(gu[g], cand[c]) of the groups g0 .. g1 -> out[(q - q0) * nc + c] for every query q of group g inside [q0, q0 + nq): the fill
// of rank_run_device_slab.  item: ItemKNN (the owner list is the user's), else UserKNN (the candidate's).  scratch and bad as above,
// bad[1], bad[2] = (user, item).
hipError_t knn_launch_score(bool item, PairCsr lists, const double *S, int n_ent, const double *mean, int knn, double global_mean,
                            int nwaves, int cap, KnnScratch scratch, int32_t *bad, const int32_t *cand, int nc, const int32_t *gu,
                            const int32_t *gq0, int g0, int g1, int64_t q0, int64_t nq, double *out, hipStream_t s);

} // namespace cmi
