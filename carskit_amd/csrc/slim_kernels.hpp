// slim_kernels.hpp -- device side of SLIM (slim_kernels.hip), launched by slim_api.cpp.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

#include "pair_walk.hpp"

namespace cmi {

constexpr int SLIM_WTILE = 1024; // the longest list whose weights the sweep keeps in LDS (8 KiB a wave at most); a longer list stays in global memory
constexpr int SLIM_SWEEP_LDS_MIN = 8192; // bytes of LDS a sweep wave asks for at least: 20 waves a CU, measured 1.6 x faster than 32
constexpr int SLIM_RTILE = 256;  // entries of a user's row the score kernel stages in LDS (3.3 KiB a workgroup); a longer row is read from global memory
constexpr int SLIM_SCORE_BLOCK = 256;

// the neighbour lists of every item, in the order SLIM.java walks them, and what is aligned with them
struct SlimLists {
    const int64_t *ptr = nullptr; // n_items + 1
    const int32_t *idx = nullptr; // idx[p]: neighbour i of column j, ptr[j] <= p < ptr[j + 1]
    double *w = nullptr;          // w[p] = W[idx[p]][j]
};

// One pass of SLIM.buildModel's loop body (SLIM.java:127-176) over the columns order[0 .. n_order): a wave per column.  rows: user ->
// (item, value, ok); cols: item -> (user, value); both without zero-valued cells.  term[p]: the loss term of coordinate p.  lds_len > 0: every
// listed column has at most lds_len <= SLIM_WTILE neighbours, kept in that many doubles of LDS; 0: any length, weights in global memory.
hipError_t slim_launch_sweep(PairCsr rows, PairCsr cols, SlimLists L, double *term, const int32_t *order, int n_order, int lds_len, double l1,
                             double l2, hipStream_t s);
// loss = ((0 + term[0]) + term[1]) + ... in one chain
hipError_t slim_launch_loss(const double *term, int64_t n, double *loss, hipStream_t s);
// SLIM.predict(u, j) (SLIM.java:183-209) of n tuples
hipError_t slim_launch_predict(PairCsr rows, SlimLists L, int64_t n, const int32_t *u, const int32_t *j, double *out, hipStream_t s);
// the score slab of the queries [q0, q0 + nq): S[(q - q0) * nc + c] = predict(gu[qg[q]], cand[c]), computed once per group of queries of
// one user (groups g0 .. g1 cover the queries) and written to each of the group's queries in the range
hipError_t slim_launch_score(PairCsr rows, SlimLists L, const int32_t *cand, int nc, const int32_t *gu, const int32_t *gq0, int g0, int g1,
                             int64_t q0, int64_t nq, double *S, hipStream_t s);

} // namespace cmi
