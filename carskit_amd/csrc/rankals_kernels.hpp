// rankals_kernels.hpp -- device side of RankALS (rankals_kernels.hip), launched by rankals_api.cpp.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

#include "pair_walk.hpp"

namespace cmi {

constexpr int RANKALS_MAX_K = 64;   // factors: the solve keeps `mat` and `I` (k x k doubles each, 16 k^2 bytes: 64 KiB at k = 64) in LDS
constexpr int RANKALS_BLOCK = 256;  // threads per workgroup
constexpr int RANKALS_CHUNK = 64;   // entries of a row or column staged per pass
constexpr int RANKALS_TILE = 16;    // users or items per pass of the moment kernels
constexpr int RANKALS_STAGE_MIN = 1024; // doubles of LDS at least in which a solve stages the rows of a chunk (I's room, before I exists)
// the widest row of P rankals_launch_score takes: its kernel keeps the row in a static LDS array of this many doubles (1 KiB).  The other
// factor models that fill their score slab with it (BPR, LRMF, RankSGD) assert their own k limit against it next to the call.
constexpr int RANK_SCORE_MAX_K = 128;
static_assert(RANKALS_MAX_K <= RANK_SCORE_MAX_K, "RankALS scores with rankals_launch_score: its row of P must fit the kernel's LDS row");

// everything one iteration reads and writes, on the device
struct RankAlsState {
    int k = 0, n_users = 0, n_items = 0, n_rows = 0;
    PairCsr rows, cols;            // user -> (item, value), item -> (user, value); ascending, without the zero-valued cells
    const int32_t *users = nullptr; // train.rows(): the n_rows users with a non-zero cell, ascending
    const double *s = nullptr;     // s_i per item
    double sum_s = 0.0;
    double *P = nullptr, *Q = nullptr; // n_users x k, n_items x k
    double *sum_sq = nullptr, *sum_sqq = nullptr;               // k, k x k
    double *m_sr = nullptr, *m_cr = nullptr, *m_c = nullptr;    // per user (step 3's maps)
    double *m_cq = nullptr, *ppcq_u = nullptr;                  // n_users x k: m_sum_cq[u]; pp.mult(m_sum_cq[u]) of the new P[u]
    double *cpp = nullptr, *ppc = nullptr, *ppcq = nullptr, *crp = nullptr; // k x k, k x k, k, k: the item-independent sums of the Q step
};

// RankALS.java:91-98: sum_sq and sum_sqq, every element one chain over the items ascending
hipError_t rankals_launch_item_moments(const RankAlsState &a, hipStream_t s);
// RankALS.java:102-136 and 144-166: a workgroup per user of rows(): the sums over the row, M, y, P[u] = M.inv().mult(y), the user's
// m_* values, and pp.mult(m_sum_cq[u]) of the new row
hipError_t rankals_launch_user_solve(const RankAlsState &a, hipStream_t s);
// RankALS.java:184-189: sum_cpp, sum_p_p_c, sum_p_p_cq, sum_cr_p, every element one chain over the users of rows() in order
hipError_t rankals_launch_user_moments(const RankAlsState &a, hipStream_t s);
// RankALS.java:168-204: a workgroup per item: the three sums over the item's raters with a value > 0, M, y, Q[i] = M.inv().mult(y)
hipError_t rankals_launch_item_solve(const RankAlsState &a, hipStream_t s);
// DenseMatrix.inv() of n_mats n x n matrices (row-major, one after another), a workgroup each
hipError_t rankals_launch_invert(const double *A, double *out, int n_mats, int n, hipStream_t s);
// RankALS.predict(u, j) = DenseMatrix.rowMult(P, u, Q, j) of n tuples
hipError_t rankals_launch_predict(const double *P, const double *Q, int k, int64_t n, const int32_t *u, const int32_t *j, double *out,
                                  hipStream_t s);
// the score slab of the queries [q0, q0 + nq) (rank_run_device_slab): S[(q - q0) * nc + c] = predict(gu[g], cand[c]) for every query of
// group g inside the range; hipErrorInvalidValue for k outside 1 .. RANK_SCORE_MAX_K
hipError_t rankals_launch_score(const double *P, const double *Q, int k, const int32_t *cand, int nc, const int32_t *gu, const int32_t *gq0,
                                int g0, int g1, int64_t q0, int64_t nq, double *S, hipStream_t s);

} // namespace cmi
