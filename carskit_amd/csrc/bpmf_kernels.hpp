// bpmf_kernels.hpp -- device side of BPMF (bpmf_kernels.hip), launched by bpmf_api.cpp.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

#include "java_math.hpp"
#include "pair_walk.hpp"
#include "rankals_kernels.hpp"

namespace cmi {

constexpr int BPMF_MAX_K = 64;   // factors: the row posterior keeps `mat` and `covar` (k x k doubles each, 64 KiB at k = 64) in LDS
constexpr int BPMF_BLOCK = 256;  // threads per workgroup
constexpr int BPMF_CHUNK = 64;   // entries of a row or column staged per pass
constexpr int BPMF_TILE = 32;    // rows of a factor matrix per pass of the moment kernels
constexpr int BPMF_STAGE_MIN = 1024; // doubles of LDS at least in which a row stages its chunk (covar's room, before covar exists)
constexpr int BPMF_GAUSS_BLOCK = 256; // polar attempts per workgroup of the gaussian stream; the scan takes this many workgroups a pass
static_assert(BPMF_MAX_K == RANKALS_MAX_K && BPMF_BLOCK == RANKALS_BLOCK, "BPMF inverts with rankals_invert (dense_invert.hpp)");

// ---- java.util.Random.nextGaussian() as a stream --------------------------------------------------------------------------------------
// Attempt t of the polar method starts 4 t LCG steps after the state the run starts from, whatever the attempts before it did.
// where a run of attempts ended: written by the device
struct BpmfGaussTail {
    int64_t accepted; // pairs accepted by the round (every attempt of it, also past the last one needed)
    int64_t last_t;   // the attempt that gave the last pair needed; -1: not reached in this round
    double cached;    // that pair's second value, when the run ends on its first
    int32_t have;
    int32_t pad;
};
// one round over the attempts [t0, t0 + n_att) of the run that starts at state0: the pairs are numbered from pair0, pair p goes to
// out[lead + 2 p] and out[lead + 2 p + 1] (the latter only below n), `need` pairs in all; the first round of a run with lead == 1
// writes out[0] = lead_value (the cached value the run starts with).  block_cnt / block_off: a value per workgroup of
// BPMF_GAUSS_BLOCK attempts.  tail is written in full.
hipError_t bpmf_launch_gauss_round(uint64_t state0, const JavaLcgJump &jump, int64_t t0, int64_t n_att, int64_t pair0, int64_t need,
                                   int lead, double lead_value, int64_t n, double *out, int32_t *block_cnt, int32_t *block_off,
                                   BpmfGaussTail *tail, hipStream_t s);

// ---- DenseMatrix.columnMean / cov() ---------------------------------------------------------------------------------------------------
// mean[f]: one chain over the rows, over `rows`.  cov[f][g]: the chain over the rows of (x[f] - m[f]) * (x[g] - m[g]) over rows - 1,
// m = Stats.mean of the column (NaN entries skipped, in the sum and in the count).  smean: k doubles of device scratch.
hipError_t bpmf_launch_moments(const double *X, int rows, int k, double *mean, double *smean, double *cov, hipStream_t s);

// ---- one Gibbs pass of one side (BPMF.java:155-191 / :194-229) ------------------------------------------------------------------------
struct BpmfRowArgs {
    int k = 0, n = 0;              // n workgroups
    PairCsr C;                     // the side's rows -> (partner, value), without the zero-valued cells
    const int32_t *rows = nullptr; // slot -> row: the rows with entries, ascending
    const int32_t *slots = nullptr; // workgroup -> slot; null: the workgroup's own index
    const int32_t *rank = nullptr;  // workgroup -> draw rank (its k draws start at k * rank); null: the slot
    const double *other = nullptr; // the partner side's factors
    double *own = nullptr;
    const double *alpha = nullptr, *mu = nullptr; // k x k, k
    double gm = 0.0;
    const double *Z = nullptr;     // the pass's gaussians
    int32_t *null_flag = nullptr;  // per slot: 1 where covar.cholesky() is null (the row keeps its value)
    int32_t *first_null = nullptr; // atomicMin of the null slots
};
hipError_t bpmf_launch_rows(const BpmfRowArgs &a, hipStream_t s);

// ---- loss and prediction ----------------------------------------------------------------------------------------------------------------
inline int64_t bpmf_loss_blocks(int64_t n) { return (n + BPMF_BLOCK - 1) / BPMF_BLOCK; }
// BPMF.java:232-242 over the n stored cells (cu: the user of every cell of R, CRS order).  strict: the terms added in one chain in
// cell order; else a fixed tree per 256 cells and the chain over the workgroups' sums.  term: n doubles, part: bpmf_loss_blocks(n).
hipError_t bpmf_launch_loss(const double *P, const double *Q, PairCsr R, const int32_t *cu, int64_t n, int k, double gm, bool strict,
                            double *term, double *part, double *loss, hipStream_t s);
// BPMF.predict(u, j) = globalMean + DenseMatrix.rowMult(P, u, Q, j), bounded to [lo, hi] if bound
hipError_t bpmf_launch_predict(const double *P, const double *Q, int k, double gm, int64_t n, const int32_t *u, const int32_t *j, int bound,
                               double lo, double hi, double *out, hipStream_t s);

} // namespace cmi
