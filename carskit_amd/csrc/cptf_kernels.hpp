// cptf_kernels.hpp -- device side of CPTF (src/carskit/alg/cars/adaptation/independent/CPTF.java): the order-exact epoch as one wave,
// the loss sum, prediction of key tuples and the top-N score slab.  fp64 only.  Internal.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace cmi {

constexpr int CPTF_MAX_K = 128;    // a lane owns one (k <= 64) or two consecutive factors
constexpr int CPTF_MIN_DIMS = 2;   // user, item
constexpr int CPTF_MAX_DIMS = 10;  // the rows of an entry and of the entry after it live in registers
// context rows (dimensions >= 2) are kept in LDS during an epoch when they fit this many bytes: the LDS a kernel may ask for without
// an opt-in attribute, well under the CU's 160 KiB
constexpr size_t CPTF_LDS_CTX_BYTES = 64 * 1024;

// M[0] .. M[n_dims - 1] concatenated, each dims[d] x k row-major: off[d] is the element offset of M[d]
struct CptfModel {
    double *M;
    int64_t off[CPTF_MAX_DIMS + 1];
    int k, n_dims;
};

struct CptfEpoch {
    CptfModel m;
    const int64_t *row; // n x n_dims: element offset of the row M[d][keys[d]] of every entry, entries with rate <= 0 left out
    const double *r;    // n
    int64_t n;
    double lrate, reg;
    bool strict, lds_ctx;
    // strict: slots[t * (1 + k * n_dims)] = e * e, then reg * df * df in (f, d) order: the reference's loss terms in its order.
    // otherwise parts[0] = the chain of e * e over the entries, parts[1 + f] = factor f's chain of reg * df * df in (entry, d) order
    double *slots, *parts;
};

// CPTF.java:81-109, one iteration's sweep (the loss terms left in slots / parts)
hipError_t cptf_launch_epoch(const CptfEpoch &a, hipStream_t stream);
// *loss = the terms added one by one, slots in order (strict) or parts in order; CPTF.java:111's 0.5 is the caller's
hipError_t cptf_launch_loss(const double *terms, int64_t n_terms, double *loss, hipStream_t stream);
// CPTF.java:141-155 of n key tuples (keys: n x n_dims); bound: then CPTF.java:133-136's clamp
hipError_t cptf_launch_predict(const CptfModel &m, int64_t n, const int32_t *keys, bool bound, double lo, double hi, double *out,
                               hipStream_t stream);
// Qt[f * n_items + j] = M[1][j][f]: the item matrix as the scorer reads it
hipError_t cptf_launch_transpose_items(const CptfModel &m, int n_items, double *Qt, hipStream_t stream);
// the score slab of the queries [q0, q0 + nq): S[(q - q0) * nc + c] = CPTF.predict(qu[q], cand[c], context of q) (CPTF.java:119-139),
// qkeys: per query the n_dims - 2 context keys TensorRecommender.getKeys gives its context
hipError_t cptf_launch_score(const CptfModel &m, const double *Qt, int n_items, const int32_t *cand, int nc, const int32_t *qu,
                             const int32_t *qkeys, int64_t q0, int64_t nq, double lo, double hi, double *S, hipStream_t stream);

} // namespace cmi
