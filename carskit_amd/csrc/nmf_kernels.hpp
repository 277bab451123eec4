// nmf_kernels.hpp -- device side of NMF (nmf_kernels.hip), launched by nmf_api.cpp.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

#include "pair_walk.hpp"

namespace cmi {

constexpr int NMF_MAX_K = 256;   // factors: four per lane of the wave that owns a row
constexpr int NMF_CHUNK = 64;    // entries of a row per pass: one per lane
constexpr int NMF_BLOCK = 256;   // threads per workgroup: four rows (a wave each) of the row kernel, 256 cells of the loss kernel

// One phase of NMF.buildModel's loop (NMF.java:72-89 with own = W, other = Ht, csr = rows; :92-110 with own = Ht, other = W, csr =
// columns): for each of the n_order rows named by `order` (the rows with entries, longest first), own[row] *= real / (estm + 1e-9) per
// factor, from the row as it was.  own and other are row-major with k doubles a row; `other` is only read.
hipError_t nmf_launch_rows(double *own, const double *other, PairCsr csr, const int32_t *order, int n_order, int k, hipStream_t s);
// NMF.java:113-126: 0.5 * the sum of (predict(u, j) - r)^2 over the nnz cells (user cu[q], item rows.idx[q], value rows.val[q]) with
// r > 0, into *loss.  part: room for nmf_loss_blocks(nnz) doubles.  The order of the sum depends on nnz alone.
inline int64_t nmf_loss_blocks(int64_t nnz) { return (nnz + NMF_BLOCK - 1) / NMF_BLOCK; }
hipError_t nmf_launch_loss(const double *W, const double *Ht, PairCsr rows, const int32_t *cu, int64_t nnz, int k, double *part,
                           double *loss, hipStream_t s);
// NMF.predict(u, j) = DenseMatrix.product(W, u, H, j) of n tuples, a lane each
hipError_t nmf_launch_predict(const double *W, const double *Ht, int k, int64_t n, const int32_t *u, const int32_t *j, int bound, double lo,
                              double hi, double *out, hipStream_t s);

} // namespace cmi
