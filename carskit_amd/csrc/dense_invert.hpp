// dense_invert.hpp -- librec's DenseMatrix.inv() as one workgroup-wide device routine in LDS, shared by the solves of RankALS
// (rankals_kernels.hip) and the row posterior of BPMF (bpmf_kernels.hip).  Workgroups of RANKALS_BLOCK threads.
#pragma once
#include <hip/hip_runtime.h>

#include "rankals_kernels.hpp"

namespace cmi {

// ---- DenseMatrix.inv() ----------------------------------------------------------------------------------------------------------------
// Gauss-Jordan on `mat` beside `inv` = eye(n), both n x n in LDS, by the whole workgroup; fv: n doubles of LDS.  Column i's pivot is the
// first row j in i .. n-1 whose |mat[j][i]| is strictly greater than the running maximum, which starts at 0.0: the lowest row among those
// that hold the column's largest magnitude, where a NaN (and a zero) never counts.  If no row wins, `inv` stays as it stands, partly
// reduced, as the reference returns it.  Otherwise rows p and i are swapped and row i is divided by the pivot (mat from column i on, inv
// over all columns), and every other row r takes f = mat[r][i] and subtracts the rounded product f * row i.  n == 1: 1.0 / a.
// Every thread of the workgroup calls it after a barrier that follows the last write to mat; it returns after a barrier.
__device__ inline void rankals_invert(double *mat, double *inv, double *fv, int n) {
    const int tid = threadIdx.x, lane = tid & 63;
    if (n == 1) {
        if (tid == 0) inv[0] = 1.0 / mat[0];
        __syncthreads();
        return;
    }
    for (int e = tid; e < n * n; e += RANKALS_BLOCK) inv[e] = e / n == e % n ? 1.0 : 0.0;
    int width = 2, shift = 1; // the columns of [mat | inv], padded to a power of two: a thread keeps its column, rows go round
    while (width < 2 * n) width <<= 1, ++shift;
    const int tx = tid & (width - 1), ty = tid >> shift, rows_at_once = RANKALS_BLOCK >> shift;
    double *const side = tx < n ? mat : inv; // this thread's column, in mat or in inv
    const int col = tx < n ? tx : tx - n;
    __syncthreads();
    for (int i = 0; i < n; ++i) {
        // every wave finds the pivot for itself, a lane per row
        double v = 0.0;
        if (lane >= i && lane < n) {
            v = fabs(mat[lane * n + i]);
            if (!(v > 0.0)) v = 0.0; // NaN: never strictly greater
        }
        double m = v;
        for (int off = 32; off; off >>= 1) m = fmax(m, __shfl_xor(m, off));
        if (!(m > 0.0)) break; // uniform over the workgroup: every wave read the same column (the barrier below closes this path)
        const int p = __ffsll((unsigned long long)__ballot(v == m)) - 1;
        const double piv = mat[p * n + i];
        if (tid < n) fv[tid] = tid == p ? mat[i * n + i] : mat[tid * n + i]; // f of every row as it stands after the swap
        __syncthreads();
        if (ty == 0 && tx < 2 * n && (tx >= n || col >= i)) { // swap and divide
            const double top = side[p * n + col], cur = side[i * n + col];
            side[i * n + col] = top / piv;
            if (p != i) side[p * n + col] = cur;
        }
        __syncthreads();
        if (tx < 2 * n && (tx >= n || col >= i)) {
            const double pivot_row = side[i * n + col];
            for (int r = ty; r < n; r += rows_at_once)
                if (r != i) side[r * n + col] = side[r * n + col] - fv[r] * pivot_row;
        }
        __syncthreads();
    }
    // the early return too ends at a barrier: a wave that has left its pivot search may not touch mat (the callers reuse it) while
    // another wave is still reading the column
    __syncthreads();
}

} // namespace cmi
