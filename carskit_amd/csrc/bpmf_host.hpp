// bpmf_host.hpp -- the host side of BPMF (bpmf_api.cpp; no device here): the stream of happy.coding.math.Randoms with nextGaussian's
// cached value, Randoms.gamma for alpha >= 1, librec's k x k operations in their loop orders (inv, cholesky, transpose, mult, outer,
// scale, add), BPMF.wishart, the hyper-parameter step (BPMF.java:98-149) and the draw offsets of a Gibbs pass with its exact second
// pass.  Plain C++ (tests/tools/bpmf_host_check.cpp drives it under the sanitizers); compile with -ffp-contract=off.
#pragma once
#include <cmath>
#include <cstdint>
#include <vector>

#include "java_math.hpp"

namespace cmi {

// java.util.Random as BPMF's Randoms holds it: the 48-bit state and the second value of nextGaussian's last pair
struct BpmfStream {
    uint64_t state = 0;
    int have = 0;
    double cached = 0.0;
    double nextDouble() {
        JavaStream s{state, 0};
        const double d = s.nextDouble();
        state = s.state;
        return d;
    }
    // Randoms.gaussian(0, 1) = 0 + 1 * nextGaussian(): the polar method, StrictMath.log and sqrt
    double gaussian() {
        if (have) {
            have = 0;
            return 0.0 + 1.0 * cached;
        }
        double v1, v2, s;
        do {
            v1 = 2.0 * nextDouble() - 1.0;
            v2 = 2.0 * nextDouble() - 1.0;
            s = v1 * v1 + v2 * v2;
        } while (s >= 1.0 || s == 0.0);
        const double m = std::sqrt(-2.0 * fdlibm_log(s) / s);
        cached = v2 * m, have = 1;
        return 0.0 + 1.0 * (v1 * m);
    }
};

// happy.coding.math.Randoms.gamma(alpha, lambda) for alpha >= 1, statement by statement from the bytecode (Math.* as StrictMath); the
// comparisons keep the bytecode's NaN outcomes.  alpha < 1: NaN (BPMF never asks: alpha >= numRows / 2)
inline double bpmf_gamma(BpmfStream &r, double alpha, double lambda) {
    if (!(alpha >= 1.0)) return std::nan("");
    const double inv_l = 1.0 / lambda, ss = alpha - 0.5, s = std::sqrt(ss), d = 5.656854249 - 12.0 * s;
    double v1, v2, v12;
    do {
        v1 = 2.0 * r.nextDouble() - 1.0;
        v2 = 2.0 * r.nextDouble() - 1.0;
        v12 = v1 * v1 + v2 * v2;
    } while (v12 > 1.0);
    double t = v1 * std::sqrt(-2.0 * fdlibm_log(v12) / v12);
    double x = s + 0.5 * t;
    const double gds = x * x;
    if (t >= 0.0) return gds / inv_l;
    double u = r.nextDouble();
    if (d * u <= t * t * t) return gds / inv_l;
    const double rr = 1.0 / alpha;
    const double q0 = ((((((((0.000171032 * rr + -0.0004701849) * rr + 0.0006053049) * rr + 0.0003340332) * rr + -0.0003349403) * rr +
                           0.0015746717) * rr + 0.0079849875) * rr + 0.0208333723) * rr + 0.0416666664) * rr;
    double b, si, c;
    if (alpha > 3.686) {
        if (alpha > 13.022) b = 1.77, si = 0.75, c = 0.1515 / s;
        else b = 1.654 + 0.0076 * ss, si = 1.68 / s + 0.275, c = 0.062 / s + 0.024;
    } else {
        b = 0.463 + s - 0.178 * ss, si = 1.235, c = 0.195 / s - 0.079 + 0.016 * s;
    }
    auto q_of = [&](double tt) {
        const double v = tt / (s + s);
        if (std::fabs(v) > 0.25) return q0 - s * tt + 0.25 * tt * tt + (ss + ss) * fdlibm_log(1.0 + v);
        const double p = (((((((0.104089866 * v + -0.112750886) * v + 0.11036831) * v + -0.124385581) * v + 0.142873973) * v + -0.166677482) * v +
                           0.199999867) * v + -0.249999949) * v + 0.333333333;
        return q0 + 0.5 * tt * tt * p * v;
    };
    if (x > 0.0) {
        const double q = q_of(t);
        if (fdlibm_log(1.0 - u) <= q) return gds / inv_l;
    }
    for (;;) {
        const double e = -fdlibm_log(r.nextDouble());
        u = r.nextDouble();
        u = u + u - 1.0;
        const double sign_u = u > 0.0 ? 1.0 : -1.0;
        t = b + e * si * sign_u;
        if (t <= -0.71874483771719) continue;
        const double q = q_of(t);
        if (q <= 0.0) continue;
        double w;
        if (q > 0.5) w = fdlibm_exp(q) - 1.0;
        else w = ((((((0.000247453 * q + 0.001353826) * q + 0.008345522) * q + 0.041664508) * q + 0.166666848) * q + 0.499999994) * q + 1.0) * q;
        if (!(c * u * sign_u <= w * fdlibm_exp(e - 0.5 * t * t))) continue;
        x = s + 0.5 * t;
        return x * x / inv_l;
    }
}

using BpmfMat = std::vector<double>; // n x n, row-major

// DenseMatrix.inv(): Gauss-Jordan beside eye(n); the pivot of column i is the first row from i on whose |value| is strictly greater
// than the running maximum (0.0 at first); none: the inverse as it stands.  n == 1: 1.0 / a.  (rankals_invert on the device)
inline BpmfMat bpmf_inv(BpmfMat mat, int n) {
    if (n == 1) return BpmfMat{1.0 / mat[0]};
    BpmfMat eye((size_t)n * n, 0.0);
    for (int i = 0; i < n; ++i) eye[(size_t)i * n + i] = 1.0;
    for (int i = 0; i < n; ++i) {
        double best = 0.0;
        int p = -1;
        for (int j = i; j < n; ++j) {
            const double a = std::fabs(mat[(size_t)j * n + i]);
            if (a > best) best = a, p = j;
        }
        if (p < 0) return eye;
        if (p != i)
            for (int c = 0; c < n; ++c) std::swap(mat[(size_t)i * n + c], mat[(size_t)p * n + c]), std::swap(eye[(size_t)i * n + c], eye[(size_t)p * n + c]);
        const double piv = mat[(size_t)i * n + i];
        for (int c = i; c < n; ++c) mat[(size_t)i * n + c] = mat[(size_t)i * n + c] / piv;
        for (int c = 0; c < n; ++c) eye[(size_t)i * n + c] = eye[(size_t)i * n + c] / piv;
        for (int rw = 0; rw < n; ++rw) {
            if (rw == i) continue;
            const double f = mat[(size_t)rw * n + i];
            for (int c = i; c < n; ++c) mat[(size_t)rw * n + c] = mat[(size_t)rw * n + c] - f * mat[(size_t)i * n + c];
            for (int c = 0; c < n; ++c) eye[(size_t)rw * n + c] = eye[(size_t)rw * n + c] - f * eye[(size_t)i * n + c];
        }
    }
    return eye;
}

// DenseMatrix.cholesky().transpose(): the LOWER factor into L; false where the reference returns null (a NaN diagonal after its row).
// A zero diagonal is no null: the rows below divide by it.
inline bool bpmf_cholesky(const BpmfMat &A, int n, BpmfMat &L) {
    L.assign((size_t)n * n, 0.0);
    for (int i = 0; i < n; ++i) {
        for (int j = 0; j <= i; ++j) {
            double s = 0.0;
            for (int k = 0; k < j; ++k) s += L[(size_t)i * n + k] * L[(size_t)j * n + k];
            const double d = A[(size_t)i * n + j] - s;
            L[(size_t)i * n + j] = i == j ? std::sqrt(d) : d / L[(size_t)j * n + j];
        }
        if (std::isnan(L[(size_t)i * n + i])) return false;
    }
    return true;
}

inline BpmfMat bpmf_transpose(const BpmfMat &A, int n) {
    BpmfMat T((size_t)n * n);
    for (int i = 0; i < n; ++i)
        for (int j = 0; j < n; ++j) T[(size_t)j * n + i] = A[(size_t)i * n + j];
    return T;
}
// DenseMatrix.mult(DenseMatrix): per element the chain over the inner index from 0.0
inline BpmfMat bpmf_mult(const BpmfMat &A, const BpmfMat &B, int n) {
    BpmfMat C((size_t)n * n);
    for (int i = 0; i < n; ++i)
        for (int j = 0; j < n; ++j) {
            double s = 0.0;
            for (int k = 0; k < n; ++k) s += A[(size_t)i * n + k] * B[(size_t)k * n + j];
            C[(size_t)i * n + j] = s;
        }
    return C;
}
// DenseMatrix.mult(DenseVector)
inline std::vector<double> bpmf_mult_vec(const BpmfMat &A, const std::vector<double> &y, int n) {
    std::vector<double> o((size_t)n);
    for (int i = 0; i < n; ++i) {
        double s = 0.0;
        for (int k = 0; k < n; ++k) s += A[(size_t)i * n + k] * y[(size_t)k];
        o[(size_t)i] = s;
    }
    return o;
}
inline BpmfMat bpmf_outer(const std::vector<double> &a, const std::vector<double> &b) {
    const size_t n = a.size();
    BpmfMat o(n * n);
    for (size_t i = 0; i < n; ++i)
        for (size_t j = 0; j < n; ++j) o[i * n + j] = a[i] * b[j];
    return o;
}
inline BpmfMat bpmf_scale(BpmfMat A, double v) {
    for (double &x : A) x = x * v;
    return A;
}
inline BpmfMat bpmf_add(BpmfMat A, const BpmfMat &B) {
    for (size_t e = 0; e < A.size(); ++e) A[e] = A[e] + B[e];
    return A;
}

// SparseVector.contains(key) of a vector that holds the indices 0 .. n - 1: Arrays.binarySearch over the whole index array, whose
// capacity is the next power of two and whose tail is zero
inline bool bpmf_sparse_contains(int n, int key) {
    int cap = n == 0 ? 0 : 1;
    while (cap < n) cap <<= 1;
    int low = 0, high = cap - 1;
    while (low <= high) {
        const int mid = (int)((unsigned)(low + high) >> 1), v = mid < n ? mid : 0;
        if (v < key) low = mid + 1;
        else if (v > key) high = mid - 1;
        else return true;
    }
    return false;
}

// BPMF.wishart(scale, df) (BPMF.java:258-313): false, and no draw, where scale.cholesky() is null.  z[k][c] is read as z[k * p + c]
inline bool bpmf_wishart(BpmfStream &r, const BpmfMat &scale, int p, double df, BpmfMat &out) {
    BpmfMat L;
    if (!bpmf_cholesky(scale, p, L)) return false;
    BpmfMat z((size_t)p * p);
    for (double &x : z) x = r.gaussian();
    std::vector<double> y((size_t)p);
    for (int i = 0; i < p; ++i) y[(size_t)i] = bpmf_gamma(r, (df - (i + 1)) / 2, 2.0);
    auto inner = [&](int n, int ca, int cb) { // SparseVector.inner over the column pieces z[0 .. n - 1][ca] and z[0 .. n - 1][cb]
        double s = 0.0;
        for (int k = 0; k < n; ++k)
            if (bpmf_sparse_contains(n, k)) s += z[(size_t)k * p + ca] * z[(size_t)k * p + cb];
        return s;
    };
    BpmfMat B((size_t)p * p, 0.0);
    B[0] = y[0];
    for (int j = 1; j < p; ++j) B[(size_t)j * p + j] = y[(size_t)j] + inner(j, j, j);
    for (int j = 1; j < p; ++j) B[(size_t)j] = B[(size_t)j * p] = z[(size_t)j] * std::sqrt(y[0]);
    for (int j = 2; j < p; ++j)
        for (int i = 1; i < j; ++i) B[(size_t)i * p + j] = B[(size_t)j * p + i] = z[(size_t)i * p + j] * std::sqrt(y[(size_t)i]) + inner(i, i, j);
    const BpmfMat A = bpmf_transpose(L, p); // scale.cholesky(): the upper factor
    out = bpmf_mult(bpmf_mult(L, B, p), A, p); // A.transpose().mult(B).mult(A)
    return true;
}

// BPMF.java:98-122 (users) or :125-149 (items) of one side with M rows: x_bar = columnMean, S_bar = cov(); alpha (k x k) and mu (k) in
// place.  mu0 = 0, b0 = 2, WI = eye, df = k.
inline void bpmf_hyper_side(BpmfStream &r, int k, int M, const std::vector<double> &x_bar, const BpmfMat &S_bar, BpmfMat &alpha,
                            std::vector<double> &mu) {
    const int b0 = 2;
    std::vector<double> d((size_t)k), mu_temp((size_t)k);
    for (int f = 0; f < k; ++f) d[(size_t)f] = 0.0 - x_bar[(size_t)f];
    BpmfMat eye((size_t)k * k, 0.0);
    for (int i = 0; i < k; ++i) eye[(size_t)i * k + i] = 1.0;
    const BpmfMat e = bpmf_scale(bpmf_outer(d, d), (double)(M * b0) / (b0 + M + 0.0));
    BpmfMat WI = bpmf_add(bpmf_add(bpmf_inv(eye, k), bpmf_scale(S_bar, (double)M)), e);
    WI = bpmf_inv(WI, k);
    WI = bpmf_scale(bpmf_add(WI, bpmf_transpose(WI, k)), 0.5);
    BpmfMat w;
    if (bpmf_wishart(r, WI, k, (double)(k + M), w)) alpha = w;
    for (int f = 0; f < k; ++f) mu_temp[(size_t)f] = (0.0 * (double)b0 + x_bar[(size_t)f] * (double)M) * (1 / (b0 + M + 0.0));
    BpmfMat L;
    if (bpmf_cholesky(bpmf_inv(bpmf_scale(alpha, (double)(b0 + M)), k), k, L)) {
        std::vector<double> zs((size_t)k);
        for (double &x : zs) x = r.gaussian();
        const std::vector<double> lz = bpmf_mult_vec(L, zs, k);
        for (int f = 0; f < k; ++f) mu[(size_t)f] = lz[(size_t)f] + mu_temp[(size_t)f];
    }
}

// DenseMatrix.columnMean / cov() on the host (bpmf_launch_moments on the device): mean[f] one chain over the rows over `rows`; cov from
// the columns less Stats.mean (which skips NaN entries), the inner product over rows - 1
inline void bpmf_moments_host(const double *X, int rows, int k, double *mean, double *cov) {
    std::vector<double> sm((size_t)k);
    for (int f = 0; f < k; ++f) {
        double s = 0.0, t = 0.0;
        int cnt = 0;
        for (int rw = 0; rw < rows; ++rw) {
            const double v = X[(size_t)rw * k + f];
            s += v;
            if (!std::isnan(v)) t += v, ++cnt;
        }
        mean[f] = s / (double)rows;
        sm[(size_t)f] = t / (double)cnt;
    }
    for (int f = 0; f < k; ++f)
        for (int g = 0; g < k; ++g) {
            double s = 0.0;
            for (int rw = 0; rw < rows; ++rw) s += (X[(size_t)rw * k + f] - sm[(size_t)f]) * (X[(size_t)rw * k + g] - sm[(size_t)g]);
            cov[(size_t)f * k + g] = s / (double)(rows - 1);
        }
}

// ---- the draws of a Gibbs pass ------------------------------------------------------------------------------------------------------
// The rows of a side that have entries, in order, are the pass's slots.  A slot whose posterior has no factor (null) takes no draw, so
// slot s's k draws start at k * (the slots before s that are not null).  The first launch takes slot s's draws at k * s: right for
// every slot up to the first null one.  The second pass reruns the non-null slots after it at their exact places.

// attempts of the polar method the device makes at first for `pairs` accepted ones (acceptance pi / 4, taken as 3 / 4); when fewer
// are accepted the generator goes on from where the attempts ended
inline int64_t bpmf_gauss_attempts(int64_t pairs) { return pairs + pairs / 3 + 3; }

struct BpmfRerun {
    std::vector<int32_t> slot, rank; // the slots to run again and the draw rank of each
    int64_t taken = 0;               // slots of the whole pass that take draws
};
// null[s] != 0: slot s has no factor.  Nothing to rerun (slot empty) when no slot is null.
inline BpmfRerun bpmf_rerun_plan(const std::vector<int32_t> &null) {
    BpmfRerun p;
    bool seen = false;
    int32_t rank = 0;
    for (size_t s = 0; s < null.size(); ++s) {
        if (null[s]) {
            seen = true;
            continue;
        }
        if (seen) p.slot.push_back((int32_t)s), p.rank.push_back(rank);
        ++rank;
    }
    p.taken = rank;
    return p;
}

} // namespace cmi
