// rankals_kernels.hip -- RankALS on gfx950: one iteration of RankALS.buildModel (the item moments, the P step, the item-independent sums
// of the Q step, the Q step), librec's DenseMatrix.inv() as one block-wide device routine, the prediction and the score slab.
// Everything is fp64 with the reference's operation order: every sum is one left-to-right chain from 0.0 with a rounding per multiply and
// per add (no FMA: -ffp-contract=off), and division is the correctly rounded IEEE operation Java uses.  Parallelism is taken across the
// INDEPENDENT elements only: the k or k x k elements of a sum, the users of the P step, the items of the Q step.  No sum is split, there
// are no atomics, and the same inputs give the same bits on every run.
#include "rankals_kernels.hpp"
#include "dense_invert.hpp"

namespace cmi {

namespace {

constexpr int RA_G = (RANKALS_MAX_K * RANKALS_MAX_K + RANKALS_BLOCK - 1) / RANKALS_BLOCK; // k x k elements a thread at most

// out[a] = the chain over b of inv[a][b] * y[b] (DenseMatrix.mult(DenseVector)), thread a
__device__ __forceinline__ double rankals_mult_row(const double *m, const double *y, int n, int a) {
    double s = 0.0;
    for (int b = 0; b < n; ++b) s += m[a * n + b] * y[b];
    return s;
}

} // namespace

// ---- the item moments --------------------------------------------------------------------------------------------------------------
// A thread per element of sum_sqq (k x k) and of sum_sq (k); the workgroup stages RANKALS_TILE rows of Q and their s in LDS, and every
// thread adds its element's terms in item order: (q[a] * q[b]) * s_j and q[a] * s_j.
__global__ __launch_bounds__(RANKALS_BLOCK) void rankals_item_moments_kernel(RankAlsState A) {
    __shared__ double s_q[RANKALS_TILE * RANKALS_MAX_K], s_s[RANKALS_TILE];
    const int k = A.k, kk = k * k, tid = threadIdx.x;
    const int e = (int)blockIdx.x * RANKALS_BLOCK + tid;
    const bool is_mat = e < kk, is_vec = !is_mat && e < kk + k;
    const int a = is_mat ? e / k : (is_vec ? e - kk : 0), b = is_mat ? e % k : 0;
    double acc = 0.0;
    for (int j0 = 0; j0 < A.n_items; j0 += RANKALS_TILE) {
        const int cnt = min(RANKALS_TILE, A.n_items - j0);
        __syncthreads();
        for (int t = tid; t < cnt * k; t += RANKALS_BLOCK) s_q[t] = A.Q[(int64_t)j0 * k + t];
        if (tid < cnt) s_s[tid] = A.s[j0 + tid];
        __syncthreads();
        if (is_mat)
            for (int t = 0; t < cnt; ++t) acc += (s_q[t * k + a] * s_q[t * k + b]) * s_s[t];
        else if (is_vec)
            for (int t = 0; t < cnt; ++t) acc += s_q[t * k + a] * s_s[t];
    }
    if (is_mat) A.sum_sqq[e] = acc;
    else if (is_vec) A.sum_sq[a] = acc;
}

hipError_t rankals_launch_item_moments(const RankAlsState &a, hipStream_t s) {
    const int n = a.k * a.k + a.k;
    rankals_item_moments_kernel<<<dim3((unsigned)((n + RANKALS_BLOCK - 1) / RANKALS_BLOCK)), dim3(RANKALS_BLOCK), 0, s>>>(a);
    return hipGetLastError();
}

// ---- the P step ----------------------------------------------------------------------------------------------------------------------
// LDS of a solve, in doubles: mat (k^2) | I (stage >= k^2; the solves stage the rows of a chunk there before I exists) | `vecs` vectors
// of k | `arrays` arrays of RANKALS_CHUNK (the staged entries' scalars).  The user solve has 4 vectors (sum_cq, sum_sq, y, the
// inversion's f) and 2 arrays (r, s * r); the item solve 2 vectors (y, f) and 3 arrays (r, m_sum_sr, r * m_sum_c).
static size_t rankals_solve_lds(int k, int stage, int vecs, int arrays) {
    return ((size_t)k * k + stage + vecs * k + arrays * RANKALS_CHUNK) * sizeof(double);
}

// A workgroup per user of rows().  The row's entries are staged a chunk at a time (their Q rows, r_ui and s_i * r_ui); a thread keeps up
// to RA_G elements of sum_cqq in registers and, below k, its elements of sum_cq, sum_cqr and sum_sqr; sum_sr and sum_cr are formed by
// every thread alike.  Each is one chain over the row's entries in order.  M goes to LDS element by element in the written order of
// scale / minus / minus / add, y likewise; then the inversion and the ordered mult.  The same launch leaves step 3's m_* values (the
// same chains: Q does not change between the P step and step 3) and pp.mult(m_sum_cq[u]) of the new row, which the Q step adds per user.
__global__ __launch_bounds__(RANKALS_BLOCK) void rankals_user_kernel(RankAlsState A, int stage) {
    extern __shared__ double lds[];
    const int k = A.k, kk = k * k, tid = threadIdx.x;
    double *mat = lds, *inv = lds + kk, *v_cq = inv + stage, *v_sq = v_cq + k, *v_y = v_sq + k, *v_f = v_y + k, *c_r = v_f + k,
           *c_w = c_r + RANKALS_CHUNK;
    const int u = A.users[blockIdx.x];
    const int e0 = A.rows.ptr[u], e1 = A.rows.ptr[u + 1];
    const int per = min(RANKALS_CHUNK, stage / k);
    const int ng = (kk + RANKALS_BLOCK - 1) / RANKALS_BLOCK;
    double acc[RA_G];
    int ea[RA_G], eb[RA_G];
#pragma unroll
    for (int g = 0; g < RA_G; ++g) {
        const int e = tid + RANKALS_BLOCK * g;
        acc[g] = 0.0;
        ea[g] = e < kk ? e / k : 0, eb[g] = e < kk ? e % k : 0;
    }
    double cq = 0.0, cqr = 0.0, sqr = 0.0, sum_sr = 0.0, sum_cr = 0.0;
    for (int base = e0; base < e1; base += per) {
        const int cnt = min(per, e1 - base);
        __syncthreads();
        for (int t = tid; t < cnt * k; t += RANKALS_BLOCK) {
            const int e = t / k;
            inv[t] = A.Q[(int64_t)A.rows.idx[base + e] * k + (t - e * k)];
        }
        if (tid < cnt) {
            const double r = A.rows.val[base + tid];
            c_r[tid] = r;
            c_w[tid] = A.s[A.rows.idx[base + tid]] * r;
        }
        __syncthreads();
        for (int e = 0; e < cnt; ++e) {
            const double *q = inv + e * k;
#pragma unroll
            for (int g = 0; g < RA_G; ++g)
                if (g < ng) acc[g] += q[ea[g]] * q[eb[g]];
            const double r = c_r[e], w = c_w[e];
            if (tid < k) {
                const double qa = q[tid];
                cq += qa;
                cqr += qa * r;
                sqr += qa * w;
            }
            sum_sr += w;
            sum_cr += r;
        }
    }
    __syncthreads();
    if (tid < k) v_cq[tid] = cq, v_sq[tid] = A.sum_sq[tid];
    __syncthreads();
    const double sum_c = (double)(e1 - e0), sum_s = A.sum_s;
#pragma unroll
    for (int g = 0; g < RA_G; ++g) {
        const int e = tid + RANKALS_BLOCK * g;
        if (e < kk) mat[e] = ((acc[g] * sum_s - v_cq[ea[g]] * v_sq[eb[g]]) - v_sq[ea[g]] * v_cq[eb[g]]) + A.sum_sqq[e] * sum_c;
    }
    if (tid < k) {
        v_y[tid] = ((cqr * sum_s - cq * sum_sr) - v_sq[tid] * sum_cr) + sqr * sum_c;
        A.m_cq[(int64_t)u * k + tid] = cq;
    }
    if (tid == 0) A.m_sr[u] = sum_sr, A.m_cr[u] = sum_cr, A.m_c[u] = sum_c;
    __syncthreads();
    rankals_invert(mat, inv, v_f, k);
    if (tid < k) {
        const double p = rankals_mult_row(inv, v_y, k, tid);
        A.P[(int64_t)u * k + tid] = p;
        mat[tid] = p; // mat is free now
    }
    __syncthreads();
    if (tid < k) {
        const double pa = mat[tid];
        double t = 0.0;
        for (int b = 0; b < k; ++b) t += (pa * mat[b]) * v_cq[b];
        A.ppcq_u[(int64_t)u * k + tid] = t;
    }
}

hipError_t rankals_launch_user_solve(const RankAlsState &a, hipStream_t s) {
    if (a.n_rows <= 0) return hipSuccess;
    const int stage = a.k * a.k > RANKALS_STAGE_MIN ? a.k * a.k : RANKALS_STAGE_MIN;
    const size_t lds = rankals_solve_lds(a.k, stage, 4, 2);
    if (lds > 64 * 1024)
        (void)hipFuncSetAttribute(reinterpret_cast<const void *>(rankals_user_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    rankals_user_kernel<<<dim3((unsigned)a.n_rows), dim3(RANKALS_BLOCK), lds, s>>>(a, stage);
    return hipGetLastError();
}

// ---- the item-independent sums of the Q step -----------------------------------------------------------------------------------------
// For every item the reference adds, over the users of rows() in order, pp, pp.scale(m_sum_c[u]), pp.mult(m_sum_cq[u]) and
// pu.scale(m_sum_cr[u]): none of the terms reads the item, so the four sums are the same chains for every item.  Here each element is
// formed once: a thread per element of the two matrices (one product pu[a] * pu[b] serves both) and per element of the two vectors, the
// workgroup staging RANKALS_TILE users a pass.
__global__ __launch_bounds__(RANKALS_BLOCK) void rankals_user_moments_kernel(RankAlsState A) {
    __shared__ double s_p[RANKALS_TILE * RANKALS_MAX_K], s_t[RANKALS_TILE * RANKALS_MAX_K], s_c[RANKALS_TILE], s_cr[RANKALS_TILE];
    const int k = A.k, kk = k * k, tid = threadIdx.x;
    const int e = (int)blockIdx.x * RANKALS_BLOCK + tid;
    const bool is_mat = e < kk, is_vec = !is_mat && e < kk + k;
    const int a = is_mat ? e / k : (is_vec ? e - kk : 0), b = is_mat ? e % k : 0;
    double acc0 = 0.0, acc1 = 0.0; // matrix thread: cpp, ppc; vector thread: ppcq, crp
    for (int t0 = 0; t0 < A.n_rows; t0 += RANKALS_TILE) {
        const int cnt = min(RANKALS_TILE, A.n_rows - t0);
        __syncthreads();
        for (int t = tid; t < cnt * k; t += RANKALS_BLOCK) {
            const int x = t / k;
            const int64_t at = (int64_t)A.users[t0 + x] * k + (t - x * k);
            s_p[t] = A.P[at], s_t[t] = A.ppcq_u[at];
        }
        if (tid < cnt) s_c[tid] = A.m_c[A.users[t0 + tid]], s_cr[tid] = A.m_cr[A.users[t0 + tid]];
        __syncthreads();
        if (is_mat)
            for (int t = 0; t < cnt; ++t) {
                const double pp = s_p[t * k + a] * s_p[t * k + b];
                acc0 += pp;
                acc1 += pp * s_c[t];
            }
        else if (is_vec)
            for (int t = 0; t < cnt; ++t) {
                acc0 += s_t[t * k + a];
                acc1 += s_p[t * k + a] * s_cr[t];
            }
    }
    if (is_mat) A.cpp[e] = acc0, A.ppc[e] = acc1;
    else if (is_vec) A.ppcq[a] = acc0, A.crp[a] = acc1;
}

hipError_t rankals_launch_user_moments(const RankAlsState &a, hipStream_t s) {
    const int n = a.k * a.k + a.k;
    rankals_user_moments_kernel<<<dim3((unsigned)((n + RANKALS_BLOCK - 1) / RANKALS_BLOCK)), dim3(RANKALS_BLOCK), 0, s>>>(a);
    return hipGetLastError();
}

// ---- the Q step ----------------------------------------------------------------------------------------------------------------------
// A workgroup per item.  Thread a < k forms its elements of sum_cpr, sum_c_sr_p and sum_p_r_c over the item's column, users ascending
// (the order of rows()), taking the cells with a value > 0 (train.get(u, i) > 0; a stored zero is not in the column at all).  The
// column is staged a chunk at a time: the raters' values and m_* values, and their rows of P, loaded by the whole workgroup into the room
// I takes later, so the loads of a chunk are in flight together and the chains read LDS.  Then M, y, the inversion and the ordered mult.
__global__ __launch_bounds__(RANKALS_BLOCK) void rankals_item_kernel(RankAlsState A, int stage) {
    extern __shared__ double lds[];
    const int k = A.k, kk = k * k, tid = threadIdx.x;
    double *mat = lds, *inv = lds + kk, *v_y = inv + stage, *v_f = v_y + k, *c_r = v_f + k, *c_sr = c_r + RANKALS_CHUNK,
           *c_rc = c_sr + RANKALS_CHUNK;
    const int i = blockIdx.x;
    const int e0 = A.cols.ptr[i], e1 = A.cols.ptr[i + 1];
    const int per = min(RANKALS_CHUNK, stage / k);
    double cpr = 0.0, csrp = 0.0, prc = 0.0;
    for (int base = e0; base < e1; base += per) {
        const int cnt = min(per, e1 - base);
        __syncthreads();
        if (tid < cnt) {
            const int u = A.cols.idx[base + tid];
            const double r = A.cols.val[base + tid];
            c_r[tid] = r, c_sr[tid] = A.m_sr[u], c_rc[tid] = r * A.m_c[u];
        }
        for (int t = tid; t < cnt * k; t += RANKALS_BLOCK) {
            const int e = t / k;
            inv[t] = A.P[(int64_t)A.cols.idx[base + e] * k + (t - e * k)];
        }
        __syncthreads();
        if (tid < k)
            for (int e = 0; e < cnt; ++e) {
                const double r = c_r[e];
                if (r > 0) {
                    const double pa = inv[e * k + tid];
                    cpr += pa * r;
                    csrp += pa * c_sr[e];
                    prc += pa * c_rc[e];
                }
            }
    }
    __syncthreads(); // the last chunk's rows are read before I is written
    const double si = A.s[i], sum_s = A.sum_s;
    for (int e = tid; e < kk; e += RANKALS_BLOCK) mat[e] = A.cpp[e] * sum_s + A.ppc[e] * si;
    if (tid < k) {
        const double t = rankals_mult_row(A.cpp, A.sum_sq, k, tid);
        v_y[tid] = ((((t + cpr * sum_s) - csrp) + A.ppcq[tid] * si) - A.crp[tid] * si) + prc * si;
    }
    __syncthreads();
    rankals_invert(mat, inv, v_f, k);
    if (tid < k) A.Q[(int64_t)i * k + tid] = rankals_mult_row(inv, v_y, k, tid);
}

hipError_t rankals_launch_item_solve(const RankAlsState &a, hipStream_t s) {
    if (a.n_items <= 0) return hipSuccess;
    const int stage = a.k * a.k > RANKALS_STAGE_MIN ? a.k * a.k : RANKALS_STAGE_MIN;
    const size_t lds = rankals_solve_lds(a.k, stage, 2, 3);
    if (lds > 64 * 1024)
        (void)hipFuncSetAttribute(reinterpret_cast<const void *>(rankals_item_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    rankals_item_kernel<<<dim3((unsigned)a.n_items), dim3(RANKALS_BLOCK), lds, s>>>(a, stage);
    return hipGetLastError();
}

// ---- the inversion alone -------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(RANKALS_BLOCK) void rankals_invert_kernel(const double *A, double *out, int n) {
    extern __shared__ double lds[];
    double *mat = lds, *inv = lds + n * n, *fv = inv + n * n;
    const double *src = A + (int64_t)blockIdx.x * n * n;
    for (int e = threadIdx.x; e < n * n; e += RANKALS_BLOCK) mat[e] = src[e];
    __syncthreads();
    rankals_invert(mat, inv, fv, n);
    double *dst = out + (int64_t)blockIdx.x * n * n;
    for (int e = threadIdx.x; e < n * n; e += RANKALS_BLOCK) dst[e] = inv[e];
}

hipError_t rankals_launch_invert(const double *A, double *out, int n_mats, int n, hipStream_t s) {
    if (n_mats <= 0) return hipSuccess;
    if (n < 1 || n > RANKALS_MAX_K) return hipErrorInvalidValue;
    const size_t lds = ((size_t)2 * n * n + n) * sizeof(double);
    if (lds > 64 * 1024)
        (void)hipFuncSetAttribute(reinterpret_cast<const void *>(rankals_invert_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    rankals_invert_kernel<<<dim3((unsigned)n_mats), dim3(RANKALS_BLOCK), lds, s>>>(A, out, n);
    return hipGetLastError();
}

// ---- prediction and scores -------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(RANKALS_BLOCK) void rankals_predict_kernel(const double *P, const double *Q, int k, int64_t n, const int32_t *tu,
                                                                        const int32_t *tj, double *out) {
    const int64_t t = (int64_t)blockIdx.x * RANKALS_BLOCK + threadIdx.x;
    if (t >= n) return;
    const double *pp = P + (int64_t)tu[t] * k, *qp = Q + (int64_t)tj[t] * k;
    double pred = 0.0;
    for (int f = 0; f < k; ++f) pred += pp[f] * qp[f];
    out[t] = pred;
}

hipError_t rankals_launch_predict(const double *P, const double *Q, int k, int64_t n, const int32_t *u, const int32_t *j, double *out,
                                  hipStream_t s) {
    if (n <= 0) return hipSuccess;
    rankals_predict_kernel<<<dim3((unsigned)((n + RANKALS_BLOCK - 1) / RANKALS_BLOCK)), dim3(RANKALS_BLOCK), 0, s>>>(P, Q, k, n, u, j, out);
    return hipGetLastError();
}

// A workgroup per (group of queries of one user, block of RANKALS_BLOCK candidates): the user's row of P in LDS, a lane per candidate with
// its own chain over f, the score written to every query of the group inside [q0, q0 + nq).  BPR, LRMF and RankSGD fill their slabs with
// it too, so the row has RANK_SCORE_MAX_K doubles, not RANKALS_MAX_K, and is staged by a strided loop that holds for any k up to that.
__global__ __launch_bounds__(RANKALS_BLOCK) void rankals_score_kernel(const double *P, const double *Q, int k, const int32_t *cand, int nc,
                                                                      const int32_t *gu, const int32_t *gq0, int g0, int64_t q0, int64_t nq,
                                                                      double *S) {
    __shared__ double s_p[RANK_SCORE_MAX_K];
    const int g = g0 + (int)blockIdx.x;
    const int u = gu[g];
    for (int f = (int)threadIdx.x; f < k; f += RANKALS_BLOCK) s_p[f] = P[(int64_t)u * k + f];
    __syncthreads();
    const int c = (int)blockIdx.y * RANKALS_BLOCK + (int)threadIdx.x;
    if (c >= nc) return;
    const double *qp = Q + (int64_t)cand[c] * k;
    double pred = 0.0;
    for (int f = 0; f < k; ++f) pred += s_p[f] * qp[f];
    const int64_t qa = max((int64_t)gq0[g], q0), qb = min((int64_t)gq0[g + 1], q0 + nq);
    for (int64_t q = qa; q < qb; ++q) S[(size_t)(q - q0) * (size_t)nc + (size_t)c] = pred;
}

hipError_t rankals_launch_score(const double *P, const double *Q, int k, const int32_t *cand, int nc, const int32_t *gu, const int32_t *gq0,
                                int g0, int g1, int64_t q0, int64_t nq, double *S, hipStream_t s) {
    if (k < 1 || k > RANK_SCORE_MAX_K) return hipErrorInvalidValue; // the row of P would not fit the kernel's LDS array
    if (g1 <= g0 || nc <= 0 || nq <= 0) return hipSuccess;
    const dim3 grid((unsigned)(g1 - g0), (unsigned)((nc + RANKALS_BLOCK - 1) / RANKALS_BLOCK));
    rankals_score_kernel<<<grid, dim3(RANKALS_BLOCK), 0, s>>>(P, Q, k, cand, nc, gu, gq0, g0, q0, nq, S);
    return hipGetLastError();
}

} // namespace cmi
