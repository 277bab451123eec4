// bpmf_kernels.hip -- BPMF on gfx950: java.util.Random.nextGaussian() as a parallel stream, DenseMatrix.columnMean / cov(), one Gibbs
// pass of one side (the row posterior: Gram matrix, librec's inv(), the mean, DenseMatrix.cholesky() and the draw), the loss and the
// prediction.  Everything is fp64 with the reference's operation order: every sum is one left-to-right chain from 0.0 with a rounding
// per multiply and per add (no FMA: -ffp-contract=off); division and square root are the correctly rounded IEEE operations Java uses.
// Parallelism is taken across the INDEPENDENT elements only: the attempts of the polar method, the k x k elements of a sum or of a
// factor's column, the rows of a side.  No sum is split (but the loss above 2^18 terms, on request), and the same inputs give the same
// bits on every run.
#include "bpmf_kernels.hpp"
#include "dense_invert.hpp"
#include "eval_device.hpp"

namespace cmi {

namespace {

constexpr int BP_G = (BPMF_MAX_K * BPMF_MAX_K + BPMF_BLOCK - 1) / BPMF_BLOCK; // k x k elements a thread at most

// attempt t of the run that starts at state0: v1, v2 uniform in (-1, 1) from two nextDouble() each (4 LCG steps); accepted when
// 0 < s < 1.  With `values` the pair v * StrictMath.sqrt(-2 * StrictMath.log(s) / s)
__device__ __forceinline__ bool bpmf_attempt(const JavaLcgJump &J, uint64_t state0, int64_t t, bool values, double &g1, double &g2) {
    JavaStream r{java_lcg_jump(J, state0, (uint64_t)t * 4u), 0};
    const double v1 = 2.0 * r.nextDouble() - 1.0;
    const double v2 = 2.0 * r.nextDouble() - 1.0;
    const double s = v1 * v1 + v2 * v2;
    const bool ok = s < 1.0 && s != 0.0;
    if (ok && values) {
        const double m = __dsqrt_rn(-2.0 * fdlibm_log(s) / s);
        g1 = v1 * m, g2 = v2 * m;
    }
    return ok;
}

__device__ __forceinline__ double bpmf_lane_d(double v, int l) {
    const int lo = __builtin_amdgcn_readlane(__double2loint(v), l), hi = __builtin_amdgcn_readlane(__double2hiint(v), l);
    return __hiloint2double(hi, lo);
}

} // namespace

// ---- the gaussian stream ----------------------------------------------------------------------------------------------------------------
// 1. a lane per attempt: the workgroup's number of accepted attempts
__global__ __launch_bounds__(BPMF_GAUSS_BLOCK) void bpmf_gauss_count_kernel(uint64_t state0, JavaLcgJump J, int64_t t0, int64_t n_att,
                                                                            int32_t *block_cnt) {
    const int64_t t = (int64_t)blockIdx.x * BPMF_GAUSS_BLOCK + threadIdx.x;
    double g1, g2;
    const int ok = t < n_att && bpmf_attempt(J, state0, t0 + t, false, g1, g2);
    const int cnt = __syncthreads_count(ok);
    if (threadIdx.x == 0) block_cnt[blockIdx.x] = cnt;
}

// 2. one workgroup: the exclusive prefix sum of the workgroups' counts, BPMF_GAUSS_BLOCK of them a pass, the total carried on
__global__ __launch_bounds__(BPMF_GAUSS_BLOCK) void bpmf_gauss_scan_kernel(const int32_t *block_cnt, int32_t *block_off, int64_t n_blocks,
                                                                           BpmfGaussTail *tail, double *out, int write_lead,
                                                                           double lead_value) {
    __shared__ int32_t s_wave[BPMF_GAUSS_BLOCK / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int64_t carry = 0;
    for (int64_t base = 0; base < n_blocks; base += BPMF_GAUSS_BLOCK) {
        const int32_t v = base + tid < n_blocks ? block_cnt[base + tid] : 0;
        int32_t incl = v;
        for (int off = 1; off < 64; off <<= 1) {
            const int32_t up = __shfl_up(incl, off);
            if (lane >= off) incl += up;
        }
        __syncthreads(); // the last pass's reads of s_wave
        if (lane == 63) s_wave[wave] = incl;
        __syncthreads();
        int32_t before = 0, total = 0;
        for (int w = 0; w < BPMF_GAUSS_BLOCK / 64; ++w) {
            if (w < wave) before += s_wave[w];
            total += s_wave[w];
        }
        if (base + tid < n_blocks) block_off[base + tid] = (int32_t)(carry + before + incl - v);
        carry += total;
    }
    if (tid == 0) {
        tail->accepted = carry, tail->last_t = -1, tail->cached = 0.0, tail->have = 0, tail->pad = 0;
        if (write_lead) out[0] = lead_value;
    }
}

// 3. a lane per attempt again: an accepted attempt's pair number from the workgroup's offset and the lanes before it; the pairs below
//    `need` are formed and written
__global__ __launch_bounds__(BPMF_GAUSS_BLOCK) void bpmf_gauss_emit_kernel(uint64_t state0, JavaLcgJump J, int64_t t0, int64_t n_att,
                                                                           int64_t pair0, int64_t need, int lead, int64_t n,
                                                                           const int32_t *block_off, double *out, BpmfGaussTail *tail) {
    __shared__ int32_t s_wave[BPMF_GAUSS_BLOCK / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t t = (int64_t)blockIdx.x * BPMF_GAUSS_BLOCK + tid;
    double g1 = 0.0, g2 = 0.0;
    const bool ok = t < n_att && bpmf_attempt(J, state0, t0 + t, false, g1, g2);
    const unsigned long long mask = __ballot(ok);
    if (lane == 0) s_wave[wave] = __popcll(mask);
    __syncthreads();
    if (!ok) return;
    int64_t p = pair0 + block_off[blockIdx.x] + __popcll(mask & ((1ull << lane) - 1ull));
    for (int w = 0; w < wave; ++w) p += s_wave[w];
    if (p >= need) return;
    (void)bpmf_attempt(J, state0, t0 + t, true, g1, g2);
    const int64_t at = lead + 2 * p;
    out[at] = g1;
    if (at + 1 < n) out[at + 1] = g2;
    if (p == need - 1) tail->last_t = t0 + t, tail->cached = g2, tail->have = at + 1 < n ? 0 : 1;
}

hipError_t bpmf_launch_gauss_round(uint64_t state0, const JavaLcgJump &jump, int64_t t0, int64_t n_att, int64_t pair0, int64_t need,
                                   int lead, double lead_value, int64_t n, double *out, int32_t *block_cnt, int32_t *block_off,
                                   BpmfGaussTail *tail, hipStream_t s) {
    if (n_att <= 0 || n_att > ((int64_t)1 << 30)) return hipErrorInvalidValue;
    const int64_t nb = (n_att + BPMF_GAUSS_BLOCK - 1) / BPMF_GAUSS_BLOCK;
    bpmf_gauss_count_kernel<<<dim3((unsigned)nb), dim3(BPMF_GAUSS_BLOCK), 0, s>>>(state0, jump, t0, n_att, block_cnt);
    bpmf_gauss_scan_kernel<<<1, BPMF_GAUSS_BLOCK, 0, s>>>(block_cnt, block_off, nb, tail, out, lead && t0 == 0 ? 1 : 0, lead_value);
    bpmf_gauss_emit_kernel<<<dim3((unsigned)nb), dim3(BPMF_GAUSS_BLOCK), 0, s>>>(state0, jump, t0, n_att, pair0, need, lead, n, block_off, out,
                                                                                 tail);
    return hipGetLastError();
}

// ---- columnMean and cov() ------------------------------------------------------------------------------------------------------------
// a lane per column f; the workgroup stages BPMF_TILE rows a pass.  sum: every entry (columnMean); t / cnt: the entries that are no NaN
// (Stats.mean)
__global__ __launch_bounds__(BPMF_BLOCK) void bpmf_colmean_kernel(const double *X, int rows, int k, double *mean, double *smean) {
    __shared__ double s_x[BPMF_TILE * BPMF_MAX_K];
    const int tid = threadIdx.x;
    double sum = 0.0, t = 0.0;
    int cnt = 0;
    for (int r0 = 0; r0 < rows; r0 += BPMF_TILE) {
        const int n = min(BPMF_TILE, rows - r0);
        __syncthreads();
        for (int e = tid; e < n * k; e += BPMF_BLOCK) s_x[e] = X[(int64_t)r0 * k + e];
        __syncthreads();
        if (tid < k)
            for (int r = 0; r < n; ++r) {
                const double v = s_x[r * k + tid];
                sum += v;
                if (!isnan(v)) t += v, ++cnt;
            }
    }
    if (tid < k) mean[tid] = sum / (double)rows, smean[tid] = t / (double)cnt;
}

// a lane per (f, g); one chain over the rows, staged BPMF_TILE a pass (as rankals_item_moments_kernel does)
__global__ __launch_bounds__(BPMF_BLOCK) void bpmf_cov_kernel(const double *X, int rows, int k, const double *smean, double *cov) {
    __shared__ double s_x[BPMF_TILE * BPMF_MAX_K];
    const int tid = threadIdx.x, kk = k * k;
    const int e = (int)blockIdx.x * BPMF_BLOCK + tid;
    const bool live = e < kk;
    const int f = live ? e / k : 0, g = live ? e % k : 0;
    const double mf = smean[f], mg = smean[g];
    double acc = 0.0;
    for (int r0 = 0; r0 < rows; r0 += BPMF_TILE) {
        const int n = min(BPMF_TILE, rows - r0);
        __syncthreads();
        for (int t = tid; t < n * k; t += BPMF_BLOCK) s_x[t] = X[(int64_t)r0 * k + t];
        __syncthreads();
        if (live)
            for (int r = 0; r < n; ++r) acc += (s_x[r * k + f] - mf) * (s_x[r * k + g] - mg);
    }
    if (live) cov[e] = acc / (double)(rows - 1);
}

hipError_t bpmf_launch_moments(const double *X, int rows, int k, double *mean, double *smean, double *cov, hipStream_t s) {
    if (rows < 1 || k < 1 || k > BPMF_MAX_K) return hipErrorInvalidValue;
    bpmf_colmean_kernel<<<1, BPMF_BLOCK, 0, s>>>(X, rows, k, mean, smean);
    bpmf_cov_kernel<<<dim3((unsigned)((k * k + BPMF_BLOCK - 1) / BPMF_BLOCK)), dim3(BPMF_BLOCK), 0, s>>>(X, rows, k, smean, cov);
    return hipGetLastError();
}

// ---- the row posterior ----------------------------------------------------------------------------------------------------------------
// LDS, in doubles: mat (k^2) | covar (stage >= k^2; the chunk's partner rows are staged there before covar exists) | y | f | mean | z
// (k each) | r (BPMF_CHUNK).
static size_t bpmf_row_lds(int k, int stage) { return ((size_t)k * k + stage + 4 * k + BPMF_CHUNK) * sizeof(double); }

// A workgroup per row of the side (a slot of the pass).  The row's entries are staged a chunk at a time (the partners' rows and
// r - globalMean); a thread keeps up to BP_G elements of the Gram matrix MM^T MM in registers and, below k, its element of MM^T rr:
// each one chain over the row's entries in order.  Then, all in LDS:
//   mat = alpha + G * beta;  covar = mat.inv() (rankals_invert);  y = MM^T rr * beta + alpha.mult(mu);  mean = covar.mult(y);
//   the factor of covar by DenseMatrix.cholesky()'s rules, column by column: when column c is final, every later element (i, j),
//   c < j <= i, takes its term L[i][c] * L[j][c] -- each element's terms arrive in the order of c, its own chain -- and a NaN diagonal
//   is the reference's null;  the row = lam^T.mult(z) + mean (the factor's zeros above the diagonal add +-0.0 to a sum that is never
//   -0.0: they are left out).
// A null row is not written and its flag is set.
__global__ __launch_bounds__(BPMF_BLOCK) void bpmf_row_kernel(BpmfRowArgs A, int stage) {
    extern __shared__ double lds[];
    const int k = A.k, kk = k * k, tid = threadIdx.x;
    double *mat = lds, *cov = lds + kk, *v_y = cov + stage, *v_f = v_y + k, *v_mean = v_f + k, *v_z = v_mean + k, *c_r = v_z + k;
    const int slot = A.slots ? A.slots[blockIdx.x] : (int)blockIdx.x;
    const int64_t rank = A.rank ? A.rank[blockIdx.x] : slot;
    const int row = A.rows[slot];
    const int e0 = A.C.ptr[row], e1 = A.C.ptr[row + 1];
    const int per = min(BPMF_CHUNK, stage / k);
    const int ng = (kk + BPMF_BLOCK - 1) / BPMF_BLOCK;
    double acc[BP_G];
    int ea[BP_G], eb[BP_G];
#pragma unroll
    for (int g = 0; g < BP_G; ++g) {
        const int e = tid + BPMF_BLOCK * g;
        acc[g] = 0.0;
        ea[g] = e < kk ? e / k : 0, eb[g] = e < kk ? e % k : 0;
    }
    double mr = 0.0;
    for (int base = e0; base < e1; base += per) {
        const int cnt = min(per, e1 - base);
        __syncthreads();
        for (int t = tid; t < cnt * k; t += BPMF_BLOCK) {
            const int e = t / k;
            cov[t] = A.other[(int64_t)A.C.idx[base + e] * k + (t - e * k)];
        }
        if (tid < cnt) c_r[tid] = A.C.val[base + tid] - A.gm;
        __syncthreads();
        for (int e = 0; e < cnt; ++e) {
            const double *q = cov + e * k;
#pragma unroll
            for (int g = 0; g < BP_G; ++g)
                if (g < ng) acc[g] += q[ea[g]] * q[eb[g]];
            if (tid < k) mr += q[tid] * c_r[e];
        }
    }
    __syncthreads();
#pragma unroll
    for (int g = 0; g < BP_G; ++g) {
        const int e = tid + BPMF_BLOCK * g;
        if (e < kk) mat[e] = A.alpha[e] + acc[g] * 2.0;
    }
    if (tid < k) {
        double b = 0.0;
        for (int c = 0; c < k; ++c) b += A.alpha[tid * k + c] * A.mu[c];
        v_y[tid] = mr * 2.0 + b;
        v_z[tid] = A.Z[rank * k + tid];
    }
    __syncthreads();
    rankals_invert(mat, cov, v_f, k);
    if (tid < k) {
        double m = 0.0;
        for (int b = 0; b < k; ++b) m += cov[tid * k + b] * v_y[b];
        v_mean[tid] = m;
    }
    for (int e = tid; e < kk; e += BPMF_BLOCK) mat[e] = 0.0; // the running sums of the factor's elements, then the elements
    __syncthreads();
    bool null = false;
    for (int c = 0; c < k; ++c) {
        const double d = __dsqrt_rn(cov[c * k + c] - mat[c * k + c]);
        if (isnan(d)) { // the same for every thread: all read the same two words
            null = true;
            break;
        }
        __syncthreads();
        if (tid >= c && tid < k) mat[tid * k + c] = tid == c ? d : (cov[tid * k + c] - mat[tid * k + c]) / d;
        __syncthreads();
        for (int e = (c + 1) * k + tid; e < kk; e += BPMF_BLOCK) {
            const int i = e / k, j = e - i * k;
            if (j > c && j <= i) mat[e] += mat[i * k + c] * mat[j * k + c];
        }
        __syncthreads();
    }
    if (tid == 0) {
        A.null_flag[slot] = null ? 1 : 0;
        if (null) atomicMin(A.first_null, slot);
    }
    if (null || tid >= k) return;
    double s = 0.0;
    for (int b = 0; b <= tid; ++b) s += mat[tid * k + b] * v_z[b];
    A.own[(int64_t)row * k + tid] = s + v_mean[tid];
}

hipError_t bpmf_launch_rows(const BpmfRowArgs &a, hipStream_t s) {
    if (a.n <= 0) return hipSuccess;
    if (a.k < 1 || a.k > BPMF_MAX_K) return hipErrorInvalidValue;
    const int stage = a.k * a.k > BPMF_STAGE_MIN ? a.k * a.k : BPMF_STAGE_MIN;
    const size_t lds = bpmf_row_lds(a.k, stage);
    if (lds > 64 * 1024)
        (void)hipFuncSetAttribute(reinterpret_cast<const void *>(bpmf_row_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    bpmf_row_kernel<<<dim3((unsigned)a.n), dim3(BPMF_BLOCK), lds, s>>>(a, stage);
    return hipGetLastError();
}

// ---- loss ------------------------------------------------------------------------------------------------------------------------
// a lane per stored cell: (r - predict(u, j))^2
__global__ __launch_bounds__(BPMF_BLOCK) void bpmf_loss_term_kernel(const double *P, const double *Q, PairCsr R, const int32_t *cu, int64_t n,
                                                                    int k, double gm, double *term) {
    const int64_t q = (int64_t)blockIdx.x * BPMF_BLOCK + threadIdx.x;
    if (q >= n) return;
    const double *pp = P + (int64_t)cu[q] * k, *qp = Q + (int64_t)R.idx[q] * k;
    double dot = 0.0;
    for (int f = 0; f < k; ++f) dot += pp[f] * qp[f];
    const double e = R.val[q] - (gm + dot);
    term[q] = e * e;
}

// a workgroup's 256 terms in a fixed tree (shuffles inside a wave, then the four waves in order)
__global__ __launch_bounds__(BPMF_BLOCK) void bpmf_loss_tree_kernel(const double *term, int64_t n, double *part) {
    __shared__ double s_wave[BPMF_BLOCK / 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t q = (int64_t)blockIdx.x * BPMF_BLOCK + threadIdx.x;
    double t = q < n ? term[q] : 0.0;
    for (int off = 32; off; off >>= 1) t += __shfl_down(t, off);
    if (lane == 0) s_wave[wave] = t;
    __syncthreads();
    if (threadIdx.x == 0) part[blockIdx.x] = ((s_wave[0] + s_wave[1]) + s_wave[2]) + s_wave[3];
}

// one wave: the n values in one chain in order, 64 a load; the loss is half the sum
__global__ __launch_bounds__(64) void bpmf_loss_chain_kernel(const double *v, int64_t n, double *loss) {
    const int lane = threadIdx.x;
    double s = 0.0;
    double next = lane < n ? v[lane] : 0.0;
    for (int64_t base = 0; base < n; base += 64) {
        const double cur = next;
        const int64_t p = base + 64 + lane;
        next = p < n ? v[p] : 0.0;
        const int cnt = (int)min<int64_t>(64, n - base);
        for (int l = 0; l < cnt; ++l) s += bpmf_lane_d(cur, l);
    }
    if (lane == 0) *loss = s * 0.5;
}

hipError_t bpmf_launch_loss(const double *P, const double *Q, PairCsr R, const int32_t *cu, int64_t n, int k, double gm, bool strict,
                            double *term, double *part, double *loss, hipStream_t s) {
    const int64_t blocks = bpmf_loss_blocks(n);
    if (blocks > 0) bpmf_loss_term_kernel<<<dim3((unsigned)blocks), dim3(BPMF_BLOCK), 0, s>>>(P, Q, R, cu, n, k, gm, term);
    if (strict || blocks == 0) {
        bpmf_loss_chain_kernel<<<1, 64, 0, s>>>(term, n, loss);
    } else {
        bpmf_loss_tree_kernel<<<dim3((unsigned)blocks), dim3(BPMF_BLOCK), 0, s>>>(term, n, part);
        bpmf_loss_chain_kernel<<<1, 64, 0, s>>>(part, blocks, loss);
    }
    return hipGetLastError();
}

// ---- prediction ------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(BPMF_BLOCK) void bpmf_predict_kernel(const double *P, const double *Q, int k, double gm, int64_t n,
                                                                  const int32_t *tu, const int32_t *tj, int bound, double lo, double hi,
                                                                  double *out) {
    const int64_t t = (int64_t)blockIdx.x * BPMF_BLOCK + threadIdx.x;
    if (t >= n) return;
    const double *pp = P + (int64_t)tu[t] * k, *qp = Q + (int64_t)tj[t] * k;
    double dot = 0.0;
    for (int f = 0; f < k; ++f) dot += pp[f] * qp[f];
    out[t] = bound_to_scale(gm + dot, bound, lo, hi);
}

hipError_t bpmf_launch_predict(const double *P, const double *Q, int k, double gm, int64_t n, const int32_t *u, const int32_t *j, int bound,
                               double lo, double hi, double *out, hipStream_t s) {
    if (n <= 0) return hipSuccess;
    bpmf_predict_kernel<<<dim3((unsigned)((n + BPMF_BLOCK - 1) / BPMF_BLOCK)), dim3(BPMF_BLOCK), 0, s>>>(P, Q, k, gm, n, u, j, bound, lo, hi, out);
    return hipGetLastError();
}

} // namespace cmi
