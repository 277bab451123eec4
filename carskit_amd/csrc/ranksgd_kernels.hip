// ranksgd_kernels.hip -- RankSGD (carskit/alg/baseline/ranking/RankSGD.java) on gfx950: the tries of the popularity-weighted draw at
// every stream position, and the ordered sample-SGD epoch by levels.  fp64, no FMA contraction (-ffp-contract=off): products are
// rounded before sums, as in the reference.  The loss is bpr_launch_loss over one slot a sample.
#include "ranksgd_kernels.hpp"

#include "ranksgd_host.hpp"

namespace cmi {

struct RanksgdJumpArg {
    JavaLcgJump t;
};

// ---- the tries: a lane per try; a try takes exactly two draws, so try t starts 2t draws after the iteration's first state --------------
__global__ void __launch_bounds__(256) ranksgd_tries_kernel(uint64_t state0, RanksgdJumpArg jump, const int32_t *item, const double *cum,
                                                            int32_t n_table, int64_t n_tries, int32_t *out) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n_tries) return;
    out[t] = ranksgd_try(java_lcg_jump(jump.t, state0, 2 * (uint64_t)t), item, cum, n_table);
}

hipError_t ranksgd_launch_tries(uint64_t state0, const JavaLcgJump &jump, const int32_t *item, const double *cum, int32_t n_table,
                                int64_t n_tries, int32_t *out, hipStream_t s) {
    if (n_tries <= 0) return hipSuccess;
    RanksgdJumpArg ja{jump};
    hipLaunchKernelGGL(ranksgd_tries_kernel, dim3((unsigned)((n_tries + 255) / 256)), dim3(256), 0, s, state0, ja, item, cum, n_table,
                       n_tries, out);
    return hipGetLastError();
}

// ---- the epoch ------------------------------------------------------------------------------------------------------------------------
constexpr int RANKSGD_REGS = BPR_MAX_K / BPR_GROUP; // factors a lane holds

// RankSGD.java:113-132 of sample s by one 16-lane group (lane = its index in the group); factor f lives in lane f % 16, register f / 16
__device__ __forceinline__ void ranksgd_update(const RanksgdEpoch &a, int32_t s, int lane) {
    const int k = a.k;
    const int32_t u = a.u[s], i = a.i[s], j = a.j[s];
    double *pu = a.P + (size_t)u * k, *qi = a.Q + (size_t)i * k, *qj = a.Q + (size_t)j * k;
    double p[RANKSGD_REGS], q1[RANKSGD_REGS], q2[RANKSGD_REGS];
#pragma unroll
    for (int c = 0; c < RANKSGD_REGS; ++c) {
        const int f = c * BPR_GROUP + lane;
        const bool in = f < k;
        p[c] = in ? pu[f] : 0.0, q1[c] = in ? qi[f] : 0.0, q2[c] = in ? qj[f] : 0.0;
    }
    // DenseMatrix.rowMult: res += m[mrow][j] * n[nrow][j], j ascending: the products by their lanes, the two chains by every lane
    double pui = 0.0, puj = 0.0;
#pragma unroll
    for (int c = 0; c < RANKSGD_REGS; ++c) {
        if (c * BPR_GROUP < k) { // uniform
            const double m1 = p[c] * q1[c], m2 = p[c] * q2[c];
            const int n = min(BPR_GROUP, k - c * BPR_GROUP);
            for (int l = 0; l < n; ++l) {
                pui += __shfl(m1, l, BPR_GROUP);
                puj += __shfl(m2, l, BPR_GROUP);
            }
        }
    }
    const double e = (pui - puj) - (a.r[s] - 0.0);
    const double ye = a.lrate * e;
    if (lane == 0) a.slots[s] = e * e;
#pragma unroll
    for (int c = 0; c < RANKSGD_REGS; ++c) {
        const int f = c * BPR_GROUP + lane;
        if (f < k) {
            const double puf = p[c], qif = q1[c], qjf = q2[c];
            const double di = -ye * puf, dj = ye * puf;
            pu[f] = puf + -ye * (qif - qjf);
            if (i == j) {
                qi[f] = (qif + di) + dj; // two adds to the one cell, in the reference's order
            } else {
                qi[f] = qif + di;
                qj[f] = qjf + dj;
            }
        }
    }
}

// one level of any width: a 16-lane group per sample
__global__ void __launch_bounds__(BPR_BLOCK) ranksgd_level_kernel(RanksgdEpoch a, int32_t begin, int32_t end) {
    const int32_t x = begin + (int32_t)(blockIdx.x * BPR_WG_SAMPLES + threadIdx.x / BPR_GROUP);
    if (x < end) ranksgd_update(a, a.order[x], threadIdx.x % BPR_GROUP);
}

// a run of levels [l0, l1), none wider than a workgroup's samples: one workgroup, a barrier between levels
__global__ void __launch_bounds__(BPR_BLOCK) ranksgd_run_kernel(RanksgdEpoch a, int32_t l0, int32_t l1) {
    const int g = threadIdx.x / BPR_GROUP, lane = threadIdx.x % BPR_GROUP;
    for (int32_t l = l0; l < l1; ++l) {
        const int32_t x = a.level_ptr[l] + g;
        if (x < a.level_ptr[l + 1]) ranksgd_update(a, a.order[x], lane);
        __threadfence_block();
        __syncthreads();
    }
}

hipError_t ranksgd_launch_level(const RanksgdEpoch &a, int32_t begin, int32_t end, hipStream_t s) {
    if (end <= begin) return hipSuccess;
    hipLaunchKernelGGL(ranksgd_level_kernel, dim3((unsigned)((end - begin + BPR_WG_SAMPLES - 1) / BPR_WG_SAMPLES)), dim3(BPR_BLOCK), 0, s,
                       a, begin, end);
    return hipGetLastError();
}
hipError_t ranksgd_launch_run(const RanksgdEpoch &a, int32_t l0, int32_t l1, hipStream_t s) {
    if (l1 <= l0) return hipSuccess;
    hipLaunchKernelGGL(ranksgd_run_kernel, dim3(1), dim3(BPR_BLOCK), 0, s, a, l0, l1);
    return hipGetLastError();
}

} // namespace cmi
