// bpr_kernels.hip -- BPR (carskit/alg/baseline/ranking/BPR.java) on gfx950: the exact device sampler (speculation at every stream
// position, then list ranking), the ordered triple-SGD epoch by levels, and the loss.  fp64, no FMA contraction (-ffp-contract=off):
// products are rounded before sums, as in the reference.
#include "bpr_kernels.hpp"

namespace cmi {

struct JumpArg {
    JavaLcgJump t;
};

// ---- sampler (b): the sample that would start at position d ---------------------------------------------------------------------
__global__ void __launch_bounds__(256) bpr_spec_kernel(BprSampler a, JumpArg jump) {
    const int64_t d = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (d >= a.L) return;
    JavaStream rng{java_lcg_jump(jump.t, a.state0, (uint64_t)d), 0};
    int32_t u, i, j;
    const bool ok = bpr_draw(rng, a.n_users, a.n_items, a.rptr, a.ridx, BPR_DRAW_CAP, u, i, j);
    a.len[d] = ok ? (uint8_t)rng.used : (uint8_t)0;
}

// ---- sampler (c1): per block of positions, every entry point's exit and count, by pointer jumping in LDS ----------------------------
// a node's target is a position in the block (< BPR_RANK_BLOCK), past it (an exit), or BPR_OVERFLOW (it, or a node it reaches inside
// the block, overflowed or would start past L).  Every hop moves forward by 3 draws at least, so 10 doublings cover a block.
__global__ void __launch_bounds__(BPR_RANK_BLOCK) bpr_rank_block_kernel(BprSampler a) {
    __shared__ uint16_t tgt[2][BPR_RANK_BLOCK], num[2][BPR_RANK_BLOCK];
    const int t = threadIdx.x;
    const int64_t d = (int64_t)blockIdx.x * BPR_RANK_BLOCK + t;
    const int len = d < a.L ? (int)a.len[d] : 0;
    tgt[0][t] = len ? (uint16_t)(t + len) : BPR_OVERFLOW;
    num[0][t] = len ? 1 : 0;
    __syncthreads();
    int cur = 0;
    for (int r = 0; r < 10; ++r) {
        uint16_t g = tgt[cur][t], n = num[cur][t];
        if (g < BPR_RANK_BLOCK) {
            n = (uint16_t)(n + num[cur][g]);
            g = tgt[cur][g];
        }
        tgt[cur ^ 1][t] = g, num[cur ^ 1][t] = n;
        cur ^= 1;
        __syncthreads();
    }
    if (t < BPR_RANK_ENTRIES) {
        a.exit_off[(int64_t)blockIdx.x * BPR_RANK_ENTRIES + t] = tgt[cur][t];
        a.cnt[(int64_t)blockIdx.x * BPR_RANK_ENTRIES + t] = num[cur][t];
    }
}

// ---- sampler (c2): one short serial pass over the blocks -------------------------------------------------------------------------------
__global__ void bpr_rank_scan_kernel(BprSampler a) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    int64_t total = 0;
    int32_t e = 0;
    for (int64_t b = 0; b < a.n_blocks; ++b) {
        a.entry[b] = e;
        a.base[b] = total;
        if (e < 0) continue;
        const uint16_t x = a.exit_off[b * BPR_RANK_ENTRIES + e];
        total += a.cnt[b * BPR_RANK_ENTRIES + e];
        e = (x == BPR_OVERFLOW || total >= a.S) ? -1 : (int32_t)x - BPR_RANK_BLOCK;
    }
    a.result[0] = total;
}

// ---- sampler (c3): expansion: the positions of the list's nodes inside every block ---------------------------------------------------
__global__ void __launch_bounds__(256) bpr_rank_expand_kernel(BprSampler a) {
    __shared__ uint8_t len[BPR_RANK_BLOCK];
    const int64_t b = blockIdx.x, d0 = b * BPR_RANK_BLOCK;
    const int32_t e = a.entry[b];
    if (e < 0) return; // uniform over the workgroup
    for (int t = threadIdx.x; t < BPR_RANK_BLOCK; t += blockDim.x) len[t] = d0 + t < a.L ? a.len[d0 + t] : (uint8_t)0;
    __syncthreads();
    if (threadIdx.x != 0) return;
    int64_t s = a.base[b];
    for (int t = e; t < BPR_RANK_BLOCK && s < a.S && len[t]; t += len[t]) a.pos[s++] = d0 + t;
}

// ---- sampler: the triples of the first S nodes ----------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) bpr_emit_kernel(BprSampler a, JumpArg jump) {
    const int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= a.S) return;
    const int64_t d = a.pos[s];
    JavaStream rng{java_lcg_jump(jump.t, a.state0, (uint64_t)d), 0};
    int32_t u = 0, i = 0, j = 0;
    (void)bpr_draw(rng, a.n_users, a.n_items, a.rptr, a.ridx, BPR_DRAW_CAP, u, i, j); // it did not overflow at d: len[d] != 0
    a.u[s] = u, a.i[s] = i, a.j[s] = j;
    if (s == a.S - 1) a.result[1] = d + rng.used;
}

hipError_t bpr_launch_sampler(const BprSampler &a, const JavaLcgJump &jump, hipStream_t s) {
    JumpArg ja{jump};
    hipLaunchKernelGGL(bpr_spec_kernel, dim3((unsigned)((a.L + 255) / 256)), dim3(256), 0, s, a, ja);
    hipLaunchKernelGGL(bpr_rank_block_kernel, dim3((unsigned)a.n_blocks), dim3(BPR_RANK_BLOCK), 0, s, a);
    hipLaunchKernelGGL(bpr_rank_scan_kernel, dim3(1), dim3(64), 0, s, a);
    hipLaunchKernelGGL(bpr_rank_expand_kernel, dim3((unsigned)a.n_blocks), dim3(256), 0, s, a);
    return hipGetLastError();
}
// after the caller has read result[0] >= S
hipError_t bpr_launch_emit(const BprSampler &a, const JavaLcgJump &jump, hipStream_t s) {
    JumpArg ja{jump};
    hipLaunchKernelGGL(bpr_emit_kernel, dim3((unsigned)((a.S + 255) / 256)), dim3(256), 0, s, a, ja);
    return hipGetLastError();
}

// ---- the epoch ------------------------------------------------------------------------------------------------------------------------
constexpr int BPR_REGS = BPR_MAX_K / BPR_GROUP; // factors a lane holds

// BPR.java:83-102 of sample s by one 16-lane group (lane = its index in the group); factor f lives in lane f % 16, register f / 16
__device__ __forceinline__ void bpr_update(const BprEpoch &a, int32_t s, int lane) {
    const int k = a.k;
    const int32_t u = a.u[s], i = a.i[s], j = a.j[s];
    double *pu = a.P + (size_t)u * k, *qi = a.Q + (size_t)i * k, *qj = a.Q + (size_t)j * k;
    double p[BPR_REGS], q1[BPR_REGS], q2[BPR_REGS];
#pragma unroll
    for (int c = 0; c < BPR_REGS; ++c) {
        const int f = c * BPR_GROUP + lane;
        const bool in = f < k;
        p[c] = in ? pu[f] : 0.0, q1[c] = in ? qi[f] : 0.0, q2[c] = in ? qj[f] : 0.0;
    }
    // DenseMatrix.rowMult: res += m[mrow][j] * n[nrow][j], j ascending: the products by their lanes, the two chains by every lane
    double xui = 0.0, xuj = 0.0;
#pragma unroll
    for (int c = 0; c < BPR_REGS; ++c) {
        if (c * BPR_GROUP < k) { // uniform
            const double m1 = p[c] * q1[c], m2 = p[c] * q2[c];
            const int n = min(BPR_GROUP, k - c * BPR_GROUP);
            for (int l = 0; l < n; ++l) {
                xui += __shfl(m1, l, BPR_GROUP);
                xuj += __shfl(m2, l, BPR_GROUP);
            }
        }
    }
    const double xuij = xui - xuj;
    const double vals = -fdlibm_log(java_logistic(xuij));
    const double cmg = java_logistic(-xuij);
    double *slot = a.slots + (size_t)s * (k + 1);
    if (lane == 0) slot[0] = vals;
#pragma unroll
    for (int c = 0; c < BPR_REGS; ++c) {
        const int f = c * BPR_GROUP + lane;
        if (f < k) {
            const double puf = p[c], qif = q1[c], qjf = q2[c];
            const double dp = a.lrate * (cmg * (qif - qjf) - a.regU * puf);
            const double di = a.lrate * (cmg * puf - a.regI * qif);
            const double dj = a.lrate * (cmg * (-puf) - a.regI * qjf);
            pu[f] = puf + dp;
            if (i == j) {
                qi[f] = (qif + di) + dj; // two adds to the one cell, in the reference's order
            } else {
                qi[f] = qif + di;
                qj[f] = qjf + dj;
            }
            slot[1 + f] = a.regU * puf * puf + a.regI * qif * qif + a.regI * qjf * qjf;
        }
    }
}

// one level of any width: a 16-lane group per sample
__global__ void __launch_bounds__(BPR_BLOCK) bpr_level_kernel(BprEpoch a, int32_t begin, int32_t end) {
    const int32_t x = begin + (int32_t)(blockIdx.x * BPR_WG_SAMPLES + threadIdx.x / BPR_GROUP);
    if (x < end) bpr_update(a, a.order[x], threadIdx.x % BPR_GROUP);
}

// a run of levels [l0, l1), none wider than a workgroup's samples: one workgroup, a barrier between levels
__global__ void __launch_bounds__(BPR_BLOCK) bpr_run_kernel(BprEpoch a, int32_t l0, int32_t l1) {
    const int g = threadIdx.x / BPR_GROUP, lane = threadIdx.x % BPR_GROUP;
    for (int32_t l = l0; l < l1; ++l) {
        const int32_t x = a.level_ptr[l] + g;
        if (x < a.level_ptr[l + 1]) bpr_update(a, a.order[x], lane);
        __threadfence_block();
        __syncthreads();
    }
}

hipError_t bpr_launch_level(const BprEpoch &a, int32_t begin, int32_t end, hipStream_t s) {
    if (end <= begin) return hipSuccess;
    hipLaunchKernelGGL(bpr_level_kernel, dim3((unsigned)((end - begin + BPR_WG_SAMPLES - 1) / BPR_WG_SAMPLES)), dim3(BPR_BLOCK), 0, s, a,
                       begin, end);
    return hipGetLastError();
}
hipError_t bpr_launch_run(const BprEpoch &a, int32_t l0, int32_t l1, hipStream_t s) {
    if (l1 <= l0) return hipSuccess;
    hipLaunchKernelGGL(bpr_run_kernel, dim3(1), dim3(BPR_BLOCK), 0, s, a, l0, l1);
    return hipGetLastError();
}

// ---- loss -----------------------------------------------------------------------------------------------------------------------------
// BPR.java:59, :88, :101: one chain in (s, term) order.  The workgroup stages BPR_CHAIN_STAGE terms in LDS with coalesced loads, then
// its first thread adds them in order (the adds depend on one another, the LDS reads do not)
constexpr int BPR_CHAIN_STAGE = 4096;
__global__ void __launch_bounds__(256) bpr_loss_chain_kernel(const double *slots, int64_t n, double *out) {
    __shared__ double sh[BPR_CHAIN_STAGE];
    double loss = 0.0;
    for (int64_t base = 0; base < n; base += BPR_CHAIN_STAGE) {
        const int cnt = (int)min((int64_t)BPR_CHAIN_STAGE, n - base);
        for (int t = threadIdx.x; t < cnt; t += 256) sh[t] = slots[base + t];
        __syncthreads();
        if (threadIdx.x == 0) {
#pragma unroll 16
            for (int t = 0; t < cnt; ++t) loss += sh[t];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) *out = loss;
}

// a fixed tree: thread x of the grid sums the slots x, x + T, x + 2T, ... in order, the workgroup's 256 sums fold in halves in LDS
__device__ __forceinline__ double bpr_fold(double *sh, double v) {
    sh[threadIdx.x] = v;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) sh[threadIdx.x] += sh[threadIdx.x + w];
        __syncthreads();
    }
    return sh[0];
}
__global__ void __launch_bounds__(256) bpr_loss_part_kernel(const double *slots, int64_t n, double *parts) {
    __shared__ double sh[256];
    const int64_t T = (int64_t)gridDim.x * 256;
    double v = 0.0;
    for (int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x; t < n; t += T) v += slots[t];
    v = bpr_fold(sh, v);
    if (threadIdx.x == 0) parts[blockIdx.x] = v;
}
__global__ void __launch_bounds__(256) bpr_loss_final_kernel(const double *parts, double *out) {
    __shared__ double sh[256];
    const double v = bpr_fold(sh, (int)threadIdx.x < BPR_LOSS_PARTS ? parts[threadIdx.x] : 0.0);
    if (threadIdx.x == 0) *out = v;
}

hipError_t bpr_launch_loss(const double *slots, int64_t n, bool strict, double *parts, double *out, hipStream_t s) {
    if (strict) {
        hipLaunchKernelGGL(bpr_loss_chain_kernel, dim3(1), dim3(256), 0, s, slots, n, out);
    } else {
        hipLaunchKernelGGL(bpr_loss_part_kernel, dim3(BPR_LOSS_PARTS), dim3(256), 0, s, slots, n, parts);
        hipLaunchKernelGGL(bpr_loss_final_kernel, dim3(1), dim3(256), 0, s, (const double *)parts, out);
    }
    return hipGetLastError();
}

// ---- probes ---------------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) bpr_next_ints_kernel(uint64_t state, int32_t bound, int64_t n, JumpArg jump, int32_t *val,
                                                            int32_t *used) {
    const int64_t d = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (d >= n) return;
    JavaStream rng{java_lcg_jump(jump.t, state, (uint64_t)d), 0};
    val[d] = rng.nextInt(bound, 4096); // -1: more than 4096 draws (probability 2^-4096 at the worst bound)
    used[d] = (int32_t)rng.used;
}
__global__ void __launch_bounds__(256) bpr_exp_log_kernel(int64_t n, const double *x, double *e, double *l) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n) return;
    e[t] = fdlibm_exp(x[t]);
    l[t] = fdlibm_log(x[t]);
}

hipError_t bpr_launch_next_ints(uint64_t state, int32_t bound, int64_t n, const JavaLcgJump &jump, int32_t *val, int32_t *used,
                                hipStream_t s) {
    if (n <= 0) return hipSuccess;
    JumpArg ja{jump};
    hipLaunchKernelGGL(bpr_next_ints_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, state, bound, n, ja, val, used);
    return hipGetLastError();
}
hipError_t bpr_launch_exp_log(int64_t n, const double *x, double *e, double *l, hipStream_t s) {
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(bpr_exp_log_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, n, x, e, l);
    return hipGetLastError();
}

} // namespace cmi
