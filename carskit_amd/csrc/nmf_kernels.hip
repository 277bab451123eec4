// nmf_kernels.hip -- NMF on gfx950: the multiplicative W / H update (NMF.buildModel), its loss and the prediction (NMF.predict).
// Everything is fp64 with the reference's operation order: every sum is one left-to-right chain from 0.0 with a rounding per multiply and
// per add (no FMA: -ffp-contract=off), and division is the correctly rounded IEEE operation Java uses.  A row's update depends on that
// row's entries alone, so rows never meet: no cross-row sums, no atomics, the same bits on every run.
#include "nmf_kernels.hpp"
#include "eval_device.hpp"

namespace cmi {

// lane `l`'s value of a wave-uniform lane index, through the scalar unit (v_readlane), not the LDS crossbar
__device__ __forceinline__ int nmf_lane_i(int v, int l) { return __builtin_amdgcn_readlane(v, l); }
__device__ __forceinline__ double nmf_lane_d(double v, int l) {
    const int lo = __builtin_amdgcn_readlane(__double2loint(v), l), hi = __builtin_amdgcn_readlane(__double2hiint(v), l);
    return __hiloint2double(hi, lo);
}

// ---- the row update --------------------------------------------------------------------------------------------------------------
// A wave owns a row (a user in the W phase, an item in the H phase) and keeps it in registers, a lane per factor (G factors a lane for
// k up to 64 G), with a copy in LDS that the prediction chain reads.  The row's entries are taken NMF_CHUNK at a time, in two steps:
//   1. a lane per ENTRY: the lane walks its partner's k-row and forms e_t = product(W, u, H, j) as the ordered chain over f.  64 chains
//      run side by side, none crosses a lane;
//   2. a lane per FACTOR: the wave walks the chunk's entries in order, reads entry t's partner row again (coalesced, from the cache
//      step 1 filled) and adds r_t * h and e_t * h to the lane's two running sums (DenseVector.inner(uv), inner(euv)), which are carried
//      from chunk to chunk.  r_t, e_t and the partner's index reach every lane through v_readlane.
// The row is written once, at the end: own[f] * (real / (estm + 1e-9)), from the row as it was at entry.
template <int G>
__global__ __launch_bounds__(NMF_BLOCK) void nmf_row_kernel(double *own, const double *other, PairCsr C, const int32_t *order, int n_order,
                                                            int k) {
    __shared__ double s_w[NMF_BLOCK / 64][64 * G];
    constexpr int B = G <= 2 ? 8 : 4; // entries loaded ahead in step 2: 16 k-row pieces a lane at most
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int slot = blockIdx.x * (NMF_BLOCK / 64) + wave;
    const bool has = slot < n_order;
    const int row = has ? order[slot] : 0;
    double *wrow = own + (int64_t)row * k;
    double *sw = s_w[wave];
    double w[G], real[G], estm[G];
#pragma unroll
    for (int g = 0; g < G; ++g) {
        const int f = lane + 64 * g;
        w[g] = has && f < k ? wrow[f] : 0.0;
        real[g] = estm[g] = 0.0;
        sw[f] = w[g];
    }
    __syncthreads();
    if (!has) return;
    const int e1 = C.ptr[row + 1];
    for (int base = C.ptr[row]; base < e1; base += NMF_CHUNK) {
        const int cnt = min(NMF_CHUNK, e1 - base);
        const int q = base + min(lane, cnt - 1); // the lanes past the row's end repeat its last entry; step 2 never reads them
        const int x = C.idx[q];
        const double r = C.val[q];
        const double *hp = other + (int64_t)x * k;
        double e = 0.0;
        int f = 0;
        for (; f + 8 <= k; f += 8) { // eight loads in flight ahead of the chain
            double hv[8];
#pragma unroll
            for (int a = 0; a < 8; ++a) hv[a] = hp[f + a];
#pragma unroll
            for (int a = 0; a < 8; ++a) e += sw[f + a] * hv[a];
        }
        for (; f < k; ++f) e += sw[f] * hp[f];

        int t = 0;
        for (; t + B <= cnt; t += B) { // B entries' partner rows in flight ahead of the two chains
            double h[B][G], rt[B], et[B];
#pragma unroll
            for (int a = 0; a < B; ++a) {
                const double *ht = other + (int64_t)nmf_lane_i(x, t + a) * k;
                rt[a] = nmf_lane_d(r, t + a);
                et[a] = nmf_lane_d(e, t + a);
#pragma unroll
                for (int g = 0; g < G; ++g) h[a][g] = lane + 64 * g < k ? ht[lane + 64 * g] : 0.0;
            }
#pragma unroll
            for (int a = 0; a < B; ++a)
#pragma unroll
                for (int g = 0; g < G; ++g) {
                    real[g] += rt[a] * h[a][g];
                    estm[g] += et[a] * h[a][g];
                }
        }
        for (; t < cnt; ++t) {
            const double *ht = other + (int64_t)nmf_lane_i(x, t) * k;
            const double rt = nmf_lane_d(r, t), et = nmf_lane_d(e, t);
#pragma unroll
            for (int g = 0; g < G; ++g) {
                const double h = lane + 64 * g < k ? ht[lane + 64 * g] : 0.0;
                real[g] += rt * h;
                estm[g] += et * h;
            }
        }
    }
#pragma unroll
    for (int g = 0; g < G; ++g)
        if (lane + 64 * g < k) wrow[lane + 64 * g] = w[g] * (real[g] / (estm[g] + 1e-9));
}

hipError_t nmf_launch_rows(double *own, const double *other, PairCsr csr, const int32_t *order, int n_order, int k, hipStream_t s) {
    if (n_order <= 0) return hipSuccess;
    if (k < 1 || k > NMF_MAX_K) return hipErrorInvalidValue;
    const dim3 grid((unsigned)((n_order + NMF_BLOCK / 64 - 1) / (NMF_BLOCK / 64))), block(NMF_BLOCK);
    switch ((k + 63) / 64) {
    case 1: nmf_row_kernel<1><<<grid, block, 0, s>>>(own, other, csr, order, n_order, k); break;
    case 2: nmf_row_kernel<2><<<grid, block, 0, s>>>(own, other, csr, order, n_order, k); break;
    case 3: nmf_row_kernel<3><<<grid, block, 0, s>>>(own, other, csr, order, n_order, k); break;
    default: nmf_row_kernel<4><<<grid, block, 0, s>>>(own, other, csr, order, n_order, k); break;
    }
    return hipGetLastError();
}

// ---- loss ------------------------------------------------------------------------------------------------------------------------
// A lane per cell: its term (predict(u, j) - r)^2, or 0.0 where r > 0 does not hold (adding +0.0 changes no non-negative sum).  A
// block's 256 terms are added in a fixed tree (shuffles inside a wave, then the four waves in order) into part[block]; the second kernel
// adds the partials in block order in one chain and halves the sum.
__global__ __launch_bounds__(NMF_BLOCK) void nmf_loss_kernel(const double *W, const double *Ht, PairCsr R, const int32_t *cu, int64_t nnz,
                                                             int k, double *part) {
    __shared__ double s_wave[NMF_BLOCK / 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t q = (int64_t)blockIdx.x * NMF_BLOCK + threadIdx.x;
    double term = 0.0;
    if (q < nnz) {
        const double r = R.val[q];
        if (r > 0) {
            const double *wp = W + (int64_t)cu[q] * k, *hp = Ht + (int64_t)R.idx[q] * k;
            double pred = 0.0;
            for (int f = 0; f < k; ++f) pred += wp[f] * hp[f];
            const double euj = pred - r;
            term = euj * euj;
        }
    }
    for (int off = 32; off; off >>= 1) term += __shfl_down(term, off);
    if (lane == 0) s_wave[wave] = term;
    __syncthreads();
    if (threadIdx.x == 0) part[blockIdx.x] = ((s_wave[0] + s_wave[1]) + s_wave[2]) + s_wave[3];
}

// one wave: 64 partials a load, added lane after lane by every lane alike
__global__ __launch_bounds__(64) void nmf_loss_final_kernel(const double *part, int64_t n_part, double *loss) {
    const int lane = threadIdx.x;
    double s = 0.0;
    double next = lane < n_part ? part[lane] : 0.0;
    for (int64_t base = 0; base < n_part; base += 64) {
        const double cur = next;
        const int64_t p = base + 64 + lane;
        next = p < n_part ? part[p] : 0.0;
        const int cnt = (int)min<int64_t>(64, n_part - base);
        for (int l = 0; l < cnt; ++l) s += nmf_lane_d(cur, l);
    }
    if (lane == 0) *loss = s * 0.5;
}

hipError_t nmf_launch_loss(const double *W, const double *Ht, PairCsr rows, const int32_t *cu, int64_t nnz, int k, double *part,
                           double *loss, hipStream_t s) {
    const int64_t blocks = nmf_loss_blocks(nnz);
    if (blocks > 0) nmf_loss_kernel<<<dim3((unsigned)blocks), dim3(NMF_BLOCK), 0, s>>>(W, Ht, rows, cu, nnz, k, part);
    nmf_loss_final_kernel<<<1, 64, 0, s>>>(part, blocks, loss);
    return hipGetLastError();
}

// ---- prediction ------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(NMF_BLOCK) void nmf_predict_kernel(const double *W, const double *Ht, int k, int64_t n, const int32_t *tu,
                                                                const int32_t *tj, int bound, double lo, double hi, double *out) {
    const int64_t t = (int64_t)blockIdx.x * NMF_BLOCK + threadIdx.x;
    if (t >= n) return;
    const double *wp = W + (int64_t)tu[t] * k, *hp = Ht + (int64_t)tj[t] * k;
    double pred = 0.0;
    for (int f = 0; f < k; ++f) pred += wp[f] * hp[f];
    out[t] = bound_to_scale(pred, bound, lo, hi);
}

hipError_t nmf_launch_predict(const double *W, const double *Ht, int k, int64_t n, const int32_t *u, const int32_t *j, int bound, double lo,
                              double hi, double *out, hipStream_t s) {
    if (n <= 0) return hipSuccess;
    nmf_predict_kernel<<<dim3((unsigned)((n + NMF_BLOCK - 1) / NMF_BLOCK)), dim3(NMF_BLOCK), 0, s>>>(W, Ht, k, n, u, j, bound, lo, hi, out);
    return hipGetLastError();
}

} // namespace cmi
