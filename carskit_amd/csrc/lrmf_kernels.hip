// lrmf_kernels.hip -- LRMF (carskit/alg/baseline/ranking/LRMF.java) on gfx950: the list-wise SGD epoch by user units.  One workgroup
// runs one user's cells in the matrix iterator's order with P[u] and, when they fit, the user's item rows in LDS.  fp64, no FMA
// contraction (-ffp-contract=off): products are rounded before sums, as in the reference.
#include "lrmf_kernels.hpp"

namespace cmi {

constexpr int LRMF_DOT = 8; // factors whose LDS reads are in flight together

// DenseMatrix.rowMult: res += m[mrow][j] * n[nrow][j], j ascending: one chain of adds.  The loads and the products of LRMF_DOT factors
// are issued together (a load at a time under the add that needs it costs an LDS round trip per factor); the adds stay in order
__device__ __forceinline__ double lrmf_dot(const double *p, const double *q, int k) {
    double d = 0.0;
    int f = 0;
    for (; f + LRMF_DOT <= k; f += LRMF_DOT) {
        double pv[LRMF_DOT], qv[LRMF_DOT];
#pragma unroll
        for (int x = 0; x < LRMF_DOT; ++x) pv[x] = p[f + x], qv[x] = q[f + x];
#pragma unroll
        for (int x = 0; x < LRMF_DOT; ++x) d += pv[x] * qv[x];
    }
    if (f < k) { // the last k % LRMF_DOT factors: nothing is read past the row
        double pv[LRMF_DOT], qv[LRMF_DOT];
#pragma unroll
        for (int x = 0; x < LRMF_DOT; ++x) {
            const bool in = f + x < k;
            pv[x] = in ? p[f + x] : 0.0, qv[x] = in ? q[f + x] : 0.0;
        }
#pragma unroll
        for (int x = 0; x < LRMF_DOT; ++x)
            if (f + x < k) d += pv[x] * qv[x];
    }
    return d;
}

// LRMF.java:75-103 of user u's cells by one workgroup.  sh: LRMF_LDS_FIXED doubles, then the unit's rows at lrmf_stride(k) if it keeps
// them in LDS.  The LDS form and the global form are one text: they differ in where a row pointer points, and in the staging and the
// write-back.  The form is a template argument so that every row pointer has one address space: a pointer that may be either makes
// each row access a flat one, with which the LDS form was no faster than the global one (profiles/README.md, lrmf_bench.json)
template <bool lds>
__device__ __forceinline__ void lrmf_unit_form(const LrmfEpoch &a, int32_t u, double *sh) {
    const int k = a.k, tid = (int)threadIdx.x;
    const int32_t c0 = a.ptr[u], n = a.ptr[u + 1] - c0;
    double *shP = sh, *shE = sh + LRMF_MAX_K, *shS = shE + 2 * LRMF_BLOCK, *shQ = sh + LRMF_LDS_FIXED;
    const int stride = lrmf_stride(k);
    double *pu = a.P + (size_t)u * k;
    for (int f = tid; f < k; f += LRMF_BLOCK) shP[f] = pu[f];
    if (lds)
        for (int x = tid; x < n * k; x += LRMF_BLOCK) {
            const int r = x / k, f = x - r * k;
            shQ[r * stride + f] = a.Q[(size_t)a.col[c0 + r] * k + f];
        }
    // what the first pass's lane needs of its item in every cell: read once
    const bool nz0 = tid < n && a.nz[c0 + tid];
    const int32_t r0 = min(tid, n - 1); // a lane past the last item holds a valid pointer it never reads through
    const double *q0 = lds ? shQ + r0 * stride : a.Q + (size_t)a.col[c0 + r0] * k;
    double A = a.A[c0], A_prev = 0.0; // of the cell at hand and of the one before; the next cell's is loaded a cell ahead
    __syncthreads();
    int buf = 0;
    for (int32_t c = 0; c < n; ++c) {
        const double A_next = c + 1 < n ? a.A[c0 + c + 1] : 0.0;
        // :84-87: a lane per stored item forms rowMult(P, u, Q, i) as one chain in factor order and its exp; thread 0 adds the exps in
        // item order, one chain from 0.0 across the passes.  A stored zero is no member of getColumns(u): its lane contributes +0.0,
        // which leaves every partial sum (all of them are >= +0.0, or NaN) bit for bit as it is; so do the lanes past the last item,
        // which lets the chain run in whole blocks.  The cell's own lane also leaves pred (:81) and exp(pred): the same chain and the
        // same function of it
        double uexp = 0.0;
        for (int32_t base = 0; base < n; base += LRMF_BLOCK) {
            const int32_t r = base + tid;
            double e = 0.0;
            if (r < n) {
                const double *q = base == 0 ? q0 : (lds ? shQ + r * stride : a.Q + (size_t)a.col[c0 + r] * k);
                const double d = lrmf_dot(shP, q, k);
                e = fdlibm_exp(d);
                if (r == c) shS[1] = d, shS[2] = e;
                if (!(base == 0 ? nz0 : (bool)a.nz[c0 + r])) e = 0.0;
            }
            shE[buf * LRMF_BLOCK + tid] = e;
            __syncthreads();
            if (tid == 0) { // the other threads go on to the next pass, which fills the other buffer
                const int cnt = min(LRMF_BLOCK, n - base);
                const double *e8 = shE + buf * LRMF_BLOCK;
                double v[8];
#pragma unroll
                for (int x = 0; x < 8; ++x) v[x] = e8[x];
                for (int t = 0; t < cnt; t += 8) { // the next block's reads under this block's adds
                    const int nt = t + 8 < LRMF_BLOCK ? t + 8 : t;
                    double w[8];
#pragma unroll
                    for (int x = 0; x < 8; ++x) w[x] = e8[nt + x];
#pragma unroll
                    for (int x = 0; x < 8; ++x) uexp += v[x];
#pragma unroll
                    for (int x = 0; x < 8; ++x) v[x] = w[x];
                }
            }
            buf ^= 1;
        }
        if (tid == 0) shS[0] = uexp;
        // while thread 0 adds the last pass's chain, three idle threads take what does not wait for uexp off the cell's path:
        // g(pred) and g(-pred) of gd(pred) = g(pred) * g(-pred) (Recommender.java:1140-1149; Math.exp(-(-pred)) is the exp(pred) the
        // cell's lane left), and the loss term of the cell before, whose log feeds nothing but the loss
        if (tid == LRMF_BLOCK - 1) shS[3] = java_logistic(shS[1]);
        if (tid == LRMF_BLOCK - 2) shS[4] = 1.0 / (1.0 + shS[2]);
        if (tid == LRMF_BLOCK - 3 && c > 0) a.slots[(size_t)(c0 + c - 1) * (k + 1)] = -(A_prev * fdlibm_log(shS[5])); // loss -= x is loss += -x
        __syncthreads();
        if (tid < k) { // :89-102: a lane per factor; puf and qjf are read before either add
            const int f = tid;
            double *qj = lds ? shQ + c * stride : a.Q + (size_t)a.col[c0 + c] * k;
            const double B = shS[2] / shS[0];
            const double d = (A - B) * (shS[3] * shS[4]);
            const double puf = shP[f], qjf = qj[f];
            shP[f] = puf + a.lrate * (d * qjf - a.regU * puf);
            qj[f] = qjf + a.lrate * (d * puf - a.regI * qjf);
            if (f == 0) shS[5] = B;
            a.slots[(size_t)(c0 + c) * (k + 1) + 1 + f] = 0.5 * a.regU * puf * puf + 0.5 * a.regI * qjf * qjf;
        }
        A_prev = A, A = A_next;
        __threadfence_block();
        __syncthreads();
    }
    if (tid == LRMF_BLOCK - 3) a.slots[(size_t)(c0 + n - 1) * (k + 1)] = -(A_prev * fdlibm_log(shS[5]));
    for (int f = tid; f < k; f += LRMF_BLOCK) pu[f] = shP[f];
    if (lds)
        for (int x = tid; x < n * k; x += LRMF_BLOCK) {
            const int r = x / k, f = x - r * k;
            a.Q[(size_t)a.col[c0 + r] * k + f] = shQ[r * stride + f];
        }
}

__device__ __forceinline__ void lrmf_unit(const LrmfEpoch &a, int32_t u, double *sh) {
    if (a.ptr[u + 1] - a.ptr[u] <= a.lds_rows) lrmf_unit_form<true>(a, u, sh); // uniform over the workgroup
    else lrmf_unit_form<false>(a, u, sh);
}

// one level: a workgroup per unit
__global__ void __launch_bounds__(LRMF_BLOCK) lrmf_level_kernel(LrmfEpoch a, int32_t x0) {
    extern __shared__ double lrmf_sh[];
    lrmf_unit(a, a.order[x0 + (int32_t)blockIdx.x], lrmf_sh);
}

// single-unit levels order[x0, x1): one workgroup, a barrier between units
__global__ void __launch_bounds__(LRMF_BLOCK) lrmf_run_kernel(LrmfEpoch a, int32_t x0, int32_t x1) {
    extern __shared__ double lrmf_sh[];
    for (int32_t x = x0; x < x1; ++x) {
        lrmf_unit(a, a.order[x], lrmf_sh);
        __threadfence_block();
        __syncthreads();
    }
}

// a launch of more than 64 KiB of dynamic LDS states so first
template <typename Kernel>
static hipError_t lrmf_allow_lds(Kernel kernel, size_t bytes) {
    if (bytes <= 64 * 1024) return hipSuccess;
    return hipFuncSetAttribute(reinterpret_cast<const void *>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
}

hipError_t lrmf_launch_level(const LrmfEpoch &a, int32_t x0, int32_t x1, int32_t rows, hipStream_t s) {
    if (x1 <= x0) return hipSuccess;
    const size_t bytes = lrmf_lds_bytes(a.k, rows);
    if (bytes > (size_t)LRMF_LDS_BYTES) return hipErrorInvalidValue;
    if (hipError_t e = lrmf_allow_lds(lrmf_level_kernel, bytes)) return e;
    hipLaunchKernelGGL(lrmf_level_kernel, dim3((unsigned)(x1 - x0)), dim3(LRMF_BLOCK), bytes, s, a, x0);
    return hipGetLastError();
}
hipError_t lrmf_launch_run(const LrmfEpoch &a, int32_t x0, int32_t x1, int32_t rows, hipStream_t s) {
    if (x1 <= x0) return hipSuccess;
    const size_t bytes = lrmf_lds_bytes(a.k, rows);
    if (bytes > (size_t)LRMF_LDS_BYTES) return hipErrorInvalidValue;
    if (hipError_t e = lrmf_allow_lds(lrmf_run_kernel, bytes)) return e;
    hipLaunchKernelGGL(lrmf_run_kernel, dim3(1), dim3(LRMF_BLOCK), bytes, s, a, x0, x1);
    return hipGetLastError();
}

} // namespace cmi
