// cptf_kernels.hip -- CPTF (src/carskit/alg/cars/adaptation/independent/CPTF.java) on gfx950, fp64.
//
// The epoch (CPTF.java:81-109) is ONE wave, like CAMF_C's (camfc_pipe.hip): nearly every entry touches the same few context rows, so the
// sweep is a single dependency chain.  Factor f of an entry is untouched until its own turn in the reference's loops, so the update is
// parallel over f and only `pred` (and the loss) crosses factors:
//   * lane l owns the MAXC consecutive factors [l * MAXC, (l + 1) * MAXC) of every row of the entry (MAXC = 1 for k <= 64, else 2);
//     a lane past k computes factor k - 1 again from the same inputs and stores the same value to the same word, so no memory operation
//     of the loop sits under a lane mask or a branch;
//   * the rows of entry t + 1 are requested before entry t computes (their offsets a further entry ahead, so no address waits for a
//     scalar load).  A requested row is stale exactly when entry t writes it (same dimension, same key): it is then replaced from the
//     registers that hold entry t's updated row.  Writers further back had issued their stores before the request, and a wave's stores
//     and later loads of one address stay ordered;
//   * context rows (dimensions >= 2) live in LDS for the whole epoch when they fit CPTF_LDS_CTX_BYTES (a wave's LDS operations are in
//     order), else they travel through memory like the user and item rows.
// `sgd` is the product `pred` took (same operands, same order, nothing written in between), so it is formed once.
#include "cptf_kernels.hpp"

namespace cmi {
namespace {

template <int CTRL, int ROW_MASK>
__device__ __forceinline__ double cdpp(double x) {
    const int lo = __builtin_amdgcn_update_dpp(0, __double2loint(x), CTRL, ROW_MASK, 0xf, false);
    const int hi = __builtin_amdgcn_update_dpp(0, __double2hiint(x), CTRL, ROW_MASK, 0xf, false);
    return __hiloint2double(hi, lo);
}
__device__ __forceinline__ double crl(double x, int lane) {
    return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(x), lane), __builtin_amdgcn_readlane(__double2loint(x), lane));
}
// the fixed tree of camfc_pipe.hip's pwave_sum: rotations by 8, 4, 2, 1 inside the rows of 16 lanes, then row 0 into row 1 and row 2
// into row 3, then row 1 into rows 2 and 3; lane 63 holds (r3 + r2) + (r1 + r0)
__device__ __forceinline__ double cwave_sum(double x) {
    x += cdpp<0x128, 0xf>(x);
    x += cdpp<0x124, 0xf>(x);
    x += cdpp<0x122, 0xf>(x);
    x += cdpp<0x121, 0xf>(x);
    x += cdpp<0x142, 0xa>(x);
    x += cdpp<0x143, 0xc>(x);
    return crl(x, 63);
}

template <int ND, int MAXC, bool LDSCTX>
__global__ __launch_bounds__(64) void cptf_epoch_kernel(CptfEpoch a) {
    extern __shared__ double s_ctx[];
    constexpr int GD = LDSCTX ? 2 : ND; // the dimensions whose rows travel through memory
    const int lane = (int)threadIdx.x, k = a.m.k;
    double *__restrict__ M = a.m.M;
    const int64_t n = a.n, ctx0 = a.m.off[2], ctx_n = a.m.off[ND] - ctx0;
    const int64_t S = 1 + (int64_t)k * ND;
    if (LDSCTX) {
        for (int64_t i = lane; i < ctx_n; i += 64) s_ctx[i] = M[ctx0 + i];
        __syncthreads();
    }
    int fo[MAXC];
    bool act[MAXC];
#pragma unroll
    for (int c = 0; c < MAXC; ++c) {
        const int f = lane * MAXC + c;
        act[c] = f < k;
        fo[c] = act[c] ? f : k - 1;
    }
    double nxt[GD][MAXC], cur[ND][MAXC], upd[ND][MAXC], acc[MAXC], acc_e = 0.0;
    int64_t o_c[ND], o_n[ND], o_nn[ND];
#pragma unroll
    for (int c = 0; c < MAXC; ++c) acc[c] = 0.0;
    const int64_t t1 = n > 1 ? 1 : 0;
#pragma unroll
    for (int d = 0; d < ND; ++d) o_n[d] = a.row[d], o_nn[d] = a.row[t1 * ND + d];
#pragma unroll
    for (int d = 0; d < GD; ++d)
#pragma unroll
        for (int c = 0; c < MAXC; ++c) nxt[d][c] = M[o_n[d] + fo[c]];

    for (int64_t t = 0; t < n; ++t) {
#pragma unroll
        for (int d = 0; d < ND; ++d) o_c[d] = o_n[d], o_n[d] = o_nn[d];
#pragma unroll
        for (int d = 0; d < GD; ++d)
#pragma unroll
            for (int c = 0; c < MAXC; ++c) cur[d][c] = nxt[d][c];
        const double rr = a.r[t];
        // the rows of entry t + 1 (of the last entry: its own again, unused) and the offsets of entry t + 2
#pragma unroll
        for (int d = 0; d < GD; ++d)
#pragma unroll
            for (int c = 0; c < MAXC; ++c) nxt[d][c] = M[o_n[d] + fo[c]];
        const int64_t t2 = t + 2 < n ? t + 2 : n - 1;
#pragma unroll
        for (int d = 0; d < ND; ++d) o_nn[d] = a.row[t2 * ND + d];
        if (LDSCTX) {
#pragma unroll
            for (int d = 2; d < ND; ++d)
#pragma unroll
                for (int c = 0; c < MAXC; ++c) cur[d][c] = s_ctx[(int)(o_c[d] - ctx0) + fo[c]];
        }

        // CPTF.java:141-155: the product starts at 1 and runs over d; the sum is a chain in f (strict) or the fixed tree
        double prod[MAXC];
#pragma unroll
        for (int c = 0; c < MAXC; ++c) {
            double p = 1.0;
#pragma unroll
            for (int d = 0; d < ND; ++d) p *= cur[d][c];
            prod[c] = p;
        }
        double pred = 0.0;
        if (a.strict) {
            for (int f = 0; f < k; ++f) {
                double v = prod[0];
#pragma unroll
                for (int c = 1; c < MAXC; ++c)
                    if (f % MAXC == c) v = prod[c];
                pred += crl(v, f / MAXC);
            }
        } else {
            double part = act[0] ? prod[0] : 0.0;
#pragma unroll
            for (int c = 1; c < MAXC; ++c) part += act[c] ? prod[c] : 0.0;
            pred = cwave_sum(part);
        }
        const double e = rr - pred; // :89
        const double ee = e * e;    // :91
        acc_e += ee;
        if (a.strict && lane == 0) a.slots[t * S] = ee;
        // :93-108
#pragma unroll
        for (int c = 0; c < MAXC; ++c) {
            const double sgd = prod[c];
#pragma unroll
            for (int d = 0; d < ND; ++d) {
                const double df = cur[d][c];
                const double gdf = sgd / df * e;
                upd[d][c] = df + a.lrate * (gdf - a.reg * df);
                const double term = a.reg * df * df;
                acc[c] += term;
                if (a.strict && act[c]) a.slots[t * S + 1 + (int64_t)(lane * MAXC + c) * ND + d] = term;
            }
        }
#pragma unroll
        for (int d = 0; d < ND; ++d)
#pragma unroll
            for (int c = 0; c < MAXC; ++c) {
                if (d < GD) {
                    M[o_c[d] + fo[c]] = upd[d][c];
                    if (o_n[d] == o_c[d]) nxt[d][c] = upd[d][c]; // the requested row of entry t + 1 is the one just written
                } else {
                    s_ctx[(int)(o_c[d] - ctx0) + fo[c]] = upd[d][c];
                }
            }
    }
    if (!a.strict) {
        if (lane == 0) a.parts[0] = acc_e;
#pragma unroll
        for (int c = 0; c < MAXC; ++c)
            if (act[c]) a.parts[1 + lane * MAXC + c] = acc[c];
    }
    if (LDSCTX) {
        __syncthreads();
        for (int64_t i = lane; i < ctx_n; i += 64) M[ctx0 + i] = s_ctx[i];
    }
}

template <int ND, int MAXC>
hipError_t epoch_launch(const CptfEpoch &a, hipStream_t s) {
    if (a.lds_ctx) {
        const size_t bytes = (size_t)(a.m.off[ND] - a.m.off[2]) * sizeof(double);
        hipLaunchKernelGGL((cptf_epoch_kernel<ND, MAXC, true>), dim3(1), dim3(64), bytes, s, a);
    } else {
        hipLaunchKernelGGL((cptf_epoch_kernel<ND, MAXC, false>), dim3(1), dim3(64), 0, s, a);
    }
    return hipGetLastError();
}

template <int MAXC>
hipError_t epoch_dims(const CptfEpoch &a, hipStream_t s) {
    switch (a.m.n_dims) {
    case 2: return epoch_launch<2, MAXC>(a, s);
    case 3: return epoch_launch<3, MAXC>(a, s);
    case 4: return epoch_launch<4, MAXC>(a, s);
    case 5: return epoch_launch<5, MAXC>(a, s);
    case 6: return epoch_launch<6, MAXC>(a, s);
    case 7: return epoch_launch<7, MAXC>(a, s);
    case 8: return epoch_launch<8, MAXC>(a, s);
    case 9: return epoch_launch<9, MAXC>(a, s);
    case 10: return epoch_launch<10, MAXC>(a, s);
    }
    return hipErrorInvalidValue;
}

__global__ void cptf_loss_kernel(const double *__restrict__ terms, int64_t n, double *loss) {
    double l = 0.0;
    for (int64_t i = 0; i < n; ++i) l += terms[i];
    *loss = l;
}

__device__ __forceinline__ double cptf_clamp(double pred, double lo, double hi) {
    if (pred > hi) pred = hi; // CPTF.java:133-136: a NaN stays
    if (pred < lo) pred = lo;
    return pred;
}

__global__ __launch_bounds__(256) void cptf_predict_kernel(CptfModel m, int64_t n, const int32_t *__restrict__ keys, bool bound, double lo,
                                                           double hi, double *__restrict__ out) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n) return;
    const double *row[CPTF_MAX_DIMS];
#pragma unroll
    for (int d = 0; d < CPTF_MAX_DIMS; ++d) row[d] = d < m.n_dims ? m.M + m.off[d] + (int64_t)keys[t * m.n_dims + d] * m.k : m.M;
    double pred = 0.0;
    for (int f = 0; f < m.k; ++f) {
        double p = 1.0;
#pragma unroll
        for (int d = 0; d < CPTF_MAX_DIMS; ++d)
            if (d < m.n_dims) p *= row[d][f];
        pred += p;
    }
    out[t] = bound ? cptf_clamp(pred, lo, hi) : pred;
}

__global__ __launch_bounds__(256) void cptf_transpose_kernel(const double *__restrict__ Q, int n_items, int k, double *__restrict__ Qt) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (int64_t)n_items * k) return;
    const int f = (int)(i / n_items), j = (int)(i % n_items);
    Qt[i] = Q[(int64_t)j * k + f];
}

// a block: one query and 256 candidates; a thread: one candidate, the factors in order.  The query's user row and context rows are
// staged in LDS (every thread reads the same word: a broadcast); the item matrix is read transposed, adjacent lanes adjacent items
__global__ __launch_bounds__(256) void cptf_score_kernel(CptfModel m, const double *__restrict__ Qt, int n_items,
                                                         const int32_t *__restrict__ cand, int nc, const int32_t *__restrict__ qu,
                                                         const int32_t *__restrict__ qkeys, int64_t q0, double lo, double hi,
                                                         double *__restrict__ S) {
    __shared__ double s_rows[(CPTF_MAX_DIMS - 1) * CPTF_MAX_K];
    const int64_t q = q0 + blockIdx.x;
    const int k = m.k, nx = m.n_dims - 1; // the staged rows: the user's, then the context's
    for (int i = (int)threadIdx.x; i < nx * k; i += (int)blockDim.x) {
        const int x = i / k, f = i % k;
        const int d = x == 0 ? 0 : x + 1;
        const int64_t key = x == 0 ? qu[q] : qkeys[q * (m.n_dims - 2) + (x - 1)];
        s_rows[i] = m.M[m.off[d] + key * k + f];
    }
    __syncthreads();
    const int c = (int)blockIdx.y * (int)blockDim.x + (int)threadIdx.x;
    if (c >= nc) return;
    const int64_t item = cand[c];
    double pred = 0.0;
    for (int f = 0; f < k; ++f) {
        double p = 1.0;
        p *= s_rows[f];
        p *= Qt[(int64_t)f * n_items + item];
        for (int x = 1; x < nx; ++x) p *= s_rows[x * k + f];
        pred += p;
    }
    S[(int64_t)blockIdx.x * nc + c] = cptf_clamp(pred, lo, hi);
}

} // namespace

hipError_t cptf_launch_epoch(const CptfEpoch &a, hipStream_t stream) {
    if (a.n <= 0) return hipSuccess;
    return a.m.k <= 64 ? epoch_dims<1>(a, stream) : epoch_dims<2>(a, stream);
}

hipError_t cptf_launch_loss(const double *terms, int64_t n_terms, double *loss, hipStream_t stream) {
    hipLaunchKernelGGL(cptf_loss_kernel, dim3(1), dim3(1), 0, stream, terms, n_terms, loss);
    return hipGetLastError();
}

hipError_t cptf_launch_predict(const CptfModel &m, int64_t n, const int32_t *keys, bool bound, double lo, double hi, double *out,
                               hipStream_t stream) {
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(cptf_predict_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, m, n, keys, bound, lo, hi, out);
    return hipGetLastError();
}

hipError_t cptf_launch_transpose_items(const CptfModel &m, int n_items, double *Qt, hipStream_t stream) {
    const int64_t total = (int64_t)n_items * m.k;
    hipLaunchKernelGGL(cptf_transpose_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream, m.M + m.off[1], n_items, m.k, Qt);
    return hipGetLastError();
}

hipError_t cptf_launch_score(const CptfModel &m, const double *Qt, int n_items, const int32_t *cand, int nc, const int32_t *qu,
                             const int32_t *qkeys, int64_t q0, int64_t nq, double lo, double hi, double *S, hipStream_t stream) {
    if (nq <= 0 || nc <= 0) return hipSuccess;
    hipLaunchKernelGGL(cptf_score_kernel, dim3((unsigned)nq, (unsigned)((nc + 255) / 256)), dim3(256), 0, stream, m, Qt, n_items, cand, nc,
                       qu, qkeys, q0, lo, hi, S);
    return hipGetLastError();
}

} // namespace cmi
