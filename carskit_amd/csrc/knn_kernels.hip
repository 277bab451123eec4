// knn_kernels.hip -- ItemKNN / UserKNN on gfx950: the similarity build (Recommender.buildCorrs + correlation + happy.coding.math.Sims)
// and the neighbourhood prediction (ItemKNN.predict / UserKNN.predict).  Everything is fp64 with the reference's operation order:
// every per-pair sum runs sequentially in one lane along the ascending contracted index (no lane-split reductions, no FMA:
// -ffp-contract=off), and division / sqrt are the correctly rounded IEEE operations Java uses.
#include "knn_kernels.hpp"

#include <algorithm>

#include "eval_device.hpp"
#include "java_hash.hpp"
#include "../../include/carskit_mi355x.h"

namespace cmi {

// ---- similarity build ----------------------------------------------------------------------------------------------------------
// A workgroup owns an anchor row a and its partners b > a, one per lane (chunks of PAIR_BUILD_BLOCK), and meets every pair's common
// entries in ascending order by the shared walk (pair_walk.hpp); the measure's running sums stay in the lane's registers.  pcc sweeps
// the anchor's tiles twice (the means of the common lists first, then the centred sums), as Sims.pcc does.
template <int M>
__global__ __launch_bounds__(PAIR_BUILD_BLOCK) void knn_build_kernel(PairCsr R, int n, const double *norm2, int shrinkage, double median,
                                                                     double *S) {
    // correlation(): iv.contains(idx) misses an anchor entry; cos-binary counts those entries and keeps the byte beside the value
    __shared__ PairTile<M == CMI_SIM_COS_BINARY ? PairOk::BESIDE : PairOk::FOUND> T;
    const int a = blockIdx.x;
    const int a0 = R.ptr[a], a1 = R.ptr[a + 1];
    if (a0 == a1 || a + 1 >= n) return; // Recommender.buildCorrs skips empty rows
    pair_tile_init(T);
    int gen = 0;
    constexpr int PASSES = M == CMI_SIM_PCC ? 2 : 1;
    for (int c = a + 1; c < n; c += blockDim.x) {
        const int b = c + (int)threadIdx.x;
        const int b0 = b < n ? R.ptr[b] : 0, b1 = b < n ? R.ptr[b + 1] : 0;
        const bool act = b0 < b1;
        int k = 0;
        double x1 = 0.0, x2 = 0.0, x3 = 0.0, mua = 0.0, mub = 0.0;
        for (int pass = 0; pass < PASSES; ++pass) {
            if (pass == 1) { // Stats.mean of the two common lists, then the centred sums start from zero
                mua = x1 / (double)k;
                mub = x2 / (double)k;
                x1 = x2 = 0.0;
            }
            // va, vb: is.add(iv.get(idx)), js.add(jv.get(idx))
            pair_sweep(R, a0, a1, b0, b1, act, T, gen, [&](double va, double vb, int slot, int cur) {
                if (M == CMI_SIM_PCC) {
                    if (pass == 0) {
                        x1 += va;
                        x2 += vb;
                        ++k;
                    } else {
                        const double da = va - mua, db = vb - mub;
                        x1 += da * db;
                        x2 += da * da;
                        x3 += db * db;
                    }
                } else if (M == CMI_SIM_MSD) {
                    const double d = va - vb; // Math.pow(d, 2.0) == d * d
                    x1 += d * d;
                    ++k;
                } else if (M == CMI_SIM_CPC) {
                    const double da = va - median, db = vb - median;
                    x1 += da * db;
                    x2 += da * da;
                    x3 += db * db;
                    ++k;
                } else if (M == CMI_SIM_COS_BINARY) {
                    if (R.ok[cur]) x1 += va * vb; // iv.inner(jv): jv.contains(idx)
                    k += T.ok[slot];              // n = is.size(): the entries iv.contains finds
                } else { // cos, exjaccard
                    x1 += va * vb;
                    x2 += va * va;
                    x3 += vb * vb;
                    ++k;
                }
            });
        }
        if (!act) continue;
        double sim;
        if (M == CMI_SIM_PCC) sim = k < 2 ? __builtin_nan("") : x1 / (__dsqrt_rn(x2) * __dsqrt_rn(x3));
        else if (M == CMI_SIM_COS || M == CMI_SIM_CPC) sim = k == 0 ? __builtin_nan("") : x1 / (__dsqrt_rn(x2) * __dsqrt_rn(x3));
        else if (M == CMI_SIM_COS_BINARY) sim = x1 / (__dsqrt_rn(norm2[a]) * __dsqrt_rn(norm2[b]));
        else if (M == CMI_SIM_MSD) {
            sim = (double)k / x1;
            if (__builtin_isinf(sim)) sim = 1.0;
        } else sim = x1 / (x2 + x3 - x1); // exJaccard
        if (__builtin_isnan(sim)) continue; // NaN is not stored
        if (shrinkage > 0) sim *= (double)k / (double)(k + shrinkage);
        S[(int64_t)a * n + b] = sim;
        S[(int64_t)b * n + a] = sim;
    }
}

hipError_t knn_launch_build(PairCsr rows, int n, const double *norm2, int measure, int shrinkage, double median, double *S,
                            hipStream_t s) {
    if (n <= 1) return hipSuccess;
    const dim3 g(n), b(PAIR_BUILD_BLOCK);
    switch (measure) {
    case CMI_SIM_COS: knn_build_kernel<CMI_SIM_COS><<<g, b, 0, s>>>(rows, n, norm2, shrinkage, median, S); break;
    case CMI_SIM_COS_BINARY: knn_build_kernel<CMI_SIM_COS_BINARY><<<g, b, 0, s>>>(rows, n, norm2, shrinkage, median, S); break;
    case CMI_SIM_MSD: knn_build_kernel<CMI_SIM_MSD><<<g, b, 0, s>>>(rows, n, norm2, shrinkage, median, S); break;
    case CMI_SIM_CPC: knn_build_kernel<CMI_SIM_CPC><<<g, b, 0, s>>>(rows, n, norm2, shrinkage, median, S); break;
    case CMI_SIM_EXJACCARD: knn_build_kernel<CMI_SIM_EXJACCARD><<<g, b, 0, s>>>(rows, n, norm2, shrinkage, median, S); break;
    default: knn_build_kernel<CMI_SIM_PCC><<<g, b, 0, s>>>(rows, n, norm2, shrinkage, median, S); break;
    }
    return hipGetLastError();
}

__global__ void knn_row_stats_kernel(PairCsr R, int n, double *mean, double *norm2) {
    const int v = blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= n) return;
    double s = 0.0, q = 0.0;
    for (int e = R.ptr[v]; e < R.ptr[v + 1]; ++e) { // Stats.sum(data) / count; inner(v, v) -- both in index order
        s += R.val[e];
        if (R.ok[e]) q += R.val[e] * R.val[e]; // iv.inner(iv): iv.contains(idx)
    }
    const int c = R.ptr[v + 1] - R.ptr[v];
    mean[v] = c > 0 ? s / (double)c : __builtin_nan("");
    norm2[v] = q;
}

hipError_t knn_launch_row_stats(PairCsr rows, int n, double *mean, double *norm2, hipStream_t s) {
    if (n <= 0) return hipSuccess;
    knn_row_stats_kernel<<<(n + 255) / 256, 256, 0, s>>>(rows, n, mean, norm2);
    return hipGetLastError();
}

// ---- prediction --------------------------------------------------------------------------------------------------------------
// ItemKNN / UserKNN.predict iterate a java.util.HashMap<Integer, Double>: java_hash.hpp has its rule (Integer.hashCode() is the value).
// The table's growth while keys kat(0..n-1) are put in that order; cap == 0: a new map (16 slots at the first put).  *tree: a bin
// would be treeified (its order is not modelled).  Called by the whole wave; cnt: 64 ints of LDS.
template <class K>
__device__ void hm_grow(K kat, int n, int &cap, int &thr, int &tree, int32_t *cnt) {
    const int lane = threadIdx.x;
    __shared__ int32_t sh[3];
    if (cap == 0) cap = 16, thr = 12;
    if (lane == 0) { // tables below 64 slots: the serial walk (at most 48 puts)
        sh[0] = java_walk_below_64(kat, n, cap, thr, cnt);
        sh[1] = cap, sh[2] = thr;
    }
    __syncthreads();
    const int t0 = sh[0];
    cap = sh[1], thr = sh[2];
    __syncthreads();
    // 64 slots and more, the parallel form of JavaHashTable::fill's rule: the capacity follows the size alone, and a put that finds 8
    // nodes in its bin at the capacity in force for that put is refused.  Nine keys in one bucket of such a table share their low 6
    // hash bits, so a histogram mod 64 rules most maps out before the exact count.
    int flag = 0;
    if (t0 < n) {
        if (lane < 64) cnt[lane] = 0;
        __syncthreads();
        for (int i = lane; i < n; i += 64) atomicAdd(&cnt[java_spread(kat(i)) & 63], 1);
        __syncthreads();
        bool maybe = false;
        for (int b = 0; b < 64; ++b) maybe |= cnt[b] >= 9;
        __syncthreads();
        if (maybe) {
            for (int i = t0 + lane; i < n; i += 64) {
                int ci = cap, ti = thr;
                while (i > ti) ci <<= 1, ti <<= 1; // the table when key i is put (size i)
                const uint32_t hi = java_spread(kat(i));
                int same = 0;
                for (int s = 0; s < i; ++s) same += ((java_spread(kat(s)) ^ hi) & (uint32_t)(ci - 1)) == 0;
                flag |= same >= 8;
            }
        }
        while (n > thr) cap <<= 1, thr <<= 1;
    }
    tree |= __any(flag) ? 1 : 0;
}

// ItemKNN / UserKNN.predict(u, j) for one tuple, by the whole wave; lane 0 returns the unbounded prediction.  list_at(q, e, rv, me)
// gives entry q of the owner's list (id, rating, mean[id]), ascending; Sg is the target's row of S, mg its mean.  RANKING is the keep
// rule.  false (ItemKNN.java:94, UserKNN.java:96): sim > 0 (NaN = unset fails) and a rating > 0.  true (isRankingPred, ItemKNN.java:92,
// UserKNN.java:94): a rating > 0 alone, over the indices of corrs.row(target), from which librec's SymmMatrix.row() leaves out the
// entries equal to zero: sim is set, sim != 0.0 and a rating > 0.  Everything after the filter is one text for both.
template <bool RANKING, class ListAt>
__device__ double knn_tuple(int n_list, ListAt list_at, const double *Sg, double mg, int knn, double gm, const KnnScratch w, int32_t *cnt,
                            int &tree) {
    const int lane = threadIdx.x;
    int32_t *key = w.key, *pos = w.pos, *sel = w.sel;
    double *sim = w.sim, *dlt = w.dlt;
    // candidates in ascending id order
    int m = 0;
    for (int base = 0; base < n_list; base += 64) {
        const int q = base + lane;
        bool keep = false;
        int e = 0;
        double sv = 0.0, rv = 0.0, me = 0.0;
        if (q < n_list) {
            list_at(q, e, rv, me);
            sv = Sg[e];
            keep = RANKING ? (sv == sv && sv != 0.0 && rv > 0.0) : (sv > 0.0 && rv > 0.0);
        }
        const uint64_t bal = __ballot(keep);
        const int off = m + __popcll(bal & ((1ull << lane) - 1ull));
        if (keep) key[off] = e, sim[off] = sv, dlt[off] = rv - me;
        m += __popcll(bal);
    }
    __syncthreads();
    double pred = gm;
    if (m > 0) {
        int cap = 0, thr = 0;
        hm_grow([&](int i) { return key[i]; }, m, cap, thr, tree, cnt);
        const uint32_t mask1 = (uint32_t)(cap - 1);
        for (int i = lane; i < m; i += 64) { // HashMap position: (bucket, insertion)
            const uint32_t bi = java_spread(key[i]) & mask1;
            int p = 0;
            for (int s = 0; s < m; ++s) {
                const uint32_t bs = java_spread(key[s]) & mask1;
                p += bs < bi || (bs == bi && s < i);
            }
            pos[i] = p;
        }
        __syncthreads();
        int len = m;
        int32_t *ord = sel;
        if (knn > 0 && knn < m) {
            // Lists.sortMap(nns, true): a stable sort by value, descending, of the HashMap's entry list; the first knn survive
            for (int i = lane; i < m; i += 64) {
                int r = 0;
                for (int s = 0; s < m; ++s) r += sim[s] > sim[i] || (sim[s] == sim[i] && pos[s] < pos[i]);
                if (r < knn) sel[r] = i;
            }
            __syncthreads();
            // nns.clear() keeps the table; the survivors are put back in sorted order
            hm_grow([&](int r) { return key[sel[r]]; }, knn, cap, thr, tree, cnt);
            const uint32_t mask2 = (uint32_t)(cap - 1);
            for (int r = lane; r < knn; r += 64) {
                const uint32_t br = java_spread(key[sel[r]]) & mask2;
                int p = 0;
                for (int s = 0; s < knn; ++s) {
                    const uint32_t bs = java_spread(key[sel[s]]) & mask2;
                    p += bs < br || (bs == br && s < r);
                }
                pos[p] = sel[r];
            }
            ord = pos;
            len = knn;
        } else {
            for (int i = lane; i < m; i += 64) sel[pos[i]] = i;
        }
        __syncthreads();
        if (lane == 0) { // the weighted sum in the final iteration order
            double sum = 0.0, ws = 0.0;
            for (int r = 0; r < len; ++r) {
                const int i = ord[r];
                sum += sim[i] * dlt[i];
                ws += fabs(sim[i]);
            }
            pred = ws > 0.0 ? (__builtin_isnan(mg) ? gm : mg) + sum / ws : gm;
        }
    }
    return pred;
}

// the first tuple whose HashMap would treeify a bin: bad[0] counts them, bad[1], bad[2] name the first one counted
__device__ void knn_record_tree(int32_t *bad, int u, int j) {
    if (atomicAdd(&bad[0], 1) == 0) bad[1] = u, bad[2] = j;
}

template <bool RANKING>
__global__ __launch_bounds__(64) void knn_predict_kernel(PairCsr L, const double *S, int n_ent, const double *mean, int64_t n,
                                                         const int32_t *owner, const int32_t *target, int knn, double gm, int bound,
                                                         double lo, double hi, double *out, int cap_entries, KnnScratch all, int32_t *bad) {
    __shared__ int32_t cnt[64];
    const int lane = threadIdx.x;
    const size_t w0 = (size_t)blockIdx.x * cap_entries;
    const KnnScratch w{all.key + w0, all.pos + w0, all.sel + w0, all.sim + w0, all.dlt + w0};
    for (int64_t t = blockIdx.x; t < n; t += gridDim.x) {
        const int o = owner[t], g = target[t];
        const int l0 = L.ptr[o];
        int tree = 0;
        double pred = knn_tuple<RANKING>(
            L.ptr[o + 1] - l0, [&](int q, int &e, double &rv, double &me) { e = L.idx[l0 + q], rv = L.val[l0 + q], me = mean[e]; },
            S + (int64_t)g * n_ent, mean[g], knn, gm, w, cnt, tree);
        if (lane == 0) {
            pred = bound_to_scale(pred, bound, lo, hi);
            if (tree) {
                knn_record_tree(bad, o, g);
                pred = __builtin_nan("");
            }
            out[t] = pred;
        }
        __syncthreads();
    }
}

hipError_t knn_launch_predict(PairCsr lists, const double *S, int n_ent, const double *mean, int64_t n, const int32_t *owner,
                              const int32_t *target, int knn, double global_mean, bool ranking, int bound, double lo, double hi,
                              double *out, int nwaves, int cap, KnnScratch scratch, int32_t *bad, hipStream_t s) {
    if (n <= 0) return hipSuccess;
    if (ranking)
        knn_predict_kernel<true><<<nwaves, 64, 0, s>>>(lists, S, n_ent, mean, n, owner, target, knn, global_mean, bound, lo, hi, out, cap,
                                                       scratch, bad);
    else
        knn_predict_kernel<false><<<nwaves, 64, 0, s>>>(lists, S, n_ent, mean, n, owner, target, knn, global_mean, bound, lo, hi, out, cap,
                                                        scratch, bad);
    return hipGetLastError();
}

// ---- top-N scores --------------------------------------------------------------------------------------------------------------
// ranking(u, j) = predict(u, j) under isRankingPred for the slab of an evaluation (rank_run_device_slab).  A wave takes a unit of
// work, (group of queries of one user, tile of KNN_SCORE_TILE candidates), and scores the tile's candidates in turn with knn_tuple; the
// tile's scores wait in LDS and go, a lane per candidate, to every query of the group inside [q0, q0 + nq).  ItemKNN: the owner list is
// the user's row, the same for every candidate, so its ids, ratings and mean[id] are staged in LDS once per unit (a row longer than
// KNN_STAGE is read from memory) and only S[j][ids] is gathered per candidate.  UserKNN: the target row S[u] is fixed per unit and the
// owner list is the candidate's column.
template <bool ITEM>
__global__ __launch_bounds__(64) void knn_score_kernel(PairCsr L, const double *S, int n_ent, const double *mean, const int32_t *cand, int nc,
                                                       const int32_t *gu, const int32_t *gq0, int g0, int ng, int64_t q0, int64_t nq, int knn,
                                                       double gm, double *out, int cap_entries, KnnScratch all, int32_t *bad) {
    __shared__ int32_t cnt[64];
    __shared__ int32_t s_id[ITEM ? KNN_STAGE : 1];
    __shared__ double s_rate[ITEM ? KNN_STAGE : 1], s_mean[ITEM ? KNN_STAGE : 1];
    __shared__ double s_pred[KNN_SCORE_TILE];
    const int lane = threadIdx.x;
    const size_t w0 = (size_t)blockIdx.x * cap_entries;
    const KnnScratch w{all.key + w0, all.pos + w0, all.sel + w0, all.sim + w0, all.dlt + w0};
    const int tiles = (nc + KNN_SCORE_TILE - 1) / KNN_SCORE_TILE;
    for (int64_t unit = blockIdx.x; unit < (int64_t)ng * tiles; unit += gridDim.x) {
        // tile-major: the waves in flight share a tile's rows of S (ItemKNN) or columns (UserKNN), and a wave's units differ in tile
        // and group alike (group-major, a wave would keep one tile index whenever the grid is a multiple of the tile count)
        const int g = g0 + (int)(unit % ng);
        const int c0 = (int)(unit / ng) * KNN_SCORE_TILE, c1 = min(nc, c0 + KNN_SCORE_TILE);
        const int u = gu[g];
        const int u0 = ITEM ? L.ptr[u] : 0, ulen = ITEM ? L.ptr[u + 1] - u0 : 0;
        const bool staged = ITEM && ulen <= KNN_STAGE;
        if (staged)
            for (int q = lane; q < ulen; q += 64) {
                const int e = L.idx[u0 + q];
                s_id[q] = e, s_rate[q] = L.val[u0 + q], s_mean[q] = mean[e];
            }
        __syncthreads();
        for (int c = c0; c < c1; ++c) {
            const int j = cand[c];
            int tree = 0;
            double pred;
            if (staged) {
                pred = knn_tuple<true>(
                    ulen, [&](int q, int &e, double &rv, double &me) { e = s_id[q], rv = s_rate[q], me = s_mean[q]; },
                    S + (int64_t)j * n_ent, mean[j], knn, gm, w, cnt, tree);
            } else {
                const int o = ITEM ? u : j, t = ITEM ? j : u;
                const int l0 = L.ptr[o];
                pred = knn_tuple<true>(
                    L.ptr[o + 1] - l0, [&](int q, int &e, double &rv, double &me) { e = L.idx[l0 + q], rv = L.val[l0 + q], me = mean[e]; },
                    S + (int64_t)t * n_ent, mean[t], knn, gm, w, cnt, tree);
            }
            if (lane == 0) {
                if (tree) {
                    knn_record_tree(bad, u, j);
                    pred = __builtin_nan("");
                }
                s_pred[c - c0] = pred;
            }
            __syncthreads();
        }
        const int64_t qa = max((int64_t)gq0[g], q0), qb = min((int64_t)gq0[g + 1], q0 + nq);
        if (c0 + lane < c1)
            for (int64_t q = qa; q < qb; ++q) out[(size_t)(q - q0) * (size_t)nc + (size_t)(c0 + lane)] = s_pred[lane];
        __syncthreads();
    }
}

hipError_t knn_launch_score(bool item, PairCsr lists, const double *S, int n_ent, const double *mean, int knn, double global_mean,
                            int nwaves, int cap, KnnScratch scratch, int32_t *bad, const int32_t *cand, int nc, const int32_t *gu,
                            const int32_t *gq0, int g0, int g1, int64_t q0, int64_t nq, double *out, hipStream_t s) {
    if (g1 <= g0 || nc <= 0 || nq <= 0) return hipSuccess;
    const int64_t units = (int64_t)(g1 - g0) * ((nc + KNN_SCORE_TILE - 1) / KNN_SCORE_TILE);
    const int grid = (int)std::min<int64_t>(units, nwaves);
    if (item)
        knn_score_kernel<true><<<grid, 64, 0, s>>>(lists, S, n_ent, mean, cand, nc, gu, gq0, g0, g1 - g0, q0, nq, knn, global_mean, out, cap,
                                                   scratch, bad);
    else
        knn_score_kernel<false><<<grid, 64, 0, s>>>(lists, S, n_ent, mean, cand, nc, gu, gq0, g0, g1 - g0, q0, nq, knn, global_mean, out, cap,
                                                    scratch, bad);
    return hipGetLastError();
}

} // namespace cmi
